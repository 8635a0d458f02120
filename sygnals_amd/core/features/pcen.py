"""PCEN (per-channel energy normalisation, librosa.pcen) on the device, over the kernels of csrc/pcen.hip.

pcen takes librosa's signature for one [M, T] array (NumPy or tensor in, NumPy float64 out); pcen_batch takes [B, M, T]
device tensors (or arrays that are uploaded) and stays on the device; pcen_mel_batch goes from clips [B, L] to the PCEN of
their mel block without leaving the device.  Parity with librosa is unpinned (it is not a dependency): the float64
restatement tests/pcen_ref.py is the contract.  What is not served raises ValueError."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ... import _pcen as PC
from ... import ops
from ..audio.features import _as_clips

__all__ = ["pcen", "pcen_batch", "pcen_mel_batch"]

torch = ops.torch


def _dev3(S, who: str):
    """[B, M, T] float32 on the device (a float32 tensor is taken as it is; an array is uploaded)."""
    if hasattr(S, "is_cuda"):
        return S
    a = np.asarray(S)
    if np.iscomplexobj(a):
        raise ValueError(f"{who}: S must be real and non-negative (a magnitude or power spectrogram; take np.abs first)")
    if a.ndim != 3:
        raise ValueError(f"{who}: S must be [B, M, T] (got {a.ndim} dimensions)")
    if a.size == 0:
        raise ValueError(f"{who}: empty input (shape {list(a.shape)})")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(ops.require_gpu())


def pcen_batch(S, sr: float = 22050, hop_length: int = 512, gain=0.98, bias=2.0, power=0.5, time_constant: float = 0.4,
               eps=1e-6, b=None, max_size: int = 1, scale: float = 1.0, zi=None, return_zf: bool = False, out=None, form=None):
    """ops.pcen on [B, M, T] (a device tensor, or an array that is uploaded): float32 [B, M, T] on the device, with
    return_zf also the closing filter state [B, M] float64."""
    return ops.pcen(_dev3(S, "pcen_batch"), sr, hop_length, gain, bias, power, time_constant, eps, b, max_size, scale, zi,
                    return_zf, out, form)


def pcen(S, *, sr: float = 22050, hop_length: int = 512, gain: float = 0.98, bias: float = 2.0, power: float = 0.5,
         time_constant: float = 0.4, eps: float = 1e-6, b: Optional[float] = None, max_size: int = 1, ref=None, axis: int = -1,
         max_axis: Optional[int] = None, zi=None, return_zf: bool = False):
    """librosa.pcen of one [M, T] array (bands, frames), or of [T]: float64 NumPy, with return_zf also zf in librosa's shape
    [M, 1].  zi: librosa's [M, 1] (or [M]).  Served: axis = -1 with the bands on the axis in front of it (max_axis None or
    that axis); ref= arrays are not served (the reference is S or its running maximum over max_size bands)."""
    who = "pcen"
    if ref is not None:
        raise ValueError(f"{who}: ref= arrays are not served (the reference signal is S, or with max_size > 1 its running "
                         "maximum over bands)")
    a = S.detach().cpu().numpy() if hasattr(S, "detach") else np.asarray(S)
    if np.iscomplexobj(a):
        raise ValueError(f"{who}: S must be real and non-negative (a magnitude or power spectrogram; take np.abs first)")
    if a.ndim not in (1, 2):
        raise ValueError(f"{who}: S must be [M, T] or [T] (got {a.ndim} dimensions); pcen_batch takes [B, M, T]")
    if axis not in (-1, a.ndim - 1):
        raise ValueError(f"{who}: axis = {axis} is not served (frames are the last axis: axis = -1)")
    if max_axis is not None and (a.ndim != 2 or max_axis not in (0, -2)):
        raise ValueError(f"{who}: max_axis = {max_axis} is not served (bands are the axis in front of the frames)")
    if max_size != 1 and a.ndim == 1:
        raise ValueError(f"{who}: max_size > 1 needs a band axis (S is one-dimensional)")
    if a.size == 0:
        raise ValueError(f"{who}: empty input (shape {list(a.shape)})")
    a2 = a.reshape(-1, a.shape[-1])
    M = a2.shape[0]
    if zi is not None:
        z = zi.detach().cpu().numpy() if hasattr(zi, "detach") else np.asarray(zi, dtype=np.float64)
        if z.shape not in ((M, 1), (M,)):
            raise ValueError(f"{who}: zi must be [M, 1] = [{M}, 1] (scipy.signal.lfilter's state of every band; got {list(z.shape)})")
        zi = np.ascontiguousarray(z, dtype=np.float64).reshape(1, M)
    res = pcen_batch(a2[None], sr, hop_length, gain, bias, power, time_constant, eps, b, max_size, 1.0, zi, return_zf)
    if return_zf:
        y, zf = res
        return y[0].cpu().numpy().astype(np.float64).reshape(a.shape), zf.cpu().numpy().reshape(M, 1)
    return res[0].cpu().numpy().astype(np.float64).reshape(a.shape)


def pcen_mel_batch(y, sr: float = 22050, n_fft: int = 2048, hop: int = 512, n_mels: int = 128, fmin: float = 0.0, fmax=None,
                   mel_power: float = 1.0, scale: float = 2 ** 31, **pcen_args):
    """Clips y [B, L] -> PCEN of their mel block, float32 [B, n_mels, T] on the device: stft_front(..., power=mel_power)
    followed by ops.pcen (hop_length = hop; scale as librosa's documentation recommends for magnitude mels).  pcen_args:
    gain, bias, power, time_constant, eps, b, max_size, zi, return_zf, form."""
    extra = set(pcen_args) - {"gain", "bias", "power", "time_constant", "eps", "b", "max_size", "zi", "return_zf", "form"}
    if extra:
        raise ValueError(f"pcen_mel_batch: unknown arguments {sorted(extra)}")
    if isinstance(n_mels, bool) or not isinstance(n_mels, (int, np.integer)) or n_mels < 1:
        raise ValueError(f"pcen_mel_batch: n_mels must be an integer >= 1 (got {n_mels!r})")
    PC.check_scale(scale, "pcen_mel_batch")
    mel = ops.stft_front(_as_clips(y), sr, n_fft, hop, n_mels=int(n_mels), fmin=fmin, fmax=fmax, power=mel_power)[0]
    return ops.pcen(mel, sr=sr, hop_length=hop, scale=scale, **pcen_args)
