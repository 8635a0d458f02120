"""Kaldi-compatible fbank and MFCC (torchaudio.compliance.kaldi.fbank / mfcc) on the device, over csrc/kaldi_front.hip.

fbank and mfcc take torchaudio's keywords for one waveform (a 1-D array, or (channels, L) with channel=) and return NumPy
[T, C] (Kaldi's layout); fbank_batch and mfcc_batch take clips [B, L] (a float32 device tensor, or an array that is
uploaded) and stay on the device.  Parity with torchaudio / Kaldi is unpinned (neither is a dependency): the float64
restatement tests/kaldi_ref.py is the contract.  Not served, and refused with a ValueError: vtln_warp != 1,
round_to_power_of_two=False, padded frame lengths outside 256 ... 2048."""
from __future__ import annotations

import numpy as np

from ... import _kaldi as KD
from ... import ops

__all__ = ["fbank", "mfcc", "fbank_batch", "mfcc_batch"]

torch = ops.torch


def _clips(y, who: str):
    if hasattr(y, "is_cuda"):
        return y
    a = np.asarray(y)
    if a.ndim != 2 or np.iscomplexobj(a):
        raise ValueError(f"{who}: y must be real clips [B, L] (got shape {list(a.shape)})")
    if a.size == 0:
        raise ValueError(f"{who}: empty input (shape {list(a.shape)})")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(ops.require_gpu())


def fbank_batch(y, sample_frequency: float = 16000.0, layout: str = "tc", seed: int = 0, out=None, **kw):
    """ops.kaldi_fbank on clips [B, L]: float32 [B, T, C] on the device (layout "tc", Kaldi's own) or [B, C, T] ("ct")."""
    KD.check("fbank_batch", False, sample_frequency, kw)
    KD.check_layout("fbank_batch", layout)
    return ops.kaldi_fbank(_clips(y, "fbank_batch"), sample_frequency, layout, seed, out, **kw)


def mfcc_batch(y, sample_frequency: float = 16000.0, layout: str = "tc", seed: int = 0, out=None, return_fbank: bool = False,
               **kw):
    """ops.kaldi_mfcc on clips [B, L]: float32 [B, T, num_ceps] on the device ("tc") or [B, num_ceps, T] ("ct")."""
    KD.check("mfcc_batch", True, sample_frequency, kw)
    KD.check_layout("mfcc_batch", layout)
    return ops.kaldi_mfcc(_clips(y, "mfcc_batch"), sample_frequency, layout, seed, out, return_fbank, **kw)


def _one(who, is_mfcc, waveform, channel, sample_frequency, seed, kw):
    KD.check(who, is_mfcc, sample_frequency, kw)
    a = waveform.detach().cpu().numpy() if hasattr(waveform, "detach") else np.asarray(waveform)
    if np.iscomplexobj(a) or a.ndim not in (1, 2):
        raise ValueError(f"{who}: waveform must be real, [L] or [channels, L] (got shape {list(a.shape)})")
    if a.ndim == 2:
        if isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or not -1 <= channel < a.shape[0]:
            raise ValueError(f"{who}: channel = {channel!r} is outside the {a.shape[0]} channels (-1: the first, as in torchaudio)")
        a = a[max(int(channel), 0)]
    if a.shape[0] < 1:
        raise ValueError(f"{who}: empty waveform")
    f = (mfcc_batch if is_mfcc else fbank_batch)(a[None], sample_frequency, "tc", seed, **kw)
    return f[0].cpu().numpy()


def fbank(waveform, *, channel: int = -1, sample_frequency: float = 16000.0, seed: int = 0, **kw) -> np.ndarray:
    """torchaudio.compliance.kaldi.fbank of one waveform: NumPy float32 [T, num_mel_bins + use_energy].  **kw: torchaudio's
    keywords with its defaults (povey window, 25 ms / 10 ms, 23 bins, pre-emphasis 0.97, dither 0 ...)."""
    return _one("fbank", False, waveform, channel, sample_frequency, seed, kw)


def mfcc(waveform, *, channel: int = -1, sample_frequency: float = 16000.0, seed: int = 0, **kw) -> np.ndarray:
    """torchaudio.compliance.kaldi.mfcc of one waveform: NumPy float32 [T, num_ceps]."""
    return _one("mfcc", True, waveform, channel, sample_frequency, seed, kw)


def kaldi_fbank(waveform, **kw) -> np.ndarray:
    """fbank under the name the plugin registers it by."""
    return fbank(waveform, **kw)


def kaldi_mfcc(waveform, **kw) -> np.ndarray:
    """mfcc under the name the plugin registers it by."""
    return mfcc(waveform, **kw)
