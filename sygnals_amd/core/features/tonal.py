"""Tonal features on the device: librosa 0.10's feature.chroma_stft / chroma_cqt / chroma_cens / tonnetz, estimate_tuning,
pitch_tuning and piptrack over the kernels of csrc/chroma.hip, after the device STFT and CQT.

The *_batch calls take clips y [B, L] (a float32 device tensor, or an array that is uploaded) or a precomputed S= / C= /
chroma= in librosa's layout with a leading batch axis ([B, F, T], [B, K, T], [B, n_chroma, T]; arrays or device tensors), and
return float32 device tensors [B, n_chroma, T] (tonnetz [B, 6, T]).  The single-clip calls take librosa's signatures and
return NumPy.  tuning=None estimates the tuning per clip (the estimate is a histogram's argmax, taken on the host from
integer counts); clips with distinct tunings get one table per distinct value.  Parity with librosa is unpinned (it is not a
dependency): the float64 restatement of tests/chroma_ref.py is the contract.  What is not served raises ValueError."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ... import _chroma as CH
from ... import ops
from ..audio.features import _as_clips

__all__ = ["chroma_stft", "chroma_cqt", "chroma_cens", "tonnetz", "estimate_tuning", "pitch_tuning", "piptrack",
           "chroma_stft_batch", "chroma_cqt_batch", "chroma_cens_batch", "tonnetz_batch", "estimate_tuning_batch",
           "piptrack_batch"]

torch = ops.torch
pitch_tuning = CH.pitch_tuning          # a histogram of a list of frequencies: host arithmetic, as librosa's


def _dev_real(a, dims: int, who: str, what: str):
    """A real array or tensor of `dims` dimensions as a float32 device tensor."""
    if hasattr(a, "is_cuda"):
        t = a
        if t.dim() != dims:
            raise ValueError(f"{who}: {what} must have {dims} dimensions (got {t.dim()})")
        return t if (t.is_cuda and t.dtype == torch.float32) else t.to(device=ops.require_gpu(), dtype=torch.float32)
    a = np.asarray(a)
    if a.ndim != dims:
        raise ValueError(f"{who}: {what} must have {dims} dimensions (got {a.ndim})")
    if np.iscomplexobj(a):
        raise ValueError(f"{who}: {what} must be real (a magnitude or power spectrogram)")
    if a.size == 0:
        raise ValueError(f"{who}: {what} is empty (shape {list(a.shape)})")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(ops.require_gpu())


def _check_stft(n_fft, hop_length, win_length, pad_mode, who):
    n_fft = CH.check_n_fft(n_fft, who)
    CH.check_pad_mode(pad_mode, who)
    hop = n_fft // 4 if hop_length is None else hop_length
    if not (isinstance(hop, (int, np.integer)) and hop >= 1):
        raise ValueError(f"{who}: hop_length must be a positive integer")
    if win_length is not None and not (isinstance(win_length, (int, np.integer)) and 1 <= win_length <= n_fft):
        raise ValueError(f"{who}: win_length must be in 1 .. n_fft")
    return n_fft, int(hop)


def _spectrogram(y, S, n_fft, hop, win_length, window, center, who):
    """(X frame-major on the device: complex [B, T, F, 2] from y, or real [B, T, F] from S [B, F, T]; n_fft)."""
    if S is not None:
        S = _dev_real(S, 3, who, "S")
        if S.shape[1] < 2:
            raise ValueError(f"{who}: S must have at least 2 frequency bins")
        if n_fft // 2 + 1 != S.shape[1]:
            n_fft = 2 * (int(S.shape[1]) - 1)
        return S.transpose(1, 2).contiguous(), n_fft
    if y is None:
        raise ValueError(f"{who}: either the audio y or S must be given")
    return ops.stft_any(_as_clips(y), n_fft, hop, center, window, win_length), n_fft


def _groups(tunings: np.ndarray):
    """(value, clip indices) per distinct tuning, in order of first appearance."""
    seen = {}
    for i, v in enumerate(np.asarray(tunings, dtype=np.float64).tolist()):
        seen.setdefault(v, []).append(i)
    return list(seen.items())


def _take(x, idx, B):
    return x if len(idx) == B else x.index_select(0, torch.as_tensor(idx, device=x.device))


# ---------------------------------------------------------------------------------------------------------------- tuning
def _pip_kwargs(kwargs, who):
    k = dict(kwargs)
    fmin, fmax, threshold = k.pop("fmin", 150.0), k.pop("fmax", 4000.0), k.pop("threshold", 0.1)
    hop, win_length, window = k.pop("hop_length", None), k.pop("win_length", None), k.pop("window", "hann")
    center, pad_mode, ref = k.pop("center", True), k.pop("pad_mode", "constant"), k.pop("ref", None)
    if k:
        raise ValueError(f"{who}: unknown arguments {sorted(k)} (served: fmin, fmax, threshold, hop_length, win_length, window, "
                         "center, pad_mode)")
    CH.check_pip(threshold, ref, who)
    CH.check_pad_mode(pad_mode, who)
    return fmin, fmax, threshold, hop, win_length, window, center


def estimate_tuning_batch(y=None, sr: float = 22050, S=None, n_fft: Optional[int] = 2048, resolution: float = 0.01,
                          bins_per_octave: int = 12, **kwargs) -> np.ndarray:
    """librosa.estimate_tuning of every clip -> float64 [B] NumPy array (fractions of a bin in [-0.5, 0.5)).  S [B, F, T]: a
    magnitude spectrogram (any non-negative spectrogram is taken as it is).  kwargs: piptrack's."""
    who = "estimate_tuning"
    fmin, fmax, threshold, hop, win_length, window, center = _pip_kwargs(kwargs, who)
    CH.check_resolution(resolution, who)
    n_fft, hop = _check_stft(2048 if n_fft is None else n_fft, hop, win_length, "constant", who)
    CH.pip_bins(sr, n_fft, fmin, fmax)
    X, n_fft = _spectrogram(y, S, n_fft, hop, win_length, window, center, who)
    return ops.estimate_tuning(X, sr, n_fft, 1, resolution, bins_per_octave, fmin, fmax, threshold)


def piptrack_batch(y=None, sr: float = 22050, S=None, n_fft: Optional[int] = 2048, hop_length: Optional[int] = None,
                   fmin: float = 150.0, fmax: float = 4000.0, threshold: float = 0.1, win_length: Optional[int] = None,
                   window="hann", center: bool = True, pad_mode: str = "constant", ref=None):
    """librosa.piptrack of every clip -> (pitches, magnitudes), float32 device tensors [B, F, T] (views of the kernel's
    frame-major result)."""
    who = "piptrack"
    CH.check_pip(threshold, ref, who)
    n_fft, hop = _check_stft(2048 if n_fft is None else n_fft, hop_length, win_length, pad_mode, who)
    CH.pip_bins(sr, n_fft, fmin, fmax)
    X, n_fft = _spectrogram(y, S, n_fft, hop, win_length, window, center, who)
    p, m = ops.piptrack(X, sr, n_fft, 1, fmin, fmax, threshold)
    return p.transpose(1, 2), m.transpose(1, 2)


# ---------------------------------------------------------------------------------------------------------------- chroma
def _filter_kwargs(kwargs, who):
    k = dict(kwargs)
    f = {"ctroct": k.pop("ctroct", 5.0), "octwidth": k.pop("octwidth", 2), "base_c": k.pop("base_c", True)}
    if k:
        raise ValueError(f"{who}: unknown arguments {sorted(k)} (served: ctroct, octwidth, base_c)")
    return f


def _filterbank_dev(sr, n_fft, n_chroma, tuning, f):
    key = ("chroma_fb", float(sr), n_fft, n_chroma, float(tuning), float(f["ctroct"]),
           None if f["octwidth"] is None else float(f["octwidth"]), bool(f["base_c"]))
    return ops._cached(key, lambda: ops.ChromaTable(CH.chroma_filterbank(sr, n_fft, n_chroma, tuning, **f)), limit=32)


def chroma_stft_batch(y=None, sr: float = 22050, S=None, norm=np.inf, n_fft: int = 2048, hop_length: int = 512,
                      win_length: Optional[int] = None, window="hann", center: bool = True, pad_mode: str = "constant",
                      tuning=None, n_chroma: int = 12, out=None, return_tuning: bool = False, **kwargs):
    """librosa.feature.chroma_stft of every clip -> float32 [B, n_chroma, T] device tensor: the complex STFT (the 2048 kernel
    or stft_any), then one fold that takes |X|^2 on load, the filter bank, and the norm (`syg_chroma_fold_rows_f32`).
    S [B, F, T]: a power spectrogram.  kwargs: ctroct, octwidth, base_c of librosa.filters.chroma.  return_tuning: (chroma,
    the tuning used per clip, float64 [B] on the host)."""
    who = "chroma_stft"
    nc = CH.check_n_chroma(n_chroma, who)
    CH.check_norm(norm, who)
    f = _filter_kwargs(kwargs, who)
    n_fft, hop = _check_stft(n_fft, hop_length, win_length, pad_mode, who)
    if tuning is not None:
        tuning = CH.check_tuning(tuning, who)
    X, n_fft = _spectrogram(y, S, n_fft, hop, win_length, window, center, who)
    B = int(X.shape[0])
    if tuning is None:
        tun = ops.estimate_tuning(X, sr, n_fft, 2, bins_per_octave=nc)          # librosa: on the power spectrogram
    else:
        tun = np.full(B, tuning)
    groups = _groups(tun)
    if len(groups) == 1:
        res = ops.chroma_fold(X, _filterbank_dev(sr, n_fft, nc, groups[0][0], f), "rows", 2, None, norm, out=out)
        return (res, tun) if return_tuning else res
    res = ops._out(out, (B, nc, int(X.shape[1])), X, f"{who}: out", contiguous=True)
    for value, idx in groups:
        res[idx] = ops.chroma_fold(_take(X, idx, B), _filterbank_dev(sr, n_fft, nc, value, f), "rows", 2, None, norm)
    return (res, tun) if return_tuning else res


def _cqt_input(C, who):
    """C [B, K, T] real, or complex [B, K, T, 2] as ops.cqt leaves it (NumPy complex arrays are interleaved), on the device."""
    if hasattr(C, "is_cuda"):
        if C.dim() == 4 and C.shape[-1] == 2:
            return C if (C.is_cuda and C.dtype == torch.float32) else C.to(device=ops.require_gpu(), dtype=torch.float32)
        return _dev_real(C, 3, who, "C")
    a = np.asarray(C)
    if np.iscomplexobj(a):
        if a.ndim != 3 or a.size == 0:
            raise ValueError(f"{who}: C must be [B, K, T]")
        return torch.from_numpy(np.stack([a.real, a.imag], axis=-1).astype(np.float32)).to(ops.require_gpu())
    return _dev_real(a, 3, who, "C")


def _phi_dev(nc):
    return ops._cached(("tonnetz_phi", nc), lambda: ops._dev(CH.tonnetz_phi(nc)))


def _chroma_cqt(who, y, sr, C, hop_length, fmin, norm, threshold, tuning, n_chroma, n_octaves, window, bins_per_octave, cqt_mode,
                transform=None, out=None, return_tuning=False):
    """transform: None, or a function n_chroma -> the device table of the output transform (asked for after the checks).
    return_tuning: (result, the tuning used per clip, float64 [B] on the host); from audio only."""
    nc = CH.check_n_chroma(n_chroma, who)
    CH.check_norm(norm, who)
    CH.check_threshold(threshold, who)
    CH.check_cqt_mode(cqt_mode, who)
    bpo = CH.check_merge(nc if bins_per_octave is None else bins_per_octave, nc, who)
    if not (isinstance(n_octaves, (int, np.integer)) and n_octaves >= 1):
        raise ValueError(f"{who}: n_octaves must be a positive integer")
    if not (isinstance(hop_length, (int, np.integer)) and hop_length >= 1):
        raise ValueError(f"{who}: hop_length must be a positive integer")
    if tuning is not None:
        tuning = CH.check_tuning(tuning, who)

    def table(K):
        wkey = None if window is None else np.asarray(window, dtype=np.float64).tobytes()
        key = ("cq2chroma", K, bpo, nc, None if fmin is None else float(fmin), wkey)
        return ops._cached(key, lambda: ops.ChromaTable(CH.cq_to_chroma(K, bpo, nc, fmin, window)), limit=32)

    if C is None and y is None:
        raise ValueError(f"{who}: either the audio y or C must be given")
    if C is not None and return_tuning:
        raise ValueError(f"{who}: return_tuning needs the audio y: a given C was made with a tuning of the caller's")
    if C is not None:
        Cd = _cqt_input(C, who)
        transform = transform(nc) if transform else None
        return ops.chroma_fold(Cd, table(int(Cd.shape[1])), "bins", 1, threshold, norm, transform, out=out)
    y = _as_clips(y)
    transform = transform(nc) if transform else None
    B = int(y.shape[0])
    K = int(n_octaves) * bpo
    if tuning is None:
        tun = ops.estimate_tuning(ops.stft2048_c2c(y), sr, 2048, 1, bins_per_octave=bpo)      # librosa: on |STFT|, n_fft 2048
    else:
        tun = np.full(B, tuning)
    groups = _groups(tun)
    if len(groups) == 1:
        Cd = ops.cqt(y, sr, int(hop_length), fmin, K, bpo, groups[0][0])
        res = ops.chroma_fold(Cd, table(K), "bins", 1, threshold, norm, transform, out=out)
        return (res, tun) if return_tuning else res
    res = None
    for value, idx in groups:
        Cd = ops.cqt(_take(y, idx, B), sr, int(hop_length), fmin, K, bpo, value)
        part = ops.chroma_fold(Cd, table(K), "bins", 1, threshold, norm, transform)
        if res is None:
            res = ops._out(out, (B,) + tuple(part.shape[1:]), part, f"{who}: out", contiguous=True)
        res[idx] = part
    return (res, tun) if return_tuning else res


def chroma_cqt_batch(y=None, sr: float = 22050, C=None, hop_length: int = 512, fmin=None, norm=np.inf, threshold=0.0,
                     tuning=None, n_chroma: int = 12, n_octaves: int = 7, window=None, bins_per_octave: Optional[int] = 36,
                     cqt_mode: str = "full", out=None, return_tuning: bool = False):
    """librosa.feature.chroma_cqt of every clip -> float32 [B, n_chroma, T] device tensor: the device CQT, then one fold that
    takes |C| on load, the merge table, the threshold and the norm (`syg_chroma_fold_bins_f32`).  C [B, K, T]: a CQT
    magnitude (or the complex [B, K, T, 2] that ops.cqt returns)."""
    return _chroma_cqt("chroma_cqt", y, sr, C, hop_length, fmin, norm, threshold, tuning, n_chroma, n_octaves, window,
                       bins_per_octave, cqt_mode, out=out, return_tuning=return_tuning)


def chroma_cens_batch(y=None, sr: float = 22050, C=None, hop_length: int = 512, fmin=None, tuning=None, n_chroma: int = 12,
                      n_octaves: int = 7, bins_per_octave: Optional[int] = 36, cqt_mode: str = "full", window=None, norm=2,
                      win_len_smooth: Optional[int] = 41, smoothing_window="hann", out=None, return_tuning: bool = False):
    """librosa.feature.chroma_cens of every clip -> float32 [B, n_chroma, T] device tensor: chroma_cqt without a norm, then
    `syg_chroma_cens_f32` (L1, quantiser, smoothing, closing norm)."""
    who = "chroma_cens"
    CH.check_norm(norm, who)
    CH.check_win_len_smooth(win_len_smooth, who)
    ch = _chroma_cqt(who, y, sr, C, hop_length, fmin, None, 0.0, tuning, n_chroma, n_octaves, window, bins_per_octave, cqt_mode,
                     return_tuning=return_tuning)
    ch, tun = ch if return_tuning else (ch, None)
    res = ops.chroma_cens(ch, win_len_smooth, smoothing_window, norm, out=out)
    return (res, tun) if return_tuning else res


def tonnetz_batch(y=None, sr: float = 22050, chroma=None, out=None, return_tuning: bool = False, **kwargs):
    """librosa.feature.tonnetz of every clip -> float32 [B, 6, T] device tensor.  chroma [B, n_chroma, T] given: one launch
    (the identity fold with the transform); else chroma_cqt(y, sr, **kwargs) with the transform in the fold's own launch."""
    who = "tonnetz"
    if chroma is not None:
        if kwargs or return_tuning:
            raise ValueError(f"{who}: chroma= is given, so {sorted(kwargs) + ['return_tuning'] * bool(return_tuning)} would be ignored")
        ch = _dev_real(chroma, 3, who, "chroma")
        nc = CH.check_n_chroma(int(ch.shape[1]), who)
        eye = ops._cached(("chroma_eye", nc), lambda: ops.ChromaTable(np.eye(nc, dtype=np.float32)))
        return ops.chroma_fold(ch, eye, "bins", 1, None, None, _phi_dev(nc), out=out)
    if y is None:
        raise ValueError(f"{who}: either the audio y or chroma must be given")
    names = ("C", "hop_length", "fmin", "norm", "threshold", "tuning", "n_chroma", "n_octaves", "window", "bins_per_octave", "cqt_mode")
    bad = sorted(set(kwargs) - set(names))
    if bad:
        raise ValueError(f"{who}: unknown arguments {bad} (served: chroma_cqt's {', '.join(names)})")
    a = {"C": None, "hop_length": 512, "fmin": None, "norm": np.inf, "threshold": 0.0, "tuning": None, "n_chroma": 12, "n_octaves": 7,
         "window": None, "bins_per_octave": 36, "cqt_mode": "full"}
    a.update(kwargs)
    return _chroma_cqt(who, y, sr, a["C"], a["hop_length"], a["fmin"], a["norm"], a["threshold"], a["tuning"], a["n_chroma"],
                       a["n_octaves"], a["window"], a["bins_per_octave"], a["cqt_mode"], transform=_phi_dev, out=out,
                       return_tuning=return_tuning)


# ---------------------------------------------------------------------------------------------------------- single clips
def _one(a, dims, who, what):
    if a is None:
        return None
    if hasattr(a, "is_cuda"):
        if a.dim() != dims:
            raise ValueError(f"{who}: {what} must have {dims} dimension(s)")
        return a[None]
    a = np.asarray(a)
    if a.ndim != dims:
        raise ValueError(f"{who}: {what} must have {dims} dimension(s) (got {a.ndim})")
    return a[None]


def chroma_stft(y=None, sr: float = 22050, S=None, norm=np.inf, n_fft: int = 2048, hop_length: int = 512,
                win_length: Optional[int] = None, window="hann", center: bool = True, pad_mode: str = "constant", tuning=None,
                n_chroma: int = 12, **kwargs) -> np.ndarray:
    """librosa.feature.chroma_stft of one clip -> float32 [n_chroma, T]."""
    return chroma_stft_batch(_one(y, 1, "chroma_stft", "y"), sr, _one(S, 2, "chroma_stft", "S"), norm, n_fft, hop_length, win_length,
                             window, center, pad_mode, tuning, n_chroma, **kwargs)[0].cpu().numpy()


def chroma_cqt(y=None, sr: float = 22050, C=None, hop_length: int = 512, fmin=None, norm=np.inf, threshold=0.0, tuning=None,
               n_chroma: int = 12, n_octaves: int = 7, window=None, bins_per_octave: Optional[int] = 36,
               cqt_mode: str = "full") -> np.ndarray:
    """librosa.feature.chroma_cqt of one clip -> float32 [n_chroma, T]."""
    return chroma_cqt_batch(_one(y, 1, "chroma_cqt", "y"), sr, _one(C, 2, "chroma_cqt", "C"), hop_length, fmin, norm, threshold, tuning,
                            n_chroma, n_octaves, window, bins_per_octave, cqt_mode)[0].cpu().numpy()


def chroma_cens(y=None, sr: float = 22050, C=None, hop_length: int = 512, fmin=None, tuning=None, n_chroma: int = 12,
                n_octaves: int = 7, bins_per_octave: Optional[int] = 36, cqt_mode: str = "full", window=None, norm=2,
                win_len_smooth: Optional[int] = 41, smoothing_window="hann") -> np.ndarray:
    """librosa.feature.chroma_cens of one clip -> float32 [n_chroma, T]."""
    return chroma_cens_batch(_one(y, 1, "chroma_cens", "y"), sr, _one(C, 2, "chroma_cens", "C"), hop_length, fmin, tuning, n_chroma,
                             n_octaves, bins_per_octave, cqt_mode, window, norm, win_len_smooth, smoothing_window)[0].cpu().numpy()


def tonnetz(y=None, sr: float = 22050, chroma=None, **kwargs) -> np.ndarray:
    """librosa.feature.tonnetz of one clip -> float32 [6, T]."""
    if "C" in kwargs:
        kwargs["C"] = _one(kwargs["C"], 2, "tonnetz", "C")
    return tonnetz_batch(_one(y, 1, "tonnetz", "y"), sr, _one(chroma, 2, "tonnetz", "chroma"), **kwargs)[0].cpu().numpy()


def estimate_tuning(y=None, sr: float = 22050, S=None, n_fft: Optional[int] = 2048, resolution: float = 0.01,
                    bins_per_octave: int = 12, **kwargs) -> float:
    """librosa.estimate_tuning of one clip -> float (fractions of a bin)."""
    return float(estimate_tuning_batch(_one(y, 1, "estimate_tuning", "y"), sr, _one(S, 2, "estimate_tuning", "S"), n_fft, resolution,
                                       bins_per_octave, **kwargs)[0])


def piptrack(y=None, sr: float = 22050, S=None, n_fft: Optional[int] = 2048, hop_length: Optional[int] = None, fmin: float = 150.0,
             fmax: float = 4000.0, threshold: float = 0.1, win_length: Optional[int] = None, window="hann", center: bool = True,
             pad_mode: str = "constant", ref=None):
    """librosa.piptrack of one clip -> (pitches, magnitudes), float32 [F, T]."""
    p, m = piptrack_batch(_one(y, 1, "piptrack", "y"), sr, _one(S, 2, "piptrack", "S"), n_fft, hop_length, fmin, fmax, threshold,
                          win_length, window, center, pad_mode, ref)
    return p[0].cpu().numpy(), m[0].cpu().numpy()
