"""Batched device operators: thin Python over the C ABI.

torch is used only as the device-array container (allocation, H2D/D2H, streams); every
arithmetic step runs in libsygnals_hip.so.  All functions take/return CUDA(ROCm) float32
tensors with a leading batch axis; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from . import _cepstrum as CP
from . import _chroma as CH
from . import _cwt as CW
from . import _dynamics as DY
from . import _kaldi as KD
from . import _laplace as LP
from . import _loudness as LD
from . import _lpc
from . import _pcen as PC
from . import _resample as RS
from . import _rhythm as RH
from . import _rng as RNG
from . import _sequence as SQ
from . import _specaug as SA
from . import _structure as ST
from . import _tables as T
from ._fftplan import (MAX_LDS_FFT, MAX_MIXED_FFT, MAX_ROWS, conv_fft_len, fft_plan, is_pow2,      # noqa: F401 (re-exported)
                       next_direct_len, smooth_split)
from ._front import front_route, pow2_takes, stats2048_takes
from ._lib import SygnalsHipError, check, lib


# ------------------------------------------------------------------ device plumbing
def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise SygnalsHipError("sygnals_amd needs an AMD GPU (torch.cuda.is_available() is False); "
                              "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _call(name: str, *args) -> None:
    """The entry `name` of the library on the current stream (its last argument); a non-zero status raises under that
    name.  (`lib` is looked up here, at call time: tests replace it with a spy.)"""
    check(getattr(lib(), name)(*args, C.c_void_p(_stream_ptr())), name)


def _ld(t: torch.Tensor) -> int:
    """Row stride in elements (a size-1 leading axis may carry an arbitrary stride)."""
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def to_device_f32(x, device=None) -> torch.Tensor:
    """Host array / tensor -> contiguous float32 device tensor (2-D: [B, L])."""
    device = device or require_gpu()
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).to(device)
    return t.contiguous()


_dev_cache: dict = {}          # (device, family, ...) -> table; a limited family's entries stand least recently used first


def _cached(key, builder, limit: Optional[int] = None):
    """The device table of `key` (family name first) on the current device, built on first use.  limit: the most entries
    the family keeps (over all devices), the least recently used one going first; None: unbounded."""
    k = (torch.cuda.current_device(),) + key
    v = _dev_cache.get(k)
    if v is None:
        v = builder()
        _dev_cache[k] = v
        if limit:
            held = [q for q in _dev_cache if q[1] == key[0]]
            if len(held) > limit:
                del _dev_cache[held[0]]
    elif limit:
        _dev_cache[k] = _dev_cache.pop(k)
    return v


def clear_caches() -> None:
    """Drops everything this module keeps on a device: the tables, the prepared MFCC calls and the side streams."""
    _dev_cache.clear()
    _mfcc_calls.clear()
    _side_streams.clear()


def _dev(arr: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(arr)).to(require_gpu())


def _f32(x, what: str, dims: int, tail: tuple = (), axes: Optional[str] = None) -> None:
    """First stage of the input check, judged without a device: x is a float32 tensor of `dims` dimensions whose last
    sizes are `tail`.  axes: the shape as the message names it (default: * for a free size)."""
    if not isinstance(x, torch.Tensor) or x.dim() != dims or x.dtype != torch.float32 or \
            (tail and tuple(x.shape[-len(tail):]) != tuple(tail)):
        axes = axes or "[" + ", ".join(["*"] * (dims - len(tail)) + [str(n) for n in tail]) + "]"
        raise ValueError(f"{what} must be a float32 tensor {axes}")


def _on_device(x: torch.Tensor, what: str) -> None:
    """Second stage: there is a device and x is on it."""
    require_gpu()
    if not x.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor")


def _unit_stride(x: torch.Tensor) -> torch.Tensor:
    """x with unit stride along its last axis (a copy if it has another)."""
    return x if (x.stride(-1) == 1 or x.shape[-1] == 1) else x.contiguous()


def _f32_in(x, what: str, dims: int, tail: tuple = (), axes: Optional[str] = None) -> torch.Tensor:
    """The input check, both stages: a float32 device tensor of `dims` dimensions, returned with unit stride along its last
    axis."""
    _f32(x, what, dims, tail, axes)
    _on_device(x, what)
    return _unit_stride(x)


def _out(out, shape, x: torch.Tensor, what: str = "out", dtype=torch.float32, contiguous: bool = False) -> torch.Tensor:
    """A new tensor of this shape and dtype on x's device, or `out` checked: contiguous, or unit stride along its last
    axis only."""
    shape = tuple(shape)
    if out is None:
        return torch.empty(shape, dtype=dtype, device=x.device)
    ok = isinstance(out, torch.Tensor) and tuple(out.shape) == shape and out.dtype == dtype and out.device == x.device
    if not (ok and (out.is_contiguous() if contiguous else (shape[-1] <= 1 or out.stride(-1) == 1))):
        raise ValueError(f"{what} must be a {str(dtype)[6:]} tensor {list(shape)} on the input's device, "
                         + ("contiguous" if contiguous else "with unit stride along its last axis"))
    return out


# sizing entries whose refusal (a negative size) leaves no message in syg_last_error
_SILENT_SIZERS = frozenset(("syg_pack_rows_work_bytes", "syg_welch_work_bytes", "syg_csd_work_bytes",
                            "syg_onset_strength_work_bytes", "syg_dwt_work_bytes", "syg_dynamics_work_bytes",
                            "syg_spec_augment_work_bytes", "syg_tempogram_work_bytes", "syg_tempo_pick_work_bytes",
                            "syg_beat_local_score_work_bytes", "syg_tuning_hist_work_bytes", "syg_viterbi_work_bytes"))


def _work_bytes(entry: str, *args, error: Optional[Exception] = None) -> int:
    """The bytes the sizing entry asks for at these arguments; a negative answer raises `error`, or SygnalsHipError with
    the library's message (the entry and its arguments where it leaves none)."""
    n = int(getattr(lib(), entry)(*args))
    if n < 0:
        if error is not None:
            raise error
        if entry in _SILENT_SIZERS:
            raise SygnalsHipError(f"{entry}({', '.join(str(a) for a in args)}) refuses these arguments")
        check(-1, entry)
    return n


def _workspace(entry: str, *args, dtype, device, error: Optional[Exception] = None) -> Optional[torch.Tensor]:
    """The workspace of _work_bytes(entry, *args): None for 0 bytes, else a buffer of `dtype` of at least that size."""
    n = _work_bytes(entry, *args, error=error)
    return torch.empty(-(-n // dtype.itemsize), dtype=dtype, device=device) if n else None


def _nbytes(work: Optional[torch.Tensor]) -> int:
    return 0 if work is None else work.numel() * work.element_size()


def _constants(entry: str, names) -> dict:
    """The library's figures by name, read now: names[i] -> entry(i) of an indexed entry; a dict name -> suffix names the
    per-figure entries entry_suffix()."""
    h = lib()
    if isinstance(names, dict):
        return {name: int(getattr(h, f"{entry}_{suffix}")()) for name, suffix in names.items()}
    fn = getattr(h, entry)
    return {name: int(fn(i)) for i, name in enumerate(names)}


_LAUNCH_KEYS = ("max_grid_y", "lpc_frames_wgs_per_cu", "lpc_envelope_wgs_per_cu", "pitch_frames_wgs_per_cu",
                "noise_wgs_per_cu")                                                                  # SYG_LAUNCH_*


def launch_constants() -> dict:
    """The launch caps of the library (it owns them): rows of a grid's y dimension (MAX_ROWS restates it) and the workgroups
    a CU of the persistent grids of the LPC frame and envelope kernels, the pitch frame kernel and the noise mixes."""
    return _constants("syg_launch_constants", _LAUNCH_KEYS)


def _row_blocks(n: int):
    """(first row, row count) of the launches that take n rows MAX_ROWS (the grid's 65535) at a time."""
    for lo in range(0, n, MAX_ROWS):
        yield lo, min(MAX_ROWS, n - lo)


def _window_key(window, win_length, n_fft):
    if isinstance(window, (np.ndarray, list)):
        a = np.asarray(window, dtype=np.float64)
        return ("arr", a.tobytes(), win_length, n_fft)
    return (window, win_length, n_fft)


def window_dev(window, win_length, n_fft) -> torch.Tensor:
    return _cached(("win",) + _window_key(window, win_length, n_fft),
                   lambda: _dev(T.analysis_window(window, win_length, n_fft).astype(np.float32)))


def twiddle_dev(n) -> torch.Tensor:
    return _cached(("tw", n), lambda: _dev(T.twiddles(n)))


def dct_dev(K, M, dct_type=2, norm="ortho") -> torch.Tensor:
    return _cached(("dct", K, M, dct_type, norm), lambda: _dev(T.dct_matrix(K, M, dct_type, norm)))


def num_frames(L: int, n_fft: int, hop: int, center: bool) -> int:
    """Frame-count rule of sygnals/core/features/manager.py:149-157 (frames_expected of csrc/host.h)."""
    if center:
        return 1 + L // hop
    return 1 + (L - n_fft) // hop if L >= n_fft else 0


def num_frames_padded(L: int, frame: int, hop: int, center: bool) -> int:
    """librosa's count on the signal padded by frame // 2 on both sides (frames_padded of csrc/host.h): num_frames() for
    an even frame length, one less for an odd one when hop divides L (the padding is one sample short of the frame)."""
    if center:
        return 1 + (L + 2 * (frame // 2) - frame) // hop
    return 1 + (L - frame) // hop if L >= frame else 0


# ------------------------------------------------------------------ fused 2048 path
class _Settings:
    """Process-wide switches between kernels that the tests hold to the same results (plain attributes: nothing is read
    from the environment; tests and tools set them with `ops.override(...)`):
      waves                 16 (one workgroup per CU) | 8: waves per workgroup of the matrix-form fused 2048 kernels
      cqt_mode              "bf16x3" (default) | "gemm" | "fft": octave kernel of compute_cqt
      cqt_streams           1 | 2: octave products on a side stream (measured: no gain)
      cqt_chain             True: up to three decimation levels per pass; False: one launch per level
      cqt_fused             True: the one-launch form (syg_cqt_fused_f32) where the plan has its shape; False: level by level
      one_launch_features   True: extract_features routes MFCC + statistics / contrast requests to the one-launch kernels
    Options that live in the library (syg_set_option): reserved_cus, stft_load, sos_clip, cqt_staged, dwt_form,
    fx_delay_form, stft_freerun, stft_meet."""
    waves = T.WAVES
    cqt_mode = "bf16x3"
    cqt_streams = 1
    cqt_chain = True
    cqt_fused = True
    one_launch_features = True


settings = _Settings()
_LIB_OPTIONS = {"reserved_cus": 0, "stft_load": 1, "sos_clip": 2, "cqt_staged": 3, "dwt_form": 4, "fx_delay_form": 5,
                "stft_freerun": 6, "stft_meet": 7}      # SYG_OPT_* of include/sygnals_hip.h


def set_option(name: str, value: int) -> None:
    """syg_set_option by name (reserved_cus | stft_load | sos_clip | cqt_staged | dwt_form | fx_delay_form | stft_freerun | stft_meet)."""
    check(lib().syg_set_option(_LIB_OPTIONS[name], int(value)), "syg_set_option")


def get_option(name: str) -> int:
    return int(lib().syg_get_option(_LIB_OPTIONS[name]))


def set_reserved_cus(n: int) -> None:
    """Leave `n` CUs out of the persistent grids of the fused 2048 kernels (room for a collective's workgroups)."""
    set_option("reserved_cus", n)


class override:
    """Context manager: `with ops.override(cqt_mode="fft", cqt_staged=0): ...` sets Python-side settings and library
    options for the block and puts the previous values back."""

    def __init__(self, **kw):
        self.kw = kw
        self.old = {}

    def __enter__(self):
        for k, v in self.kw.items():
            if k in _LIB_OPTIONS:
                self.old[k] = get_option(k)
                set_option(k, v)
            else:
                if not hasattr(_Settings, k):
                    raise KeyError(k)
                self.old[k] = getattr(settings, k)
                setattr(settings, k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if k in _LIB_OPTIONS:
                set_option(k, v)
            else:
                setattr(settings, k, v)
        return False


def fused_waves() -> int:
    """Waves per workgroup of the fused kernel: 8 (two workgroups per CU) or 16 (one)."""
    return int(settings.waves)


class MelConfig:
    """Device tables for one (sr, n_fft, n_mels, fmin, fmax) mel front end."""

    def __init__(self, sr, n_fft, n_mels, fmin, fmax, waves=None):
        basis = T.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
        self.basis_host = basis
        self.n_mels = n_mels
        waves = fused_waves() if waves is None else waves
        self.wpacked = None
        self.plan = None
        if n_fft == 2048 and n_mels <= 256:
            try:
                wp, plan = T.pack_mel_plan(basis, waves)
            except ValueError:
                pass        # more groups of four rows than the plan has slots (8-wave mode, n_mels > 128): dense path
            else:
                self.wpacked = _dev(wp)
                self.plan = np.ascontiguousarray(plan, dtype=np.int32)
        self.basis = _dev(basis)
        # piece table of the per-wave projection by segment sums (MODE 6 of the fused kernel): triangular filterbanks
        # whose pieces fit 128 lane slots (n_mels = 40 at any usual rate; 64 and more do not)
        self.segtab = None
        # ... and the four-pass table of the tile form (MODE 8 / 9: up to 256 pieces -- the reference's default of 128
        # bands, 64 ... 128 bands at the usual rates; row_base 4: a short first piece needs room for its lead)
        self.segtab4 = None
        if n_fft == 2048:
            try:
                self.segtab = _dev(T.pack_mel_segments(sr, n_fft, n_mels, fmin, fmax, basis=basis).reshape(-1))
            except ValueError:
                pass
            if n_mels <= 255:
                try:
                    self.segtab4 = _dev(T.pack_mel_segments(sr, n_fft, n_mels, fmin, fmax, basis=basis, n_pass=4,
                                                            row_base=4).reshape(-1))
                except ValueError:
                    pass


def mel_config(sr, n_fft, n_mels, fmin=0.0, fmax=None, waves=None) -> MelConfig:
    fmax = sr / 2.0 if fmax is None else fmax
    waves = fused_waves() if waves is None else waves
    return _cached(("mel", float(sr), n_fft, n_mels, float(fmin), float(fmax), waves),
                   lambda: MelConfig(sr, n_fft, n_mels, fmin, fmax, waves))


def fused_mel_ok(sr, n_fft, n_mels, fmin=0.0, fmax=None) -> bool:
    """True when the fused frame-length-2048 kernel has a block-sparse plan or a four-pass piece table for this filterbank
    (n_mels <= 256, and <= 128 in the 8-wave development mode); otherwise callers take the generic chain
    (stft_any -> mel_dense)."""
    if n_fft != 2048 or not 1 <= n_mels <= 256:
        return False
    cfg = mel_config(sr, n_fft, n_mels, fmin, fmax)
    return cfg.wpacked is not None or cfg.segtab4 is not None


def fused_pow2_ok(n_fft, n_mels) -> bool:
    """True when the fused kernel for the other power-of-two frame lengths (stft_mel_pow2.hip) takes this shape."""
    return pow2_takes(n_fft, n_mels)


def _basis_padded(cfg: "MelConfig", n_fft: int):
    """[16 ceil(M / 16), Fp] zero-padded dense filterbank (Fp = F rounded up to a multiple of 16) on the device."""
    if getattr(cfg, "basis_padded", None) is None:
        M, F = cfg.basis_host.shape
        Mp, Fp = -(-M // 16) * 16, -(-F // 16) * 16
        bp = np.zeros((Mp, Fp), np.float32)
        bp[:M, :F] = cfg.basis_host
        cfg.basis_padded, cfg.Fp = _dev(bp), Fp
    return cfg.basis_padded, cfg.Fp


def _at_least_one(Tn: int) -> int:
    if Tn <= 0:
        raise ValueError("signal too short for one frame")
    return Tn


def _frames(L: int, n_fft: int, hop: int, center: bool) -> int:
    """num_frames, or ValueError when the clip holds no frame."""
    return _at_least_one(num_frames(L, n_fft, hop, center))


def _rows_out(B, Tn, want_stats, contrast, device, who=None):
    """Outputs of the statistics / contrast rows of a fused kernel: (smask, stats [B, 8, Tn] | None, contrast_pv
    [B, 2, R, Tn] | None, cplan pointer | None -- it keeps the plan array alive).  want_stats: False, True (all rows) or a
    bit mask; `who`: the rows are what the call is for, so asking for none is an error."""
    smask = 31 if want_stats is True else int(want_stats or 0)
    if who and not smask and contrast is None:
        raise ValueError(f"{who}: no statistics requested (want_stats and contrast are both empty)")
    stats = torch.zeros((B, 8, Tn), dtype=torch.float32, device=device) if smask else None
    cpv = cplan_p = None
    if contrast is not None:
        cplan = np.ascontiguousarray(contrast, dtype=np.int32)
        cpv = torch.empty((B, 2, int(cplan[0]), Tn), dtype=torch.float32, device=device)
        cplan_p = cplan.ctypes.data_as(C.c_void_p)
    return smask, stats, cpv, cplan_p


def _pow2_front(y, sr, n_fft, hop, center, window, win_length, n_mels, fmin, fmax):
    y = _f32_in(y, "y", 2)
    if not fused_pow2_ok(n_fft, n_mels):
        raise SygnalsHipError(f"no fused kernel for n_fft={n_fft}, n_mels={n_mels} (powers of two 64 ... 1024; 2048: stft2048_mel)")
    B, L = y.shape
    Tn = _frames(L, n_fft, hop, center)
    cfg = mel_config(sr, n_fft, n_mels, fmin, fmax)
    bp, Fp = _basis_padded(cfg, n_fft)
    win = window_dev(window, n_fft if win_length is None else win_length, n_fft)
    # (n_fft 512 / 256: the twiddle block is followed by W_1024^k -- four / eight frames share one 1024-point wave transform)
    tw = twiddle_rfft_dev(n_fft) if n_fft not in (256, 512) else _cached(("twr+1024", n_fft), lambda: _dev(np.concatenate(
        [T.twiddles(n_fft), T.twiddles(n_fft // 2), T.twiddles(1024)], axis=0)))
    return y, B, L, Tn, bp, Fp, win, tw


def stft_mel_pow2(y: torch.Tensor, sr: float, n_fft: int, hop: int, center: bool = True, window="hann", win_length=None,
                  n_mels: int = 128, fmin: float = 0.0, fmax=None, power: int = 2) -> torch.Tensor:
    """Fused STFT(n_fft = 64 ... 1024) -> |X|^power -> mel [B, n_mels, T]: one launch, no spectrogram in HBM."""
    y, B, L, Tn, bp, Fp, win, tw = _pow2_front(y, sr, n_fft, hop, center, window, win_length, n_mels, fmin, fmax)
    mel = torch.empty((B, n_mels, Tn), dtype=torch.float32, device=y.device)
    _call("syg_stft_mel_pow2_f32", _ptr(y), B, L, _ld(y), n_fft, hop, int(center), Tn, _ptr(win), _ptr(tw), _ptr(bp),
          Fp, n_mels, int(power), _ptr(mel))
    return mel


def mfcc_pow2_fits(n_fft, n_mels, n_frames, n_mfcc) -> bool:
    return bool(lib().syg_stft_mfcc_pow2_fits(int(n_fft), int(n_mels), int(n_frames), int(n_mfcc)))


def stft_mfcc_pow2(y: torch.Tensor, sr: float, n_fft: int, hop: int, center: bool = True, window="hann", win_length=None,
                   n_mels: int = 128, n_mfcc: int = 13, fmin: float = 0.0, fmax=None, lifter: float = 0.0,
                   amin: float = 1e-10, top_db: Optional[float] = 80.0, keep_mel: bool = False):
    """One launch for the other power-of-two frame lengths: [B, L] clips -> MFCC [B, n_mfcc, T] (a workgroup owns a
    clip; its mel matrix stays in LDS).  Returns (mfcc, mel_power | None)."""
    y, B, L, Tn, bp, Fp, win, tw = _pow2_front(y, sr, n_fft, hop, center, window, win_length, n_mels, fmin, fmax)
    if not mfcc_pow2_fits(n_fft, n_mels, Tn, n_mfcc):
        raise SygnalsHipError("stft_mfcc_pow2: the clip's mel matrix does not fit the LDS; use stft_mel_pow2 + logmel_dct")
    dct = dct_dev(n_mfcc, n_mels)
    lw = T.lifter_weights(n_mfcc, lifter)
    lif = None if lw is None else _dev(lw)
    mf = torch.empty((B, n_mfcc, Tn), dtype=torch.float32, device=y.device)
    mel = torch.empty((B, n_mels, Tn), dtype=torch.float32, device=y.device) if keep_mel else None
    _call("syg_stft_mfcc_pow2_f32", _ptr(y), B, L, _ld(y), n_fft, hop, int(center), Tn, _ptr(win), _ptr(tw), _ptr(bp),
          Fp, n_mels, _ptr(dct), n_mfcc, None if lif is None else _ptr(lif), float(amin),
          -1.0 if top_db is None else float(top_db), 1, 1.0, None if mel is None else _ptr(mel), _ptr(mf))
    return mf, mel


# ---- the segment-sum kernels of the other frame lengths (stft_mel_w1024_seg.hip, stft_mel_w4096.hip, stft_mel_wseg_small.hip):
# frame length -> entry points (mel alone / with rows), length of the twiddle table, packer of the piece table and its
# arguments, largest n_mels; small: the entry points take n_fft and the rows form projects nothing.  The public wrappers
# below carry the entry points' names without syg_ / _f32 (error messages use them).
_SMALL = dict(mel="syg_stft_mel_wseg_small_f32", rows="syg_stft_rows_wsmall_f32", tw=1024,
              pack=T.pack_mel_segments_rows, max_mels=48, small=True)      # (the [band][16 frames] tile holds 48 bands)
_SEG = {
    1024: dict(mel="syg_stft_mel_w1024_seg_f32", rows="syg_stft_rows_w1024_f32", tw=1024,
               pack=T.pack_mel_segments_rows, pack_kw={}, max_mels=255, small=False),
    4096: dict(mel="syg_stft_mel_w4096_f32", rows="syg_stft_rows_w4096_f32", tw=4096,
               pack=T.pack_mel_segments, pack_kw=dict(n_pass=4), max_mels=255, small=False),
    512: dict(_SMALL, pack_kw=dict(rows=4, row_words=296, n_pass=1, block=16)),
    256: dict(_SMALL, pack_kw=dict(rows=4, row_words=160, n_pass=1, block=8)),
}


def _small_only(who, n_fft):
    if n_fft not in (512, 256):
        raise SygnalsHipError(f"{who}: frame length must be 512 or 256")


def _segtab(n_fft, sr, n_mels, fmin=0.0, fmax=None):
    """Piece table of the segment-sum kernel of frame length n_fft for this filterbank on the device, or None."""
    k = _SEG[n_fft]
    if n_mels > k["max_mels"]:
        return None
    fmax = sr / 2.0 if fmax is None else fmax

    def build():
        try:
            basis = T.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
            return _dev(k["pack"](sr, n_fft, n_mels, fmin, fmax, basis=basis, **k["pack_kw"]).reshape(-1))
        except ValueError:
            return False
    tab = _cached((f"seg{n_fft}", float(sr), n_mels, float(fmin), float(fmax)), build)
    return None if tab is False else tab


def _seg_args(k, y, n_fft, hop, center, Tn, window, win_length):
    """Leading arguments of the entry points of _SEG: clips, framing, window, twiddles."""
    return (_ptr(y), y.shape[0], y.shape[1], _ld(y)) + ((n_fft,) if k["small"] else ()) + (
        hop, int(center), Tn, _ptr(window_dev(window, win_length or n_fft, n_fft)), _ptr(twiddle_dev(k["tw"])))


def _seg_mel(n_fft, y, sr, hop, center, window, win_length, n_mels, fmin, fmax):
    """Mel power [B, n_mels, T] from the segment-sum kernel of frame length n_fft (power 2)."""
    k = _SEG[n_fft]
    y = _f32_in(y, "y", 2)
    tab = _segtab(n_fft, sr, n_mels, fmin, fmax)
    if tab is None:
        raise SygnalsHipError(f"{k['mel'][4:-4]}: no piece table for this frame length / filterbank "
                              "(stft_mel_segments says so with None; stft_mel_pow2 / the generic chain take any filterbank)")
    Tn = _frames(y.shape[1], n_fft, hop, center)
    out = torch.empty((y.shape[0], n_mels, Tn), dtype=torch.float32, device=y.device)
    _call(k["mel"], *_seg_args(k, y, n_fft, hop, center, Tn, window, win_length), _ptr(tab), int(tab.numel()), n_mels,
          _ptr(out))
    return out


def _seg_rows(n_fft, y, sr, hop, center, window, win_length, n_mels, fmin, fmax, want_stats, roll_percent, bw_p, contrast):
    """Statistics / contrast rows from the segment-sum kernel of frame length n_fft, with the mel power block when n_mels is
    given (1024 / 4096).  Returns (mel | None, stats | None, contrast_pv | None)."""
    k = _SEG[n_fft]
    who = k["rows"][4:-4]
    y = _f32_in(y, "y", 2)
    B, L = y.shape
    Tn = _frames(L, n_fft, hop, center)
    smask, stats, cpv, cplan_p = _rows_out(B, Tn, want_stats, contrast, y.device, who)
    mel_args, mel = (), None
    if not k["small"]:
        tab = None
        if n_mels is not None:
            tab = _segtab(n_fft, sr, n_mels, fmin, fmax)
            if tab is None:
                raise SygnalsHipError(f"{who}: no piece table for this filterbank")
            mel = torch.empty((B, n_mels, Tn), dtype=torch.float32, device=y.device)
        mel_args = (_ptr(tab), int(tab.numel()) if tab is not None else 0, int(n_mels or 0), _ptr(mel))
    _call(k["rows"], *_seg_args(k, y, n_fft, hop, center, Tn, window, win_length), *mel_args, float(sr), float(roll_percent),
          float(bw_p), smask, _ptr(stats), cplan_p, _ptr(cpv))
    return mel, stats, cpv


def w4096_segtab(sr, n_mels, fmin=0.0, fmax=None):
    """Four-pass piece table of the frame-length-4096 kernel for this filterbank on the device, or None."""
    return _segtab(4096, sr, n_mels, fmin, fmax)


def w1024_segtab(sr, n_mels, fmin=0.0, fmax=None):
    """Two-row piece table of the frame-length-1024 segment-sum kernel for this filterbank on the device, or None."""
    return _segtab(1024, sr, n_mels, fmin, fmax)


def wsmall_segtab(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """Four-row piece table of the frame-length-512 / 256 segment-sum kernel for this filterbank on the device, or None."""
    return _segtab(n_fft, sr, n_mels, fmin, fmax) if n_fft in (512, 256) else None


def stft_mel_w1024_seg(y: torch.Tensor, sr: float, hop: int = 256, center: bool = True, window="hann", win_length=None,
                       n_mels: int = 128, fmin: float = 0.0, fmax=None) -> torch.Tensor:
    """frame_length 1024, power 2: [B, L] clips -> mel power [B, n_mels, T] in one launch, free-running waves (two frames
    per wave transform, mel by segment sums).  Raises SygnalsHipError when the filterbank has no piece table."""
    return _seg_mel(1024, y, sr, hop, center, window, win_length, n_mels, fmin, fmax)


def stft_rows_w1024(y: torch.Tensor, sr: float, hop: int = 256, center: bool = True, window="hann", win_length=None,
                    n_mels: Optional[int] = None, fmin: float = 0.0, fmax=None, want_stats=False, roll_percent: float = 0.85,
                    bw_p: float = 2.0, contrast: Optional[np.ndarray] = None):
    """frame_length 1024: the statistics / contrast rows of stft2048_mel from the segment-sum kernel's launch
    (syg_stft_rows_w1024_f32), with the mel power block when n_mels is given (needs a piece table: w1024_segtab).
    Returns (mel [B, M, T] | None, stats [B, 8, T] | None, contrast_pv [B, 2, R, T] | None)."""
    return _seg_rows(1024, y, sr, hop, center, window, win_length, n_mels, fmin, fmax, want_stats, roll_percent, bw_p, contrast)


def stft_mel_wseg_small(y: torch.Tensor, sr: float, n_fft: int, hop: int, center: bool = True, window="hann", win_length=None,
                        n_mels: int = 128, fmin: float = 0.0, fmax=None) -> torch.Tensor:
    """frame_length 512 / 256, power 2: [B, L] clips -> mel power [B, n_mels, T] in one launch, free-running waves (four /
    eight frames per wave transform, mel by segment sums).  Raises SygnalsHipError without a piece table."""
    _small_only("stft_mel_wseg_small", n_fft)
    return _seg_mel(n_fft, y, sr, hop, center, window, win_length, n_mels, fmin, fmax)


def stft_rows_wsmall(y: torch.Tensor, sr: float, n_fft: int, hop: int, center: bool = True, window="hann", win_length=None,
                     want_stats=False, roll_percent: float = 0.85, bw_p: float = 2.0, contrast: Optional[np.ndarray] = None):
    """frame_length 512 / 256: the statistics / contrast rows of stft2048_mel from the segment-sum kernel's transform
    (syg_stft_rows_wsmall_f32; nothing is projected).  Returns (stats [B, 8, T] | None, contrast_pv [B, 2, R, T] | None)."""
    _small_only("stft_rows_wsmall", n_fft)
    return _seg_rows(n_fft, y, sr, hop, center, window, win_length, None, 0.0, None, want_stats, roll_percent, bw_p, contrast)[1:]


def stft_rows_w4096(y: torch.Tensor, sr: float, hop: int = 1024, center: bool = True, window="hann", win_length=None,
                    n_mels: Optional[int] = None, fmin: float = 0.0, fmax=None, want_stats=False, roll_percent: float = 0.85,
                    bw_p: float = 2.0, contrast: Optional[np.ndarray] = None):
    """frame_length 4096: the statistics / contrast rows of stft2048_mel from the one-wave-per-frame kernel's launch
    (syg_stft_rows_w4096_f32), with the mel power block when n_mels is given (needs a piece table: w4096_segtab).
    Returns (mel [B, M, T] | None, stats [B, 8, T] | None, contrast_pv [B, 2, R, T] | None)."""
    return _seg_rows(4096, y, sr, hop, center, window, win_length, n_mels, fmin, fmax, want_stats, roll_percent, bw_p, contrast)


def stft_mel_segments(y, sr, n_fft, hop, center, window, win_length, n_mels, fmin, fmax):
    """Mel power by one of the segment-sum kernels of the other frame lengths (1024, 512, 256, 4096), or None when the
    frame length / filterbank has none."""
    if n_fft not in _SEG or _segtab(n_fft, sr, n_mels, fmin, fmax) is None:
        return None
    return stft_front(y, sr, n_fft, hop, center, window, win_length, n_mels, fmin, fmax)[0]


def stft_mel_w4096(y: torch.Tensor, sr: float, hop: int = 1024, center: bool = True, window="hann", win_length=None,
                   n_mels: int = 128, fmin: float = 0.0, fmax=None) -> torch.Tensor:
    """frame_length 4096: [B, L] clips -> mel power [B, n_mels, T] in one launch (one wave per frame, mel by segment
    sums).  Raises SygnalsHipError when the filterbank has no four-pass piece table."""
    return _seg_mel(4096, y, sr, hop, center, window, win_length, n_mels, fmin, fmax)


def stft2048_mel(y: torch.Tensor, sr: float, hop: int = 512, center: bool = True, window="hann",
                 win_length: int = 2048, n_mels: int = 128, fmin: float = 0.0, fmax=None,
                 want_stats=False, roll_percent: float = 0.85, bw_p: float = 2.0,
                 contrast: Optional[np.ndarray] = None, projection: str = "auto", tri_waves: int = 16):
    """Fused STFT(2048) -> power -> mel.  Returns (mel [B, M, T], stats [B, 8, T] | None,
    contrast_pv [B, 2, R, T] | None).  `want_stats`: False, True (all rows) or a bit mask (1 centroid,
    2 bandwidth, 4 flatness, 8 rolloff, 16 dominant): only the selected rows are computed / written.
    projection: "segments" (syg_stft2048_mel_tri_f32: per-wave segment sums -- the two-pass table where the filterbank has
    one, else the four-pass table -- no barriers in the projection; tri_waves = 16 | 8 waves per workgroup), "matrix"
    (syg_stft2048_mel_f32: block-sparse weights on the matrix cores), "auto": the matrix form wherever it has a plan."""
    y = _f32_in(y, "y", 2)
    B, L = y.shape
    Tn = _frames(L, 2048, hop, center)
    cfg = mel_config(sr, 2048, n_mels, fmin, fmax)
    if projection not in ("auto", "segments", "matrix"):
        raise ValueError("projection must be 'auto', 'segments' or 'matrix'")
    tab = cfg.segtab if cfg.segtab is not None else cfg.segtab4
    tri = tab is not None and fused_waves() == 16 and Tn * n_mels < (1 << 29) and projection != "matrix"
    if projection == "auto" and cfg.wpacked is not None:
        # measured (profiles/r04_rows_start.json vs r04b): the matrix form wins wherever it has a plan -- 128 bands 0.206 ms per
        # 1024 clips (mel + dB / DCT launch) against 0.241 for four passes of masked segment sums (about 380 vector
        # instructions per frame), 64 bands 0.178 against 0.214 -- so "auto" keeps it; the segment form serves the plans the
        # matrix form cannot hold (8-wave development mode beyond 128 bands) and stays selectable
        tri = False
    if projection == "segments" and not tri:
        raise SygnalsHipError("stft2048_mel: no piece table for this filterbank (projection='segments')")
    if not tri and cfg.wpacked is None:
        raise SygnalsHipError("fused path: no block-sparse plan for this filterbank (n_mels <= 256; <= 128 with 8 waves)")
    win = window_dev(window, win_length, 2048)
    tw = twiddle_dev(2048)
    mel = torch.empty((B, n_mels, Tn), dtype=torch.float32, device=y.device)
    smask, stats, cpv, cplan_p = _rows_out(B, Tn, want_stats, contrast, y.device)
    if tri:
        _call("syg_stft2048_mel_tri_f32", _ptr(y), B, L, _ld(y), hop, int(center), Tn, _ptr(win), _ptr(tw), _ptr(tab),
              int(tab.numel()), n_mels, _ptr(mel), float(sr), float(roll_percent), float(bw_p), smask, _ptr(stats), cplan_p,
              _ptr(cpv), int(tri_waves))
        return mel, stats, cpv
    _call("syg_stft2048_mel_f32", _ptr(y), B, L, _ld(y), hop, int(center), Tn, _ptr(win), _ptr(tw), _ptr(cfg.wpacked),
          cfg.plan.ctypes.data_as(C.c_void_p), n_mels, _ptr(mel), float(sr), float(roll_percent), float(bw_p), smask,
          _ptr(stats), cplan_p, _ptr(cpv))
    return mel, stats, cpv


def stft2048_stats_fits(hop: int, L: int = 0) -> bool:
    """Whether stft2048_stats takes this call (_front.stats2048_takes: the C side's conditions and the 16-wave kernel)."""
    return stats2048_takes(hop, L, fused_waves())


def stft2048_stats(y: torch.Tensor, sr: float, hop: int = 512, center: bool = True, window="hann", win_length: int = 2048,
                   want_stats=True, roll_percent: float = 0.85, bw_p: float = 2.0, contrast: Optional[np.ndarray] = None):
    """The statistics / contrast rows of stft2048_mel WITHOUT the mel spectrogram (syg_stft2048_stats_f32: transform + row
    functions, nothing projected) -- what spectral_centroid / bandwidth / flatness / rolloff / contrast need
    (manager.py:289-343).  Returns (stats [B, 8, T] | None, contrast_pv [B, 2, R, T] | None), bit-identical to
    stft2048_mel's."""
    y = _f32_in(y, "y", 2)
    B, L = y.shape
    Tn = _frames(L, 2048, hop, center)
    smask, stats, cpv, cplan_p = _rows_out(B, Tn, want_stats, contrast, y.device, "stft2048_stats")
    win = window_dev(window, win_length, 2048)
    tw = twiddle_dev(2048)
    _call("syg_stft2048_stats_f32", _ptr(y), B, L, _ld(y), hop, int(center), Tn, _ptr(win), _ptr(tw), float(sr),
          float(roll_percent), float(bw_p), smask or 1, _ptr(stats), cplan_p, _ptr(cpv))
    return stats, cpv


def front_caps(sr, n_fft, n_mels, fmin=0.0, fmax=None) -> dict:
    """What _front.front_route needs to know about the tables, as plain values (n_mels None: no mel block is wanted)."""
    return dict(waves=fused_waves(), plan2048=fused_mel_ok(sr, n_fft, n_mels or 16, fmin, fmax),
                table=n_mels is not None and n_fft in _SEG and _segtab(n_fft, sr, n_mels, fmin, fmax) is not None)


def stft_front(y, sr, n_fft, hop, center=True, window="hann", win_length=None, n_mels=None, fmin=0.0, fmax=None, power=2.0,
               want_stats=False, roll_percent=0.85, bw_p=2.0, contrast=None, route=None):
    """[B, L] clips -> (mel [B, n_mels, T] of |STFT|^power | None, stats [B, 8, T] | None, contrast_pv [B, 2, R, T] | None)
    for any frame length, by the kernels _front.front_route names (route: an answer of it that the caller already has).
    n_mels None: no mel block; want_stats / contrast: as stft2048_mel."""
    smask = 31 if want_stats is True else int(want_stats or 0)
    by_rows, by_mel = route or front_route(n_fft, hop, y.shape[1], power, n_mels, bool(smask) or contrast is not None,
                                           front_caps(sr, n_fft, n_mels, fmin, fmax))
    mel = stats = cpv = None
    if "generic" in (by_rows, by_mel):
        # the complex STFT of any frame length in HBM, then |X|, the row kernels and the dense mel matrix
        X = stft_any(y, n_fft, hop, center, window, win_length)
        B, Tn, F = X.shape[:3]
        if smask or contrast is not None:
            mag = cabs_pow(X, 1).reshape(B * Tn, F)
            if smask:
                freqs = to_device_f32(np.fft.rfftfreq(n_fft, 1.0 / sr))
                stats = spectral_stats(mag, freqs, roll_percent, bw_p).reshape(8, B, Tn).permute(1, 0, 2)
            if contrast is not None:
                cpv = contrast_pv(mag, contrast).reshape(2, int(contrast[0]), B, Tn).permute(2, 0, 1, 3).contiguous()
        if n_mels is not None:
            if power not in (1.0, 2.0):
                raise SygnalsHipError("mel power must be 1.0 or 2.0 on the device")
            mel = mel_dense(cabs_pow(X, int(power)), mel_config(sr, n_fft, n_mels, fmin, fmax).basis)
        return mel, stats, cpv

    def call(name, *tail):
        # the wrapper by name, looked up now: tests replace them with spies (those of 512 / 256 and the dense one take n_fft)
        frame = (n_fft,) if name in ("stft_rows_wsmall", "stft_mel_wseg_small", "stft_mel_pow2") else ()
        return globals()[name](y, sr, *frame, hop, center, window, win_length or n_fft, *tail)
    rows_args = (smask, roll_percent, bw_p, contrast)
    if by_rows in ("stft2048_stats", "stft_rows_wsmall"):
        stats, cpv = call(by_rows, *rows_args)
    elif by_rows:
        # stft2048_mel (no mel wanted: 16 stand-in bands, discarded below); stft_rows_w1024 / w4096: the mel block too,
        # unless it has a launch of its own
        m = (n_mels or 16) if by_rows == "stft2048_mel" else (None if by_mel else n_mels)
        mel, stats, cpv = call(by_rows, m, fmin, fmax, *rows_args)
    if by_mel == "stft2048_mel":
        mel = call(by_mel, n_mels, fmin, fmax)[0]
    elif by_mel:
        mel = call(by_mel, n_mels, fmin, fmax, *((int(power),) if by_mel == "stft_mel_pow2" else ()))
    return (mel if n_mels is not None else None), stats, cpv


def stft2048_c2c(y: torch.Tensor, hop: int = 512, center: bool = True, window="hann", win_length: int = 2048):
    """Complex STFT, frame-major [B, T, 1025, 2] float32."""
    y = _f32_in(y, "y", 2)
    B, L = y.shape
    Tn = _frames(L, 2048, hop, center)
    win = window_dev(window, win_length, 2048)
    tw = twiddle_dev(2048)
    out = torch.empty((B, Tn, 1025, 2), dtype=torch.float32, device=y.device)
    _call("syg_stft2048_c2c_f32", _ptr(y), B, L, _ld(y), hop, int(center), Tn, _ptr(win), _ptr(tw), _ptr(out))
    return out


def _db_args(amin, top_db, ref, takes_db=False):
    """The power_to_db arguments of the entry points, checked: (amin, top_db -- -1: none --, ref_is_max, ref_value).
    ref: "max" / np.max (per-clip maximum), a scalar or, with takes_db, "db": the input is in dB already (DCT only)."""
    if amin <= 0:
        raise ValueError("amin must be strictly positive")
    if top_db is not None and top_db < 0:
        raise ValueError("top_db must be non-negative")
    if takes_db and isinstance(ref, str) and ref == "db":
        how = (2, 1.0)
    elif (isinstance(ref, str) and ref == "max") or ref is np.max:
        how = (1, 1.0)
    else:
        how = (0, float(ref))
    return (float(amin), float(top_db) if top_db is not None else -1.0) + how


def logmel_dct(mel: torch.Tensor, n_mfcc: Optional[int] = 13, dct_type: int = 2, norm="ortho", lifter: float = 0.0,
               amin: float = 1e-10, top_db: Optional[float] = 80.0, ref="max", keep_mel: bool = False):
    """power_to_db (ref = per-clip max or a scalar) then DCT.  Returns (logmel [B,M,T], mfcc [B,K,T] | None).

    `mel` is converted to dB in place unless keep_mel=True.
    """
    require_gpu()
    B, M, Tn = mel.shape
    db = _db_args(amin, top_db, ref, takes_db=True)
    logmel = torch.empty_like(mel) if keep_mel else None
    mf = dct = lif = None
    K = 0
    if n_mfcc is not None:
        K = int(n_mfcc)
        dct = dct_dev(K, M, dct_type, norm)
        lw = T.lifter_weights(K, float(lifter))
        lif = _dev(lw) if lw is not None else None
        mf = torch.empty((B, K, Tn), dtype=torch.float32, device=mel.device)
    _call("syg_logmel_dct_f32", _ptr(mel), B, M, Tn, _ptr(dct), K, _ptr(lif), *db, _ptr(logmel), _ptr(mf))
    return (logmel if keep_mel else mel), mf


def mel_mfcc(mel: torch.Tensor, n_mfcc: int = 13, dct_type: int = 2, norm="ortho", lifter: float = 0.0, amin: float = 1e-10,
             top_db: Optional[float] = 80.0, ref="max") -> torch.Tensor:
    """MFCC [B, K, T] from a mel POWER matrix [B, M, T] that the caller no longer needs (it is scratch for the call): dB +
    DCT as logmel_dct, without writing the dB matrix to HBM."""
    require_gpu()
    B, M, Tn = mel.shape
    db = _db_args(amin, top_db, ref)
    K = int(n_mfcc)
    dct = dct_dev(K, M, dct_type, norm)
    lw = T.lifter_weights(K, float(lifter))
    lif = _dev(lw) if lw is not None else None
    mf = torch.empty((B, K, Tn), dtype=torch.float32, device=mel.device)
    _call("syg_mel_mfcc_f32", _ptr(mel), B, M, Tn, _ptr(dct), K, _ptr(lif), *db, _ptr(mf))
    return mf


def mfcc_fused_fits(n_mels: int, n_frames: int, n_mfcc: int = 13) -> bool:
    """True when the clip's mel matrix + DCT rows fit the LDS left beside the fused kernel's buffers (the library
    owns the formula: syg_stft2048_mfcc_fits)."""
    return bool(lib().syg_stft2048_mfcc_fits(int(n_mels), int(n_frames), int(n_mfcc)))


def mfcc_fused_pays(n_mels: int, n_frames: int, n_mfcc: int = 13) -> bool:
    """True when mfcc_batch's default should take the one-launch form: the clip's mel matrix fits beside the stage buffer,
    or it fits in the buffer's place (frames then come straight from global memory) and is wide enough for the saved
    second launch to outweigh that (128 bands: 186 against 196 us per 1024 clips; 64 bands: 176 against 166)."""
    f = int(lib().syg_stft2048_mfcc_fits(int(n_mels), int(n_frames), int(n_mfcc)))
    return f == 2 or (f == 1 and n_mels >= 96)


class _MfccCall:
    """Prepared argument list of syg_stft2048_mfcc_f32 for one (shape, parameters) combination: a steady-state
    call then costs two allocations and one ctypes call (the kernel runs ~0.2 ms; rebuilding keys, tables and
    22 ctypes arguments per call costs the host about as much)."""

    def __init__(self, B, L, ld, device, sr, hop, center, window, n_mels, n_mfcc, fmin, fmax, lifter, amin, top_db,
                 ref, dct_type, norm, keep_mel, projection="auto"):
        db = _db_args(amin, top_db, ref)
        Tn = num_frames(L, 2048, hop, center)
        if Tn <= 0:
            raise ValueError("signal too short for one frame")
        self.cfg = mel_config(sr, 2048, n_mels, fmin, fmax, waves=16)
        K = int(n_mfcc)
        self.dct = dct_dev(K, n_mels, dct_type, norm)
        lw = T.lifter_weights(K, float(lifter))
        self.lif = _dev(lw) if lw is not None else None
        self.win = window_dev(window, 2048, 2048)
        self.tw = twiddle_dev(2048)
        self.shape = (B, L, ld)
        self.device = device
        self.mel_shape = (B, n_mels, Tn) if keep_mel else None
        self.out_shape = (B, K, Tn)
        tail = (n_mels, _ptr(self.dct), K, _ptr(self.lif)) + db
        # projection: "segments" = each wave projects its own power row by segment sums (no weight matrix, no workgroup
        # barrier in the projection: 133 against 149 us at config C2), "matrix" = block-sparse weights on the matrix
        # cores; "auto" takes the segment form when the filterbank has a piece table, the staged loads apply (hop <= 512),
        # no copy of the mel matrix is asked for and the two mel matrices fit the LDS
        if projection not in ("auto", "matrix", "segments"):
            raise ValueError("projection must be 'auto', 'matrix' or 'segments'")
        tri_ok = (self.cfg.segtab is not None and not keep_mel and hop <= 512
                  and bool(lib().syg_stft2048_mfcc_tri_fits(int(n_mels), int(Tn), K)))
        if projection == "segments" and not tri_ok:
            raise SygnalsHipError("stft2048_mfcc: no segment-sum projection for this call (filterbank without a piece table, "
                                  "keep_mel, hop > 512, or the clip's two mel matrices do not fit the LDS)")
        self.tri = tri_ok and projection != "matrix"
        if self.tri:
            self.fn, self.name = lib().syg_stft2048_mfcc_tri_f32, "syg_stft2048_mfcc_tri_f32"
            self.head = (B, L, ld, hop, int(center), Tn, _ptr(self.win), _ptr(self.tw), _ptr(self.cfg.segtab),
                         int(self.cfg.segtab.numel())) + tail
        else:
            self.fn, self.name = lib().syg_stft2048_mfcc_f32, "syg_stft2048_mfcc_f32"
            self.head = (B, L, ld, hop, int(center), Tn, _ptr(self.win), _ptr(self.tw), _ptr(self.cfg.wpacked),
                         self.cfg.plan.ctypes.data_as(C.c_void_p)) + tail

    def __call__(self, y):
        mel = torch.empty(self.mel_shape, dtype=torch.float32, device=self.device) if self.mel_shape else None
        mf = torch.empty(self.out_shape, dtype=torch.float32, device=self.device)
        if self.tri:
            rc = self.fn(y.data_ptr(), *self.head, mf.data_ptr(), _stream_ptr())
        else:
            rc = self.fn(y.data_ptr(), *self.head, mel.data_ptr() if mel is not None else None, mf.data_ptr(),
                         _stream_ptr())
        if rc:
            check(rc, self.name)
        return mf, mel


_mfcc_calls: dict = {}


def stft2048_mfcc(y: torch.Tensor, sr: float, hop: int = 512, center: bool = True, window="hann", n_mels: int = 128,
                  n_mfcc: int = 13, fmin: float = 0.0, fmax=None, lifter: float = 0.0, amin: float = 1e-10,
                  top_db: Optional[float] = 80.0, ref="max", dct_type: int = 2, norm="ortho", keep_mel: bool = False,
                  projection: str = "auto"):
    """One launch: [B, L] clips -> MFCC [B, n_mfcc, T]; the mel matrix of a clip never leaves LDS.
    projection: "auto" | "segments" | "matrix" -- how a power row becomes mel bands (see _MfccCall).

    Returns (mfcc, mel_power | None).  Raises SygnalsHipError when the clip's mel matrix does not fit
    (mfcc_fused_fits) -- mfcc_batch() falls back to the two-launch form by itself.
    """
    if y.dim() != 2 or y.dtype != torch.float32 or not y.is_cuda:
        require_gpu()
        raise ValueError("y must be a float32 [B, L] device tensor")
    if y.stride(1) != 1:
        y = y.contiguous()
    wkey = window if isinstance(window, str) else _window_key(window, 2048, 2048)
    rkey = "max" if (ref is np.max or ref == "max") else float(ref)
    key = (y.device.index, y.shape[0], y.shape[1], _ld(y), float(sr), hop, bool(center), wkey, n_mels, n_mfcc,
           float(fmin), fmax, float(lifter), amin, top_db, rkey, dct_type, norm, keep_mel, projection)
    call = _mfcc_calls.get(key)
    if call is None:
        require_gpu()
        call = _MfccCall(y.shape[0], y.shape[1], _ld(y), y.device, sr, hop, center, window, n_mels, n_mfcc, fmin,
                         fmax, lifter, amin, top_db, ref, dct_type, norm, keep_mel, projection)
        if len(_mfcc_calls) > 64:
            _mfcc_calls.clear()
        _mfcc_calls[key] = call
    return call(y)


def stft2048_features_tri(y, sr, hop, center, window, n_mels, fmin, fmax, n_mfcc, smask, roll_percent, bw_p, cplan,
                          out=None, stats=None):
    """MFCC rows + statistics rows + contrast tail means of [B, L] device clips from ONE launch
    (syg_stft2048_features_tri_f32: frame_length 2048, power 2, DCT-II ortho, no lifter, ref = max, top_db 80), prepared: a
    callable whose every call is that one library call and returns (out, stats [B, 8, T] | None, contrast_pv [B, 2, R, T]
    | None) -- or None when the shape has no one-launch form (two-pass piece table for the filterbank, staged loads:
    hop <= 512, 16 waves, the clip's mel matrices in LDS).  smask: statistics rows wanted, cplan: the contrast plan or None.
    out: a [B, rows >= n_mfcc, T] block whose first n_mfcc rows take the MFCC (default: a new [B, n_mfcc, T]); stats: the
    caller's own buffer (default: zeros, so that rows not asked for read 0)."""
    B, L = y.shape
    Tn = num_frames(L, 2048, hop, center)
    cfg = mel_config(sr, 2048, n_mels, fmin, fmax, waves=16)
    if not (cfg.segtab is not None and hop <= 512 and fused_waves() == 16
            and lib().syg_stft2048_mfcc_tri_fits(int(n_mels), int(Tn), int(n_mfcc))):
        return None
    if y.stride(1) != 1:
        y = y.contiguous()
    if out is None:
        out = torch.empty((B, n_mfcc, Tn), dtype=torch.float32, device=y.device)
    if stats is None and smask:
        stats = torch.zeros((B, 8, Tn), dtype=torch.float32, device=y.device)
    cph = cpv = None
    if cplan is not None:
        cph = np.ascontiguousarray(cplan, np.int32)
        cpv = torch.empty((B, 2, int(cph[0]), Tn), dtype=torch.float32, device=y.device)
    args = (_ptr(y), B, L, _ld(y), hop, int(center), Tn, _ptr(window_dev(window, 2048, 2048)), _ptr(twiddle_dev(2048)),
            _ptr(cfg.segtab), int(cfg.segtab.numel()), n_mels, _ptr(dct_dev(n_mfcc, n_mels)), n_mfcc, None, 1e-10, 80.0, 1, 1.0,
            float(sr), float(roll_percent), float(bw_p), (smask | 32) if smask else 1, _ptr(stats),
            cph.ctypes.data_as(C.c_void_p) if cph is not None else None, _ptr(cpv), _ptr(out), out.shape[1])

    def launch(_alive=(y, cph)):                     # (the arguments point into these)
        _call("syg_stft2048_features_tri_f32", *args)
        return out, stats, cpv
    return launch


def mfcc_batch(y: torch.Tensor, sr: float, n_fft: int = 2048, hop: int = 512, n_mels: int = 128, n_mfcc: int = 13,
               center: bool = True, window="hann", fmin: float = 0.0, fmax=None, lifter: float = 0.0, fused=None):
    """Config C2: [B, L] clips -> MFCC [B, n_mfcc, T] (manager path a1..a5), all on device.

    fused=None picks the one-launch clip-resident form when the clip's mel matrix fits in LDS and there are
    enough clips to fill the chip (a workgroup owns whole clips); True / False force either form.
    """
    if not fused_mel_ok(sr, n_fft, n_mels, fmin, fmax):
        if fused and fused_pow2_ok(n_fft, n_mels):
            # the other power-of-two frame lengths, fused=True: ONE launch (a workgroup owns a clip, needs the clip's mel
            # matrix to fit the LDS).  The default is the mel launch + dB / DCT -- two launches, but more workgroups per CU
            # (n_fft 1024: 266 us against 318 us per 1024 clips x 1 s; n_fft 512: 709 against 973 us)
            if not mfcc_pow2_fits(n_fft, n_mels, num_frames(y.shape[1], n_fft, hop, center), n_mfcc):
                raise SygnalsHipError("mfcc_batch: the clip's mel matrix does not fit the LDS of the one-launch form")
            return stft_mfcc_pow2(y, sr, n_fft, hop, center, window, None, n_mels, n_mfcc, fmin, fmax, lifter)[0]
        # the mel launch front_route names (segment sums at 1024 / 512 / 256 / 4096: 0.162 against 0.235 ms per 1024 clips
        # x 1 s at 1024 for the dense kernel's; 0.265 against 0.334 ms, 0.330 against 0.356 ms), then dB + DCT; fused=False,
        # or no fused kernel for the shape: complex STFT (any frame length) -> |X|^2 -> dense mel
        route = (None, "generic")
        if fused is not False:
            route = front_route(n_fft, hop, y.shape[1], 2.0, n_mels, False, front_caps(sr, n_fft, n_mels, fmin, fmax))
        if fused and route[1] == "generic":
            raise SygnalsHipError(f"mfcc_batch: no fused kernel for n_fft={n_fft}, n_mels={n_mels}")
        mel = stft_front(y, sr, n_fft, hop, center, window, None, n_mels, fmin, fmax, route=route)[0]
        return mel_mfcc(mel, n_mfcc, lifter=lifter)
    if fused is None:
        fused = mfcc_fused_pays(n_mels, num_frames(y.shape[1], 2048, hop, center), n_mfcc) and y.shape[0] >= 128
    if fused:
        return stft2048_mfcc(y, sr, hop, center, window, n_mels, n_mfcc, fmin, fmax, lifter)[0]
    mel, _, _ = stft2048_mel(y, sr, hop, center, window, 2048, n_mels, fmin, fmax)
    return mel_mfcc(mel, n_mfcc, lifter=lifter)


# ------------------------------------------------------------------ generic pow2 kernels
def twiddle_rfft_dev(n_fft) -> torch.Tensor:
    """[n_fft + n_fft/2, 2]: W_nfft^k followed by W_{nfft/2}^k (layout of stft_pow2 / welch)."""
    return _cached(("twr", n_fft), lambda: _dev(np.concatenate([T.twiddles(n_fft), T.twiddles(n_fft // 2)], axis=0)))


def fft_pow2(x: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Batched complex FFT of x [batch, n, 2] float32, n a power of two <= 8192."""
    require_gpu()
    if x.dim() != 3 or x.shape[2] != 2 or x.dtype != torch.float32:
        raise ValueError("x must be float32 [batch, n, 2]")
    x = x.contiguous()
    batch, n, _ = x.shape
    out = torch.empty_like(x)
    _call("syg_fft_pow2_c2c_f32", _ptr(x), _ptr(out), batch, n, int(inverse), _ptr(twiddle_dev(n)))
    return out


def stft_pow2(y: torch.Tensor, n_fft: int, hop: int, center: bool = True, window="hann", win_length=None):
    """Generic framed STFT, frame-major complex [B, T, 1 + n_fft/2, 2]."""
    require_gpu()
    if y.stride(1) != 1:
        y = y.contiguous()
    B, L = y.shape
    win_length = n_fft if win_length is None else win_length
    Tn = _frames(L, n_fft, hop, center)
    win = window_dev(window, win_length, n_fft)
    out = torch.empty((B, Tn, n_fft // 2 + 1, 2), dtype=torch.float32, device=y.device)
    _call("syg_stft_pow2_c2c_f32", _ptr(y), B, L, _ld(y), n_fft, hop, int(center), Tn, _ptr(win),
          _ptr(twiddle_rfft_dev(n_fft)), _ptr(out))
    return out


def stft_any(y, n_fft, hop, center=True, window="hann", win_length=None):
    """Complex STFT [B, T, F, 2]: the wave-FFT kernel for n_fft = 2048, the LDS Stockham kernel otherwise."""
    if n_fft == 2048:
        return stft2048_c2c(y, hop, center, window, 2048 if win_length is None else win_length)
    if is_pow2(n_fft) and 8 <= n_fft <= 16384:
        return stft_pow2(y, n_fft, hop, center, window, win_length)
    return stft_rows(y, n_fft, hop, center, window, win_length)


def pack_frames(y: torch.Tensor, n_rows: int, length: int, step: int, first: int, n_out: int,
                window: Optional[torch.Tensor] = None, detrend=False, cplx: bool = True) -> torch.Tensor:
    """Frames first .. first + n_rows - 1 (length `length`, start (first + r) * step) of EVERY row of the contiguous
    y [B, Lp] -> [B * n_rows, n_out(, 2)] detrended / windowed / zero-padded rows, clip-major: one launch for the whole
    batch (syg_pack_frames_f32; B * n_rows <= 65535)."""
    B, Lp = y.shape
    rows = B * n_rows
    out = torch.empty((rows, n_out, 2) if cplx else (rows, n_out), dtype=torch.float32, device=y.device)
    dcode = detrend_code(detrend)
    work = _workspace("syg_pack_rows_work_bytes", rows, dtype=torch.float64, device=y.device) if dcode else None
    base = y.data_ptr() + 4 * first * step
    _call("syg_pack_frames_f32", C.c_void_p(base), rows, length, step, n_rows, Lp, _ptr(window), dcode, 0, int(cplx),
          _ptr(out), n_out, _ptr(work))
    return out


def stft_rows(y: torch.Tensor, n_fft: int, hop: int, center: bool = True, window="hann", win_length=None):
    """Framed STFT for ANY n_fft >= 1 (librosa.stft accepts any frame length): the frames of each clip are windowed
    and packed as overlapping rows, transformed with the arbitrary-length FFT (four-step / Bluestein) and cut to the
    1 + n_fft//2 non-negative bins.  Frame-major complex [B, T, F, 2] like the power-of-two kernels."""
    require_gpu()
    B, L = y.shape
    win_length = n_fft if win_length is None else win_length
    pad = n_fft // 2 if center else 0
    Tn = _at_least_one(num_frames_padded(L, n_fft, hop, center))       # librosa's count on the padded signal
    yp = y
    if pad or y.stride(1) != 1 or not y.is_contiguous():
        yp = torch.zeros((B, L + 2 * pad), dtype=torch.float32, device=y.device)     # zero padding: data movement only
        yp[:, pad:pad + L] = y
    win = window_dev(window, win_length, n_fft)
    F = n_fft // 2 + 1
    out = torch.empty((B, Tn, F, 2), dtype=torch.float32, device=y.device)
    yp = yp.contiguous()
    if Tn <= MAX_ROWS:                                        # whole clips per launch: as many as fit 65535 rows
        per = max(1, MAX_ROWS // Tn)
        for b0 in range(0, B, per):
            bc = min(per, B - b0)
            X = fft_any(pack_frames(yp[b0:b0 + bc], Tn, n_fft, hop, 0, n_fft, window=win))
            out[b0:b0 + bc] = X.view(bc, Tn, n_fft, 2)[:, :, :F]
        return out
    for b in range(B):                                        # long clips: 65535 frames of one clip at a time
        for t0, tc in _row_blocks(Tn):
            X = fft_any(pack_frames(yp[b:b + 1], tc, n_fft, hop, t0, n_fft, window=win))
            out[b, t0:t0 + tc] = X[:, :F]
    return out


def cabs_pow(x: torch.Tensor, power: int = 1) -> torch.Tensor:
    """|x|^power (power 1 or 2) of an interleaved complex tensor [..., 2] -> [...]."""
    require_gpu()
    x = x.contiguous()
    out = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    _call("syg_cabs_pow_f32", _ptr(x), out.numel(), int(power), _ptr(out))
    return out


def mel_dense(P: torch.Tensor, basis: torch.Tensor) -> torch.Tensor:
    """mel [B, M, T] from frame-major power P [B, T, F] and a dense basis [M, F]."""
    require_gpu()
    P = P.contiguous()
    B, Tn, F = P.shape
    M = basis.shape[0]
    out = torch.empty((B, M, Tn), dtype=torch.float32, device=P.device)
    _call("syg_mel_dense_f32", _ptr(P), B, Tn, F, _ptr(basis), M, _ptr(out))
    return out


def spectral_stats(mag: torch.Tensor, freqs: torch.Tensor, roll_percent: float = 0.85, bw_p: float = 2.0):
    """Per-frame statistics of frame-major magnitudes mag [N, F]; returns [8, N] (SYG_STAT_* rows)."""
    require_gpu()
    if not 0.0 <= roll_percent <= 1.0:
        raise ValueError("roll_percent must be between 0.0 and 1.0.")
    if bw_p <= 0:
        raise ValueError("Order 'p' for spectral bandwidth must be positive.")
    mag = mag.contiguous()
    N, F = mag.shape
    out = torch.empty((8, N), dtype=torch.float32, device=mag.device)
    _call("syg_spectral_stats_f32", _ptr(mag), N, F, _ptr(freqs), float(roll_percent), float(bw_p), _ptr(out))
    return out


FS_ROWS = ("mean_amplitude", "std_dev_amplitude", "skewness", "kurtosis", "peak_amplitude", "crest_factor",
           "signal_entropy", "rms_energy", "zero_crossing_rate")      # row r <-> mask bit r of syg_frame_stats_f32


def frame_stats(y: torch.Tensor, frame_length: int = 2048, hop: int = 512, center: bool = True, num_bins: int = 10,
                mask: int = 0x1FF) -> torch.Tensor:
    """Time-domain frame features of clips y [B, L]: [B, 9, T] float32, rows as FS_ROWS (only the rows
    selected by `mask` are written)."""
    y = _f32_in(y, "y", 2)
    B, L = y.shape
    Tn = _frames(L, frame_length, hop, center)
    out = torch.zeros((B, 9, Tn), dtype=torch.float32, device=y.device)
    _call("syg_frame_stats_f32", _ptr(y), B, L, _ld(y), int(frame_length), int(hop), int(center), Tn, int(num_bins),
          int(mask), _ptr(out))
    return out


def rms_from_spec(S: torch.Tensor, frame_length: int) -> torch.Tensor:
    """librosa.feature.rms(S=...) for frame-major magnitudes S [N, F] -> [N]."""
    require_gpu()
    S = S.contiguous()
    N, F = S.shape
    out = torch.empty((N,), dtype=torch.float32, device=S.device)
    _call("syg_rms_from_spec_f32", _ptr(S), N, F, int(frame_length), _ptr(out))
    return out


def contrast_pv(mag: torch.Tensor, cplan: np.ndarray) -> torch.Tensor:
    """Peak / valley tail means [2, R, N] of frame-major magnitudes mag [N, F]."""
    require_gpu()
    mag = mag.contiguous()
    N, F = mag.shape
    cplan = np.ascontiguousarray(cplan, dtype=np.int32)
    out = torch.empty((2, int(cplan[0]), N), dtype=torch.float32, device=mag.device)
    _call("syg_contrast_pv_f32", _ptr(mag), N, F, cplan.ctypes.data_as(C.c_void_p), _ptr(out))
    return out


def sosfiltfilt(x: torch.Tensor, sos: np.ndarray, zi: np.ndarray, padlen: int) -> torch.Tensor:
    """Batched zero-phase SOS filtering of x [B, L] (scipy.signal.sosfiltfilt semantics)."""
    require_gpu()
    if x.stride(1) != 1:
        x = x.contiguous()
    B, L = x.shape
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    zi = np.ascontiguousarray(zi, dtype=np.float64)
    S = sos.shape[0]
    if L <= padlen:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {padlen}.")
    # (0 bytes: the clip-resident form keeps the clip in registers and needs no workspace)
    work = _workspace("syg_sosfiltfilt_work_bytes", B, L, padlen, S, dtype=torch.float64, device=x.device,
                      error=SygnalsHipError(f"sosfiltfilt: unsupported configuration (sections={S}, max 8)"))
    y = torch.empty((B, L), dtype=torch.float32, device=x.device)
    _call("syg_sosfiltfilt_f32", _ptr(x), B, L, _ld(x), sos.ctypes.data_as(C.c_void_p), zi.ctypes.data_as(C.c_void_p), S,
          int(padlen), _ptr(y), _ld(y), _ptr(work))
    return y


SOSFILT_KEYS = ("chunk", "tile", "chunks_per_wave", "scan_ahead", "group_sections", "max_sections", "two_level_chunks")


def sosfilt_constants() -> dict:
    """Geometry of the causal SOS kernels (syg_sosfilt_constants), by name."""
    return _constants("syg_sosfilt_constants", SOSFILT_KEYS)


def sosfilt(x: torch.Tensor, sos: np.ndarray, zi: Optional[torch.Tensor] = None, return_state: bool = False,
            out: Optional[torch.Tensor] = None):
    """Batched causal SOS filtering of x [B, L]: y, zf = scipy.signal.sosfilt(sos, x, zi=zi) per row.

    x: float32 device rows, unit stride along L, any row stride.  sos: host [n_sections, 6], 1 to 32 sections.
    zi: device float64 [B, n_sections, 2] (scipy's per-section states) or None for a zero state.  Returns y, or (y, zf)
    with return_state=True; zf [B, n_sections, 2] float64 stays on the device and is the next block's zi.  out: the
    tensor y is written to (it may be x itself)."""
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("Input sos must be a 2D array with shape (n_sections, 6).")
    S = sos.shape[0]
    if not 1 <= S <= 32:
        raise ValueError(f"sosfilt: {S} sections; the causal kernels serve 1 to 32 sections per call "
                         "(split a longer cascade and carry y from call to call).")
    if np.any(sos[:, 3] == 0.0):
        raise ValueError("sosfilt: a0 of a section is zero.")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("sosfilt: x must be a float32 tensor of shape [B, L].")
    B, L = x.shape
    if B < 1 or L < 1:
        raise ValueError(f"sosfilt: x must hold at least one row of at least one sample (got [{B}, {L}]).")
    if zi is not None and (not isinstance(zi, torch.Tensor) or zi.dtype != torch.float64 or tuple(zi.shape) != (B, S, 2)):
        raise ValueError(f"sosfilt: zi must be a float64 tensor of shape [B, n_sections, 2] = [{B}, {S}, 2].")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (B, L)
                            or out.stride(1) != 1):
        raise ValueError(f"sosfilt: out must be a float32 tensor of shape [{B}, {L}] with unit stride along L.")
    require_gpu()
    if x.stride(1) != 1:
        x = x.contiguous()
    if zi is not None:
        zi = zi.to(x.device).contiguous()
    y = out if out is not None else torch.empty((B, L), dtype=torch.float32, device=x.device)
    zf = torch.empty((B, S, 2), dtype=torch.float64, device=x.device) if return_state else None
    nbytes = _work_bytes("syg_sosfilt_work_bytes", B, L, S,
                         error=SygnalsHipError(f"sosfilt: unsupported configuration (B={B}, L={L}, sections={S})"))
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device) if L > sosfilt_constants()["chunk"] else None
    _call("syg_sosfilt_f32", _ptr(x), B, L, _ld(x), sos.ctypes.data_as(C.c_void_p), S, _ptr(zi), _ptr(y), _ld(y), _ptr(zf),
          _ptr(work))
    return (y, zf) if return_state else y


def detrend_code(detrend) -> int:
    """scipy's detrend argument -> the C ABI's code: 0 none (False / None / 'none'), 1 'constant' (True), 2 'linear'."""
    if detrend in (False, None, "none", 0):
        return 0
    if detrend in (True, "constant", 1):
        return 1
    if detrend in ("linear", 2):
        return 2
    raise ValueError("Trend type must be 'linear' or 'constant'.")     # scipy.signal.detrend's message


def welch(x: torch.Tensor, nperseg: int, noverlap: int, nfft: int, window_host: np.ndarray, detrend,
          scale: float) -> torch.Tensor:
    """Welch PSD [B, 1 + nfft/2] of x [B, L]; detrend as scipy.signal.welch (False / 'constant' / 'linear')."""
    require_gpu()
    if x.stride(1) != 1:
        x = x.contiguous()
    B, L = x.shape
    if not (is_pow2(nfft) and 8 <= nfft <= 16384):
        return welch_rows(x, nperseg, noverlap, nfft, window_host, detrend, scale)
    win = _dev(np.asarray(window_host, dtype=np.float32))
    work = _workspace("syg_welch_work_bytes", B, nfft, dtype=torch.float32, device=x.device)
    out = torch.empty((B, nfft // 2 + 1), dtype=torch.float32, device=x.device)
    _call("syg_welch_f32", _ptr(x), B, L, _ld(x), nperseg, nperseg - noverlap, nfft, _ptr(win), _ptr(twiddle_rfft_dev(nfft)),
          detrend_code(detrend), float(scale), _ptr(out), _ptr(work))
    return out


def welch_rows(x: torch.Tensor, nperseg: int, noverlap: int, nfft: int, window_host: np.ndarray, detrend,
               scale: float) -> torch.Tensor:
    """Welch for ANY nperseg / nfft (scipy.signal.welch takes any): segments as overlapping rows -> detrend + window
    (syg_pack_rows_f32) -> arbitrary-length FFT -> one-sided |X|^2 -> float64 average in segment order."""
    B, L = x.shape
    step = nperseg - noverlap
    nseg = (L - noverlap) // step
    if nseg < 1:
        raise ValueError("welch: the signal is shorter than one segment")
    win = _dev(np.asarray(window_host, dtype=np.float32))
    F = nfft // 2 + 1
    out = torch.empty((B, F), dtype=torch.float32, device=x.device)
    acc = torch.empty(F, dtype=torch.float64, device=x.device)
    x = x.contiguous()
    for b in range(B):
        for s0, sc in _row_blocks(nseg):
            X = fft_any(pack_frames(x[b:b + 1], sc, nperseg, step, s0, nfft, window=win, detrend=detrend))
            P = torch.empty((sc, F), dtype=torch.float32, device=x.device)
            _call("syg_psd_onesided_f32", _ptr(X), sc, nfft, float(scale), _ptr(P))
            _call("syg_col_mean_f32", _ptr(P), sc, F, _ptr(acc), int(s0 == 0), int(s0 + sc == nseg), float(nseg),
                  _ptr(out[b]))
    return out


# ------------------------------------------------------------------ cross-spectral analysis, generalised cross-correlation
CSD_WANTS = ("pxy", "pxx", "pyy", "coherence")
CSD_MAX_FUSED = 8192                 # longest nfft of the fused cross-spectrum kernel (two ping-pong buffers: 128 KiB)
GCC_WEIGHTINGS = ("none", "phat")


def _pair_rows(x, y, who: str, same_len: bool = False):
    """x [B, L] and y [1 or B, L] float32 device tensors with unit stride along L (made so where they are not)"""
    for t, name in ((x, "x"), (y, "y")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{who}: {name} must be a [rows, samples] float32 device tensor")
        if t.is_complex():
            raise ValueError(f"{who}: complex input is not served: {name} must be real (float32)")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: {name} must be float32, got {t.dtype}")
        if t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{who}: {name} is empty (shape {tuple(t.shape)}); at least one row of one sample is needed")
    if y.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"{who}: y must have one row (a reference channel) or one row per row of x ({x.shape[0]}), "
                         f"got {y.shape[0]}")
    if same_len and x.shape[1] != y.shape[1]:
        raise ValueError(f"{who}: rows of unequal length are not served: x has {x.shape[1]} samples and y {y.shape[1]} "
                         "(scipy zero-pads the shorter one; here the caller does)")
    _on_device(x, f"{who}: x")
    _on_device(y, f"{who}: y")
    return _unit_stride(x), _unit_stride(y)


def csd_fused_takes(nfft: int) -> bool:
    return is_pow2(nfft) and 8 <= nfft <= CSD_MAX_FUSED


def cross_spectrum(x: torch.Tensor, y: torch.Tensor, nperseg: int, noverlap: int, nfft: int, window_host: np.ndarray, detrend,
                   scale: float, want=CSD_WANTS) -> dict:
    """Segment-averaged one-sided spectra of the row pairs (x[b], y[b]) of [B, L] float32 device tensors (y: B rows or one
    reference row, never expanded): the requested ones of pxy [B, F, 2] = mean conj(X) Y, pxx, pyy and coherence [B, F],
    scipy.signal.csd's rules (welch's).  One fused launch for nfft a power of two in [8, 8192]; packed rows and the
    arbitrary-length FFT for every other nperseg >= 1 and nfft >= nperseg."""
    want = tuple(want)
    if not want or any(w not in CSD_WANTS for w in want):
        raise ValueError(f"cross_spectrum: want must name some of {CSD_WANTS}, got {want}")
    x, y = _pair_rows(x, y, "cross_spectrum", same_len=True)
    B, L = x.shape
    step = nperseg - noverlap
    if not (1 <= nperseg <= nfft and 1 <= step <= nperseg):
        raise ValueError("cross_spectrum: need 1 <= nperseg <= nfft and 0 <= noverlap < nperseg")
    nseg = (L - noverlap) // step
    if L < nperseg or nseg < 1:
        raise ValueError("cross_spectrum: the signal is shorter than one segment")
    F = nfft // 2 + 1
    dcode = detrend_code(detrend)
    out = {k: torch.empty((B, F, 2) if k == "pxy" else (B, F), dtype=torch.float32, device=x.device) for k in want}
    win = _dev(np.asarray(window_host, dtype=np.float32))
    if csd_fused_takes(nfft):
        for b0, bc in _row_blocks(B):
            xs, ys = x[b0:b0 + bc], (y if y.shape[0] == 1 else y[b0:b0 + bc])
            work = _workspace("syg_csd_work_bytes", bc, nseg, nfft, dtype=torch.float64, device=x.device)
            _call("syg_csd_f32", _ptr(xs), _ptr(ys), bc, ys.shape[0], L, _ld(xs), _ld(ys), nperseg, step, nfft, _ptr(win),
                  _ptr(twiddle_dev(nfft)), dcode, float(scale), *(_ptr(out[k][b0:b0 + bc]) if k in out else None for k in CSD_WANTS),
                  _ptr(work))
        return out
    acc = torch.empty((4, F), dtype=torch.float64, device=x.device)
    one_y = y.shape[0] == 1 and nseg <= MAX_ROWS           # the reference row's spectra: once for every x row
    Yc = None
    for b in range(B):
        for s0, sc in _row_blocks(nseg):
            X = fft_any(pack_frames(x[b:b + 1], sc, nperseg, step, s0, nfft, window=win, detrend=detrend))
            if Yc is None or not one_y:
                yb = y if y.shape[0] == 1 else y[b:b + 1]
                Yc = fft_any(pack_frames(yb, sc, nperseg, step, s0, nfft, window=win, detrend=detrend))
            _call("syg_csd_rows_f32", _ptr(X), _ptr(Yc), sc, nfft, _ptr(acc), int(s0 == 0), int(s0 + sc == nseg), nseg,
                  float(scale), *(_ptr(out[k][b]) if k in out else None for k in CSD_WANTS))
    return out


def gcc_fft_len(Lx: int, Ly: int) -> int:
    return conv_fft_len(Lx + Ly - 1)


def gcc(x: torch.Tensor, y: torch.Tensor, max_lag: int, weighting: str = "none") -> torch.Tensor:
    """r [B, 2 max_lag + 1]: r[:, max_lag + t] = irfft(W X conj(Y), n)[t mod n] for the lags t = -max_lag .. max_lag of the
    rows of x [B, Lx] against y [1 or B, Ly]; n = conv_fft_len(Lx + Ly - 1); W = 1 ("none") or 1 / |X conj(Y)| ("phat").
    scipy.signal.correlate's sign: x[n] = y[n - d] peaks at lag +d.  Plain real-input transforms (true bins), the
    weighting kernel, the inverse transform and the lag crop, all on the device."""
    if weighting not in GCC_WEIGHTINGS:
        raise ValueError(f"gcc: weighting {weighting!r} is not served (served: {', '.join(GCC_WEIGHTINGS)})")
    x, y = _pair_rows(x, y, "gcc")
    B, Lx = x.shape
    By, Ly = y.shape
    if not (0 <= max_lag <= min(Lx, Ly) - 1):
        raise ValueError(f"gcc: max_lag = {max_lag} is outside 0 ... min(Lx, Ly) - 1 = {min(Lx, Ly) - 1}")
    n = gcc_fft_len(Lx, Ly)
    W = 2 * max_lag + 1
    out = torch.empty((B, W), dtype=torch.float32, device=x.device)
    Y = fft_any(pack_rows(y, n, cplx=True)) if By == 1 else None
    for b0, bc in _row_blocks(B):
        X = fft_any(pack_rows(x[b0:b0 + bc], n, cplx=True))
        Yb = Y if By == 1 else fft_any(pack_rows(y[b0:b0 + bc], n, cplx=True))
        _call("syg_gcc_weight_c64", _ptr(X), _ptr(Yb), bc, Yb.shape[0], n, int(weighting == "phat"), _ptr(X))
        c = fft_any(X, True)
        _call("syg_gcc_crop_f32", _ptr(c), bc, n, max_lag, _ptr(out[b0:b0 + bc]))
    return out


def peak_pick(r: torch.Tensor, lag0: int, fs: float = 1.0):
    """Per row of r [B, W] (float32, device): (delay float64 [B], lag int64 [B], peak float64 [B]) of the first maximum,
    refined by the parabola through its neighbours where it is interior and the parabola opens downwards; the lag of
    column i is lag0 + i, delay = (lag + shift) / fs."""
    r = _f32_in(r, "peak_pick: r", 2)
    B, W = r.shape
    if B < 1 or W < 1:
        raise ValueError("peak_pick: empty input")
    if not (fs > 0 and np.isfinite(fs)):
        raise ValueError(f"peak_pick: fs must be positive and finite, got {fs}")
    delay = torch.empty(B, dtype=torch.float64, device=r.device)
    lag = torch.empty(B, dtype=torch.int64, device=r.device)
    peak = torch.empty(B, dtype=torch.float64, device=r.device)
    _call("syg_peak_pick_f32", _ptr(r), B, W, _ld(r), int(lag0), float(fs), _ptr(delay), _ptr(lag), _ptr(peak))
    return delay, lag, peak


def contrast_db(pv: torch.Tensor, amin: float = 1e-10, top_db: Optional[float] = 80.0, linear: bool = False) -> torch.Tensor:
    """pv [B, 2, R, T] (peak, valley means) -> spectral contrast [B, R, T]: dB difference, or the plain difference
    of the means with linear=True (librosa's `linear` option)."""
    if linear:
        amin = 0.0
    require_gpu()
    pv = pv.contiguous()
    B, two, R, Tn = pv.shape
    out = torch.empty((B, R, Tn), dtype=torch.float32, device=pv.device)
    _call("syg_contrast_db_f32", _ptr(pv), B, R, Tn, float(amin), float(top_db) if top_db is not None else -1.0, _ptr(out))
    return out


# ------------------------------------------------------------------ arbitrary-length FFT
FFT_REAL_IN, FFT_ABS_OUT, FFT_PAIR_IN = 1, 2, 4          # the fused ends: SYG_FFT_* of include/sygnals_hip.h


def _fft_strided(kind, x, out, outer, batch, n, inverse, strides, bign=0, scale=1.0, flags=0, mask_n=0, in_valid=0):
    """One launch of the strided transform of engine `kind` ("pow2" / "mixed"): the _ex_ entry where a fused end is asked
    for, the _c2c_ entry otherwise."""
    args = (_ptr(x), _ptr(out), outer, batch, n, int(inverse), _ptr(twiddle_dev(n)), *strides, bign, float(scale))
    if flags or mask_n or in_valid:
        _call("syg_fft_%s_strided_ex_f32" % kind, *args, int(flags), int(mask_n), int(in_valid))
    else:
        _call("syg_fft_%s_strided_c2c_f32" % kind, *args)


def _run_plan(plan, x, out, rows, inverse, scale=1.0, ld=None, flags=0, mask_n=0, in_valid=0):
    """Runs fft_plan's (kind, n1, n2) on `rows` rows of x into out: one launch, or the four-step passes A and B through a
    temporary.  The fused ends: FFT_REAL_IN / FFT_PAIR_IN (with in_valid) and mask_n act where x is loaded, FFT_ABS_OUT
    where out is stored; ld is the row stride of x (default n; in floats for a pair input)."""
    kind, n1, n2 = plan
    n = n1 * n2
    ld = n if ld is None else ld
    if n2 == 1 and not (flags or mask_n or in_valid):
        _fft_strided(kind, x, out, 1, rows, n, inverse, (0, n, 1, 0, n, 1), scale=scale)
    elif n2 == 1:
        # (one transform per row: the ROW is the outer index, so that an element's position inside the row is its bin)
        _fft_strided(kind, x, out, rows, 1, n, inverse, (ld, 0, 1, n, 0, 1), scale=scale, flags=flags, mask_n=mask_n,
                     in_valid=in_valid)
    else:
        tmp = torch.empty((rows, n, 2), dtype=torch.float32, device=x.device)
        # pass A: n2 transforms of length n1 over the slow index (input stride n2), twiddle W_n^(i2 k1), stored [i2][k1];
        # pass B: n1 transforms of length n2 over i2 (input stride n1), output X[k1 + n1 k2]
        _fft_strided(kind, x, tmp, rows, n2, n1, inverse, (ld, 1, n2, n, n1, 1), bign=n, flags=flags & ~FFT_ABS_OUT,
                     mask_n=mask_n, in_valid=in_valid)
        _fft_strided(kind, tmp, out, rows, n1, n2, inverse, (n, 1, n1, n, 1, n1), scale=scale, flags=flags & FFT_ABS_OUT)
    return out


def _fft_direct(x: torch.Tensor, inverse: bool, plan) -> torch.Tensor:
    """The plain complex transform of the rows of x [rows, n, 2] by its plan."""
    rows, n, _ = x.shape
    if plan is None:
        raise SygnalsHipError(f"FFT length {n} exceeds the supported maximum 2^26")
    if plan[2] == 1 and plan[0] == "pow2":
        return fft_pow2(x, inverse)                 # (contiguous rows: the kernel without strides)
    if plan[2] > 1 and rows > MAX_ROWS:
        raise SygnalsHipError("too many rows for the four-step FFT")
    x = x.contiguous()
    return _run_plan(plan, x, torch.empty_like(x), rows, inverse, scale=(1.0 / n if inverse else 1.0))


def fft_pow2_any(x: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Complex FFT of rows of x [rows, n, 2], n any power of two up to 2^26 (four-step above 8192)."""
    return _fft_direct(x, inverse, fft_plan(x.shape[1]))


def cmul(a: torch.Tensor, b: torch.Tensor, conj_b: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a [.., na, 2] * b [nb, 2] broadcast over i mod nb."""
    a = a.contiguous(); b = b.contiguous()
    out = torch.empty_like(a) if out is None else out
    _call("syg_cmul_c64", _ptr(a), _ptr(b), _ptr(out), a.numel() // 2, b.numel() // 2, int(conj_b))
    return out


def pack_real(x: torch.Tensor, n: int, window: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Real rows [rows, len] -> complex rows [rows, n, 2], windowed, zero-padded / truncated to n."""
    if x.stride(1) != 1:
        x = x.contiguous()
    rows, ln = x.shape
    out = torch.empty((rows, n, 2), dtype=torch.float32, device=x.device)
    _call("syg_pack_real_c64", _ptr(x), rows, ln, _ld(x), _ptr(window), _ptr(out), n)
    return out


def _bluestein_tables(n: int):
    """Host float64 tables for the chirp-z form of an n-point DFT, forward and inverse.

    w[k] = exp(-i*pi*k^2/n); forward: X = w * IFFT_M(FFT_M(x*w) * FFT_M(wrap(conj w)));
    the inverse uses the conjugate chirp and folds the 1/n into the final multiply.
    """
    m = next_direct_len(max(2, 2 * n - 1))     # any length the FFT kernels take directly will do for the chirp convolution
    k = np.arange(n, dtype=np.int64)
    w = np.exp(-1j * np.pi * ((k * k) % (2 * n)).astype(np.float64) / n)

    def wrapped_fft(c):
        b = np.zeros(m, dtype=np.complex128)
        b[:n] = c
        b[m - n + 1:] = c[1:][::-1]
        return np.fft.fft(b)

    as2 = lambda z: _dev(np.stack([z.real, z.imag], axis=-1).astype(np.float32))
    fwd = (as2(w), as2(wrapped_fft(np.conj(w))), as2(w))
    inv = (as2(np.conj(w)), as2(wrapped_fft(w)), as2(np.conj(w) / n))
    return m, fwd, inv


def fft_smooth(x: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Complex FFT of rows of x [rows, n, 2] for n = 2^a 3^b 5^c 7^d: one mixed-radix launch up to 8192 points,
    four-step (two passes of mixed-radix transforms) above."""
    split = smooth_split(x.shape[1])
    if split is None:
        raise SygnalsHipError(f"fft_smooth: n = {x.shape[1]} is not a product of 2, 3, 5, 7 that splits into factors <= 8192")
    return _fft_direct(x, inverse, ("mixed",) + split)


def fft_any(x: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Complex FFT / IFFT of rows of x [rows, n, 2] for ANY n >= 1: LDS / four-step kernels for powers of two, the
    mixed-radix kernel for other products of 2, 3, 5, 7 (48000, 44100, 16000 ...), Bluestein for the rest."""
    require_gpu()
    rows, n, _ = x.shape
    if n == 1:
        return x.clone()
    if rows > MAX_ROWS and n > MAX_LDS_FFT:
        # the four-step passes put the rows on a grid axis of at most 65535: long transforms of very many rows go
        # through in blocks (without this a Bluestein length above 8192 would recurse on the same row count)
        out = torch.empty_like(x)
        for r0, rc in _row_blocks(rows):
            out[r0:r0 + rc] = fft_any(x[r0:r0 + rc], inverse)
        return out
    plan = fft_plan(n)
    if plan is not None or is_pow2(n):           # (a power of two without a plan is too long: _fft_direct says so)
        return _fft_direct(x, inverse, plan)
    m, fwd, inv = _cached(("blue", n), lambda: _bluestein_tables(n))
    w_in, bf, w_out = inv if inverse else fwd
    a = torch.zeros((rows, m, 2), dtype=torch.float32, device=x.device)
    a[:, :n].copy_(cmul(x, w_in))                 # zero-padded copy (data movement)
    A = fft_any(a, False)
    cmul(A, bf, out=A)
    c = fft_any(A, True)
    return cmul(c[:, :n].contiguous(), w_out)


# ------------------------------------------------------------------ feature formatting for ML
def _mat32(x: torch.Tensor) -> torch.Tensor:
    return _f32_in(x, "x", 2).contiguous()


def col_stats(x: torch.Tensor) -> torch.Tensor:
    """[5, F] float64: count of non-NaN, mean, population variance, min, max of every column of x [n, F]."""
    x = _mat32(x)
    n, F = x.shape
    out = torch.empty((5, F), dtype=torch.float64, device=x.device)
    _call("syg_col_stats_f32", _ptr(x), n, F, _ptr(out))
    return out


def affine_cols(x: torch.Tensor, sub, mul, add) -> torch.Tensor:
    """(x - sub[c]) * mul[c] + add[c] per column, float64 arithmetic; sub / mul / add: length-F float64 (host or device)."""
    x = _mat32(x)
    n, F = x.shape
    vecs = [torch.as_tensor(np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64)).to(x.device)
            for v in (sub, mul, add)]
    if any(v.shape != (F,) for v in vecs):
        raise ValueError(f"sub / mul / add must have length {F}")
    out = torch.empty_like(x)
    _call("syg_affine_cols_f32", _ptr(x), n, F, _ptr(vecs[0]), _ptr(vecs[1]), _ptr(vecs[2]), _ptr(out))
    return out


def col_quantiles(x: torch.Tensor, q) -> torch.Tensor:
    """np.nanpercentile(x, 100 * q, axis=0) -> [len(q), F] float64 (q: fractions in [0, 1]); at most 32768 rows."""
    x = _mat32(x)
    n, F = x.shape
    qv = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qv.ndim != 1 or qv.size < 1 or (qv < 0).any() or (qv > 1).any():
        raise ValueError("q must be fractions in [0, 1]")
    qd = torch.from_numpy(qv).to(x.device)
    out = torch.empty((qv.size, F), dtype=torch.float64, device=x.device)
    _call("syg_col_quantiles_f32", _ptr(x), n, F, _ptr(qd), int(qv.size), _ptr(out))
    return out


def zoom2d(img: torch.Tensor, out_shape, order: int = 1) -> torch.Tensor:
    """scipy.ndimage.zoom(img, out_shape / img.shape, order=0|1, mode='nearest') of a [H, W] float32 device tensor."""
    img = _mat32(img)
    H, W = img.shape
    H2, W2 = int(out_shape[0]), int(out_shape[1])
    out = torch.empty((H2, W2), dtype=torch.float32, device=img.device)
    _call("syg_zoom_f32", _ptr(img), H, W, H2, W2, int(order), _ptr(out))
    return out


# ------------------------------------------------------------------ batched ingest
_PCM_BITS = {torch.int16: 16, torch.int32: 32, torch.uint8: 8}


def pcm_to_f32(pcm: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Integer PCM [B, L] or [B, L, C] (int16 / int32 / uint8, interleaved channels, on the device) -> float32 mono
    clips [B, L]: samples / 2^(bits-1), channels averaged (librosa.load(mono=True) semantics)."""
    require_gpu()
    if pcm.dtype not in _PCM_BITS or pcm.dim() not in (2, 3) or not pcm.is_cuda:
        raise ValueError("pcm must be an int16 / int32 / uint8 device tensor of shape [B, L] or [B, L, C]")
    pcm = pcm.contiguous()
    B, L = pcm.shape[0], pcm.shape[1]
    Cn = pcm.shape[2] if pcm.dim() == 3 else 1
    if out is None:
        out = torch.empty((B, L), dtype=torch.float32, device=pcm.device)
    elif out.shape != (B, L) or out.dtype != torch.float32 or out.stride(1) != 1:
        raise ValueError("out must be a float32 [B, L] tensor with unit inner stride")
    _call("syg_pcm_to_f32", _ptr(pcm), _PCM_BITS[pcm.dtype], B, L, Cn, L * Cn, _ptr(out), _ld(out))
    return out


# ------------------------------------------------------------------ FFT-backed 1-D operations
def pack_rows(x: torch.Tensor, n: int, window: Optional[torch.Tensor] = None, detrend=False,
              reverse: bool = False, cplx: bool = False) -> torch.Tensor:
    """Rows of x [rows, len] -> [rows, n] real (or [rows, n, 2] complex) rows: mean ('constant') or least-squares
    line ('linear') removed, windowed, optionally time-reversed, zero-padded / truncated to n."""
    x = _f32_in(x, "x", 2)
    rows, ln = x.shape
    out = torch.empty((rows, n, 2) if cplx else (rows, n), dtype=torch.float32, device=x.device)
    dcode = detrend_code(detrend)
    work = _workspace("syg_pack_rows_work_bytes", rows, dtype=torch.float64, device=x.device) if dcode else None
    _call("syg_pack_rows_f32", _ptr(x), rows, ln, _ld(x), _ptr(window), dcode, int(bool(reverse)), int(bool(cplx)),
          _ptr(out), n, _ptr(work))
    return out


def rfft_conv(x: torch.Tensor, k: torch.Tensor, reverse_k: bool = False) -> torch.Tensor:
    """Full linear convolution of the rows of x [B, n] with k [1 or B, m] -> [B, n + m - 1] (a view of the
    transform buffer).  reverse_k convolves with the time-reversed k, i.e. cross-correlates."""
    B, n = x.shape
    Bk, m = k.shape
    if Bk not in (1, B):
        raise ValueError("k must have one row or one row per row of x")
    M = conv_fft_len(n + m - 1)
    H = M // 2
    za = fft_pair_rows(x, H)
    if za is None:
        za = fft_any(pack_rows(x, M).view(B, H, 2))
    zb = fft_any(pack_rows(k, M, reverse=reverse_k).view(Bk, H, 2))
    _call("syg_rconv_spectrum_c64", _ptr(za), _ptr(zb), B, Bk, H, _ptr(za))
    return fft_any(za, True).view(B, M)[:, : n + m - 1]


def fft_pair_rows(x: torch.Tensor, H: int):
    """Forward transform of length H of the rows of the REAL tensor x [B, n] read as the complex sequences
    (x[2 p], x[2 p + 1]), zero beyond n -- pack_rows(x, 2 H) folded into the first pass's load.  None without a plan."""
    B, n = x.shape
    plan = fft_plan(H)
    if plan is None or B > MAX_ROWS or x.dtype != torch.float32 or not x.is_cuda or n > 2 * H:
        return None
    if x.stride(1) != 1:
        x = x.contiguous()
    out = torch.empty((B, H, 2), dtype=torch.float32, device=x.device)
    return _run_plan(plan, x, out, B, False, ld=x.stride(0), flags=FFT_PAIR_IN, in_valid=n)


def analytic_fused(x: torch.Tensor, magnitude: bool):
    """scipy.signal.hilbert of the rows of x [B, n] (float32, contiguous) with the packing, masking and |.| passes folded
    into the transforms' loads and stores: complex [B, n, 2], or the envelope [B, n] when magnitude.  Returns None where
    the length has no plan (powers of two up to 2^26 and 7-smooth lengths that split into two factors <= 8192 have one;
    other lengths go through Bluestein in analytic_signal)."""
    B, n = x.shape
    plan = fft_plan(n)
    if plan is None or B > MAX_ROWS:
        return None
    x = x.contiguous()
    X = torch.empty((B, n, 2), dtype=torch.float32, device=x.device)
    out = torch.empty((B, n) if magnitude else (B, n, 2), dtype=torch.float32, device=x.device)
    # forward: the load reads the REAL rows; inverse: the load weights the spectrum, the store takes |.|
    _run_plan(plan, x, X, B, False, flags=FFT_REAL_IN)
    return _run_plan(plan, X, out, B, True, scale=1.0 / n, flags=FFT_ABS_OUT if magnitude else 0, mask_n=n)


def analytic_signal(x: torch.Tensor) -> torch.Tensor:
    """scipy.signal.hilbert of the rows of x [B, n] -> complex [B, n, 2] (exact length-n transforms)."""
    B, n = x.shape
    if x.dtype == torch.float32 and x.is_cuda:
        fused = analytic_fused(x, False)
        if fused is not None:
            return fused
    X = fft_any(pack_rows(x, n, cplx=True))
    _call("syg_analytic_mask_c64", _ptr(X), B, n)
    return fft_any(X, True)


def periodogram(x: torch.Tensor, nfft: int, window_host: Optional[np.ndarray], detrend, scale: float
                ) -> torch.Tensor:
    """One-sided periodogram [B, nfft//2 + 1] of the first min(len, nfft) samples of the rows of x."""
    B = x.shape[0]
    win = None if window_host is None else _dev(np.asarray(window_host, dtype=np.float32))
    X = fft_any(pack_rows(x, nfft, window=win, detrend=detrend, cplx=True))
    out = torch.empty((B, nfft // 2 + 1), dtype=torch.float32, device=x.device)
    _call("syg_psd_onesided_f32", _ptr(X), B, nfft, float(scale), _ptr(out))
    return out


# ------------------------------------------------------------------ constant-Q transform
_side_streams: dict = {}


def _side_stream(device) -> "torch.cuda.Stream":
    """One extra HIP stream per device for work that runs beside the caller's stream (CQT octave products)."""
    k = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    st = _side_streams.get(k)
    if st is None:
        st = torch.cuda.Stream(device=k)
        _side_streams[k] = st
    return st


def cqt_pack_gemm(basis: np.ndarray, n_fft: int) -> np.ndarray:
    """A operands of syg_cqt_octave_gemm_f32 for one octave: the frequency-domain rows basis [n_filt, 1 + n_fft/2]
    (complex) act on rfft(frame); the same linear map in the time domain is out[f] = sum_n frame[n] g_f[n] with
    g_f[n] = sum_k basis[f, k] exp(-2 pi i k n / n_fft) (float64 here).  Rows 2f / 2f + 1 of G^T hold Re / Im of g_f;
    packed [row tile][n_fft/16][4][64] float32 with entry (mt, s, u, lane) = G[16 s + 4 (lane >> 4) + u][16 mt + lane % 16]."""
    basis = np.asarray(basis, dtype=np.complex128)
    nf, F = basis.shape
    k = np.arange(F)[:, None]
    n = np.arange(n_fft)[None, :]
    g = basis @ np.exp(-2j * np.pi * ((k * n) % n_fft) / n_fft)            # [nf, n_fft]
    ntile = (2 * nf + 15) // 16
    G = np.zeros((n_fft, 16 * ntile), dtype=np.float64)
    G[:, 0:2 * nf:2] = g.real.T
    G[:, 1:2 * nf:2] = g.imag.T
    lane = np.arange(64)
    S = n_fft // 16
    out = np.empty((ntile, S, 4, 64), dtype=np.float32)
    for mt in range(ntile):
        for s in range(S):
            for u in range(4):
                out[mt, s, u] = G[16 * s + 4 * (lane >> 4) + u, 16 * mt + (lane & 15)]
    return np.ascontiguousarray(out)


def _bf16_rne(x32: np.ndarray) -> np.ndarray:
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even (what v_cvt_pk_bf16_f32 does)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def cqt_pack_bf16x3(basis: np.ndarray, n_fft: int, row_tiles: Optional[int] = None) -> np.ndarray:
    """Operand table of syg_cqt_octave_bf16x3_f32: float32(G) (cqt_pack_gemm's matrix) split into three bfloat16 terms
    hi + mid + lo (hi = bf16(g), mid = bf16(g - hi), lo = bf16(g - hi - mid); the two differences are exact in
    float32), packed uint16 [3][row tile][n_fft / 32][64 lanes][8]: entry (p, mt, s, lane, j) = term p of
    G[32 s + 8 (lane >> 4) + j][16 mt + (lane & 15)].  Row tiles: (2 n_filt + 15) // 16 -- ONE for eight filters or
    fewer, which is what the level-by-level kernels index -- or `row_tiles` if that is more (the added tiles are zero)."""
    basis = np.asarray(basis, dtype=np.complex128)
    nf, F = basis.shape
    k = np.arange(F)[:, None]
    n = np.arange(n_fft)[None, :]
    g = basis @ np.exp(-2j * np.pi * ((k * n) % n_fft) / n_fft)
    ntile = max((2 * nf + 15) // 16, int(row_tiles or 0))
    G = np.zeros((n_fft, 16 * ntile), dtype=np.float32)
    G[:, 0:2 * nf:2] = g.real.T
    G[:, 1:2 * nf:2] = g.imag.T

    def f32_of(b16):
        return (b16.astype(np.uint32) << 16).view(np.float32)
    hi = _bf16_rne(G)
    r1 = G - f32_of(hi)
    mid = _bf16_rne(r1)
    lo = _bf16_rne(r1 - f32_of(mid))
    lane = np.arange(64)
    S = n_fft // 32
    out = np.empty((3, ntile, S, 64, 8), dtype=np.uint16)
    for p, term in enumerate((hi, mid, lo)):
        for mt in range(ntile):
            for s_ in range(S):
                for j in range(8):
                    out[p, mt, s_, :, j] = term[32 * s_ + 8 * (lane >> 4) + j, 16 * mt + (lane & 15)]
    return np.ascontiguousarray(out)


def cqt_fused_table(basis: np.ndarray) -> np.ndarray:
    """Operand table of syg_cqt_fused_f32 for the octaves' common basis [n_filt <= 16, 129]: cqt_pack_bf16x3 at frame length
    256 with ALWAYS two row tiles, uint16 [3][2][8][64][8] -- the kernel's waves index it as [term][tile][step][lane]
    whatever n_filt is (the second tile is zero for eight filters or fewer; its rows are never stored)."""
    tab = cqt_pack_bf16x3(basis, 256, row_tiles=2)
    assert tab.shape == (3, 2, 8, 64, 8), tab.shape
    return tab


def decimate2(x: torch.Tensor, taps: torch.Tensor, scale: float) -> torch.Tensor:
    """FIR decimation by two of x [B, L] -> [B, ceil(L/2)] (zero padded ends)."""
    require_gpu()
    if x.stride(1) != 1:
        x = x.contiguous()
    B, L = x.shape
    y = torch.empty((B, (L + 1) // 2), dtype=torch.float32, device=x.device)
    _call("syg_decimate2_f32", _ptr(x), B, L, _ld(x), _ptr(taps), taps.numel(), float(scale), _ptr(y), _ld(y))
    return y


def decimate2_chain(x: torch.Tensor, taps: torch.Tensor, scale: float, levels: int, keep=None) -> list:
    """`levels` successive decimate2 steps; up to 4 at a time go through one pass of syg_decimate2_chain_f32 (identical
    bits, every level written once).  keep[s] False: level s is not wanted (returned as None; never the last one)."""
    require_gpu()
    if x.stride(1) != 1:
        x = x.contiguous()
    keep = [True] * levels if keep is None else list(keep)
    keep[-1] = True
    out = []
    cur = x
    s = 0
    while s < levels:
        n = levels - s if levels - s <= 4 else 3        # three levels per pass; a remainder of four goes in one
        B, L = cur.shape
        ys, lens = [], L
        for j in range(n):
            lens = (lens + 1) // 2
            # (a level that feeds the next pass is needed even when the caller does not want it)
            need = keep[s + j] or j == n - 1
            ys.append(torch.empty((B, lens), dtype=torch.float32, device=x.device) if need else None)
        yp = (C.c_void_p * n)(*[(_ptr(t) if t is not None else None) for t in ys])
        ld = (C.c_int64 * n)(*[(_ld(t) if t is not None else 0) for t in ys])
        _call("syg_decimate2_chain_f32", _ptr(cur), B, L, _ld(cur), _ptr(taps), taps.numel(), float(scale), n, yp, ld)
        out += [t if keep[s + j] else None for j, t in enumerate(ys)]
        cur = ys[-1]
        s += n
    return out


def cqt(y: torch.Tensor, sr: float, hop_length: int = 512, fmin=None, n_bins: int = 84, bins_per_octave: int = 12,
        tuning: float = 0.0, filter_scale: float = 1.0, sparsity: float = 0.01) -> torch.Tensor:
    """Constant-Q transform of y [B, L] -> complex [B, n_bins, T, 2] float32, T = 1 + L // hop_length.
    Every octave runs on the entry point _cqt.cqt_route names: frame lengths 128 / 256 with <= 16 filters on the bfloat16-split
    matrix form (or, for the usual shape, the whole transform in one launch), 128 / 256 / 512 with <= 64 filters on the fp32
    matrix form, anything else up to frame length 1024 on rfft x sparse rows in groups of 24 filters; a combination of
    bins_per_octave and filter_scale whose octaves need a longer frame raises ValueError before anything is launched."""
    from ._cqt import CqtPlan, RFFT_MAXFILT, bf16x3_takes, cqt_route, decimation_taps, gemm_takes
    require_gpu()
    key = ("cqt", float(sr), int(hop_length), None if fmin is None else float(fmin), int(n_bins), int(bins_per_octave),
           float(tuning), float(filter_scale), float(sparsity))

    def build():
        p = CqtPlan(sr, hop_length, fmin, n_bins, bins_per_octave, tuning, filter_scale, sparsity)
        cqt_route(p, "fft", False)      # an octave frame no kernel takes (> 1024 samples) is refused here, in every mode
        for o in p.octaves:
            b = o["basis"]
            b32 = np.stack([b.real, b.imag], axis=-1).astype(np.float32)
            o["basis_dev"] = _dev(b32)
            nz = (b32[..., 0] != 0) | (b32[..., 1] != 0)          # librosa's sparsified basis: a short run per row
            k0 = np.array([int(np.argmax(r)) if r.any() else 0 for r in nz], dtype=np.int32)
            k1 = np.array([int(len(r) - np.argmax(r[::-1])) if r.any() else 0 for r in nz], dtype=np.int32)
            hull = np.ascontiguousarray(np.concatenate([k0, k1 - k0]).astype(np.int32))
            # syg_cqt_octave_f32 takes RFFT_MAXFILT filters a call: (first filter, count, hull of the group)
            o["fft_groups"] = [(g, min(RFFT_MAXFILT, len(b) - g),
                                np.ascontiguousarray(hull.reshape(2, -1)[:, g:g + RFFT_MAXFILT].ravel()))
                               for g in range(0, len(b), RFFT_MAXFILT)]
            o["gpacked_dev"] = _dev(cqt_pack_gemm(b, o["n_fft"])) if gemm_takes(o["n_fft"], len(b)) else None
            o["gsplit_dev"] = (torch.from_numpy(cqt_pack_bf16x3(b, o["n_fft"]).view(np.int16)).to(require_gpu())
                               if bf16x3_takes(o["n_fft"], len(b)) else None)
        p.taps_dev = _dev(decimation_taps().astype(np.float32))
        # the one-launch form (syg_cqt_fused_f32) where the plan has its shape (CqtPlan.one_launch_shape): its table always
        # has two row tiles (cqt_fused_table), so eight filters or fewer do not share octave 0's one-tile table
        oc = p.octaves
        p.fused_tab_dev = None
        if p.one_launch_shape():
            p.fused_tab_dev = (oc[0]["gsplit_dev"] if oc[0]["n"] > 8 else
                               torch.from_numpy(cqt_fused_table(oc[0]["basis"]).view(np.int16)).to(require_gpu()))
            assert p.fused_tab_dev.numel() == 3 * 2 * 8 * 64 * 8
        p.row0 = np.ascontiguousarray([o["row0"] for o in oc], dtype=np.int32)
        p.routes = {}
        return p
    plan = _cached(key, build)
    # which entry point each octave runs on (_cqt.cqt_route: raises here, before any launch, for an octave nothing serves)
    rkey = (settings.cqt_mode, bool(settings.cqt_fused))
    if rkey not in plan.routes:
        plan.routes[rkey] = cqt_route(plan, *rkey)
    one_launch, route = plan.routes[rkey]
    if y.stride(1) != 1:
        y = y.contiguous()
    B, L = y.shape
    # output frames = the smallest centred frame count over the octaves (librosa's __trim_stack); this is
    # 1 + L // hop_length except when the rounded-up decimated lengths add a frame to every octave
    Lc = L
    for _ in range(plan.early):
        Lc = (Lc + 1) // 2
    Tn = None
    for o in plan.octaves:
        To = 1 + Lc // o["hop"]
        Tn = To if Tn is None else min(Tn, To)
        if o["decimate_after"]:
            Lc = (Lc + 1) // 2
    out = torch.empty((B, plan.n_bins, Tn, 2), dtype=torch.float32, device=y.device)      # every row is written
    s2 = float(np.sqrt(2.0))
    if one_launch:
        _call("syg_cqt_fused_f32", _ptr(y), B, L, _ld(y), _ptr(plan.taps_dev), plan.taps_dev.numel(), s2,
              _ptr(plan.fused_tab_dev), plan.octaves[0]["n"], len(plan.octaves), plan.row0.ctypes.data_as(C.c_void_p), Tn,
              _ptr(out), plan.n_bins * Tn)
        return out
    # octave kernel (route): "bf16x3" (default: the framed product with bfloat16-split operands, fp32-equivalent), "gemm"
    # (the single-instruction fp32 MFMA form), "fft" (rfft x sparse rows; also what other frame lengths take)
    # settings.cqt_streams = 2: the decimation chain (memory-bound) on the caller's stream, the octave products
    # (matrix-core bound, no LDS) on a side stream, so that octave i runs beside the decimation towards octave i + 1.
    # Measured on one 1-hour stream: 1.03 ms against 1.05 ms on one stream -- the two kernels slow each other down by
    # about what the overlap saves -- so one stream is the default.
    main = torch.cuda.current_stream()
    two = settings.cqt_streams == 2
    side = _side_stream(y.device) if two else main
    if two:
        side.wait_stream(main)                    # `out` and `y` are ready for the side stream
    # every decimation level up front (three levels per pass; settings.cqt_chain = False: one launch per level)
    n_dec = plan.early + sum(1 for o in plan.octaves[:-1] if o["decimate_after"])
    chain = settings.cqt_chain and not two and n_dec > 0
    levels = None
    if chain:
        keepl = [i >= plan.early - 1 for i in range(n_dec)]
        levels = [y] + decimate2_chain(y, plan.taps_dev, s2, n_dec, keepl)
    cur = y
    lvl = plan.early
    if chain:
        cur = levels[lvl]
    else:
        for _ in range(plan.early):
            cur = decimate2(cur, plan.taps_dev, s2)
    for oi, o in enumerate(plan.octaves):
        entry = route[oi][0]
        if entry is not None:
            if two:
                ev = torch.cuda.Event()
                ev.record(main)                   # `cur` has been produced on the main stream
                side.wait_event(ev)
                cur.record_stream(side)
            sp = C.c_void_p(side.cuda_stream)
            if entry == "syg_cqt_octave_bf16x3_f32":
                rc = lib().syg_cqt_octave_bf16x3_f32(_ptr(cur), B, cur.shape[1], _ld(cur), o["n_fft"], o["hop"], Tn,
                                                     _ptr(o["gsplit_dev"]), o["n"], _ptr(out), plan.n_bins * Tn, o["row0"], sp)
                check(rc, entry)
            elif entry == "syg_cqt_octave_gemm_f32":
                rc = lib().syg_cqt_octave_gemm_f32(_ptr(cur), B, cur.shape[1], _ld(cur), o["n_fft"], o["hop"], Tn,
                                                   _ptr(o["gpacked_dev"]), o["n"], _ptr(out), plan.n_bins * Tn, o["row0"], sp)
                check(rc, entry)
            else:
                for g0, ng, hull in o["fft_groups"]:
                    rc = lib().syg_cqt_octave_f32(_ptr(cur), B, cur.shape[1], _ld(cur), o["n_fft"], o["hop"], Tn,
                                                  _ptr(twiddle_rfft_dev(o["n_fft"])), _ptr(o["basis_dev"][g0:g0 + ng]), ng,
                                                  hull.ctypes.data_as(C.c_void_p), _ptr(out),
                                                  plan.n_bins * Tn, o["row0"] + g0, sp)
                    check(rc, entry)
        if o["decimate_after"] and oi + 1 < len(plan.octaves):
            lvl += 1
            cur = levels[lvl] if chain else decimate2(cur, plan.taps_dev, s2)
    if two:
        main.wait_stream(side)
    return out


# ------------------------------------------------------------------ pitch (yin / pyin)
def _pitch_setup(y, sr, fmin, fmax, frame_length, win_length, hop, center):
    from . import _pitch as P
    y = _f32_in(y, "y", 2)
    win_length = int(win_length) if win_length is not None else frame_length // 2
    hop = int(hop) if hop is not None else frame_length // 4
    if not (0 < fmin < fmax <= sr / 2):
        raise ValueError(f"pitch: need 0 < fmin < fmax <= sr / 2 (got fmin={fmin}, fmax={fmax}, sr={sr})")
    if not (0 < win_length < frame_length):
        raise ValueError(f"win_length={win_length} must be a positive integer less than frame_length={frame_length}")
    min_p, max_p = P.periods(sr, fmin, fmax, frame_length, win_length)
    B, L = y.shape
    Tn = _at_least_one(P.num_frames(L, frame_length, hop, center))
    return P, y, win_length, hop, min_p, max_p, B, L, Tn


def pitch_frames(y: torch.Tensor, sr: float, fmin: float, fmax: float, frame_length: int = 2048,
                 win_length: Optional[int] = None, hop: Optional[int] = None, center: bool = True, mode: str = "pyin",
                 trough_threshold: float = 0.1, want_cmndf: bool = False) -> dict:
    """Frame stage of yin / pyin on clips y [B, L] (syg_pitch_frames_f32): f0 (yin) or the pYIN candidate lists,
    plus the CMNDF [B, T, n_lag] when want_cmndf."""
    P, y, win_length, hop, min_p, max_p, B, L, Tn = _pitch_setup(y, sr, fmin, fmax, frame_length, win_length, hop, center)
    dev = y.device
    n_lag = max_p - min_p + 1
    n_bins = P.n_pitch_bins(fmin, fmax)
    K = P.cand_stride(n_lag)
    out = dict(T=Tn, n_bins=n_bins, K=K, min_p=min_p, max_p=max_p, hop=hop)
    cm = torch.empty((B, Tn, max(n_lag, 1)), dtype=torch.float32, device=dev) if want_cmndf else None
    f0 = cb = cp = cc = vp = ptab = None
    if mode == "yin":
        f0 = torch.empty((B, Tn), dtype=torch.float32, device=dev)
    elif mode == "pyin":
        cb = torch.empty((B, Tn, K), dtype=torch.int32, device=dev)
        cp = torch.empty((B, Tn, K), dtype=torch.float32, device=dev)
        cc = torch.empty((B, Tn), dtype=torch.int32, device=dev)
        vp = torch.empty((B, Tn), dtype=torch.float32, device=dev)
        ptab = _cached(("pyin_tab", K), lambda: _dev(P.pyin_device_table(K)))
    else:
        raise ValueError(f"Unsupported pitch estimation method: {mode}. Choose 'pyin' or 'yin'.")
    _call("syg_pitch_frames_f32", _ptr(y), B, L, _ld(y), int(frame_length), win_length, hop, int(center), Tn, float(sr),
          min_p, max_p, 0 if mode == "yin" else 1, float(trough_threshold), float(fmin), n_bins, _ptr(ptab), K,
          _ptr(twiddle_dev(2048)), _ptr(f0), _ptr(cb), _ptr(cp), _ptr(cc), _ptr(vp), _ptr(cm))
    out.update(f0=f0, cand_bin=cb, cand_prob=cp, cand_count=cc, voiced_prob=vp, cmndf=cm)
    return out


def pyin_viterbi(cand_bin: torch.Tensor, cand_prob: torch.Tensor, cand_count: torch.Tensor, voiced_prob: torch.Tensor,
                 n_bins: int, width: int, fmin: float):
    """Viterbi decode of pYIN candidate lists (syg_pyin_viterbi_f32) -> f0 [B, T] (NaN unvoiced), voiced (bool),
    state (int32)."""
    from . import _pitch as P
    B, Tn, K = cand_bin.shape
    dev = cand_bin.device
    tabs, R, h = P.transition_tables(int(n_bins), int(width))
    ltab = _cached(("pyin_ltab", int(n_bins), int(width)), lambda: _dev(tabs))
    lconst = np.ascontiguousarray(P.log_consts(int(n_bins)))
    work = _workspace("syg_pyin_work_bytes", B, Tn, int(n_bins), dtype=torch.uint8, device=dev,
                      error=ValueError(f"pyin_viterbi: bad shape B={B} T={Tn} n_bins={n_bins}"))
    f0 = torch.empty((B, Tn), dtype=torch.float32, device=dev)
    voiced = torch.empty((B, Tn), dtype=torch.uint8, device=dev)
    state = torch.empty((B, Tn), dtype=torch.int32, device=dev)
    _call("syg_pyin_viterbi_f32", _ptr(cand_bin.contiguous()), _ptr(cand_prob.contiguous()), _ptr(cand_count.contiguous()),
          _ptr(voiced_prob.contiguous()), B, Tn, K, int(n_bins), h, _ptr(ltab), R, lconst.ctypes.data_as(C.c_void_p),
          float(fmin), _ptr(work), _nbytes(work), _ptr(f0), _ptr(voiced), _ptr(state))
    return f0, voiced.bool(), state


def pitch_yin(y: torch.Tensor, sr: float, fmin: float, fmax: float, frame_length: int = 2048,
              win_length: Optional[int] = None, hop: Optional[int] = None, center: bool = True,
              trough_threshold: float = 0.1) -> torch.Tensor:
    """librosa.yin on clips y [B, L] -> f0 [B, T] float32 device tensor."""
    return pitch_frames(y, sr, fmin, fmax, frame_length, win_length, hop, center, "yin", trough_threshold)["f0"]


def pitch_pyin(y: torch.Tensor, sr: float, fmin: float, fmax: float, frame_length: int = 2048,
               win_length: Optional[int] = None, hop: Optional[int] = None, center: bool = True):
    """librosa.pyin on clips y [B, L] -> (f0 [B, T] float32 with NaN unvoiced, voiced_flag [B, T] bool,
    voiced_prob [B, T] float32), device tensors."""
    from . import _pitch as P
    fr = pitch_frames(y, sr, fmin, fmax, frame_length, win_length, hop, center, "pyin")
    f0, voiced, _ = pyin_viterbi(fr["cand_bin"], fr["cand_prob"], fr["cand_count"], fr["voiced_prob"], fr["n_bins"],
                                 P.transition_width(sr, fr["hop"]), fmin)
    return f0, voiced, fr["voiced_prob"]


# ------------------------------------------------------------------ HPSS (harmonic / percussive separation)
def _pair(v, what):
    if np.isscalar(v):
        return v, v
    v = tuple(v)
    if len(v) != 2:
        raise ValueError(f"{what} must be a scalar or a pair")
    return v[0], v[1]


def _hpss_stft_args(n_fft, hop_length, win_length, window, center):
    if n_fft != 2048:
        raise ValueError(f"hpss: n_fft={n_fft} is not offloaded (only 2048)")
    win_length = 2048 if win_length is None else int(win_length)
    hop = win_length // 4 if hop_length is None else int(hop_length)
    if win_length != 2048 or hop != 512 or not isinstance(window, str) or window != "hann" or not center:
        raise ValueError("hpss: only window='hann', win_length=2048, hop 512 and center=True are offloaded "
                         f"(got window={window!r}, win_length={win_length}, hop={hop}, center={center})")
    return hop


def window64_dev() -> torch.Tensor:
    """Periodic Hann window of 2048 points as float64 (the synthesis window of istft2048)."""
    return _cached(("win64", "hann", 2048), lambda: _dev(T.analysis_window("hann", 2048, 2048)))


def istft2048(D: torch.Tensor, hop: int = 512, length: Optional[int] = None, center: bool = True, window="hann",
              win_length: Optional[int] = None, mask=None, ldy: Optional[int] = None) -> torch.Tensor:
    """librosa.istft(n_fft=2048) of the frame-major complex STFT D [B, T, 1025, 2] (syg_istft2048_f32) -> y [B, length].
    mask: None, one real mask [B, T, 1025] applied to D on load, or a pair of masks -> a pair of outputs (one read of D).
    length defaults to 512 (T - 1), librosa's center=True length.  ldy: row stride of the output (>= length)."""
    require_gpu()
    _hpss_stft_args(2048, hop, win_length, window, center)
    D = _f32_in(D, "D", 4, (1025, 2)).contiguous()
    B, Tn = D.shape[0], D.shape[1]
    length = 512 * (Tn - 1) if length is None else int(length)
    if length < 1:
        raise ValueError("istft2048: length must be >= 1")
    ld = length if ldy is None else int(ldy)
    two = isinstance(mask, (tuple, list))
    masks = [m.contiguous() if m is not None else None for m in (mask if two else (mask,))]
    for m in masks:
        if m is not None and (m.shape != (B, Tn, 1025) or m.dtype != torch.float32):
            raise ValueError("mask must be float32 [B, T, 1025]")
    outs = [torch.zeros((B, ld), dtype=torch.float32, device=D.device) for _ in masks]
    _call("syg_istft2048_f32", _ptr(D), B, Tn, int(hop), int(bool(center)), length, _ptr(window64_dev()),
          _ptr(twiddle_dev(2048)), _ptr(masks[0]), _ptr(outs[0]), _ptr(masks[1]) if two else None,
          _ptr(outs[1]) if two else None, ld)
    outs = [o[:, :length] for o in outs]
    return tuple(outs) if two else outs[0]


def hpss_masks(D: torch.Tensor, kernel_size=31, power: float = 2.0, margin=1.0, medians: bool = False):
    """decompose.hpss(mask=True) on the complex STFT D [B, T, 1025, 2] (syg_hpss_masks_f32) -> (mask_harm, mask_perc)
    [B, T, 1025] float32, plus the medians (H, P) when `medians`."""
    require_gpu()
    kh, kp = _pair(kernel_size, "kernel_size")
    mh, mp = _pair(margin, "margin")
    if mh < 1 or mp < 1:
        raise ValueError("Margins must be >= 1.0. A typical range is between 1 and 10.")
    if not (power > 0):
        raise ValueError("power must be strictly positive")
    D = _f32_in(D, "D", 4, (1025, 2)).contiguous()
    B, Tn = D.shape[0], D.shape[1]
    new = lambda: torch.empty((B, Tn, 1025), dtype=torch.float32, device=D.device)  # noqa: E731
    Mh, Mp = new(), new()
    H, P = (new(), new()) if medians else (None, None)
    _call("syg_hpss_masks_f32", _ptr(D), B, Tn, int(kh), int(kp), float(power), float(mh), float(mp), _ptr(Mh), _ptr(Mp),
          _ptr(H), _ptr(P))
    return (Mh, Mp, H, P) if medians else (Mh, Mp)


def hpss(y: torch.Tensor, kernel_size=31, power: float = 2.0, margin=1.0, hop_length: Optional[int] = None,
         win_length: Optional[int] = None, window="hann", center: bool = True, n_fft: int = 2048):
    """librosa.effects.hpss on clips y [B, L] -> (y_harm, y_perc) [B, L] float32 device tensors:
    syg_stft2048_c2c_f32 -> syg_hpss_masks_f32 -> syg_istft2048_f32 (both components from one read of D)."""
    require_gpu()
    hop = _hpss_stft_args(n_fft, hop_length, win_length, window, center)
    y = _f32_in(y, "y", 2)
    if y.shape[0] < 1 or y.shape[1] < 1:
        raise ValueError("hpss: empty input")
    D = stft2048_c2c(y, hop, True, "hann", 2048)
    Mh, Mp = hpss_masks(D, kernel_size, power, margin)
    return istft2048(D, hop, y.shape[1], True, "hann", 2048, mask=(Mh, Mp))


def hnr_rows(y_harm: torch.Tensor, y_perc: torch.Tensor, frame_length: int = 2048, hop: Optional[int] = None,
             center: bool = True, rms: bool = False):
    """Per-frame HNR of the reference's harmonic_to_noise_ratio from the two components [B, L] (syg_hnr_rows_f32) ->
    hnr [B, T] float32 (NaN / +-80 rules of the reference), plus (rms_harm, rms_perc) [B, T] when `rms`."""
    require_gpu()
    hop = frame_length // 4 if hop is None else int(hop)
    if frame_length < 1 or hop < 1:
        raise ValueError("hnr_rows: frame_length and hop must be >= 1")
    if y_harm.shape != y_perc.shape or y_harm.dim() != 2:
        raise ValueError("hnr_rows: y_harm and y_perc must have the same shape [B, L]")
    yh, yp = y_harm, y_perc
    if yh.stride(1) != 1 or yp.stride(1) != 1 or _ld(yh) != _ld(yp):
        yh, yp = yh.contiguous(), yp.contiguous()
    B, L = yh.shape
    Tn = _at_least_one(num_frames_padded(L, frame_length, hop, center))
    out = torch.empty((B, Tn), dtype=torch.float32, device=yh.device)
    rh = torch.empty_like(out) if rms else None
    rp = torch.empty_like(out) if rms else None
    _call("syg_hnr_rows_f32", _ptr(yh), _ptr(yp), B, L, _ld(yh), int(frame_length), hop, int(bool(center)), Tn, _ptr(out),
          _ptr(rh), _ptr(rp))
    return (out, rh, rp) if rms else out


# ------------------------------------------------------------------ onset detection
def onset_strength(mel: torch.Tensor, lag: int = 1, max_size: int = 1, pad: int = 0, T_out: Optional[int] = None,
                   amin: float = 1e-10, top_db: Optional[float] = 80.0, detrend: bool = False) -> torch.Tensor:
    """librosa.onset.onset_strength after the mel front end (syg_onset_strength_f32): mel POWER [B, M, T] -> envelope
    [B, T_out] float32, `pad` zeros in front (T_out defaults to pad + T - lag, the uncut envelope).  The dB matrix is
    formed on the fly (ref 1.0, top_db relative to each clip's maximum) and never stored."""
    mel = _f32_in(mel, "mel", 3, axes="[B, M, T]")
    if not isinstance(lag, (int, np.integer)) or lag < 1:
        raise ValueError("lag must be a positive integer")
    if not isinstance(max_size, (int, np.integer)) or max_size < 1:
        raise ValueError("max_size must be a positive integer")
    mel = mel.contiguous()
    B, M, Tn = mel.shape
    T_out = int(pad) + Tn - int(lag) if T_out is None else int(T_out)
    work = _workspace("syg_onset_strength_work_bytes", B, M, Tn, dtype=torch.float32, device=mel.device)
    env = torch.empty((B, max(T_out, 0)), dtype=torch.float32, device=mel.device)
    _call("syg_onset_strength_f32", _ptr(mel), B, M, Tn, float(amin), float(top_db) if top_db is not None else -1.0,
          int(lag), int(max_size), int(pad), T_out, int(bool(detrend)), _ptr(env), _ptr(work))
    return env


def onset_peaks(env: torch.Tensor, pre_max: int, post_max: int, pre_avg: int, post_avg: int, delta: float, wait: int,
                normalize: bool = True, backtrack: bool = False, energy: Optional[torch.Tensor] = None):
    """util.peak_pick with onset_detect's normalisation and backtracking (syg_onset_peaks_f32) on envelopes [B, T] ->
    (frames [B, T] int32: the onsets in ascending order, -1 beyond them; count [B] int32), both on the device."""
    env = _f32_in(env, "env", 2)
    B, Tn = env.shape
    if energy is not None:
        energy = _f32_in(energy, "energy", 2)
        if energy.shape != env.shape:
            raise ValueError("energy must have the envelope's shape")
        if _ld(energy) != _ld(env):
            env, energy = env.contiguous(), energy.contiguous()
    frames = torch.empty((B, Tn), dtype=torch.int32, device=env.device)
    count = torch.empty((B,), dtype=torch.int32, device=env.device)
    _call("syg_onset_peaks_f32", _ptr(env), B, Tn, _ld(env), int(pre_max), int(post_max), int(pre_avg), int(post_avg),
          float(delta), int(wait), int(bool(normalize)), int(bool(backtrack)), _ptr(energy), _ptr(frames), _ptr(count))
    return frames, count


def clip_metrics(y: torch.Tensor) -> torch.Tensor:
    """Per-clip totals of y [B, L] (syg_clip_metrics_f32) -> [B, 2] float32: sum of squares, peak |y|."""
    y = _f32_in(y, "y", 2)
    B, L = y.shape
    out = torch.empty((B, 2), dtype=torch.float32, device=y.device)
    _call("syg_clip_metrics_f32", _ptr(y), B, L, _ld(y), _ptr(out))
    return out


# ------------------------------------------------------------------ discrete wavelet transform
def _wavelet_dev(wavelet):
    """The four filters of a served wavelet as float32 device arrays (dec_lo, dec_hi, rec_lo, rec_hi) and their length."""
    from . import _wavelets as W
    order = W.filter_length(wavelet) // 2           # raises ValueError for a wavelet that is not served
    return _cached(("dwt", order), lambda: tuple(_dev(f.astype(np.float32)) for f in W.filters(wavelet))), 2 * order


def dwt_fits(L: int, wavelet="db4", level: int = 1) -> bool:
    """True when rows of L samples take the clip-resident form of syg_dwt_f32 (the library owns the rule)."""
    from . import _wavelets as W
    return bool(lib().syg_dwt_fits(int(L), W.filter_length(wavelet), int(level)))


def dwt(y: torch.Tensor, wavelet="db4", level: Optional[int] = None, mode: str = "symmetric"):
    """pywt.wavedec of every row of y [B, L] (syg_dwt_f32) -> (packed [B, total] float32 device tensor, lens): row b is
    [cA_n | cD_n | ... | cD_1] of clip b, `lens` the lengths of those arrays in that order (a list of ints), so a row is
    directly a feature vector and `packed.split(lens, dim=1)` the coefficient arrays.  `level=None` is
    max(1, dwt_max_level); a level above the maximum warns, as PyWavelets does."""
    from . import _wavelets as W
    y = _f32_in(y, "y", 2)
    B, L = y.shape
    if L < 1:
        raise ValueError("y must hold at least one sample")
    code = W.mode_code(mode)
    (dec_lo, dec_hi, _, _), F = _wavelet_dev(wavelet)
    level = W.resolve_level(L, F, level)
    h = lib()
    lens_c = (C.c_int64 * (level + 1))()
    total = h.syg_dwt_lengths(L, F, level, C.cast(lens_c, C.c_void_p))
    if total < 0:
        check(-1, "syg_dwt_lengths")
    work = _workspace("syg_dwt_work_bytes", B, L, F, level, dtype=torch.float32, device=y.device)
    out = torch.empty((B, total), dtype=torch.float32, device=y.device)
    _call("syg_dwt_f32", _ptr(y), B, L, _ld(y), _ptr(dec_lo), _ptr(dec_hi), F, code, level, _ptr(out), total, _ptr(work))
    return out, [int(v) for v in lens_c]


def idwt(packed: torch.Tensor, lens, wavelet="db4", mode: str = "symmetric") -> torch.Tensor:
    """pywt.waverec of every row of `packed` [B, sum(lens)] (the layout of `dwt`, lens = [len cA_n, len cD_n, ...,
    len cD_1]; syg_idwt_f32) -> [B, L'] float32.  Where an approximation is one sample longer than its detail its last
    sample is dropped, as pywt.waverec does; any other mismatch is a ValueError.  The served modes extend nothing on the
    way back, so `mode` is only checked."""
    from . import _wavelets as W
    packed = _f32_in(packed, "packed", 2)
    W.mode_code(mode)
    (_, _, rec_lo, rec_hi), F = _wavelet_dev(wavelet)
    lens = [int(v) for v in lens]
    Lout = W.waverec_length(lens, F)
    B = packed.shape[0]
    if packed.shape[1] != sum(lens):
        raise ValueError(f"packed rows hold {packed.shape[1]} coefficients, lens adds up to {sum(lens)}")
    levels = len(lens) - 1
    lens_c = (C.c_int64 * len(lens))(*lens)
    lp = C.cast(lens_c, C.c_void_p)
    work = _workspace("syg_idwt_work_bytes", B, lp, levels, F, dtype=torch.float32, device=packed.device)
    y = torch.empty((B, Lout), dtype=torch.float32, device=packed.device)
    _call("syg_idwt_f32", _ptr(packed), B, _ld(packed), lp, levels, _ptr(rec_lo), _ptr(rec_hi), F, _ptr(y), Lout, _ptr(work))
    return y


# ------------------------------------------------------------------ audio effects
LFO_SHAPES = {"sine": 0, "triangle": 1, "square": 2}          # SYG_LFO_* of include/sygnals_hip.h
TREMOLO_MAX_ROWS = 8 * MAX_ROWS                               # syg_fx_tremolo_f32: eight rows a workgroup, no row loop


def fx_delay_chunk() -> int:
    """Steps of a chain per chunk in the chunked form of syg_fx_delay_f32 (the library owns the figure)."""
    return int(lib().syg_fx_delay_chunk())


def fx_delay(x: torch.Tensor, delay_samples: int, feedback: float = 0.4, wet: float = 0.5, dry: float = 1.0,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Feedback delay of every row of x [B, L] (syg_fx_delay_f32): w[n] = x[n] + feedback w[n - D], out[n] = dry x[n] +
    wet w[n - D] with D = delay_samples >= 1 (D >= L: out = dry x).  `out` may be x."""
    x = _f32_in(x, "x", 2)
    B, L = x.shape
    D = int(delay_samples)
    if B < 1 or L < 1:
        raise ValueError("fx_delay: empty input")
    if D < 1:
        raise ValueError("fx_delay: delay_samples must be >= 1")
    if not 0.0 <= feedback < 1.0:
        raise ValueError("fx_delay: feedback must be in [0, 1)")
    out = _out(out, x.shape, x)
    work = _workspace("syg_fx_delay_work_bytes", B, L, D, dtype=torch.float32, device=x.device)
    _call("syg_fx_delay_f32", _ptr(x), B, L, _ld(x), D, float(feedback), float(dry), float(wet), _ptr(out), _ld(out),
          _ptr(work))
    return out


def fx_mix(x: torch.Tensor, y: Optional[torch.Tensor] = None, a: float = 1.0, b: float = 1.0, length: Optional[int] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r, n] = a x[r, n] + b y[r, n] for n < length (syg_fx_mix_f32); x [B, Lx] and y [B, Ly] read as zero past
    their own lengths, y may be None (a x); length defaults to the longer of the two.  `out` may be x."""
    x = _f32_in(x, "x", 2)
    B, Lx = x.shape
    Ly = 0
    if y is not None:
        y = _f32_in(y, "y", 2)
        if y.shape[0] != B:
            raise ValueError("fx_mix: x and y must hold the same number of rows")
        Ly = y.shape[1]
    L = max(Lx, Ly) if length is None else int(length)
    if B < 1 or L < 1 or Lx < 1 or (y is not None and Ly < 1):
        raise ValueError("fx_mix: empty input")
    out = _out(out, (B, L), x)
    _call("syg_fx_mix_f32", _ptr(x), Lx, _ld(x), _ptr(y), Ly, _ld(y) if y is not None else 0, B, L, float(a), float(b),
          _ptr(out), _ld(out))
    return out


def fx_tremolo(x: torch.Tensor, sr: float, rate: float = 5.0, depth: float = 0.5, shape: str = "sine", n0: int = 0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x ((1 - depth) + depth lfo) on rows x [B, L] (syg_fx_tremolo_f32), the LFO in float64 on the device; n0 is the
    index of the rows' first sample (a row that continues an earlier one).  `out` may be x."""
    x = _f32_in(x, "x", 2)
    if shape not in LFO_SHAPES:
        raise ValueError("LFO shape must be 'sine', 'triangle', or 'square'.")
    if not 0.0 <= depth <= 1.0:
        raise ValueError("fx_tremolo: depth must be in [0, 1]")
    if not rate > 0 or not sr > 0:
        raise ValueError("fx_tremolo: rate and sr must be positive")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("fx_tremolo: empty input")
    if x.shape[0] > TREMOLO_MAX_ROWS:
        raise ValueError(f"fx_tremolo: too many rows ({x.shape[0]}; one call takes at most {TREMOLO_MAX_ROWS})")
    out = _out(out, x.shape, x)
    _call("syg_fx_tremolo_f32", _ptr(x), x.shape[0], x.shape[1], _ld(x), float(sr), float(rate), float(depth),
          LFO_SHAPES[shape], int(n0), _ptr(out), _ld(out))
    return out


def fx_compress(x: torch.Tensor, threshold: float = 0.8, ratio: float = 4.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Downward compression of rows x [B, L] (syg_fx_compress_f32): |x| > threshold -> threshold + (|x| - threshold) /
    ratio with the sign kept; the other samples are copied bit for bit.  `out` may be x."""
    x = _f32_in(x, "x", 2)
    if not threshold >= 0.0:
        raise ValueError("fx_compress: threshold must be >= 0")
    if not ratio >= 1.0:
        raise ValueError("fx_compress: ratio must be >= 1")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("fx_compress: empty input")
    out = _out(out, x.shape, x)
    _call("syg_fx_compress_f32", _ptr(x), x.shape[0], x.shape[1], _ld(x), float(threshold), float(ratio), _ptr(out), _ld(out))
    return out


def fx_midside(x: torch.Tensor, width: float = 1.5) -> torch.Tensor:
    """Mid / side widening of stereo clips x [B, 2, L] (syg_fx_midside_f32) -> [B, 2, L]: mid +- width side."""
    require_gpu()
    if x.dim() != 3 or x.shape[1] != 2 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor of shape [B, 2, L]")
    if not width >= 0.0:
        raise ValueError("fx_midside: width must be >= 0")
    B, _, L = x.shape
    if B < 1 or L < 1:
        raise ValueError("fx_midside: empty input")
    x = x.contiguous()
    out = torch.empty_like(x)
    _call("syg_fx_midside_f32", _ptr(x), B, L, L, float(width), _ptr(out), L)
    return out


def spectral_gate(D: torch.Tensor, Dn: torch.Tensor, amount: float = 1.0, profile: bool = False):
    """The spectral-subtraction gain of noise_reduction_spectral (syg_spectral_gate_f32): D [B, T, 1025, 2] the clip's
    STFT, Dn [B, Tn, 1025, 2] the STFT of its noise segment -> G [B, T, 1025] float32 = sqrt(max(0, 1 - amount N / |D|^2))
    (0 where |D|^2 is 0), a mask for istft2048; with `profile` also N [B, 1025], the mean noise power per bin."""
    D, Dn = (_f32_in(t, name, 4, (1025, 2)).contiguous() for name, t in (("D", D), ("Dn", Dn)))
    if Dn.shape[0] != D.shape[0]:
        raise ValueError("D and Dn must hold the same number of clips")
    if not amount >= 0.0:
        raise ValueError("reduction_amount must be non-negative.")
    B, Tn = D.shape[0], D.shape[1]
    if B < 1 or Tn < 1 or Dn.shape[1] < 1:
        raise ValueError("spectral_gate: empty input")
    G = torch.empty((B, Tn, 1025), dtype=torch.float32, device=D.device)
    N = torch.empty((B, 1025), dtype=torch.float32, device=D.device)
    _call("syg_spectral_gate_f32", _ptr(D), B, Tn, _ptr(Dn), Dn.shape[1], float(amount), _ptr(G), _ptr(N))
    return (G, N) if profile else G


# ------------------------------------------------------------------ augmentation
VOCODER_FORMS = {None: -1, "chain": 0, "chunked": 1}


def phase_vocoder_chunk() -> int:
    """Steps per chunk in the chunked form of syg_phase_vocoder_f32 (the library owns the figure)."""
    return int(lib().syg_phase_vocoder_chunk())


def phase_vocoder(D: torch.Tensor, rate: float, form: Optional[str] = None) -> torch.Tensor:
    """librosa.phase_vocoder (n_fft 2048, hop 512) on the frame-major STFT D [B, T, 1025, 2] -> [B, ceil(T / rate), 1025, 2]
    (syg_phase_vocoder_f32).  form: None (the library's rule) | "chain" | "chunked", for tests and the benchmark."""
    D = _f32_in(D, "D", 4, (1025, 2))
    if form not in VOCODER_FORMS:
        raise ValueError("form must be None, 'chain' or 'chunked'")
    if not rate > 0:
        raise ValueError("Time stretch rate must be positive.")
    D = D.contiguous()
    B, Tn = D.shape[0], D.shape[1]
    if B < 1 or Tn < 1:
        raise ValueError("phase_vocoder: empty input")
    col, alpha = (_dev(a) for a in T.vocoder_steps(Tn, rate))      # not cached: an augmenter draws a new rate per call
    To, f = int(col.shape[0]), VOCODER_FORMS[form]
    work = _workspace("syg_phase_vocoder_work_bytes", B, To, f, dtype=torch.float64, device=D.device)
    out = torch.empty((B, To, 1025, 2), dtype=torch.float32, device=D.device)
    _call("syg_phase_vocoder_f32", _ptr(D), B, Tn, _ptr(col), _ptr(alpha), To, _ptr(out), _ptr(work), f)
    return out


def time_stretch(y: torch.Tensor, rate: float) -> torch.Tensor:
    """librosa.effects.time_stretch of clips y [B, L] -> [B, round(L / rate)] (Python's round, half to even, as librosa):
    stft2048_c2c -> phase_vocoder -> istft2048(length=...), hann, hop 512, centred."""
    y = _f32_in(y, "y", 2)
    if not rate > 0:
        raise ValueError("Time stretch rate must be positive.")
    if y.shape[0] < 1 or y.shape[1] < 1:
        raise ValueError("time_stretch: empty input")
    length = int(round(y.shape[1] / rate))
    if length < 1:
        raise ValueError(f"time_stretch: rate {rate} leaves no sample of a clip of {y.shape[1]}")
    return istft2048(phase_vocoder(stft2048_c2c(y), rate), length=length)


def fx_add_noise_resident_max() -> int:
    """Longest row that syg_fx_add_noise_f32 serves in one launch (the library owns the figure)."""
    return int(lib().syg_fx_add_noise_resident_max())


def _snr_dev(snr_db, B: int, who: str) -> torch.Tensor:
    """snr_db (a number, one per row, or a float64 device tensor [B]) as the float64 device array [B] of the mix."""
    if isinstance(snr_db, torch.Tensor) and snr_db.is_cuda:          # one per row, already on the device: no round trip
        if snr_db.dtype != torch.float64 or tuple(snr_db.shape) != (B,):
            raise ValueError(f"{who}: a device snr_db must be a float64 tensor [B]")
        return snr_db.contiguous()
    snr = np.asarray(snr_db, dtype=np.float64)
    if snr.ndim > 1 or (snr.ndim == 1 and snr.shape[0] != B) or not np.all(np.isfinite(snr)):
        raise ValueError(f"{who}: snr_db must be a finite number or one per row")
    return _dev(np.broadcast_to(snr, (B,)))


def fx_add_noise(y: torch.Tensor, noise: torch.Tensor, snr_db, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y + noise scaled per row to the signal-to-noise ratio snr_db (a number, or one per row), powers in float64
    (syg_fx_add_noise_f32); a row whose signal or noise power is below the float64 epsilon is copied.  `out` may be y."""
    y, noise = _f32_in(y, "y", 2), _f32_in(noise, "noise", 2)
    if noise.shape != y.shape:
        raise ValueError("fx_add_noise: y and noise must have the same shape")
    B, L = y.shape
    if B < 1 or L < 1:
        raise ValueError("fx_add_noise: empty input")
    snr = _snr_dev(snr_db, B, "fx_add_noise")
    out = _out(out, y.shape, y)
    work = _workspace("syg_fx_add_noise_work_bytes", B, L, dtype=torch.float64, device=y.device)
    _call("syg_fx_add_noise_f32", _ptr(y), B, L, _ld(y), _ptr(noise), _ld(noise), _ptr(snr), _ptr(out), _ld(out), _ptr(work))
    return out


# ------------------------------------------------------------------ noise generation
def rng_constants() -> dict:
    """The figures the device generator rests on (the library owns them): Philox rounds, the stream ids of noise samples
    and of per-row draws, the row limit, the longest coloured row."""
    return _constants("syg_rng_constants", ("rounds", "stream_noise", "stream_row", "row_limit", "colored_max"))


def philox_words(counter, key) -> torch.Tensor:
    """Raw Philox4x32-10 words of the device generator: counter [n, 4], key [n, 2] (or one key [2]) uint32 host arrays ->
    int32 device tensor [n, 4] holding the words' bits (`.cpu().numpy().view(np.uint32)`)."""
    device = require_gpu()
    c = np.array(counter, dtype=np.uint32).reshape(-1, 4)
    k = np.broadcast_to(np.asarray(key, dtype=np.uint32).reshape(-1, 2), (c.shape[0], 2)).copy()
    if c.shape[0] < 1:
        raise ValueError("philox_words: no counters")
    cd = torch.from_numpy(c.view(np.int32)).to(device)
    kd = torch.from_numpy(k.view(np.int32)).to(device)
    out = torch.empty_like(cd)
    _call("syg_rng_philox_u32", _ptr(cd), _ptr(kd), c.shape[0], _ptr(out))
    return out


def _rng_shape(who: str, B, L, seed, first_row):
    if not (isinstance(B, (int, np.integer)) and isinstance(L, (int, np.integer))) or B < 1 or L < 1:
        raise ValueError(f"{who}: B and L must be positive integers")
    return int(B), int(L), RNG.check_seed(seed), RNG.check_rows(first_row, int(B))


def randn(B: int, L: int, seed: int, first_row: int = 0, offset: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Standard normals [B, L] float32 on the device (syg_rng_normal_f32): samples offset .. offset + L - 1 of rows
    first_row .. first_row + B - 1 of `seed`.  A sample depends on (seed, row, sample index) alone, so a batch equals its
    rows and randn(L)[k:] equals randn(L - k, offset=k), bit for bit.  `out`: a float32 device tensor [B, L] with unit
    stride along a row (any row stride) to write into."""
    B, L, seed, first_row = _rng_shape("randn", B, L, seed, first_row)
    if isinstance(offset, bool) or not isinstance(offset, (int, np.integer)) or not 0 <= offset < (1 << 62):
        raise ValueError(f"randn: offset must be an integer in [0, 2^62) (got {offset!r})")
    if out is None:
        out = torch.empty((B, L), dtype=torch.float32, device=require_gpu())
    elif tuple(out.shape) != (B, L) or out.dtype != torch.float32 or not out.is_cuda or out.stride(1) != 1:
        raise ValueError(f"out must be a float32 device tensor {(B, L)} with unit stride along a row")
    _call("syg_rng_normal_f32", _ptr(out), B, L, _ld(out), seed, first_row, int(offset))
    return out


def colored_noise_fft_len(L: int) -> int:
    """M of colored_noise: the smallest power of two >= max(L, 2)."""
    return 1 << max(1, (int(L) - 1).bit_length())


def colored_noise(B: int, L: int, seed: int, exponent: float, first_row: int = 0) -> torch.Tensor:
    """Power-law noise [B, L] float32 on the device, spectral density ~ 1 / f^exponent (1 pink, 2 brown; 0 <= exponent <= 2):
    noise[r] = irfft(rfft(w_r) g, M)[:L] with M = colored_noise_fft_len(L), w_r the M white samples of (seed, row r) that
    randn gives, g[0] = 0 and g[k] = k^(-exponent / 2) (Timmer & Koenig 1995): exact in slope, zero-mean over M, free of
    wrap-around correlation unless L = M.  At exponent 0 the gain is 1 everywhere (0^0 = 1) and the row is randn's.  Rows
    r and r ^ 1 (absolute indices) share one complex transform, so a row's bits never depend on the batch it came in.
    L = 1 gives a zero row (one zero-mean sample).  L <= 2^26.  The unit of the result is arbitrary: mix it at a
    signal-to-noise ratio (fx_add_noise)."""
    B, L, seed, first_row = _rng_shape("colored_noise", B, L, seed, first_row)
    exponent = float(exponent)
    if not 0.0 <= exponent <= 2.0:                                   # (NaN fails both comparisons)
        raise ValueError(f"colored_noise: exponent must be in [0, 2] (got {exponent})")
    M = colored_noise_fft_len(L)
    if M > int(lib().syg_rng_constants(4)):
        raise SygnalsHipError(f"colored_noise: L = {L} exceeds the supported maximum 2^26")
    device = require_gpu()
    if L == 1:
        return torch.zeros((B, 1), dtype=torch.float32, device=device)
    out = torch.empty((B, L), dtype=torch.float32, device=device)
    pair0, pair1 = first_row >> 1, (first_row + B - 1) >> 1          # absolute pairs (r >> 1) the rows lie in
    step = max(1, min(MAX_ROWS // 2, (1 << 26) // M))                # pairs of one pass: <= 512 MiB a buffer
    for p in range(pair0, pair1 + 1, step):
        P = min(step, pair1 + 1 - p)
        Z = torch.empty((P, M, 2), dtype=torch.float32, device=device)
        _call("syg_rng_normal_pairs_c64", _ptr(Z), P, M, seed, 2 * p)
        X = fft_pow2_any(Z)
        _call("syg_rng_power_gain_c64", _ptr(X), P, M, exponent)
        Z = fft_pow2_any(X, inverse=True)
        r0, r1 = max(first_row, 2 * p), min(first_row + B, 2 * (p + P))      # the asked rows of these pairs
        rows = out[r0 - first_row:r1 - first_row]
        _call("syg_rng_unpack_pairs_f32", _ptr(Z), M, r0, _ptr(rows), r1 - r0, L, L)
    return out


def fx_add_noise_gen(y: torch.Tensor, snr_db, seed: int, first_row: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fx_add_noise(y, randn(B, L, seed, first_row), snr_db) without the noise ever existing in memory
    (syg_fx_add_noise_gen_f32): within one float32 ulp of that call (the sums are taken in another order).  `out` may be y."""
    y = _f32_in(y, "y", 2)
    B, L = y.shape
    if B < 1 or L < 1:
        raise ValueError("fx_add_noise_gen: empty input")
    seed, first_row = RNG.check_seed(seed), RNG.check_rows(first_row, B)
    snr = _snr_dev(snr_db, B, "fx_add_noise_gen")
    out = _out(out, y.shape, y)
    work = _workspace("syg_fx_add_noise_gen_work_bytes", B, L, dtype=torch.float64, device=y.device)
    _call("syg_fx_add_noise_gen_f32", _ptr(y), B, L, _ld(y), seed, first_row, _ptr(snr), _ptr(out), _ld(out), _ptr(work))
    return out


# ------------------------------------------------------------------ numerical Laplace transform
LAPLACE_FORMS = {None: -1, "whole": 0, "segmented": 1}
_LAPLACE_FIGURES = {"C": "chunk", **{n: n for n in ("tile_rows", "tile_cols", "segment", "steep", "fac_stride")}}


def laplace_constants() -> dict:
    """The figures syg_laplace_f32 rests on (the library owns them): samples per chunk, the tile's chunk rows and s-value
    columns, samples per segment of the segmented form, samples a steep column reads, float64 factors per column."""
    return _constants("syg_laplace", _LAPLACE_FIGURES)


def _laplace_plan_dev(s_bytes: bytes, t_step: float):
    def build():
        k = laplace_constants()
        p = LP.plan(np.frombuffer(s_bytes, dtype=np.complex128), t_step, k["C"], k["tile_cols"], k["segment"], k["steep"],
                    k["fac_stride"])
        return p, _dev(p.table), _dev(p.fac), _dev(p.col)
    return _cached(("laplace_plan", s_bytes, t_step), build, 16)


def _laplace_anchor_dev(s_bytes: bytes, t_step: float, L: int):
    return _cached(("laplace_anchor", s_bytes, t_step, L),
                   lambda: _dev(LP.anchors(_laplace_plan_dev(s_bytes, t_step)[0], L)), 64)


def laplace_plan(s_values, t_step: float = 1.0):
    """(plan, table, fac, col): the host plan (sygnals_amd/_laplace.LaplacePlan) of a list of s-values and its device
    tables, cached on the s-values' bytes and t_step."""
    require_gpu()
    s = LP.check_s_values(s_values, t_step)
    return _laplace_plan_dev(s.tobytes(), float(t_step))


def laplace(y: torch.Tensor, s_values, t_step: float = 1.0, out: Optional[torch.Tensor] = None,
            form: Optional[str] = None) -> torch.Tensor:
    """Numerical Laplace transform of every clip of y [B, L] at the complex s_values [S]:
    F[b, i] = t_step sum_n y[b, n] exp(-s_i n t_step) -> [B, S] complex128 on the device (syg_laplace_f32).  Served:
    finite t_step and s with -Re(s) t_step (L - 1) <= 700.  form: None (the library's rule) | "whole" | "segmented", for
    tests and the benchmark."""
    y = _f32_in(y, "y", 2)
    if form not in LAPLACE_FORMS:
        raise ValueError("form must be None, 'whole' or 'segmented'")
    B, L = y.shape
    s = LP.check_s_values(s_values, t_step)
    S = s.size
    if B < 1 or L < 1 or S < 1:
        raise ValueError("laplace: empty input")
    LP.check_domain(s, t_step, L)
    out = _out(out, (B, S), y, dtype=torch.complex128, contiguous=True)
    key, f = s.tobytes(), LAPLACE_FORMS[form]
    p, table, fac, col = _laplace_plan_dev(key, float(t_step))
    anchor = _laplace_anchor_dev(key, float(t_step), int(L))
    work = _workspace("syg_laplace_work_bytes", B, L, p.S16, f, dtype=torch.float64, device=y.device)
    _call("syg_laplace_f32", _ptr(y), B, L, _ld(y), _ptr(table), _ptr(fac), _ptr(anchor), _ptr(col), p.S_fwd, p.S_rev,
          p.S_steep_fwd, p.S_steep_rev, S, float(t_step), _ptr(out), _ptr(work), f)
    return out


# ------------------------------------------------------------------ polyphase resampling
RESAMPLE_FORMS = {None: -1, "lds": 0, "global": 1}
_RESAMPLE_FIGURES = {n: n for n in ("tile", "table_lds_rule", "table_lds_max", "table_max", "span_max", "rate_max")}


def resample_constants() -> dict:
    """The figures syg_resample_poly_f32 rests on (the library owns them): outputs per tile, the table size (up * Kp * 4
    bytes) up to which the rule puts the table in LDS, the size up to which form='lds' may (on up * (Kp | 1) * 4: rows
    are stored with an odd stride), the size of a served table (up * Kp * 4), the input samples a tile stages at most,
    the largest up / down."""
    return _constants("syg_resample", _RESAMPLE_FIGURES)


def resample_table_in_lds(up: int, Kp: int) -> bool:
    """The library's placement rule: True where the table of up phases x Kp taps sits in LDS when form is None."""
    return up * Kp * 4 <= resample_constants()["table_lds_rule"]


def resample_table_fits_lds(up: int, Kp: int) -> bool:
    """True where form='lds' is served for a table of up phases x Kp taps."""
    return up * (Kp | 1) * 4 <= resample_constants()["table_lds_max"]


def _resample_check_size(up: int, down: int, nbytes: int) -> None:
    k = resample_constants()
    if up > k["rate_max"] or down > k["rate_max"]:
        raise ValueError(f"resample_poly: up={up}, down={down} exceed the served bound of {k['rate_max']}")
    if nbytes > k["table_max"]:
        raise ValueError(f"resample_poly: the filter table of up={up}, down={down} takes {nbytes} bytes, above the bound of "
                         f"{k['table_max']} bytes")


def _resample_table_dev(up: int, down: int, wkey, L: int):
    def build():
        p = RS._plan(up, down, wkey, L)
        return p, _dev(p.table)
    return _cached(("resample", up, down, wkey, L), build, 64)


def resample_plan(up, down, L, window=RS.DEFAULT_WINDOW):
    """(plan, table): the host plan (sygnals_amd/_resample.ResamplePlan) of rows of L samples at up / down and its device
    table [up, Kp] float32, cached per (up, down, window, L).  up == down after reduction has no table: (plan, None)."""
    up, down = RS.reduce_ratio(up, down)
    if up == 1 and down == 1:
        return RS.resample_plan(1, 1, L), None
    wkey = RS.window_key(window)
    _resample_check_size(up, down, RS.table_bytes(up, down, window))
    require_gpu()
    if int(L) != L or L < 1:
        raise ValueError(f"L must be a positive integer, got {L}")
    return _resample_table_dev(up, down, wkey, int(L))


def resample_poly(y: torch.Tensor, up, down, window=RS.DEFAULT_WINDOW, padtype: str = "constant", cval=None,
                  form: Optional[str] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scipy.signal.resample_poly along the rows of y [B, L] (float32, on the device; rows may be strided) ->
    [B, ceil(L up / down)] float32 (syg_resample_poly_f32).  window: firwin's window specification or a 1-D array of
    taps.  padtype: constant (cval, default 0), mean, minimum, maximum, edge, wrap, symmetric, reflect.  form: None (the
    library's rule) | "lds" | "global", the table's placement, for tests and the benchmark.  up == down after reduction
    returns a copy without a launch."""
    up, down = RS.reduce_ratio(up, down)
    if form not in RESAMPLE_FORMS:
        raise ValueError("form must be None, 'lds' or 'global'")
    _f32(y, "y", 2)
    B, L = y.shape
    if B < 1 or L < 1:
        raise ValueError("resample_poly: empty input")
    RS.check_padtype(padtype, L)
    if cval is not None and padtype != "constant":
        raise ValueError("cval has no effect unless padtype is 'constant'")
    same = up == 1 and down == 1
    if not same:
        _resample_check_size(up, down, RS.table_bytes(up, down, window))
    _on_device(y, "y")
    if same:
        if out is None:
            return y.clone(memory_format=torch.contiguous_format)
        out.copy_(y)
        return out
    p, table = resample_plan(up, down, L, window)
    _resample_check_size(up, down, p.table.nbytes)
    if form == "lds" and not resample_table_fits_lds(p.up, p.Kp):
        raise ValueError(f"resample_poly: form='lds' needs up * (Kp | 1) * 4 <= {resample_constants()['table_lds_max']} bytes "
                         f"(up={p.up}, Kp={p.Kp})")
    y = _unit_stride(y)
    out = _out(out, (B, p.n_out), y)
    stat = None
    if padtype in RS.STAT_PADS:                                  # the row minus its statistic, zeros outside, added back
        stat = {"mean": lambda t: t.mean(dim=1, keepdim=True), "minimum": lambda t: t.amin(dim=1, keepdim=True),
                "maximum": lambda t: t.amax(dim=1, keepdim=True)}[padtype](y)
        y = y - stat
    pad = RS.PAD_CODES.get(padtype, 0)
    fill = float(cval) if (cval is not None and stat is None) else 0.0
    for lo, n in _row_blocks(B):
        yb, ob = y[lo:lo + n], out[lo:lo + n]
        _call("syg_resample_poly_f32", _ptr(yb), n, L, _ld(yb), p.up, p.down, p.n_pre_remove, p.Kp, _ptr(table), pad,
              fill, RESAMPLE_FORMS[form], p.n_out, _ptr(ob), _ld(ob))
    if stat is not None:
        out += stat
    return out


# ------------------------------------------------------------------ continuous wavelet transform
CWT_FORMS = (None, "direct", "spectral")
CWT_WORK_BYTES = 1 << 30            # the spectral form takes the clips in blocks whose work buffers stay below this
CWT_MAX_ELEMS = 1 << 31             # B S ceil(L / stride) at most
_CWT_FIGURES = {n: n for n in ("tile", "direct_taps_max", "scales_per_group", "span_max", "taps_lds_max")}


def cwt_constants() -> dict:
    """The figures syg_cwt_f32 rests on (the library owns them): output columns per tile, the tap count up to which the
    rule runs a filter direct, the scales a block serves from one staged span, the input samples a block stages at most,
    the words of taps a block stages at most (the stride-1 form)."""
    return _constants("syg_cwt", _CWT_FIGURES)


def _cwt_table_dev(name: str, s_bytes: bytes):
    def build():
        p = CW._plan(name, s_bytes)
        return p, _dev(p.table)
    return _cached(("cwt_table", name, s_bytes), build, 32)


def _cwt_direct_dev(name: str, s_bytes: bytes, idx_bytes: bytes):
    def build():
        p = CW._plan(name, s_bytes)
        idx = np.frombuffer(idx_bytes, dtype=np.int64)
        idx = idx[np.argsort(p.taps[idx], kind="stable")]          # filters of like length share a group's span
        return _dev(p.meta(idx)), p.reach(idx, cwt_constants()["scales_per_group"])
    return _cached(("cwt_direct", name, s_bytes, idx_bytes), build, 64)


def cwt_fft_len(L: int, taps_max: int) -> int:
    """Transform length of the spectral form: conv_fft_len of the full convolution's length, which must itself have a plan."""
    M = conv_fft_len(L + taps_max - 1)
    if fft_plan(M) is None:
        M = next_direct_len(M)
    if fft_plan(M) is None:
        raise ValueError(f"cwt: rows of {L} samples under a filter of {taps_max} taps need a transform of {M} points, above the "
                         "longest plan (2^26)")
    return M


def _cwt_spectral_dev(name: str, s_bytes: bytes, idx_bytes: bytes, L: int):
    """(M, R, H [R, M, 2] the filter rows' transforms, rmeta): per wavelet, scale list, spectral subset and row length."""
    def build():
        p = CW._plan(name, s_bytes)
        idx = np.frombuffer(idx_bytes, dtype=np.int64)
        rows = CW.spectral_rows(p, idx)
        M = cwt_fft_len(L, int(p.taps[idx].max()))
        h, rmeta = CW.spectral_tables(p, rows, M)
        return M, len(rows), fft_any(_dev(h)), _dev(rmeta)
    return _cached(("cwt_spectral", name, s_bytes, idx_bytes, L), build, 8)


def cwt_plan(scales, wavelet="morl", L=None):
    """(plan, table): the host plan (sygnals_amd/_cwt.CwtPlan: one differenced filter per scale, its tap count, crop
    offset and l1 norm) and its device table, cached per wavelet and scale list.  With L, the transforms of the spectral
    form's filter rows for rows of L samples are made and cached as well."""
    p = CW.cwt_plan(scales, wavelet)
    require_gpu()
    key = p.scales.tobytes()
    if L is not None:
        if int(L) != L or L < 1:
            raise ValueError(f"L must be a positive integer, got {L}")
        _, spec = CW.split_forms(p, cwt_constants()["direct_taps_max"], None)
        if spec.size:
            _cwt_spectral_dev(p.wavelet.name, key, spec.astype(np.int64).tobytes(), int(L))
    return _cwt_table_dev(p.wavelet.name, key)


def cwt_out_shape(B: int, S: int, L: int, stride: int, cplx: bool, output: str):
    n_out = -(-L // stride)
    return (B, S, n_out, 2) if (cplx and output == "coef") else (B, S, n_out)


def cwt(y: torch.Tensor, scales, wavelet="morl", output: str = "coef", stride: int = 1, form: Optional[str] = None,
        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Continuous wavelet transform (pywt.cwt's arithmetic; tests/cwt_ref.py) of every clip of y [B, L] (float32, on the
    device; rows may be strided, rows less than L apart are copied) at the scales [S] -> [B, S, ceil(L / stride)] float32, or [..., 2] (re, im) for the `coef`
    of a complex wavelet.  wavelet: morl | mexh | gaus1 | cmorB-C.  output: coef | magnitude |W| | power |W|^2.  stride
    keeps the columns 0, stride, 2 stride ...: exactly W[..., ::stride].  form: None (the rule: filters of at most
    cwt_constants()['direct_taps_max'] taps run direct, the longer ones through the transforms) | "direct" | "spectral",
    for tests and the benchmark."""
    w = CW.parse_wavelet(wavelet)
    if output not in CW.OUTPUTS:
        raise ValueError("output must be 'coef', 'magnitude' or 'power'")
    if form not in CWT_FORMS:
        raise ValueError("form must be None, 'direct' or 'spectral'")
    if isinstance(stride, bool) or int(stride) != stride or stride < 1:
        raise ValueError(f"stride must be an integer >= 1, got {stride}")
    stride = int(stride)
    _f32(y, "y", 2)
    B, L = y.shape
    if B < 1 or L < 1:
        raise ValueError("cwt: empty input")
    p = CW.cwt_plan(scales, wavelet)
    S = p.S
    shape = cwt_out_shape(B, S, L, stride, w.complex, output)
    n_out = shape[2]
    if B * S * n_out > CWT_MAX_ELEMS:
        raise ValueError(f"cwt: the result of {B} clips x {S} scales x {n_out} columns has {B * S * n_out} elements, above the "
                         f"bound of 2^31; take fewer clips a call or a larger stride")
    _on_device(y, "y")
    if y.stride(1) != 1 or _ld(y) < L:                               # (rows that overlap, an expanded row: a copy)
        y = y.contiguous()
    out = _out(out, shape, y, contiguous=True)
    key, code, cplx = p.scales.tobytes(), CW.OUTPUTS[output], int(w.complex)
    _, table = _cwt_table_dev(w.name, key)
    direct, spec = CW.split_forms(p, cwt_constants()["direct_taps_max"], form)
    if direct.size:
        meta, reach = _cwt_direct_dev(w.name, key, direct.astype(np.int64).tobytes())
        for lo, n in _row_blocks(B):
            yb, ob = y[lo:lo + n], out[lo:lo + n]
            _call("syg_cwt_f32", _ptr(yb), n, L, _ld(yb), _ptr(table), _ptr(meta), int(direct.size), S, cplx, reach,
                  code, stride, n_out, _ptr(ob))
    if spec.size:
        M, R, H, rmeta = _cwt_spectral_dev(w.name, key, spec.astype(np.int64).tobytes(), int(L))
        plan = fft_plan(M)
        per_clip = _work_bytes("syg_cwt_work_bytes", 1, R, M)
        bb = int(max(1, min(B, MAX_ROWS // R, CWT_WORK_BYTES // per_clip)))
        for lo in range(0, B, bb):
            yb, ob = y[lo:lo + bb], out[lo:lo + bb]
            nb = yb.shape[0]
            X = torch.empty((nb, M, 2), dtype=torch.float32, device=y.device)
            _run_plan(plan, pack_rows(yb, M), X, nb, False, flags=FFT_REAL_IN)      # once for all scales
            Z = torch.empty((nb * R, M, 2), dtype=torch.float32, device=y.device)
            _call("syg_cwt_spectrum_c64", _ptr(X), _ptr(H), nb, R, M, _ptr(Z))
            Wz = _run_plan(plan, Z, torch.empty_like(Z), nb * R, True, scale=1.0 / M)
            _call("syg_cwt_crop_f32", _ptr(Wz), nb, R, M, _ptr(rmeta), L, S, cplx, code, stride, n_out, _ptr(ob))
    return out


# ------------------------------------------------------------------ dynamic time warping
DTW_FORMS ={None: -1, "resident": 0, "tiled": 1}
DTW_METRICS = {"euclidean": 0, "sqeuclidean": 1, "cityblock": 2, "cosine": 3}
_DTW_FIGURES = {n: n for n in ("tile", "tile_max", "resident_max_cols", "run_max", "cost_tile")}


def dtw_constants() -> dict:
    """The figures syg_dtw_f32 / syg_dtw_cost_f32 rest on (the library owns them): the tiled form's product tile edge and
    the largest edge it takes, the widest matrix of the pair-resident form, the longest column run of a lane, the cost
    kernel's tile edge."""
    return _constants("syg_dtw", _DTW_FIGURES)


def dtw_plan(B: int, N: int, M: int, want_steps: bool = True, form: Optional[str] = None, tile: int = 0) -> dict:
    """What a call of dtw() on B pairs of N x M takes: form ('resident' | 'tiled', the library's rule unless `form` names
    one), work_bytes (the tiled form's float64 seam workspace) and steps_bytes (one byte a cell when the step codes are
    wanted, which the path needs).  No device work."""
    if form not in DTW_FORMS:
        raise ValueError("form must be None, 'resident' or 'tiled'")
    f = lib().syg_dtw_form(int(B), int(N), int(M), DTW_FORMS[form])
    wb = _work_bytes("syg_dtw_work_bytes", int(B), int(N), int(M), DTW_FORMS[form], int(tile))
    if f < 0:
        check(-1, "syg_dtw_work_bytes")
    return dict(form="tiled" if f == 1 else "resident", work_bytes=wb,
                steps_bytes=int(B) * int(N) * int(M) if want_steps else 0)


def _dtw_lens(v, B: int, device, name: str):
    """(device int32 [B], host ctypes pointer, keep-alive) of a per-pair length list, or (None, None, None)."""
    if v is None:
        return None, None, None
    host = np.ascontiguousarray((v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.int32))
    if host.shape != (B,):
        raise ValueError(f"{name} must hold one length per pair ([{B}]), got shape {host.shape}")
    dev = v if (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.int32 and v.is_contiguous()) \
        else torch.from_numpy(host).to(device)
    return dev, host.ctypes.data_as(C.c_void_p), host


def _dtw_seq(t, name):
    """t [B, K, length] checked, with its row and batch strides (copied where rows overlap or a stride is negative)."""
    t = _f32_in(t, name, 3)
    B, K, L = t.shape
    ld = int(t.stride(1)) if K > 1 else L
    bs = int(t.stride(0)) if B > 1 else 0
    if ld < L or bs < 0:
        t = t.contiguous()
        ld, bs = L, (K * L if B > 1 else 0)
    return t, ld, bs


def dtw_cost(X: torch.Tensor, Y: torch.Tensor, metric: str = "euclidean", x_len=None, y_len=None) -> torch.Tensor:
    """Pairwise frame costs C[b, n, m] = metric(X[b, :, n], Y[b, :, m]) of X [B, K, N] and Y [B, K, M] (float32, on the
    device; rows may be strided, a batch stride of 0 shares one sequence) -> [B, N, M] float32 (syg_dtw_cost_f32).
    metric: euclidean | sqeuclidean | cityblock | cosine.  x_len / y_len [B]: ragged batches; cells outside a pair's
    x_len x y_len corner are written as 0 and nothing outside it is read."""
    require_gpu()
    if metric not in DTW_METRICS:
        raise ValueError(f"metric must be one of {sorted(DTW_METRICS)}, got {metric!r}")
    X, ldx, bsx = _dtw_seq(X, "X")
    Y, ldy, bsy = _dtw_seq(Y, "Y")
    B, K, N = X.shape
    if Y.shape[0] != B or Y.shape[1] != K:
        raise ValueError(f"X {tuple(X.shape)} and Y {tuple(Y.shape)} must agree in B and K")
    xd, xh, _kx = _dtw_lens(x_len, B, X.device, "x_len")
    yd, yh, _ky = _dtw_lens(y_len, B, X.device, "y_len")
    M = Y.shape[2]
    out = torch.empty((B, N, M), dtype=torch.float32, device=X.device)
    _call("syg_dtw_cost_f32", _ptr(X), _ptr(Y), B, K, N, M, ldx, ldy, bsx, bsy, _ptr(xd), _ptr(yd), xh, yh,
          DTW_METRICS[metric], _ptr(out))
    return out


def dtw(C_: torch.Tensor, x_len=None, y_len=None, weights_mul=None, weights_add=None, subseq: bool = False,
        want_D: bool = False, want_steps: bool = False, want_path: bool = True, form: Optional[str] = None,
        tile: int = 0) -> dict:
    """The DTW recurrence (librosa's default step set) and the backtrack on every pair of the cost tensor C_ [B, N, M]
    (float32, on the device; rows may be strided) -> dict of device tensors (syg_dtw_f32):
      cost [B] float64, end_col [B] int32 always; D [B, N, M] float64 (want_D); steps [B, N, M] uint8 (want_steps or
      want_path); path [B, N + M - 1, 2] int32, end first, (-1, -1) past path_len [B] int32 (want_path).
    With none of the three wanted nothing of size N M is written (the distance-only path).  weights_mul / weights_add:
    three finite values each (default 1 and 0).  x_len / y_len [B]: ragged batches; cells of D and steps outside a pair's
    corner are 0.  form: None (the library's rule) | 'resident' | 'tiled'; tile: the tiled form's tile edge (0: the
    product tile), for tests and the benchmark."""
    C_, ldc, bsc = _dtw_seq(C_, "C")
    if form not in DTW_FORMS:
        raise ValueError("form must be None, 'resident' or 'tiled'")
    B, N, M = C_.shape
    w = []
    for v, name in ((weights_mul, "weights_mul"), (weights_add, "weights_add")):
        if v is None:
            w.append(None)
            continue
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
        if a.shape != (3,) or not np.isfinite(a).all():
            raise ValueError(f"{name} must hold three finite values (one per step of [[1,1],[0,1],[1,0]])")
        w.append(a)
    dev = C_.device
    xd, xh, _kx = _dtw_lens(x_len, B, dev, "x_len")
    yd, yh, _ky = _dtw_lens(y_len, B, dev, "y_len")
    ragged = xd is not None or yd is not None
    alloc = torch.zeros if ragged else torch.empty
    f = DTW_FORMS[form]
    work = _workspace("syg_dtw_work_bytes", B, N, M, f, int(tile), dtype=torch.float64, device=dev)
    D = alloc((B, N, M), dtype=torch.float64, device=dev) if want_D else None
    steps = alloc((B, N, M), dtype=torch.uint8, device=dev) if (want_steps or want_path) else None
    cost = torch.empty((B,), dtype=torch.float64, device=dev)
    end_col = torch.empty((B,), dtype=torch.int32, device=dev)
    path = torch.empty((B, N + M - 1, 2), dtype=torch.int32, device=dev) if want_path else None
    path_len = torch.empty((B,), dtype=torch.int32, device=dev) if want_path else None
    _call("syg_dtw_f32", _ptr(C_), B, N, M, ldc, bsc, _ptr(xd), _ptr(yd), xh, yh,
          w[0].ctypes.data_as(C.c_void_p) if w[0] is not None else None,
          w[1].ctypes.data_as(C.c_void_p) if w[1] is not None else None,
          1 if subseq else 0, f, int(tile), _ptr(D), _ptr(steps), _ptr(cost), _ptr(end_col), _ptr(path), _ptr(path_len),
          _ptr(work), _nbytes(work))
    return dict(cost=cost, end_col=end_col, D=D, steps=steps, path=path, path_len=path_len)


# ------------------------------------------------------------------ cepstral analysis
CEPSTRUM_FORMS = (None, "fused", "chain")
CEPS_SLAB_ELEMS = 1 << 26          # complex points a buffer of the chain form holds at most (512 MiB)
_CEPS_KEYS = ("frame", "tile_frames", "waves", "scan", "lds_fixed", "lds_max")      # SYG_CEPS_* of include/sygnals_hip.h


def cepstrum_constants() -> dict:
    """The figures csrc/cepstrum.hip rests on (the library owns them): the fused kernel's frame length, the frames a
    workgroup stages and stores together, its waves, the bins a block of the phase unwrap scans, and the bytes of LDS a
    workgroup holds beside its stage and at n_ceps = 2048."""
    return _constants("syg_cepstrum_constants", _CEPS_KEYS)


def _ceps_tensor(x, what: str, dims: int = 2):
    """_f32, and no empty axis."""
    _f32(x, what, dims)
    if min(x.shape) < 1:
        raise ValueError(f"{what}: empty input")


def _ceps_on_device(x, what: str):
    """_on_device; rows with unit stride that do not overlap (copied if not)."""
    _on_device(x, what)
    return x.contiguous() if (x.dim() == 2 and _ld(x) < x.shape[1]) else _unit_stride(x)


def cepstrogram_frames(L: int, n_fft: int, hop: int, center: bool) -> int:
    """The frame count of stft_any (compute_stft) for clips of L samples."""
    if n_fft == 2048 or (is_pow2(n_fft) and 8 <= n_fft <= 16384):
        return _frames(L, n_fft, hop, center)
    return _at_least_one(num_frames_padded(L, n_fft, hop, center))


def _ceps_chain_rows(X, n: int, Q: int, T: int, amin: float, out_ptr) -> None:
    """One-sided spectra X [rows, n // 2 + 1, 2] of frames -> their first Q quefrencies at out_ptr (laid out [.., Q, T])."""
    rows = X.shape[0]
    Z = torch.empty((rows, n, 2), dtype=torch.float32, device=X.device)
    _call("syg_cepstrum_logmag_c64", _ptr(X), rows, n // 2 + 1, n, amin, _ptr(Z))
    Cz = fft_any(Z, inverse=True)
    _call("syg_cepstrum_gather_f32", _ptr(Cz), rows, n, Q, T, amin, out_ptr)


def cepstrogram(y: torch.Tensor, n_fft: int = 2048, hop: int = 512, center: bool = True, window="hann", win_length=None,
                n_ceps=None, amin: float = CP.AMIN, form: Optional[str] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Real cepstrum of every windowed frame of the clips y [B, L] (float32, on the device; rows may be strided) ->
    [B, Q, T] float32, quefrencies 0 .. Q - 1, Q = n_ceps or n_fft // 2 + 1: c = ifft(log(max(|X|, amin))).real
    (tests/cepstrum_ref.py).  Framing, zero centre padding, frame count, window and win_length are stft_any's.
    form: None (the rule: the fused kernel at n_fft = 2048, the chain stft_any -> log|X| -> inverse transform elsewhere)
    | "fused" (n_fft = 2048 only) | "chain"."""
    if form not in CEPSTRUM_FORMS:
        raise ValueError("form must be None, 'fused' or 'chain'")
    if isinstance(n_fft, bool) or int(n_fft) != n_fft or n_fft < 2 or n_fft > CP.MAX_N:
        raise ValueError(f"n_fft must be an integer in [2, 2^26], got {n_fft}")
    if isinstance(hop, bool) or int(hop) != hop or hop < 1:
        raise ValueError(f"hop must be an integer >= 1, got {hop}")
    n_fft, hop = int(n_fft), int(hop)
    Q = CP.check_n_ceps(n_ceps, n_fft)
    amin = CP.check_amin(amin)
    if form == "fused" and n_fft != 2048:
        raise ValueError(f"cepstrogram: the fused form serves n_fft = 2048 only (got {n_fft}); other lengths take form='chain'")
    _ceps_tensor(y, "y")
    B, L = y.shape
    T = cepstrogram_frames(L, n_fft, hop, bool(center))
    CP.check_size("cepstrogram", (B, Q, T), ("clips", "quefrencies", "frames"))
    y = _ceps_on_device(y, "y")
    out = _out(out, (B, Q, T), y, contiguous=True)
    if n_fft == 2048 and form != "chain":
        win = window_dev(window, 2048 if win_length is None else win_length, 2048)
        _call("syg_cepstrogram2048_f32", _ptr(y), B, L, _ld(y), 2048, hop, int(bool(center)), T, _ptr(win), _ptr(twiddle_dev(2048)),
              Q, amin, _ptr(out))
        return out
    F = n_fft // 2 + 1
    rows_max = max(1, min(MAX_ROWS, CEPS_SLAB_ELEMS // n_fft))
    if T <= rows_max:                                           # whole clips a pass
        per = rows_max // T
        for b0 in range(0, B, per):
            X = stft_any(y[b0:b0 + per], n_fft, hop, center, window, win_length)
            _ceps_chain_rows(X.view(-1, F, 2), n_fft, Q, T, amin, _ptr(out[b0:b0 + per]))
        return out
    for b in range(B):                                          # long clips: runs of frames of one clip
        X = stft_any(y[b:b + 1], n_fft, hop, center, window, win_length).view(T, F, 2)
        for t0 in range(0, T, rows_max):
            _ceps_chain_rows(X[t0:t0 + rows_max], n_fft, Q, T, amin, C.c_void_p(out[b].data_ptr() + 4 * t0))
    return out


def _ceps_rows(x, n, who: str, n_min: int = 1):
    _ceps_tensor(x, "x")
    B, L = x.shape
    n = CP.row_length(n, L, n_min)
    CP.check_size(who, (B, n), ("rows", "points"))
    return _ceps_on_device(x, "x"), B, n


def _ceps_slabs(B: int, n: int):
    per = max(1, min(B, MAX_ROWS, CEPS_SLAB_ELEMS // n))
    return [(b0, min(per, B - b0)) for b0 in range(0, B, per)]


def real_cepstrum(x: torch.Tensor, n=None, amin: float = CP.AMIN) -> torch.Tensor:
    """Real cepstrum of every row of x [B, L] -> [B, n] float32: ifft(log(max(|fft(x, n)|, amin))).real; x is zero-padded
    or cut to n (default L)."""
    amin = CP.check_amin(amin)
    x, B, n = _ceps_rows(x, n, "real_cepstrum")
    out = torch.empty((B, n), dtype=torch.float32, device=x.device)
    for b0, bc in _ceps_slabs(B, n):
        X = fft_any(pack_real(x[b0:b0 + bc], n))
        _call("syg_cepstrum_logmag_c64", _ptr(X), bc, n, n, amin, _ptr(X))
        _call("syg_cepstrum_gather_f32", _ptr(fft_any(X, inverse=True)), bc, n, n, 1, amin, _ptr(out[b0:b0 + bc]))
    return out


def complex_cepstrum(x: torch.Tensor, n=None, amin: float = CP.AMIN):
    """Complex cepstrum of every row of x [B, L] -> (c [B, n] float32, ndelay [B] int32): the phase is unwrapped by
    np.unwrap's rule (bin 0: 0 or +pi by the sign of Re X[0]) and its linear term pi ndelay k / center is taken out.  A right
    shift of a minimum-phase row by d samples gives ndelay = -d.  n >= 2."""
    amin = CP.check_amin(amin)
    x, B, n = _ceps_rows(x, n, "complex_cepstrum", 2)
    out = torch.empty((B, n), dtype=torch.float32, device=x.device)
    nd = torch.empty((B,), dtype=torch.int32, device=x.device)
    for b0, bc in _ceps_slabs(B, n):
        X = fft_any(pack_real(x[b0:b0 + bc], n))
        work = _workspace("syg_cepstrum_unwrap_work_bytes", bc, n, dtype=torch.int32, device=x.device)
        Z = torch.empty_like(X)
        _call("syg_cepstrum_unwrap_c64", _ptr(X), bc, n, amin, _ptr(work), _nbytes(work), _ptr(Z), _ptr(nd[b0:b0 + bc]))
        _call("syg_cepstrum_gather_f32", _ptr(fft_any(Z, inverse=True)), bc, n, n, 1, amin, _ptr(out[b0:b0 + bc]))
    return out, nd


def inverse_complex_cepstrum(c: torch.Tensor, ndelay) -> torch.Tensor:
    """The rows x [B, n] whose complex cepstrum is (c [B, n], ndelay [B]):
    ifft(exp(Re Xh + i (Im Xh + pi ndelay k / center))).real, Xh = fft(c).  Exact for even n at any ndelay; for odd n only
    at ndelay = 0 (the linear term is then no circular shift: errors of 1e-2 at n = 255, ndelay = -31)."""
    x, B, n = _ceps_rows(c, None, "inverse_complex_cepstrum", 2)
    nd = ndelay if isinstance(ndelay, torch.Tensor) else torch.as_tensor(np.asarray(ndelay, dtype=np.int32).reshape(-1))
    if nd.dim() != 1 or nd.shape[0] != B or nd.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"ndelay must hold one integer per row ({B})")
    nd = nd.to(device=x.device, dtype=torch.int32).contiguous()
    out = torch.empty((B, n), dtype=torch.float32, device=x.device)
    for b0, bc in _ceps_slabs(B, n):
        Xh = fft_any(pack_real(x[b0:b0 + bc], n))
        _call("syg_cepstrum_exp_c64", _ptr(Xh), bc, n, _ptr(nd[b0:b0 + bc]), _ptr(Xh))
        _call("syg_cepstrum_gather_f32", _ptr(fft_any(Xh, inverse=True)), bc, n, n, 1, 0.0, _ptr(out[b0:b0 + bc]))
    return out


def cepstrum_peaks(ceps: torch.Tensor, qmin: int, qmax: int, sr: float, threshold: float = CP.THRESHOLD):
    """The cepstral peak of every frame of ceps [B, Q, T] (float32, on the device): q* = the first maximum of
    c[qmin .. qmax], a parabolic shift where the peak is interior and the parabola opens downwards (float64, from the float32
    values) -> (f0 [B, T] float64 = sr / (q* + shift), NaN where the peak is below threshold; strength [B, T] float32 =
    c[q*]; qstar [B, T] int32; voiced [B, T] bool)."""
    _ceps_tensor(ceps, "ceps", 3)
    B, Q, Tn = ceps.shape
    if any(isinstance(v, bool) or int(v) != v for v in (qmin, qmax)) or not 1 <= qmin <= qmax < Q:
        raise ValueError(f"cepstrum_peaks: need 1 <= qmin <= qmax < Q (got qmin={qmin}, qmax={qmax}, Q={Q})")
    if not (float(sr) > 0 and np.isfinite(float(sr))) or np.isnan(float(threshold)):
        raise ValueError(f"cepstrum_peaks: bad sr={sr} / threshold={threshold}")
    _on_device(ceps, "ceps")
    ceps = ceps.contiguous()
    dev = ceps.device
    f0 = torch.empty((B, Tn), dtype=torch.float64, device=dev)
    strength = torch.empty((B, Tn), dtype=torch.float32, device=dev)
    qstar = torch.empty((B, Tn), dtype=torch.int32, device=dev)
    voiced = torch.empty((B, Tn), dtype=torch.uint8, device=dev)
    _call("syg_cepstrum_peaks_f32", _ptr(ceps), B, Q, Tn, int(qmin), int(qmax), float(sr), float(threshold), _ptr(f0), _ptr(strength),
          _ptr(qstar), _ptr(voiced))
    return f0, strength, qstar, voiced.bool()


def pitch_cepstrum(y: torch.Tensor, sr: float, fmin: float, fmax: float, frame_length: int = 2048, hop: Optional[int] = None,
                   center: bool = True, window="hann", threshold: float = CP.THRESHOLD, amin: float = CP.AMIN):
    """Cepstral pitch of clips y [B, L] -> (f0 [B, T] float32 with NaN unvoiced, voiced [B, T] bool, strength [B, T]
    float32): the peak of the real cepstrum of every frame between the quefrencies ceil(sr / fmax) and
    min(floor(sr / fmin), frame_length // 2 - 1).  Any frame length (2048: the fused kernel)."""
    qmin, qmax = CP.quefrency_range(sr, fmin, fmax, int(frame_length))
    hop = int(hop) if hop is not None else int(frame_length) // 4
    ceps = cepstrogram(y, int(frame_length), hop, center, window, None, qmax + 1, amin)
    f0, strength, _, voiced = cepstrum_peaks(ceps, qmin, qmax, sr, threshold)
    return f0.float(), voiced, strength


# ------------------------------------------------------------------ linear prediction
_LPC_KEYS = ("max_frame", "max_order", "waves", "tile_frames", "span_max", "stage_chunk", "acorr_chunk")      # SYG_LPC_* of include/sygnals_hip.h


def lpc_constants() -> dict:
    """The figures csrc/lpc.hip rests on (the library owns them): the longest frame of the frame kernel, the highest
    order, the waves of its workgroup, the frames a workgroup takes together, the floats of a tile's span that are read
    once into LDS, and the samples a workgroup of the two whole-row forms owns."""
    return _constants("syg_lpc_constants", _LPC_KEYS)


def lpc_window_table(window, N: int):
    """The float32 window table of N points, float64 on the host (None: no window; 'ones': all ones; else stft_any's)."""
    if window is None:
        return None
    if isinstance(window, str) and window == "ones":
        return np.ones(N, dtype=np.float32)
    return T.analysis_window(window, N, N).astype(np.float32)


def _lpc_window_dev(window, N: int):
    if window is None:
        return None
    if isinstance(window, str) and window == "ones":
        return _cached(("lpc_ones", N), lambda: _dev(np.ones(N, dtype=np.float32)))
    return window_dev(window, N, N)


def _lpc_result(a, k, err, return_reflection, return_error):
    if not (return_reflection or return_error):
        return a
    return (a,) + ((k,) if return_reflection else ()) + ((err,) if return_error else ())


def lpc_frames(y: torch.Tensor, order: int, frame_length: int = 2048, hop: int = 512, center: bool = True, method: str = "burg",
               window=None, return_reflection: bool = False, return_error: bool = False, out: Optional[torch.Tensor] = None,
               out_k: Optional[torch.Tensor] = None, out_err: Optional[torch.Tensor] = None):
    """Linear prediction of every frame of the clips y [B, L] (float32, on the device; rows may be strided) ->
    a [B, order + 1, T] float32 with a[:, 0] = 1 (and the reflection coefficients k [B, order, T] and the prediction error
    err [B, T] when asked for), the frame index fastest.  method: 'burg' (librosa.lpc's recurrence; no window unless one is
    given) | 'autocorr' (biased autocorrelation and Levinson-Durbin; hann unless another is given; 'ones' for none).
    Framing, zero centre padding and frame count are cepstrogram_frames'.  frame_length in [order + 2, 2048]; float64 past
    the load (tests/lpc_ref.py is the contract)."""
    m = _lpc.check_method(method)
    N, hop = _lpc.check_frame(frame_length, hop)
    p = _lpc.check_order(order, N)
    _ceps_tensor(y, "y")
    B, L = y.shape
    Tn = cepstrogram_frames(L, N, hop, bool(center))
    _lpc.check_size("lpc_frames", (B, p + 1, Tn), ("clips", "coefficients", "frames"))
    y = _ceps_on_device(y, "y")
    win = _lpc_window_dev(_lpc.default_window(method, window), N)
    a = _out(out, (B, p + 1, Tn), y, "out", contiguous=True)
    k = _out(out_k, (B, p, Tn), y, "out_k", contiguous=True) if (return_reflection or out_k is not None) else None
    err = _out(out_err, (B, Tn), y, "out_err", contiguous=True) if (return_error or out_err is not None) else None
    _call("syg_lpc_frames_f32", _ptr(y), B, L, _ld(y), N, hop, int(bool(center)), Tn, _ptr(win), p, m, _ptr(a), _ptr(k), _ptr(err))
    return _lpc_result(a, k, err, return_reflection, return_error)


def lpc_rows(y: torch.Tensor, order: int, method: str = "burg", window=None, form: Optional[str] = None,
             return_reflection: bool = False, return_error: bool = False, out: Optional[torch.Tensor] = None,
             out_k: Optional[torch.Tensor] = None, out_err: Optional[torch.Tensor] = None):
    """Linear prediction of every whole row of y [B, L] -> a [B, order + 1] float32 (and k [B, order], err [B]): librosa.lpc(y,
    order) on every row for method='burg'.  form: None (the rule: rows of at most 2048 samples are one frame of the frame
    kernel, longer rows take the stage form: one launch per stage over a float64 workspace) | 'frame' (L <= 2048 only) |
    'stage'."""
    if form not in _lpc.FORMS:
        raise ValueError("form must be None, 'frame' or 'stage'")
    m = _lpc.check_method(method)
    _ceps_tensor(y, "y")
    B, L = y.shape
    _lpc.check_row(L)
    p = _lpc.check_order(order, L)
    if form == "frame" and L > _lpc.MAX_FRAME:
        raise ValueError(f"lpc_rows: the frame form serves rows of at most {_lpc.MAX_FRAME} samples (got {L}); longer rows take form='stage'")
    _lpc.check_size("lpc_rows", (B, L), ("rows", "samples"))
    y = _ceps_on_device(y, "y")
    win = _lpc_window_dev(_lpc.default_window(method, window), L)
    a = _out(out, (B, p + 1), y, "out", contiguous=True)
    k = _out(out_k, (B, p), y, "out_k", contiguous=True) if (return_reflection or out_k is not None) else None
    err = _out(out_err, (B,), y, "out_err", contiguous=True) if (return_error or out_err is not None) else None
    if form == "frame" or (form is None and L <= _lpc.MAX_FRAME):
        _call("syg_lpc_frames_f32", _ptr(y), B, L, _ld(y), L, L, 0, 1, _ptr(win), p, m, _ptr(a), _ptr(k), _ptr(err))
    else:
        work = _workspace("syg_lpc_rows_work_bytes", B, L, p, m, dtype=torch.float64, device=y.device)
        _call("syg_lpc_rows_f32", _ptr(y), B, L, _ld(y), _ptr(win), p, m, _ptr(work), _nbytes(work), _ptr(a), _ptr(k), _ptr(err))
    return _lpc_result(a, k, err, return_reflection, return_error)


def lpc_phasor_table(n_fft: int) -> np.ndarray:
    """e^{-2 pi i k / n_fft}, k = 0 .. n_fft / 2, float64 [n_fft / 2 + 1, 2]."""
    ang = -2.0 * np.pi * np.arange(n_fft // 2 + 1, dtype=np.float64) / n_fft
    return np.stack([np.cos(ang), np.sin(ang)], axis=1)


def lpc_envelope(a: torch.Tensor, err: torch.Tensor, n_fft: int = 2048, db: bool = False, amin: float = _lpc.AMIN,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The all-pole spectral envelope of a [B, order + 1, T] and err [B, T] (float32, on the device) ->
    [B, n_fft / 2 + 1, T] float32: P[k] = err / |A(e^{-2 pi i k / n_fft})|^2, A(z) = sum_j a[j] z^-j, Horner's rule in float64;
    db=True: 10 log10(max(P, amin))."""
    n_fft = _lpc.check_n_fft(n_fft)
    amin = _lpc.check_amin(amin)
    _ceps_tensor(a, "a", 3)
    _ceps_tensor(err, "err", 2)
    B, p1, Tn = a.shape
    if not 2 <= p1 <= _lpc.MAX_ORDER + 1:
        raise ValueError(f"a must hold order + 1 coefficients a frame, order in 1 ... {_lpc.MAX_ORDER} (got {p1})")
    if tuple(err.shape) != (B, Tn):
        raise ValueError(f"err must be [B, T] = [{B}, {Tn}], got {list(err.shape)}")
    K = n_fft // 2 + 1
    _lpc.check_size("lpc_envelope", (B, K, Tn), ("clips", "bins", "frames"))
    _on_device(a, "a")
    _on_device(err, "err")
    a, err = a.contiguous(), err.contiguous()
    out = _out(out, (B, K, Tn), a, "out", contiguous=True)
    ph = _cached(("lpc_phasor", n_fft), lambda: _dev(lpc_phasor_table(n_fft)))
    _call("syg_lpc_envelope_f32", _ptr(a), _ptr(err), B, p1 - 1, Tn, n_fft, _ptr(ph), int(bool(db)), amin, _ptr(out))
    return out


# ------------------------------------------------------------------ feature dynamics: deltas, CMVN, context stacking
_DYN_KEYS = ("tile", "resident_max_t", "resident_max_t_sliding", "window_max", "direct_window", "width_max", "order_max", "units",
             "max_out", "lds_max")                 # SYG_DYN_* of include/sygnals_hip.h
_DYN_FORMS = {None: 0, "resident": 1, "tiled": 2}


def dynamics_constants() -> dict:
    """The figures the dynamics kernel rests on (the library owns them): the tile (also the chunk of the global sums), the
    rule's longest resident rows, the longest sliding window of the tiled form, the window up to which sliding sums are
    explicit, the served widths and orders, the rows of a workgroup, the largest result, the LDS of a one-row workgroup
    (a forced resident row fits while 4 T, or 20 T + 16 under a long sliding window, stays within it)."""
    return _constants("syg_dynamics_constants", _DYN_KEYS)


def delta_tables(width: int = 9, order: int = 1):
    """The float32 tables of `delta` (host arrays, cached per (width, order)): c [width] = savgol_coeffs(width, order,
    deriv=order) and the interp edge matrix E [width, width]; interior frames are np.convolve(x, c, "valid")."""
    return DY.delta_tables(*DY.check_width_order(width, order, "delta_tables"))


def dynamics_form(T: int, window=None) -> str:
    """The library's rule: "resident" or "tiled" for rows of T frames (window: the sliding CMVN window, None for none)."""
    return "tiled" if lib().syg_dynamics_form(int(T), DY.check_window(window)) == 1 else "resident"


def _dyn_in(x, who: str) -> torch.Tensor:
    """_f32 and no empty axis; x with unit stride along T (the device is judged last, in _dynamics)."""
    _f32(x, f"{who}: x", 3, axes="[B, K, T]")
    if min(x.shape) < 1:
        raise ValueError(f"{who}: empty input (shape {list(x.shape)})")
    return _unit_stride(x)


def _dyn_strides(t: torch.Tensor):
    B, R, Tn = t.shape
    sk = int(t.stride(1)) if R > 1 else Tn
    sb = int(t.stride(0)) if B > 1 else (R - 1) * sk + Tn
    return sb, sk


def _dyn_span(t: torch.Tensor):
    n = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
    return t.data_ptr(), t.data_ptr() + 4 * n


def _dyn_out(who: str, out, shape, x: torch.Tensor, may_alias: bool = False) -> torch.Tensor:
    new, out = out is None, _out(out, shape, x, f"{who}: out")
    if new:
        return out
    (a0, a1), (b0, b1) = _dyn_span(x), _dyn_span(out)
    same = may_alias and out.data_ptr() == x.data_ptr() and out.stride() == x.stride()
    if a0 < b1 and b0 < a1 and not same:
        raise ValueError(f"{who}: out overlaps x" + (" (only out = x itself is served)" if may_alias else ""))
    return out


def _dyn_form(form) -> int:
    if form not in _DYN_FORMS:
        raise ValueError(f"form must be None, 'resident' or 'tiled' (got {form!r})")
    return _DYN_FORMS[form]


def _dyn_table_dev(width: int, orders) -> torch.Tensor:
    return _cached(("dyn_tab", width, tuple(orders)),
                   lambda: _dev(np.concatenate([DY.pack_table(width, o) for o in orders])))


def _dynamics(who, x, out, cm, W, variance, statics, orders, width, mode_code, cval, form):
    """One syg_dynamics_f32 call; every argument has been checked."""
    _on_device(x, f"{who}: x")                                       # (out is on x's device: _dyn_out)
    B, K, Tn = x.shape
    tiled = form == 2 or (form == 0 and lib().syg_dynamics_form(Tn, W if cm else 0) == 1)
    sliding = cm and 1 <= W < Tn
    if sliding and tiled and out.data_ptr() == x.data_ptr():
        x = x.clone()                                                # tiles read their neighbours' frames: not in place
    work = None
    if cm and not sliding and tiled:
        work = _workspace("syg_dynamics_work_bytes", B, K, Tn, dtype=torch.float64, device=x.device)
    tab = _dyn_table_dev(width, orders) if orders else None
    sxb, sxk = _dyn_strides(x)
    sob, sok = _dyn_strides(out)
    _call("syg_dynamics_f32", _ptr(x), B, K, Tn, sxb, sxk, _ptr(out), sob, sok, int(cm), W, int(bool(variance)), int(statics),
          len(orders), width, mode_code, float(cval), _ptr(tab), form, _ptr(work), _nbytes(work))
    return out


def delta(x: torch.Tensor, width: int = 9, order: int = 1, mode: str = "interp", cval: float = 0.0,
          out: Optional[torch.Tensor] = None, form: Optional[str] = None) -> torch.Tensor:
    """librosa.feature.delta along T of x [B, K, T] float32 on the device: scipy.signal.savgol_filter(x, width, deriv=order,
    polyorder=order, mode=mode, cval=cval), float32 accumulation in a fixed order (j ascending).  Served: width odd in
    3 ... 255, 1 <= order <= min(4, width - 1), modes interp (T >= width), nearest, mirror, wrap, constant.  Rows may be
    strided over B and K (unit stride along T); `out` [B, K, T] must not overlap x.  Both forms give the same bits."""
    width, order = DY.check_width_order(width, order)
    mc = DY.check_mode(mode)
    x = _dyn_in(x, "delta")
    B, K, Tn = x.shape
    DY.check_interp(width, Tn, mode)
    DY.check_size("delta", B, K, Tn)
    f = _dyn_form(form)
    out = _dyn_out("delta", out, (B, K, Tn), x)
    return _dynamics("delta", x, out, 0, 0, 0, 0, (order,), width, mc, cval, f)


def cmvn(x: torch.Tensor, window=None, variance: bool = True, out: Optional[torch.Tensor] = None,
         form: Optional[str] = None) -> torch.Tensor:
    """Per-row cepstral mean / variance normalisation of x [B, K, T]: y = (x - m) / sqrt(max(v, 1e-20)) (variance=False:
    x - m), m and v the mean and population variance over all frames (window=None) or over Kaldi's centred sliding window
    of `window` frames; float64 sums, rounded once.  A constant row, T = 1 and window = 1 give exactly 0.  `out` may be x."""
    W = DY.check_window(window)
    x = _dyn_in(x, "cmvn")
    B, K, Tn = x.shape
    DY.check_size("cmvn", B, K, Tn)
    f = _dyn_form(form)
    out = _dyn_out("cmvn", out, (B, K, Tn), x, may_alias=True)
    return _dynamics("cmvn", x, out, 1, W, variance, 1, (), 1, 0, 0.0, f)


def stack_memory(x: torch.Tensor, n_steps: int = 2, delay: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """librosa.feature.stack_memory with zero padding: out [B, n_steps K, T], out[b, i K + k, t] = x[b, k, t - i delay] and 0
    where that index is outside [0, T); delay any non-zero integer.  A pure gather, bit for bit."""
    n_steps, delay = DY.check_stack(n_steps, delay)
    x = _dyn_in(x, "stack_memory")
    B, K, Tn = x.shape
    DY.check_size("stack_memory", B, n_steps * K, Tn)
    out = _dyn_out("stack_memory", out, (B, n_steps * K, Tn), x)
    if not out.is_contiguous():
        raise ValueError("stack_memory: out must be contiguous")
    _on_device(x, "stack_memory: x")
    sxb, sxk = _dyn_strides(x)
    _call("syg_stack_memory_f32", _ptr(x), B, K, Tn, sxb, sxk, _ptr(out), n_steps, delay)
    return out


def feature_post(x: torch.Tensor, cmvn=None, variance: bool = True, deltas: int = 2, width: int = 9, mode: str = "interp",
                 out: Optional[torch.Tensor] = None, form: Optional[str] = None) -> torch.Tensor:
    """[statics | delta | delta-delta] of x [B, K, T] in one call: out [B, (deltas + 1) K, T].  cmvn: None, "global" or a
    sliding window W; it comes first and the deltas (orders 1 and 2 of the statics, not delta of delta) are taken from the
    normalised statics as rounded to float32, so the result equals cat(s, delta(s, order=1), delta(s, order=2)) with
    s = cmvn(x) bit for bit.  One read of x, deltas + 1 writes."""
    if isinstance(deltas, bool) or deltas not in (0, 1, 2):
        raise ValueError(f"feature_post: deltas must be 0, 1 or 2 (got {deltas!r})")
    if cmvn is not None and cmvn != "global" and (isinstance(cmvn, str) or isinstance(cmvn, bool)):
        raise ValueError(f"feature_post: cmvn must be None, 'global' or a sliding window >= 1 (got {cmvn!r})")
    cm = cmvn is not None
    W = 0 if cmvn in (None, "global") else DY.check_window(cmvn, "feature_post")
    mc = 0
    if deltas:
        width, _ = DY.check_width_order(width, deltas, "feature_post")
        mc = DY.check_mode(mode, "feature_post")
    x = _dyn_in(x, "feature_post")
    B, K, Tn = x.shape
    if deltas:
        DY.check_interp(width, Tn, mode, "feature_post")
    DY.check_size("feature_post", B, (deltas + 1) * K, Tn)
    f = _dyn_form(form)
    out = _dyn_out("feature_post", out, (B, (deltas + 1) * K, Tn), x)
    orders = tuple(range(1, deltas + 1))
    tiled = f == 2 or (f == 0 and lib().syg_dynamics_form(Tn, W if cm else 0) == 1)
    if cm and deltas and mode == "wrap" and tiled and Tn > dynamics_constants()["tile"]:
        # a wrapped frame of another tile would need that tile's statistics: the statics first, the deltas from them
        s = torch.empty((B, K, Tn), dtype=torch.float32, device=x.device)
        _dynamics("feature_post", x, s, 1, W, variance, 1, (), 1, 0, 0.0, f)
        out[:, :K].copy_(s)
        for d in orders:
            _dynamics("feature_post", s, out[:, d * K:(d + 1) * K], 0, 0, 0, 0, (d,), width, mc, 0.0, f)
        return out
    return _dynamics("feature_post", x, out, int(cm), W, variance, 1, orders, width if deltas else 1, mc, 0.0, f)


# ------------------------------------------------------------------ PCEN: per-channel energy normalisation
_PCEN_KEYS = ("tile", "bands", "resident_max_t", "lds_max", "grid_max", "units", "max_out", "table_words")   # SYG_PCEN_*


def pcen_constants() -> dict:
    """The figures the PCEN kernels rest on (the library owns them): the frames of a tile of the tiled form, the bands of
    a resident workgroup, the rule's longest resident row, the LDS of a workgroup (two fit a CU), the workgroups of a
    launch, the tiles of a tiled workgroup, the largest result, the float64 words of a band in the parameter table."""
    return _constants("syg_pcen_constants", _PCEN_KEYS)


def pcen_form(T: int, M: int, max_size: int = 1) -> str:
    """The library's rule: "resident" or "tiled" for [*, M, T] under a running maximum of max_size bands."""
    f = lib().syg_pcen_form(int(T), int(M), PC.check_max_size(max_size, int(M)))
    if f < 0:
        raise ValueError(f"pcen_form: T = {T} and M = {M} must be at least 1")
    return "tiled" if f == 1 else "resident"


def pcen(S: torch.Tensor, sr: float = 22050, hop_length: int = 512, gain=0.98, bias=2.0, power=0.5, time_constant: float = 0.4,
         eps=1e-6, b=None, max_size: int = 1, scale: float = 1.0, zi=None, return_zf: bool = False,
         out: Optional[torch.Tensor] = None, form: Optional[str] = None):
    """librosa.pcen along T of S [B, M, T] float32 >= 0 on the device (the definition: _pcen.py; the contract:
    tests/pcen_ref.py).  b=None takes librosa's rule from time_constant, sr and hop_length.  gain, bias, power, eps and b
    are scalars or vectors of one value per band (the special cases power = 0 and bias = 0 are decided per band).  max_size
    > 1 smooths the running maximum over that many bands (scipy's maximum_filter1d).  scale multiplies S on load.  zi
    [B, M] float64 is scipy.signal.lfilter's state of every row (None: 1 - b); return_zf adds the closing state, so a clip
    fed in pieces chained through it equals the whole.  The smoother state is float64, the law float32.  Rows may be
    strided over B and M (unit stride along T); `out` may be strided the same way and may be S itself.  form: None (the
    library's rule), "resident" or "tiled".  Negative or non-finite S is outside the contract (NaN, never a fault)."""
    who = "pcen"
    if b is None:
        b = PC.b_from_time_constant(time_constant, sr, hop_length)
    _f32(S, f"{who}: S", 3, axes="[B, M, T] (a non-negative magnitude or power mel block)")
    B, M, Tn = S.shape
    PC.check_size(who, B, M, Tn)
    vals, per_band = PC.check_params(M, gain, bias, power, eps, b)
    ms = PC.check_max_size(max_size, M)
    scale = PC.check_scale(scale)
    if Tn > 1 and S.stride(-1) != 1:
        raise ValueError(f"{who}: S must have unit stride along T (got {S.stride(-1)}; rows may be strided over B and M)")
    PC.check_zi(zi, B, M)
    f = _dyn_form(form)
    out = _dyn_out(who, out, (B, M, Tn), S, may_alias=True)
    _on_device(S, f"{who}: S")
    if ms > 1 and out.data_ptr() == S.data_ptr():
        S = S.clone()                                               # neighbouring bands are read: not in place
    tiled = f == 2 or (f == 0 and lib().syg_pcen_form(Tn, M, ms) == 1)
    work = _workspace("syg_pcen_work_bytes", B, M, Tn, dtype=torch.float64, device=S.device) if tiled else None
    tab = None
    if per_band:
        t64 = PC.pack_table(vals, pcen_constants()["tile"])
        tab = _cached(("pcen_tab", t64.tobytes()), lambda: _dev(t64), limit=16)
        vals = [0.0, 0.0, 0.0, 1.0, 1.0]                            # the entry ignores the scalars beside a table
    if zi is not None:
        zi = (zi if isinstance(zi, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(zi, dtype=np.float64)))
        zi = zi.to(device=S.device, dtype=torch.float64).contiguous()
    zf = torch.empty((B, M), dtype=torch.float64, device=S.device) if return_zf else None
    sxb, sxk = _dyn_strides(S)
    sob, sok = _dyn_strides(out)
    _call("syg_pcen_f32", _ptr(S), B, M, Tn, sxb, sxk, _ptr(out), sob, sok, *vals, _ptr(tab), ms, scale, _ptr(zi), _ptr(zf), f,
          _ptr(work), _nbytes(work))
    return (out, zf) if return_zf else out


# ------------------------------------------------------------------ SpecAugment: time warp, frequency and time masks
_SPEC_KEYS = ("stream", "max_masks", "tile", "resident_max", "max_elems")                  # SYG_SPEC_* of include/sygnals_hip.h


def spec_augment_constants() -> dict:
    """The figures the SpecAugment kernel rests on (the library owns them): the generator stream of its draws, the most
    masks of one kind, the cells of a tile (also the chunk of the mean's sums), the cells of a clip up to which "mean" is
    taken inside the one launch, the most elements of a call."""
    return _constants("syg_spec_augment_constants", _SPEC_KEYS)


def _spec_lengths(lengths, B: int, Tn: int, who: str) -> np.ndarray:
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
            raise ValueError(f"{who}: lengths must be {B} integers, one per clip (got dtype {lengths.dtype})")
        lengths = lengths.detach().cpu().numpy()
    return SA.check_lengths(lengths, B, Tn, who)


def spec_augment(x: torch.Tensor, seed: int, first_row: int = 0, freq_masks: int = 2, freq_width: int = 27, time_masks: int = 2,
                 time_width: int = 100, time_ratio: float = 1.0, time_warp: int = 0, mask_value=0.0, lengths=None,
                 out: Optional[torch.Tensor] = None, form: Optional[str] = None) -> torch.Tensor:
    """SpecAugment of x [B, K, T] float32 on the device (syg_spec_augment_f32): per clip a time warp of up to `time_warp`
    frames (two linear resizes, torch's interpolate with align_corners=False), then the union of `freq_masks` masks of up to
    `freq_width` rows and `time_masks` masks of up to min(time_width, floor(time_ratio T_b)) frames, written with
    `mask_value` (a finite float, bit for bit) or "mean" (the clip's mean over its valid frames before the warp, float64
    sums).  Clip b draws from row first_row + b of `seed` alone (sygnals_amd._specaug.params gives the same integers), so a
    batch equals its clips.  lengths [B]: valid frames T_b in [1, T]; later frames are copied.  Rows may be strided over B
    and K.  `out` may be x itself when time_warp = 0: then only masked cells are written.  form: "resident" / "tiled"
    forces how "mean" takes its sums (None: the library's rule; same bits)."""
    who = "spec_augment"
    given = x
    x = _dyn_in(x, who)
    B, K, Tn = x.shape
    SA.check_shape(B, K, Tn, who)
    nf, F, nt, Wt, p, W = SA.check_args(K, Tn, freq_masks, freq_width, time_masks, time_width, time_ratio, time_warp, who)
    mean, value = SA.check_mask_value(mask_value, who)
    seed, first_row = RNG.check_seed(seed), RNG.check_rows(first_row, B)
    f = _dyn_form(form)
    Tb = None if lengths is None else _spec_lengths(lengths, B, Tn, who)
    sxb, sxk = _dyn_strides(x)
    if out is given and x is given and W == 0:                       # onto the input itself: nothing of `out` is left to check
        sob, sok, inplace = sxb, sxk, True
    else:
        aliased = isinstance(out, torch.Tensor) and out.data_ptr() == x.data_ptr()
        out = _dyn_out(who, out, (B, K, Tn), x, may_alias=W == 0)
        sob, sok = _dyn_strides(out)
        inplace = aliased and (sob, sok) == (sxb, sxk)
    _on_device(x, f"{who}: x")
    work = None
    if mean and nf + nt and (inplace or f == 2 or (f == 0 and K * Tn > spec_augment_constants()["resident_max"])):
        work = _workspace("syg_spec_augment_work_bytes", B, K, Tn, dtype=torch.float64, device=x.device)
    ld = None if Tb is None else torch.from_numpy(Tb).to(x.device)
    _call("syg_spec_augment_f32", _ptr(x), B, K, Tn, sxb, sxk, _ptr(out), sob, sok, _ptr(ld), seed, first_row, nf, F, nt, Wt, p, W,
          int(mean), value, f, _ptr(work), _nbytes(work))
    return out


# ------------------------------------------------------------------ rhythm: tempogram, tempo, beat tracking
_BEAT_KEYS = ("win_max", "period_max", "log_table", "slice_tiles", "dp_wave_period", "max_elems")      # SYG_BEAT_* of include/sygnals_hip.h


def beat_constants() -> dict:
    """The figures the rhythm kernels rest on (the library owns them): the largest win_length and beat period, the entries
    of the log table, the tiles of frames behind one partial row of the aggregate, the period up to which the DP runs one
    wave a clip, the most elements of a result."""
    return _constants("syg_beat_constants", _BEAT_KEYS)


def tempogram_tile(win_length: int) -> int:
    """Frames of a tempogram workgroup's tile at this win_length."""
    return int(lib().syg_tempogram_tile(RH.check_win_length(win_length, "tempogram")))


def _beat_periods(period, B: int, device, who: str):
    """(device int32 [B], the host's bound on them or None) of periods given on either side."""
    if isinstance(period, torch.Tensor):
        if period.dtype != torch.int32 or tuple(period.shape) != (B,) or not period.is_cuda:
            raise ValueError(f"{who}: period must be an int32 device tensor [{B}] (or integers on the host)")
        return period.contiguous(), None
    p = RH.check_periods(period, B, who)
    return torch.from_numpy(p).to(device), max(2, int(p.max()))


def tempogram(env: torch.Tensor, win_length: int = 384, center: bool = True, window="hann", norm=np.inf,
              aggregate: Optional[str] = None, out: Optional[torch.Tensor] = None):
    """librosa.feature.tempogram (autocorrelation) of envelopes env [B, T] (rows of any stride) on the device
    (syg_tempogram_f32) -> tg [B, win_length, n] float32, frames fastest; n = T centred, else T - win_length + 1.
    aggregate: None: tg alone; "also": (tg, a) with a [B, win_length] float64, the mean of tg over frames; "only": a alone,
    and nothing of size B win_length n is written."""
    who = "tempogram"
    win = RH.check_win_length(win_length, who)
    nrm = RH.check_norm(norm, who)
    if aggregate not in (None, "also", "only"):
        raise ValueError(f'{who}: aggregate must be None, "also" or "only"')
    _f32(env, "env", 2, axes="[B, T]")
    B, Tn = env.shape
    n = RH.check_frames(Tn, win, bool(center), who)
    if aggregate != "only":
        RH.check_size(B, win, n, who)
    env = _f32_in(env, "env", 2, axes="[B, T]")
    wdev = _cached(("beat_win",) + _window_key(window, win, win), lambda: _dev(RH.window_table(window, win)), limit=16)
    tg = _out(out, (B, win, n), env, contiguous=True) if aggregate != "only" else None
    a = work = None
    if aggregate is not None:
        a = torch.empty((B, win), dtype=torch.float64, device=env.device)
        work = _workspace("syg_tempogram_work_bytes", B, Tn, win, int(bool(center)), dtype=torch.float64, device=env.device)
    _call("syg_tempogram_f32", _ptr(env), B, Tn, _ld(env), win, int(bool(center)), _ptr(wdev), nrm, _ptr(tg), _ptr(a), _ptr(work),
          _nbytes(work))
    return tg if aggregate is None else ((tg, a) if aggregate == "also" else a)


def tempo_pick(a: torch.Tensor, env: torch.Tensor, logprior: np.ndarray, bpms: np.ndarray):
    """The tempo of every row (a: the aggregate, float64 [B, win_length]) or of every frame (a: a tempogram, float32
    [B, win_length, n]) under the host-made prior (syg_tempo_pick_f32) -> (k* int32, tempo float64), [B] or [B, n]: the first
    argmax of log1p(1e6 a[k]) + logprior[k] and bpms[k*].  A row whose envelope env [B, T] is all zeros gives 0 and 0.0."""
    who = "tempo_pick"
    if not isinstance(a, torch.Tensor) or (a.dim(), a.dtype) not in ((2, torch.float64), (3, torch.float32)):
        raise ValueError(f"{who}: a must be the aggregate (float64 [B, win_length]) or a tempogram (float32 [B, win_length, n])")
    _f32(env, "env", 2, axes="[B, T]")
    B, win = a.shape[:2]
    win = RH.check_win_length(int(win), who)
    lp, bp = (np.ascontiguousarray(v, dtype=np.float64) for v in (logprior, bpms))
    if lp.shape != (win,) or bp.shape != (win,) or env.shape[0] != B:
        raise ValueError(f"{who}: logprior and bpms must hold win_length = {win} values and env {B} rows")
    _on_device(a, "a")
    env = _f32_in(env, "env", 2, axes="[B, T]")
    a = a.contiguous()
    n = 1 if a.dim() == 2 else int(a.shape[2])
    lpd, bpd = _cached(("tempo_prior", lp.tobytes(), bp.tobytes()), lambda: (_dev(lp), _dev(bp)), limit=16)
    shape = (B,) if a.dim() == 2 else (B, n)
    kstar = torch.empty(shape, dtype=torch.int32, device=a.device)
    bpm = torch.empty(shape, dtype=torch.float64, device=a.device)
    work = _workspace("syg_tempo_pick_work_bytes", B, dtype=torch.float32, device=a.device)
    _call("syg_tempo_pick_f32", _ptr(a) if a.dim() == 2 else None, _ptr(a) if a.dim() == 3 else None, B, win, n, _ptr(env),
          int(env.shape[1]), _ld(env), _ptr(lpd), _ptr(bpd), _ptr(kstar), _ptr(bpm), _ptr(work))
    return kstar, bpm


def beat_local_score(env: torch.Tensor, period):
    """beat_track's local score of envelopes env [B, T] (syg_beat_local_score_f32): the envelope over its standard
    deviation against the Gaussian taps of each row's own period (device int32 [B], or integers on the host)
    -> (ls [B, T] float32, its maxima [B] float32)."""
    env = _f32_in(env, "env", 2, axes="[B, T]")
    B, Tn = env.shape
    pd, _ = _beat_periods(period, B, env.device, "beat_local_score")
    ls = torch.empty((B, Tn), dtype=torch.float32, device=env.device)
    lsmax = torch.empty((B,), dtype=torch.float32, device=env.device)
    work = _workspace("syg_beat_local_score_work_bytes", B, dtype=torch.float64, device=env.device)
    _call("syg_beat_local_score_f32", _ptr(env), B, Tn, _ld(env), _ptr(pd), _ptr(ls), _ptr(lsmax), _ptr(work))
    return ls, lsmax


def beat_dp(ls: torch.Tensor, lsmax: torch.Tensor, period, tightness: float = 100.0, period_max: Optional[int] = None,
            out=None):
    """beat_track's dynamic programme over local scores ls [B, T] (syg_beat_dp_f32) -> (cum [B, T] float64, back [B, T]
    int32).  period: device int32 [B] or integers on the host; period_max: a bound on them (default: the largest of host
    periods, the library's maximum for a device tensor); a row above it, or below 2, gets no beats.  out: (cum, back)."""
    who = "beat_dp"
    tight = RH.check_tightness(tightness, who)
    _f32(ls, "ls", 2, axes="[B, T]")
    _f32(lsmax, "lsmax", 1, axes="[B]")
    B, Tn = ls.shape
    if lsmax.shape[0] != B:
        raise ValueError(f"{who}: lsmax must hold {B} values")
    _on_device(ls, "ls")
    ls, lsmax = ls.contiguous(), lsmax.contiguous()
    pd, bound = _beat_periods(period, B, ls.device, who)
    pmax = int(period_max) if period_max is not None else (bound or RH.PERIOD_MAX)
    if not 2 <= pmax <= RH.PERIOD_MAX:
        raise ValueError(f"{who}: period_max={pmax} is outside 2 .. {RH.PERIOD_MAX}")
    cum = _out(out[0] if out else None, (B, Tn), ls, "out[0]", torch.float64, contiguous=True)
    back = _out(out[1] if out else None, (B, Tn), ls, "out[1]", torch.int32, contiguous=True)
    logtab = _cached(("beat_log",), lambda: _dev(RH.log_table()))
    _call("syg_beat_dp_f32", _ptr(ls), _ptr(lsmax), B, Tn, _ptr(pd), pmax, tight, _ptr(logtab), _ptr(cum), _ptr(back))
    return cum, back


def beat_track(ls: torch.Tensor, cum: torch.Tensor, back: torch.Tensor, period, trim: bool = True, out=None):
    """The beats of every row from its local score and the DP's tables (syg_beat_track_f32): the last beat by the median
    of cum's local maxima, the walk along back, the trim -> (beats [B, T] int32 ascending, -1 beyond them; count [B] int32;
    last [B] int32, the last beat before the trim or -1).  out: (beats, count)."""
    who = "beat_track"
    _f32(ls, "ls", 2, axes="[B, T]")
    B, Tn = ls.shape
    for t, name, dt in ((cum, "cum", torch.float64), (back, "back", torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (B, Tn):
            raise ValueError(f"{who}: {name} must be a {str(dt)[6:]} tensor [{B}, {Tn}]")
    _on_device(ls, "ls")
    ls, cum, back = ls.contiguous(), cum.contiguous(), back.contiguous()
    pd, _ = _beat_periods(period, B, ls.device, who)
    beats = _out(out[0] if out else None, (B, Tn), ls, "out[0]", torch.int32, contiguous=True)
    count = _out(out[1] if out else None, (B,), ls, "out[1]", torch.int32, contiguous=True)
    last = torch.empty((B,), dtype=torch.int32, device=ls.device)
    _call("syg_beat_track_f32", _ptr(ls), _ptr(cum), _ptr(back), B, Tn, _ptr(pd), int(bool(trim)), _ptr(beats), _ptr(count),
          _ptr(last))
    return beats, count, last


# ------------------------------------------------------------------ tonal: chroma folds, CENS, tonnetz, tuning
_CHROMA_KEYS = ("nc_max", "row_tile", "table_lds_max", "p_max", "cens_tile", "cens_win_max", "hist_bins_max",
                "max_elems")                       # SYG_CHROMA_* of include/sygnals_hip.h


def chroma_constants() -> dict:
    """The figures the tonal kernels rest on (the library owns them): the largest n_chroma, the frames of a wave's tile of
    the frame-major fold, the LDS up to which that fold stages its table, the rows of the output transform, the frames of a
    CENS workgroup, the taps of its window, the bins of the tuning histogram, the most elements of an input."""
    return _constants("syg_chroma_constants", _CHROMA_KEYS)


class ChromaTable:
    """A fold table [n_chroma, cols] held on the device in both orientations, each made once: what a caller that folds with
    the same table again and again (core.features.tonal) hands to chroma_fold, so that no call hashes or transposes it."""

    def __init__(self, table: np.ndarray):
        a = np.ascontiguousarray(table, dtype=np.float32)
        if a.ndim != 2 or min(a.shape) < 1:
            raise ValueError("ChromaTable: the table must be a 2-D array [n_chroma, cols]")
        self.shape = tuple(a.shape)
        self._host, self._dev = a, {}

    def dev(self, transpose: bool) -> torch.Tensor:
        k = (torch.cuda.current_device(), bool(transpose))
        if k not in self._dev:
            self._dev[k] = _dev(self._host.T if transpose else self._host)
        return self._dev[k]


def _chroma_table(table, rows: Optional[int], who: str, what: str = "table", transpose: bool = False) -> torch.Tensor:
    """A float32 device table [n, cols] from a ChromaTable, a host array (cached by content: the whole array is hashed at
    every call) or a device tensor (transposed by a copy at every call); transpose: [cols, n]."""
    if isinstance(table, ChromaTable):
        require_gpu()
        return table.dev(transpose)
    if isinstance(table, torch.Tensor):
        _f32(table, f"{who}: {what}", 2)
        if rows is not None and table.shape[0] != rows:
            raise ValueError(f"{who}: {what} must have {rows} rows (got {table.shape[0]})")
        _on_device(table, f"{who}: {what}")
        return (table.t() if transpose else table).contiguous()
    a = np.ascontiguousarray(table, dtype=np.float32)
    if a.ndim != 2 or min(a.shape) < 1 or (rows is not None and a.shape[0] != rows):
        raise ValueError(f"{who}: {what} must be a 2-D float32 array" + (f" of {rows} rows" if rows is not None else ""))
    return _cached(("chroma_tab", a.shape, a.tobytes(), transpose), lambda: _dev(a.T if transpose else a), limit=32)


def _chroma_spec(x, who: str, axes: str):
    """(x, complex) of a real [B, *, *] or interleaved complex [B, *, *, 2] float32 spectrogram, judged without a device."""
    if isinstance(x, torch.Tensor) and x.dim() == 4:
        _f32(x, f"{who}: x", 4, (2,), axes=axes)
        cplx = True
    else:
        _f32(x, f"{who}: x", 3, axes=axes)
        cplx = False
    if min(x.shape) < 1:
        raise ValueError(f"{who}: empty input (shape {list(x.shape)})")
    if x.numel() // (2 if cplx else 1) > CH.MAX_ELEMS:
        raise ValueError(f"{who}: an input of more than 2^31 elements; call it on fewer rows")
    return x, cplx


def _chroma_power(power, who: str) -> int:
    if power not in (1, 2) or isinstance(power, bool):
        raise ValueError(f"{who}: power must be 1 (magnitude) or 2 (power) of a complex input (got {power!r})")
    return int(power)


def chroma_fold(x: torch.Tensor, table, layout: str = "rows", power: int = 2, threshold=None, norm=np.inf, transform=None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The chroma fold with librosa's threshold and per-frame normalisation -> [B, n_chroma, T] float32 on the device.
    layout "rows" (syg_chroma_fold_rows_f32): x frame-major [B, T, F] real or [B, T, F, 2] complex (as stft_any leaves it),
    table [n_chroma, F]; layout "bins" (syg_chroma_fold_bins_f32): x bin-major [B, K, T] real or [B, K, T, 2] complex (as
    cqt leaves it; rows may be strided over B and K), table [n_chroma, K].  A complex input gives |x|^power (1 or 2) on
    load.  threshold: sums below it become 0 (None: none); norm: inf, 1, 2 or None.  transform [P, n_chroma] (bins only):
    the result is transform @ the L1-normalised frame, [B, P, T] (tonnetz).  float32 sums in a fixed order: a batch equals
    its rows and a call repeats its bits."""
    who = "chroma_fold"
    if layout not in ("rows", "bins"):
        raise ValueError(f"{who}: layout must be 'rows' or 'bins' (got {layout!r})")
    pw = _chroma_power(power, who)
    has_thr, thr = CH.check_threshold(threshold, who)
    nrm = CH.check_norm(norm, who)
    if transform is not None and layout != "bins":
        raise ValueError(f"{who}: transform= is served by layout 'bins' alone")
    x, cplx = _chroma_spec(x, who, "[B, T, F(, 2)]" if layout == "rows" else "[B, K, T(, 2)]")
    cols = int(x.shape[2] if layout == "rows" else x.shape[1])
    tshape = tuple(table.shape) if hasattr(table, "shape") else np.shape(table)
    if len(tshape) != 2 or tshape[1] != cols:
        raise ValueError(f"{who}: table must be [n_chroma, {cols}] for this input (got {list(tshape)})")
    nc = CH.check_n_chroma(int(tshape[0]), who)
    P = 0
    if transform is not None:
        pshape = tuple(transform.shape) if hasattr(transform, "shape") else np.shape(transform)
        if len(pshape) != 2 or pshape[1] != nc or not 1 <= pshape[0] <= 8:
            raise ValueError(f"{who}: transform must be [P, {nc}] with 1 <= P <= 8 (got {list(pshape)})")
        P = int(pshape[0])
    B = int(x.shape[0])
    _on_device(x, f"{who}: x")
    if cplx and x.data_ptr() % 8:
        x = x.clone(memory_format=torch.contiguous_format)           # the kernels load (re, im) as one 8-byte word
    if layout == "rows":
        x = x.contiguous()
        Tn = int(x.shape[1])
        out = _out(out, (B, nc, Tn), x, f"{who}: out", contiguous=True)
        tab = _chroma_table(table, nc, who)
        _call("syg_chroma_fold_rows_f32", _ptr(x), B, Tn, cols, int(cplx), pw, _ptr(tab), nc, has_thr, thr, nrm, _ptr(out))
        return out
    if x.stride(-1) != 1 or (cplx and x.stride(2) != 2) or (not cplx and x.shape[2] > 1 and x.stride(2) != 1):
        x = x.contiguous()
    Tn = int(x.shape[2])
    w = 2 * Tn if cplx else Tn
    sxk = int(x.stride(1)) if cols > 1 else w
    sxb = int(x.stride(0)) if B > 1 else (cols - 1) * sxk + w
    if sxk < w or sxb < (cols - 1) * sxk + w or (cplx and (sxk % 2 or sxb % 2)):
        x = x.contiguous()
        sxk, sxb = w, cols * w
    out = _out(out, (B, P or nc, Tn), x, f"{who}: out", contiguous=True)
    wt = _chroma_table(table, nc, who, transpose=True)
    phi = _chroma_table(transform, P, who, "transform") if P else None
    for b0, bc in _row_blocks(B):
        _call("syg_chroma_fold_bins_f32", _ptr(x[b0:b0 + bc]), bc, cols, Tn, sxb, sxk, int(cplx), pw, _ptr(wt), nc, has_thr, thr,
              nrm, _ptr(phi), P, _ptr(out[b0:b0 + bc]))
    return out


def chroma_cens(chroma: torch.Tensor, win_len_smooth=41, smoothing_window="hann", norm=2,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The CENS steps after the fold (syg_chroma_cens_f32) of an unnormalised chroma [B, n_chroma, T]: the L1 norm per frame,
    the quantiser (0.25 per step 0.4 / 0.2 / 0.1 / 0.05 below the value), the smoothing along T with
    get_window(smoothing_window, win_len_smooth + 2, fftbins=False) / its sum (zeros beyond the row; None: none), the
    closing norm (librosa: 2).  Rows may be strided over B and n_chroma; `out` is contiguous."""
    who = "chroma_cens"
    wl = CH.check_win_len_smooth(win_len_smooth, who)
    nrm = CH.check_norm(norm, who)
    x = _dyn_in(chroma, who)
    B, nc, Tn = x.shape
    CH.check_n_chroma(nc, who)
    if B * nc * Tn > CH.MAX_ELEMS:
        raise ValueError(f"{who}: an input of more than 2^31 elements; call it on fewer rows")
    taps, left = CH.cens_window(wl, smoothing_window)
    _on_device(x, f"{who}: chroma")
    out = _out(out, (B, nc, Tn), x, f"{who}: out", contiguous=True)
    wkey = smoothing_window if isinstance(smoothing_window, (str, tuple)) else ("arr", np.asarray(smoothing_window).tobytes())
    wdev = _cached(("cens_win", wl, wkey), lambda: _dev(taps), limit=16)
    sxb, sxk = _dyn_strides(x)
    _call("syg_chroma_cens_f32", _ptr(x), B, nc, Tn, sxb, sxk, _ptr(wdev), len(taps), left, nrm, _ptr(out))
    return out


def _tuning_in(S, sr, n_fft, power, fmin, fmax, threshold, who: str):
    n_fft = CH.check_n_fft(n_fft, who)
    pw = _chroma_power(power, who)
    thr = CH.check_pip(threshold, None, who)
    k_lo, k_hi = CH.pip_bins(sr, n_fft, fmin, fmax)
    S, cplx = _chroma_spec(S, who, "[B, T, F(, 2)]")
    if S.shape[2] != 1 + n_fft // 2:
        raise ValueError(f"{who}: S has {S.shape[2]} bins, not 1 + n_fft // 2 = {1 + n_fft // 2}")
    _on_device(S, f"{who}: S")
    S = S.contiguous()
    if cplx and S.data_ptr() % 8:
        S = S.clone()                                                # (re, im) is loaded as one 8-byte word
    return S, cplx, n_fft, pw, thr, k_lo, k_hi


def tuning_hist(S: torch.Tensor, sr: float = 22050, n_fft: int = 2048, power: int = 1, fmin: float = 150.0, fmax: float = 4000.0,
                threshold: float = 0.1, resolution: float = 0.01, bins_per_octave: int = 12, out=None):
    """estimate_tuning's histogram per clip (syg_tuning_hist_f32) of S frame-major [B, T, F] real, or [B, T, F, 2] complex with
    |S|^power taken on load -> (counts [B, ceil(1 / resolution)] int32, n_peaks [B] int32): piptrack's peaks in float64 from the
    float32 S, the exact median of their magnitudes, the residuals of those at or above it counted by
    _chroma.tuning_bins(resolution).  out: (counts, n_peaks)."""
    who = "tuning_hist"
    nb = CH.check_resolution(resolution, who)
    if not (isinstance(bins_per_octave, (int, np.integer)) and bins_per_octave >= 1):
        raise ValueError(f"{who}: bins_per_octave must be a positive integer")
    S, cplx, n_fft, pw, thr, k_lo, k_hi = _tuning_in(S, sr, n_fft, power, fmin, fmax, threshold, who)
    B, Tn, F = (int(v) for v in S.shape[:3])
    counts = _out(out[0] if out else None, (B, nb), S, f"{who}: out[0]", torch.int32, contiguous=True)
    npk = _out(out[1] if out else None, (B,), S, f"{who}: out[1]", torch.int32, contiguous=True)
    edges = _cached(("tuning_bins", nb), lambda: _dev(CH.tuning_bins(resolution)))
    work = _workspace("syg_tuning_hist_work_bytes", B, Tn, k_lo, k_hi, dtype=torch.float64, device=S.device)
    _call("syg_tuning_hist_f32", _ptr(S), B, Tn, F, int(cplx), pw, float(sr), n_fft, k_lo, k_hi, thr, float(bins_per_octave),
          _ptr(edges), nb, _ptr(counts), _ptr(npk), None, None, _ptr(work), _nbytes(work))
    return counts, npk


def piptrack(S: torch.Tensor, sr: float = 22050, n_fft: int = 2048, power: int = 1, fmin: float = 150.0, fmax: float = 4000.0,
             threshold: float = 0.1, out=None):
    """librosa.piptrack of S frame-major [B, T, F] (or complex [B, T, F, 2], |S|^power on load) -> (pitches, magnitudes)
    float32 [B, T, F], zero away from the peaks (syg_tuning_hist_f32 without the histogram)."""
    who = "piptrack"
    S, cplx, n_fft, pw, thr, k_lo, k_hi = _tuning_in(S, sr, n_fft, power, fmin, fmax, threshold, who)
    B, Tn, F = (int(v) for v in S.shape[:3])
    pitch = _out(out[0] if out else None, (B, Tn, F), S, f"{who}: out[0]", contiguous=True)
    mag = _out(out[1] if out else None, (B, Tn, F), S, f"{who}: out[1]", contiguous=True)
    _call("syg_tuning_hist_f32", _ptr(S), B, Tn, F, int(cplx), pw, float(sr), n_fft, k_lo, k_hi, thr, 12.0, None, 0, None, None,
          _ptr(pitch), _ptr(mag), None, 0)
    return pitch, mag


def estimate_tuning(S: torch.Tensor, sr: float = 22050, n_fft: int = 2048, power: int = 1, resolution: float = 0.01,
                    bins_per_octave: int = 12, fmin: float = 150.0, fmax: float = 4000.0, threshold: float = 0.1) -> np.ndarray:
    """librosa.estimate_tuning of every clip of S (as tuning_hist takes it) -> float64 [B] on the host: the left edge of the
    first fullest bin of tuning_hist's counts, in fractions of a bin; a clip without a peak gives 0.0 under librosa's
    warning."""
    import warnings
    counts, npk = tuning_hist(S, sr, n_fft, power, fmin, fmax, threshold, resolution, bins_per_octave)
    edges = CH.tuning_bins(resolution)
    k = np.argmax(counts.cpu().numpy(), axis=1)                      # the first fullest bin
    n = npk.cpu().numpy()
    if (n == 0).any():
        warnings.warn("Trying to estimate tuning from empty frequency set.", stacklevel=2)
    return np.where(n == 0, 0.0, edges[k])


# ------------------------------------------------------------------ loudness: BS.1770 / EBU R128 meter and normaliser
_LOUDNESS_KEYS = ("chunk", "fs_min", "fs_max", "momentary_segments", "short_term_segments", "true_peak_tile", "true_peak_up_max",
                  "true_peak_taps_max")                                                              # SYG_LOUDNESS_*


def loudness_constants() -> dict:
    """The figures the loudness kernels rest on (the library owns them): samples of a chunk of the segment-power passes, the
    lowest and highest rate served, the 100 ms segments of a momentary and of a short-term block, the input samples a
    true-peak workgroup stages at a time, the largest oversampling factor and the most taps per phase."""
    return _constants("syg_loudness_constants", _LOUDNESS_KEYS)


def _loud_clips(y, who: str):
    """First stage, judged without a device: y is float32 [B, L] (mono) or [B, C, L] with at least one sample.  Returns
    the [B, C, L] view."""
    if not isinstance(y, torch.Tensor) or y.dtype != torch.float32 or y.dim() not in (2, 3):
        raise ValueError(f"{who}: y must be a float32 tensor [B, L] (mono) or [B, C, L]")
    if y.dim() == 2:
        y = y.unsqueeze(1)
    if min(y.shape) < 1:
        raise ValueError(f"{who}: empty input (shape {list(y.shape)}: at least one clip, one channel and one sample)")
    return y


def _loud_strides(x: torch.Tensor):
    return int(x.stride(0)) if x.shape[0] > 1 else 0, int(x.stride(1)) if x.shape[1] > 1 else 0


def loudness_segments(y: torch.Tensor, fs: int) -> torch.Tensor:
    """Sum of the squared K-weighted signal over every whole 100 ms segment (syg_loudness_segments_f32): y [B, L] or
    [B, C, L] float32 on the device (unit stride along L, any stride over B and C) -> float64 [B, C, n_seg],
    n_seg = 10 L div fs.  The filtered signal is never written."""
    who = "loudness_segments"
    x = _loud_clips(y, who)
    fs = LD.check_fs(fs, who)
    _on_device(x, f"{who}: y")
    x = _unit_stride(x)
    B, Cn, L = x.shape
    n_seg = LD.n_segments(L, fs)
    seg = torch.empty((B, Cn, n_seg), dtype=torch.float64, device=x.device)
    if n_seg:
        work = _workspace("syg_loudness_segments_work_bytes", B, Cn, L, fs, dtype=torch.float64, device=x.device)
        sos = LD.k_weighting_sos(fs)
        _call("syg_loudness_segments_f32", _ptr(x), B, Cn, L, *_loud_strides(x), fs, sos.ctypes.data_as(C.c_void_p), _ptr(seg),
              _ptr(work))
    return seg


def loudness_blocks(seg: torch.Tensor, fs: int, channel_weights=None):
    """Segment powers [B, C, n_seg] float64 -> (M, S, I, lra_thr) on the device (syg_loudness_blocks_f64): momentary
    [B, n_m] and short-term [B, n_s] LUFS float32 (-inf where the power is 0), integrated loudness [B] float64 (-inf where
    no block passes the gates) and the threshold [B] float64 that loudness_range gates S with.  channel_weights: one per
    channel; default ones up to 3 channels and BS.1770's 1, 1, 1, 1.41, 1.41 for 5."""
    who = "loudness_blocks"
    if not isinstance(seg, torch.Tensor) or seg.dtype != torch.float64 or seg.dim() != 3 or seg.shape[0] < 1 or seg.shape[1] < 1:
        raise ValueError(f"{who}: seg must be a float64 tensor [B, C, n_seg] (loudness_segments' result)")
    fs = LD.check_fs(fs, who)
    B, Cn, n_seg = seg.shape
    w64 = LD.channel_weights(Cn, channel_weights)
    _on_device(seg, f"{who}: seg")
    seg = seg.contiguous()
    w = _cached(("loudness_w", w64.tobytes()), lambda: _dev(w64), limit=16)
    M = torch.empty((B, max(0, n_seg - LD.MOMENTARY + 1)), dtype=torch.float32, device=seg.device)
    S = torch.empty((B, max(0, n_seg - LD.SHORT_TERM + 1)), dtype=torch.float32, device=seg.device)
    integ = torch.empty(B, dtype=torch.float64, device=seg.device)
    thr = torch.empty(B, dtype=torch.float64, device=seg.device)
    _call("syg_loudness_blocks_f64", _ptr(seg), B, Cn, n_seg, fs, _ptr(w), _ptr(M), M.shape[1], _ptr(S), S.shape[1], _ptr(integ),
          _ptr(thr))
    return M, S, integ, thr


def loudness_range(S: torch.Tensor, lra_thr: torch.Tensor) -> torch.Tensor:
    """EBU Tech 3342's loudness range [B] float32 (LU) from loudness_blocks' short-term rows S [B, n_s] and threshold
    [B]: the rows are sorted by torch.sort (1/4800 of the input) and the two percentiles of the values above the threshold
    are picked on the device (syg_loudness_lra_f32); 0 where fewer than two values are."""
    _f32(S, "loudness_range: S", 2)
    B, n_s = S.shape
    if B < 1 or not isinstance(lra_thr, torch.Tensor) or lra_thr.dtype != torch.float64 or tuple(lra_thr.shape) != (B,):
        raise ValueError(f"loudness_range: lra_thr must be a float64 tensor [{B}] (loudness_blocks' threshold), S at least one row")
    _on_device(S, "loudness_range: S")
    v = torch.sort(S, dim=1).values.contiguous()
    lra = torch.empty(B, dtype=torch.float32, device=S.device)
    _call("syg_loudness_lra_f32", _ptr(v), B, n_s, n_s, _ptr(lra_thr.contiguous()), _ptr(lra))
    return lra


def integrated_loudness(y: torch.Tensor, fs: int, channel_weights=None) -> torch.Tensor:
    """Integrated loudness [B] float64 (LUFS) of y [B, L] or [B, C, L]: loudness_segments, then loudness_blocks' gates."""
    who = "integrated_loudness"
    x = _loud_clips(y, who)
    fs = LD.check_fs(fs, who)
    LD.channel_weights(x.shape[1], channel_weights)
    return loudness_blocks(loudness_segments(x, fs), fs, channel_weights)[2]


def true_peak(y: torch.Tensor, fs: int) -> torch.Tensor:
    """Linear true peak [B] float32 of y [B, L] or [B, C, L] (syg_true_peak_f32): the largest |value| over the channels of
    resample_poly(y, up, 1) with the default filter and padtype="constant", up = 4 below 96 kHz, 2 below 192 kHz, else 1
    (the sample peak).  Every value is resample_poly's own; the oversampled signal is never written."""
    who = "true_peak"
    x = _loud_clips(y, who)
    fs = LD.check_fs(fs, who)
    _on_device(x, f"{who}: y")
    x = _unit_stride(x)
    B, Cn, L = x.shape
    up = LD.true_peak_up(fs)
    p, table = resample_plan(up, 1, L) if up > 1 else (None, None)
    peak = torch.empty(B, dtype=torch.float32, device=x.device)
    _call("syg_true_peak_f32", _ptr(x), B, Cn, L, *_loud_strides(x), up, p.n_pre_remove if p else 0, p.Kp if p else 0, _ptr(table),
          _ptr(peak))
    return peak


def loudness_gain(integ: torch.Tensor, target_lufs: float, peak: Optional[torch.Tensor] = None,
                  peak_limit_dbtp: Optional[float] = None) -> torch.Tensor:
    """Gains [B] float64 on the device (syg_loudness_gain_f64): 10^((target - I) / 20), lowered where gain x peak would
    pass 10^(peak_limit_dbtp / 20) (peak: true_peak's linear [B]), 1 where I is not finite."""
    who = "loudness_gain"
    if not isinstance(integ, torch.Tensor) or integ.dtype != torch.float64 or integ.dim() != 1 or integ.shape[0] < 1:
        raise ValueError(f"{who}: integ must be a float64 tensor [B]")
    if not np.isfinite(target_lufs) or (peak_limit_dbtp is not None and not np.isfinite(peak_limit_dbtp)):
        raise ValueError(f"{who}: target_lufs and peak_limit_dbtp must be finite")
    if (peak is None) != (peak_limit_dbtp is None):
        raise ValueError(f"{who}: peak and peak_limit_dbtp go together")
    if peak is not None:
        _f32(peak, f"{who}: peak", 1, (integ.shape[0],))
    _on_device(integ, f"{who}: integ")
    gain = torch.empty_like(integ, memory_format=torch.contiguous_format)
    _call("syg_loudness_gain_f64", _ptr(integ.contiguous()), _ptr(peak.contiguous() if peak is not None else None), integ.shape[0],
          float(target_lufs), float(peak_limit_dbtp or 0.0), _ptr(gain))
    return gain


def gain_rows(y: torch.Tensor, gain: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [B, L] or [B, C, L] float32 times the clip's gain[b] (float64 [B] on the device), rounded once
    (syg_gain_rows_f32).  `out` may be y."""
    who = "gain_rows"
    x = _loud_clips(y, who)
    B, Cn, L = x.shape
    if not isinstance(gain, torch.Tensor) or gain.dtype != torch.float64 or tuple(gain.shape) != (B,):
        raise ValueError(f"{who}: gain must be a float64 tensor [{B}]")
    _on_device(x, f"{who}: y")
    x = _unit_stride(x)
    out = _out(out, y.shape, x)
    o = out.unsqueeze(1) if out.dim() == 2 else out
    _call("syg_gain_rows_f32", _ptr(x), B, Cn, L, *_loud_strides(x), _ptr(gain.contiguous()), _ptr(o), int(o.stride(0)),
          int(o.stride(1)))
    return out


def normalize_loudness(y: torch.Tensor, fs: int, target_lufs: float = -23.0, peak_limit_dbtp: Optional[float] = None,
                       channel_weights=None, return_gain: bool = False):
    """y [B, L] or [B, C, L] scaled so that every clip's integrated loudness is target_lufs; with peak_limit_dbtp the gain is
    lowered so that the true peak stays at or under it.  A clip without a finite loudness (silence, shorter than a block)
    is copied.  Measuring, the gain and its application are launches on one stream: the host waits for nothing.
    return_gain: (out, gain [B] float64, I [B] float64)."""
    who = "normalize_loudness"
    x = _loud_clips(y, who)
    fs = LD.check_fs(fs, who)
    LD.channel_weights(x.shape[1], channel_weights)
    if not np.isfinite(target_lufs) or (peak_limit_dbtp is not None and not np.isfinite(peak_limit_dbtp)):
        raise ValueError(f"{who}: target_lufs and peak_limit_dbtp must be finite")
    integ = integrated_loudness(x, fs, channel_weights)
    peak = true_peak(x, fs) if peak_limit_dbtp is not None else None
    gain = loudness_gain(integ, target_lufs, peak, peak_limit_dbtp)
    out = gain_rows(y, gain)
    return (out, gain, integ) if return_gain else out


# ------------------------------------------------------------------ features back to audio
# Geometry of everything here: n_fft 2048, hann, win_length 2048, hop 512, centred (what istft2048 serves).


def _gl_stft_args(who, n_fft=2048, hop_length=None, win_length=None, window="hann", center=True):
    win_length = 2048 if win_length is None else win_length
    hop = 512 if hop_length is None else hop_length
    if n_fft != 2048 or win_length != 2048 or hop != 512 or not isinstance(window, str) or window != "hann" or not center:
        raise ValueError(f"{who}: only n_fft=2048, window='hann', win_length=2048, hop_length=512 and center=True are served "
                         f"(got n_fft={n_fft}, window={window!r}, win_length={win_length}, hop_length={hop}, center={center})")


def gl_alpha(momentum) -> float:
    """momentum / (1 + momentum) rounded once to float32: the alpha every projection of a run is given.  momentum must be
    in [0, 1) (librosa warns above 1; here it is refused)."""
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float, np.integer, np.floating)) or not 0 <= momentum < 1:
        raise ValueError(f"griffinlim: momentum must be in [0, 1) (got {momentum!r})")
    return float(np.float32(float(momentum) / (1.0 + float(momentum))))


def _gl_spectra(who, R, P, S):
    """The checks of a projection's inputs: S [B, T, 1025], R and P [B, T, 1025, 2], float32 on the device, made
    contiguous (as istft2048 makes D)."""
    _f32(S, f"{who}: S", 3, (1025,), "[B, T, 1025]")
    B, Tn = int(S.shape[0]), int(S.shape[1])
    if B < 1 or Tn < 1:
        raise ValueError(f"{who}: empty input (S has shape {list(S.shape)})")
    for t, name in ((R, "R"), (P, "P")):
        if t is not None:
            _f32(t, f"{who}: {name}", 4, (Tn, 1025, 2), f"[{B}, {Tn}, 1025, 2]")
            if t.shape[0] != B:
                raise ValueError(f"{who}: {name} must be a float32 tensor [{B}, {Tn}, 1025, 2]")
    _on_device(S, f"{who}: S")
    return (R.contiguous(), P.contiguous() if P is not None else None, S.contiguous(), B, Tn)


def gl_project(R: torch.Tensor, S: torch.Tensor, P: Optional[torch.Tensor] = None, alpha: float = 0.0,
               out: Optional[torch.Tensor] = None, return_sums: bool = False):
    """Griffin-Lim's projection (syg_gl_project_f32): D = S A / (|A| + FLT_MIN), A = R - alpha P (A = R without P), for
    spectra [B, T, 1025, 2] and magnitudes S [B, T, 1025].  alpha: gl_alpha(momentum).  `out` may be R.  return_sums adds
    [B, 2] float64: per clip sum (|R| - S)^2 and sum S^2, whose ratio's root is the spectral convergence of R."""
    who = "gl_project"
    if R is None:
        raise ValueError(f"{who}: R must be a float32 tensor [B, T, 1025, 2]")
    if not 0 <= alpha < 0.5:
        raise ValueError(f"{who}: alpha = momentum / (1 + momentum) must be in [0, 0.5) (got {alpha!r})")
    R, P, S, B, Tn = _gl_spectra(who, R, P, S)
    D = _out(out, R.shape, R, contiguous=True)
    sums = work = None
    if return_sums:
        sums = torch.empty((B, 2), dtype=torch.float64, device=R.device)
        work = _workspace("syg_gl_project_work_bytes", B, Tn, dtype=torch.float64, device=R.device)
    _call("syg_gl_project_f32", _ptr(R), _ptr(P), _ptr(S), B, Tn, float(alpha), _ptr(D), _ptr(sums), _ptr(work))
    return (D, sums) if return_sums else D


def griffinlim(S: torch.Tensor, n_iter: int = 32, momentum: float = 0.99, init="random", seed: int = 0, first_row: int = 0,
               length: Optional[int] = None, angles: Optional[torch.Tensor] = None, return_trace: bool = False,
               chunk: Optional[int] = None):
    """librosa 0.10 `griffinlim` on magnitudes S [B, T, 1025] float32 (frame-major, as stft2048_c2c lays its frames) ->
    y [B, length] float32; n_fft 2048, hann, hop 512, centred.  Project, then n_iter x (inverse, forward, project with the
    previous rebuilt spectrum), then a final inverse.

    init: "random" draws the first spectrum as randn(B, T * 1025 * 2, seed, first_row) -- a normalised pair of normals is
    a uniform phase; clip b of a batch is the single clip first_row + b --, None starts from phases of 1; `angles`
    [B, T, 1025, 2] gives the starting phases instead (any modulus: it is projected).  length defaults to 512 (T - 1) and
    must frame to T (1 + length // 512 == T).  momentum in [0, 1).

    An iteration is three launches: syg_gl_project_f32, syg_istft2048_f32, syg_stft2048_c2c_f32, over two rebuilt spectra
    and the projected one.  (An inverse STFT that projected on its load, so that the projected spectrum was never written,
    measured slower than the two launches and is not kept: DESIGN.md, "Feature inversion".)  return_trace adds
    [B, n_iter] float64, the spectral convergence sqrt(sum (|R| - S)^2 / sum S^2) of each rebuilt spectrum, from sums the
    projection adds in float64 while it reads R and S anyway; the clip is the same bit for bit with or without it.

    chunk: clips that run all their iterations before the next ones start, to bound the three work spectra (clips are
    independent: the result is the same bit for bit whatever the chunk).  None: the whole batch at once.  Chunks sized to
    keep a chunk's spectra in the Infinity Cache measured three times slower at 1024 clips of 65 frames (the inverse's
    waves no longer fill the device), so no chunk is chosen for the caller."""
    who = "griffinlim"
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
        raise ValueError(f"{who}: n_iter must be a non-negative integer (got {n_iter!r})")
    alpha = gl_alpha(momentum)
    if not (init is None or (isinstance(init, str) and init == "random")):
        raise ValueError(f"{who}: init must be 'random' or None (got {init!r})")
    _f32(S, f"{who}: S", 3, (1025,), "[B, T, 1025]")
    B, Tn = int(S.shape[0]), int(S.shape[1])
    if B < 1 or Tn < 1:
        raise ValueError(f"{who}: empty input (S has shape {list(S.shape)})")
    if length is None:
        if Tn < 2:
            raise ValueError(f"{who}: T={Tn} frames give the default length 512 (T - 1) = 0; pass length")
        length = 512 * (Tn - 1)
    length = int(length)
    if length < 1 or 1 + length // 512 != Tn:
        raise ValueError(f"{who}: length={length} frames to {1 + max(length, 0) // 512} frames, S has {Tn}")
    if angles is not None:
        _f32(angles, f"{who}: angles", 4, (Tn, 1025, 2), f"[{B}, {Tn}, 1025, 2]")
        if angles.shape[0] != B:
            raise ValueError(f"{who}: angles must be a float32 tensor [{B}, {Tn}, 1025, 2]")
    elif init == "random":
        seed, first_row = RNG.check_seed(seed), RNG.check_rows(first_row, B)
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1):
        raise ValueError(f"{who}: chunk must be a positive integer or None (got {chunk!r})")
    _on_device(S, f"{who}: S")
    S = S.contiguous()
    step = B if chunk is None else min(int(chunk), B)
    y = torch.empty((B, length), dtype=torch.float32, device=S.device)
    trace = torch.empty((B, n_iter), dtype=torch.float64, device=S.device) if return_trace else None
    nb = min(step, B)
    bufs = [torch.empty((nb, Tn, 1025, 2), dtype=torch.float32, device=S.device) for _ in range(3)]
    for lo in range(0, B, step):
        n = min(step, B - lo)
        Sc = S[lo:lo + n]
        cur, prev, D = bufs[0][:n], bufs[1][:n], bufs[2][:n]
        if angles is not None:
            cur.copy_(angles[lo:lo + n])
        elif init == "random":
            randn(n, Tn * 1025 * 2, seed, first_row + lo, out=cur.view(n, -1))
        else:
            cur.zero_()
            cur[..., 0] = 1.0
        yc = y[lo:lo + n]
        P = None
        for i in range(n_iter + 1):
            # cur: the rebuilt spectrum of iteration i (the starting spectrum at i = 0); P: the one before it
            if return_trace and i > 0:
                _, sums = gl_project(cur, Sc, P, alpha, out=D, return_sums=True)
                trace[lo:lo + n, i - 1] = torch.sqrt(sums[:, 0] / sums[:, 1])
            else:
                gl_project(cur, Sc, P, alpha, out=D)
            _call("syg_istft2048_f32", _ptr(D), n, Tn, 512, 1, length, _ptr(window64_dev()), _ptr(twiddle_dev(2048)), None,
                  _ptr(yc), None, None, length)
            if i == n_iter:
                break
            nxt = prev                     # the spectrum before last is no longer needed: the forward STFT overwrites it
            _call("syg_stft2048_c2c_f32", _ptr(yc), n, length, length, 512, 1, Tn, _ptr(window_dev("hann", 2048, 2048)),
                  _ptr(twiddle_dev(2048)), _ptr(nxt))
            # (the starting spectrum is nobody's previous one: the first rebuilt spectrum is projected alone)
            prev, cur, P = cur, nxt, (cur if i >= 1 else None)
    return (y, trace) if return_trace else y


def _inv_dense(who, X, W: torch.Tensor, pre_ref=None, post=None, power: float = 2.0, ref: float = 1.0,
               mel_major_out: bool = False) -> torch.Tensor:
    X = _f32_in(X, f"{who}: input", 3).contiguous()
    B, M, Tn = (int(v) for v in X.shape)
    F = int(W.shape[0])
    if B < 1 or M < 1 or Tn < 1 or W.shape[1] != M:
        raise ValueError(f"{who}: input must be [B, {int(W.shape[1])}, T] with B, T >= 1 (got {list(X.shape)})")
    out = torch.empty((B, F, Tn) if mel_major_out else (B, Tn, F), dtype=torch.float32, device=X.device)
    _call("syg_inv_dense_f32", _ptr(X), B, M, Tn, _ptr(W), F, int(pre_ref is not None), float(pre_ref or 1.0),
          {None: 0, "root": 1, "db": 2}[post], float(ref if post == "db" else power), _ptr(out), int(mel_major_out))
    return out


def inv_dense(X: torch.Tensor, W: torch.Tensor, pre_ref: Optional[float] = None, post: Optional[str] = None, power: float = 2.0,
              ref: float = 1.0, mel_major_out: bool = False) -> torch.Tensor:
    """out[b, t, f] = post(sum_m W[f, m] pre(X[b, m, t])) (syg_inv_dense_f32): X mel-major [B, M, T], W [F, M] float32 on
    the device, out frame-major [B, T, F], or [B, F, T] with mel_major_out.  pre_ref: X is in dB relative to it
    (pre = pre_ref 10^(x / 10)); post: None, "root" (max(., 0)^(1 / power)) or "db" (ref 10^(. / 10))."""
    who = "inv_dense"
    if post not in (None, "root", "db"):
        raise ValueError(f"{who}: post must be None, 'root' or 'db' (got {post!r})")
    for v, name in ((pre_ref, "pre_ref"), (power, "power"), (ref, "ref")):
        if v is not None and not (np.isfinite(v) and v > 0):
            raise ValueError(f"{who}: {name} must be positive and finite (got {v!r})")
    _f32(W, f"{who}: W", 2)
    _on_device(W, f"{who}: W")
    return _inv_dense(who, X, W.contiguous(), pre_ref, post, power, ref, mel_major_out)


def idct_lifter_table(n_mfcc: int, n_mels: int, dct_type: int = 2, norm="ortho", lifter: float = 0) -> np.ndarray:
    """W [n_mels, n_mfcc] float32 of mfcc_to_mel: the transpose of _tables.dct_matrix -- the inverse of the orthonormal
    DCT of zero-padded coefficients, scipy's idct(n=n_mels) -- with the lifter divided out as librosa does."""
    who = "mfcc_to_mel"
    if norm != "ortho" or dct_type not in (2, 3):
        raise ValueError(f"{who}: only norm='ortho' with dct_type 2 or 3 is served: the transpose inverts no other "
                         f"(got dct_type={dct_type}, norm={norm!r})")
    W = T.dct_matrix(int(n_mfcc), int(n_mels), dct_type, norm).astype(np.float64).T
    lw = T.lifter_weights(int(n_mfcc), float(lifter))
    if lw is not None:
        lw = 1.0 + (float(lifter) / 2.0) * np.sin(np.pi * np.arange(1, int(n_mfcc) + 1) / float(lifter))
        if np.any(lw == 0.0):
            raise ValueError(f"{who}: lifter={lifter} has a zero weight, which cannot be divided out")
        W = W / lw[None, :]
    return np.ascontiguousarray(W.astype(np.float32))


def mel_pinv_table(sr: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax=None) -> np.ndarray:
    """pinv(_tables.mel_filterbank(...)) [1 + n_fft / 2, n_mels], computed in float64, as float32."""
    return np.ascontiguousarray(np.linalg.pinv(T.mel_filterbank(sr, n_fft, n_mels, fmin, fmax).astype(np.float64)).astype(np.float32))


def mfcc_to_mel(mfcc: torch.Tensor, n_mels: int = 128, dct_type: int = 2, norm="ortho", ref: float = 1.0, lifter: float = 0,
                as_db: bool = False) -> torch.Tensor:
    """librosa.feature.inverse.mfcc_to_mel on MFCC rows [B, K, T] -> mel power [B, n_mels, T] float32 (mel-major, the
    layout mel rows have here): the inverse DCT with the lifter divided out, then db_to_power(ref).  as_db: the log-mel
    rows in dB, before db_to_power (mel_to_stft(db_ref=ref) converts them on its load)."""
    who = "mfcc_to_mel"
    _f32(mfcc, f"{who}: mfcc", 3, axes="[B, n_mfcc, T]")
    K = int(mfcc.shape[1])
    if not (np.isfinite(ref) and ref > 0):
        raise ValueError(f"{who}: ref must be positive and finite (got {ref!r})")
    if K < 1 or K > n_mels:
        raise ValueError(f"{who}: n_mfcc={K} must be in [1, n_mels={n_mels}]")
    W = idct_lifter_table(K, n_mels, dct_type, norm, lifter)         # (checked before any device work)
    _on_device(mfcc, f"{who}: mfcc")
    Wd = _cached(("idct", K, int(n_mels), dct_type, float(lifter)), lambda: _dev(W), limit=8)
    return _inv_dense(who, mfcc, Wd, None, None if as_db else "db", ref=ref, mel_major_out=True)


def mel_to_stft(mel: torch.Tensor, sr: float = 22050, n_fft: int = 2048, power: float = 2.0, fmin: float = 0.0, fmax=None,
                db_ref: Optional[float] = None) -> torch.Tensor:
    """Mel power rows [B, M, T] -> magnitudes S [B, T, 1025] float32: max(pinv(mel_filterbank) mel, 0)^(1 / power).

    This is the minimum-norm least-squares inverse, clipped at zero: torchaudio's InverseMelScale, NOT librosa's
    mel_to_stft.  librosa solves a non-negative least-squares problem by L-BFGS; with 128 equations and 1025 unknowns it
    is underdetermined, and its answer depends on the solver's path, so there is nothing to pin.  db_ref: mel holds dB
    relative to it (mfcc_to_mel(as_db=True)) and is converted on load."""
    who = "mel_to_stft"
    _gl_stft_args(who, n_fft)
    _f32(mel, f"{who}: mel", 3, axes="[B, n_mels, T]")
    M = int(mel.shape[1])
    if M < 1 or M > 1025:
        raise ValueError(f"{who}: n_mels={M} must be in [1, 1025]")
    for v, name in ((power, "power"), (db_ref, "db_ref")):
        if v is not None and not (np.isfinite(v) and v > 0):
            raise ValueError(f"{who}: {name} must be positive and finite (got {v!r})")
    _on_device(mel, f"{who}: mel")
    Wd = _cached(("melpinv", float(sr), M, float(fmin), None if fmax is None else float(fmax)),
                 lambda: _dev(mel_pinv_table(sr, 2048, M, fmin, fmax)), limit=8)
    return _inv_dense(who, mel, Wd, db_ref, "root", power=power)


def mel_to_audio(mel: torch.Tensor, sr: float = 22050, n_fft: int = 2048, power: float = 2.0, fmin: float = 0.0, fmax=None,
                 n_iter: int = 32, momentum: float = 0.99, seed: int = 0, first_row: int = 0, length: Optional[int] = None,
                 db_ref: Optional[float] = None) -> torch.Tensor:
    """griffinlim(mel_to_stft(mel)): mel power rows [B, M, T] -> clips [B, length]."""
    return griffinlim(mel_to_stft(mel, sr, n_fft, power, fmin, fmax, db_ref), n_iter, momentum, "random", seed, first_row, length)


def mfcc_to_audio(mfcc: torch.Tensor, n_mels: int = 128, dct_type: int = 2, norm="ortho", ref: float = 1.0, lifter: float = 0,
                  sr: float = 22050, fmin: float = 0.0, fmax=None, n_iter: int = 32, momentum: float = 0.99, seed: int = 0,
                  first_row: int = 0, length: Optional[int] = None) -> torch.Tensor:
    """mel_to_audio(mfcc_to_mel(mfcc)): the log-mel rows stay in dB between the two and become power on the second's load."""
    logmel = mfcc_to_mel(mfcc, n_mels, dct_type, norm, ref, lifter, as_db=True)
    return mel_to_audio(logmel, sr, 2048, 2.0, fmin, fmax, n_iter, momentum, seed, first_row, length, db_ref=ref)


# ------------------------------------------------------------------ non-negative matrix factorisation
# Frame-major: V [B, T, F] = A [B, T, K] C [B, K, F]; A is sklearn's W (activations), C its H (components).

_NMF_LOSSES = {"frobenius": 0, 2: 0, 2.0: 0, "kullback-leibler": 1, 1: 1, 1.0: 1}
_NMF_SERVED = ("served: beta_loss 'frobenius' (2) or 'kullback-leibler' (1), the multiplicative-update solver, "
               "init 'random' or given factors")


def nmf_constants() -> dict:
    """eps (float32's machine epsilon, sklearn's EPSILON) and the served ranges and tiles of csrc/nmf.hip."""
    d = _constants("syg_nmf_constants", ("max_components", "max_bins", "max_groups", "a_tile_frames", "a_chunk_bins",
                                         "c_tile_bins", "c_chunk_frames", "sums_chunk", "mfma_min_components"))
    d["eps"] = float(np.finfo(np.float32).eps)
    return d


def _nmf_loss(who, beta_loss) -> int:
    if isinstance(beta_loss, bool) or not isinstance(beta_loss, (str, int, float)) or beta_loss not in _NMF_LOSSES:
        raise ValueError(f"{who}: beta_loss={beta_loss!r} is not served (Itakura-Saito and other beta need powers of AC "
                         f"per entry); {_NMF_SERVED}")
    return _NMF_LOSSES[beta_loss]


def _nmf_factors(who, V, A, C, K=None):
    """The shape checks of (V, A, C), without a device: V [B, T, F], A [B, T, K], C [B, K, F] or [1, K, F].  Returns
    (B, T, F, K, c_shared)."""
    _f32(V, f"{who}: V", 3, (), "[B, T, F]")
    B, Tn, F = (int(n) for n in V.shape)
    if B < 1 or Tn < 1 or F < 1:
        raise ValueError(f"{who}: empty input (V has shape {list(V.shape)})")
    if F > 2049:
        raise ValueError(f"{who}: F={F} bins must be in [1, 2049]")
    if K is None:
        K = int(A.shape[-1]) if isinstance(A, torch.Tensor) and A.dim() == 3 else \
            int(C.shape[1]) if isinstance(C, torch.Tensor) and C.dim() == 3 else None
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= 64:
        raise ValueError(f"{who}: n_components={K!r} must be an integer in [1, 64]")
    K = int(K)
    if A is not None:
        _f32(A, f"{who}: A", 3, (Tn, K), f"[{B}, {Tn}, {K}]")
        if A.shape[0] != B:
            raise ValueError(f"{who}: A must be a float32 tensor [{B}, {Tn}, {K}]")
    shared = False
    if C is not None:
        _f32(C, f"{who}: C", 3, (K, F), f"[{B}, {K}, {F}] or [1, {K}, {F}]")
        if C.shape[0] != B and C.shape[0] != 1:
            raise ValueError(f"{who}: C must be a float32 tensor [{B}, {K}, {F}] or [1, {K}, {F}]")
        shared = C.shape[0] == 1 and B > 1
    return B, Tn, F, K, shared


_NMF_FORMS = {None: -1, "fma": 0, "mfma": 1}


def _nmf_on_device(who, V, **others):
    """V and every other tensor argument are on V's device (a host factor would hand the kernel a host pointer)."""
    _on_device(V, f"{who}: V")
    for name, t in others.items():
        if isinstance(t, torch.Tensor) and t.device != V.device:
            raise ValueError(f"{who}: {name} must be on the device of V ({V.device}; got {t.device})")


def nmf_divergence(V: torch.Tensor, A: torch.Tensor, C: torch.Tensor, beta_loss="frobenius") -> torch.Tensor:
    """sklearn's _beta_divergence of each clip (syg_nmf_divergence_f32): [B] float64, AC and the sums formed in float64 from
    the float32 factors.  Frobenius: sum (V - AC)^2 / 2; KL: sum over V > eps of V log(V / max(AC, eps)) - V, plus sum AC."""
    who = "nmf_divergence"
    loss = _nmf_loss(who, beta_loss)
    if A is None or C is None:
        raise ValueError(f"{who}: A and C must be float32 tensors")
    B, Tn, F, K, shared = _nmf_factors(who, V, A, C)
    _nmf_on_device(who, V, A=A, C=C)
    V, A, C = V.contiguous(), A.contiguous(), C.contiguous()
    out = torch.empty((B,), dtype=torch.float64, device=V.device)
    work = _workspace("syg_nmf_work_bytes", B, Tn, F, K, dtype=torch.float64, device=V.device)
    _call("syg_nmf_divergence_f32", _ptr(V), _ptr(A), _ptr(C), int(shared), B, Tn, F, K, loss, _ptr(out), _ptr(work))
    return out


def nmf(V: torch.Tensor, n_components: Optional[int] = None, *, A0: Optional[torch.Tensor] = None,
        C0: Optional[torch.Tensor] = None, n_iter: int = 200, beta_loss="frobenius", update_A: bool = True,
        update_C: bool = True, seed: int = 0, first_row: int = 0, return_trace: bool = False, solver: str = "mu",
        init: Optional[str] = None, form: Optional[str] = None):
    """Non-negative matrix factorisation V [B, T, F] ~ A [B, T, K] C [B, K, F] by multiplicative updates (syg_nmf_f32):
    scikit-learn's NMF(solver="mu", tol=0) in frame-major layout, A its W (activations), C its H (components).  Exactly
    n_iter iterations run, each the A-step, then the C-step with the new A; returns (A, C), new tensors (copies of A0 and
    C0 also where a factor is not updated).

    A0 / C0 start the factors; a missing one is drawn by sklearn's init="random" rule, sqrt(mean(V_b) / K) |randn|, from
    row first_row + b of `seed` (ops.randn; the components take the row's first K F normals, the activations the next
    T K), so clip b of a batch equals the single clip first_row + b.  C0 may be [1, K, F], one dictionary for every clip,
    with update_C=False (librosa's fit=False); to learn one dictionary from many clips, reshape them to one clip of B T
    frames.  return_trace adds [B, n_iter + 1] float64, nmf_divergence before the first and after every iteration; the
    factors are the same bit for bit with or without it.  form: how the contractions run, "fma" or "mfma" (the exact
    f32-input MFMA: the same products in another summation order); None takes the measured choice, MFMA from
    nmf_constants()["mfma_min_components"] components up."""
    who = "nmf"
    loss = _nmf_loss(who, beta_loss)
    if not (form is None or isinstance(form, str)) or form not in _NMF_FORMS:
        raise ValueError(f"{who}: form must be None, 'fma' or 'mfma' (got {form!r})")
    if not (isinstance(solver, str) and solver == "mu"):
        raise ValueError(f"{who}: solver={solver!r} is not served (coordinate descent is sequential per coordinate); {_NMF_SERVED}")
    if not (init is None or (isinstance(init, str) and init in ("random", "custom"))):
        raise ValueError(f"{who}: init={init!r} is not served (nndsvd, nndsvda and nndsvdar need an SVD); {_NMF_SERVED}")
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
        raise ValueError(f"{who}: n_iter must be a non-negative integer (got {n_iter!r})")
    n_iter = int(n_iter)
    if n_components is None and A0 is None and C0 is None:
        raise ValueError(f"{who}: n_components is needed when neither A0 nor C0 is given")
    B, Tn, F, K, shared = _nmf_factors(who, V, A0, C0, n_components)
    update_A, update_C = bool(update_A), bool(update_C)
    if C0 is not None and C0.shape[0] == 1 and B > 1 and update_C:
        raise ValueError(f"{who}: a shared dictionary C0 [1, {K}, {F}] cannot be updated: pass update_C=False, or reshape "
                         f"the batch to one clip of B T frames to learn one dictionary")
    if A0 is None or C0 is None:
        seed, first_row = RNG.check_seed(seed), RNG.check_rows(first_row, B)
    _nmf_on_device(who, V, A0=A0, C0=C0)
    V = V.contiguous()
    A = A0.contiguous().clone() if A0 is not None else None
    C = C0.contiguous().clone() if C0 is not None else None
    if A is None or C is None:
        scale = torch.sqrt(torch.mean(V, dim=(1, 2), dtype=torch.float64) / K).to(torch.float32)
        if C is None:
            C = (randn(B, K * F, seed, first_row).abs_() * scale[:, None]).view(B, K, F)
        if A is None:
            A = (randn(B, Tn * K, seed, first_row, offset=K * F).abs_() * scale[:, None]).view(B, Tn, K)
    work = _workspace("syg_nmf_work_bytes", B, Tn, F, K, dtype=torch.float64, device=V.device)

    def run(n):
        _call("syg_nmf_f32", _ptr(V), B, Tn, F, K, _ptr(A), _ptr(C), int(shared), n, loss, int(update_A), int(update_C),
              _NMF_FORMS[form], _ptr(work))
    if not return_trace:
        run(n_iter)
        return A, C
    trace = torch.empty((B, n_iter + 1), dtype=torch.float64, device=V.device)
    trace[:, 0] = nmf_divergence(V, A, C, beta_loss)
    for it in range(n_iter):
        run(1)
        trace[:, it + 1] = nmf_divergence(V, A, C, beta_loss)
    return A, C, trace


def nmf_masks(D: torch.Tensor, A: torch.Tensor, C: torch.Tensor, G: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The complex spectra D [B, T, F, 2] split by the soft masks of the factorisation (syg_nmf_masks_f32):
    out[b, g] = D[b] (sum_k G[g, k] A[t, k] C[k, f]) / max(sum_k A[t, k] C[k, f], eps), [B, n_groups, T, F, 2].
    G [n_groups, K] weights the components of each group (default: the identity, a group per component); the groups of a
    partition (columns of G summing to 1) add up to D.  The masks themselves are never written."""
    who = "nmf_masks"
    _f32(D, f"{who}: D", 4, (2,), "[B, T, F, 2]")
    if A is None or C is None:
        raise ValueError(f"{who}: A and C must be float32 tensors")
    B, Tn, F, K, shared = _nmf_factors(who, D[..., 0], A, C)
    if G is not None:
        _f32(G, f"{who}: G", 2, (K,), f"[n_groups, {K}]")
        if not 1 <= G.shape[0] <= 64:
            raise ValueError(f"{who}: n_groups={G.shape[0]} must be in [1, 64]")
    _nmf_on_device(who, D, A=A, C=C, G=G, out=out)
    if G is None:
        G = torch.eye(K, dtype=torch.float32, device=D.device)
    NG = int(G.shape[0])
    D, A, C, G = D.contiguous(), A.contiguous(), C.contiguous(), G.contiguous()
    o = _out(out, (B, NG, Tn, F, 2), D, contiguous=True)
    _call("syg_nmf_masks_f32", _ptr(D), _ptr(A), _ptr(C), int(shared), _ptr(G), B, Tn, F, K, NG, _ptr(o))
    return o


# ------------------------------------------------------------------ self-similarity: k-NN lists, recurrence, nn_filter
# Frame-major: X [B, T, D] the query frames, Y [B, T', D] the frames searched (X itself by default).  The float64
# restatement tests/similarity_ref.py is the contract.

SIM_METRICS = {"euclidean": 0, "sqeuclidean": 1, "cosine": 2}
SIM_MODES = {"connectivity": 0, "distance": 1, "affinity": 2}
NN_AGGREGATES = {"mean": 0, "average": 1, "median": 2}
K_MAX = 256                                   # neighbours a row keeps at most (the library's syg_sim_k_max)


def similarity_constants() -> dict:
    """k_max (the longest neighbour list, read from the library) and the names served."""
    return dict(k_max=int(lib().syg_sim_k_max()), metrics=tuple(SIM_METRICS), modes=tuple(SIM_MODES),
                aggregates=tuple(NN_AGGREGATES))


def _sim_name(who, what, value, table, note=""):
    if not isinstance(value, str) or value not in table:
        raise ValueError(f"{who}: {what}={value!r} is not served{note}; served: {', '.join(repr(n) for n in table)}")
    return table[value]


def _sim_metric(who, metric) -> int:
    return _sim_name(who, "metric", metric, SIM_METRICS, " (cityblock and the other metrics have no dot-product form)")


def _sim_int(who, name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{who}: {name}={v!r} must be an integer " + (f"in [{lo}, {hi}]" if hi is not None else f">= {lo}"))
    return int(v)


def sim_default_k(T: int, width: int = 1) -> int:
    """librosa's default neighbour count, min(K_MAX, max(1, 2 ceil(sqrt(max(1, T - 2 width + 1)))))."""
    return int(min(K_MAX, max(1, 2 * int(np.ceil(np.sqrt(max(1, T - 2 * width + 1)))))))


def _sim_frames(who, t, name):
    """t [B, T, D] checked without a device: the tensor's sizes."""
    _f32(t, f"{who}: {name}", 3, (), "[B, T, D]")
    if min(t.shape) < 1:
        raise ValueError(f"{who}: empty input ({name} has shape {list(t.shape)})")
    return tuple(int(n) for n in t.shape)


def _sim_strided(t):
    """t [B, T, D] with unit stride along D, its row and batch strides (a copy where rows overlap or a stride is negative)."""
    t = _unit_stride(t)
    B, Tn, D = t.shape
    ld = int(t.stride(1)) if Tn > 1 else D
    bs = int(t.stride(0)) if B > 1 else 0
    if ld < D or bs < 0:
        t = t.contiguous()
        ld, bs = D, (Tn * D if B > 1 else 0)
    return t, ld, bs


def _sim_lens(who, v, B, Tn, device, name):
    """A per-clip length list as a device int32 [B] (values in [0, T]), or None."""
    if v is None:
        return None
    host = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
    if host.shape != (B,) or host.dtype.kind not in "iu" or host.min() < 0 or host.max() > Tn:
        raise ValueError(f"{who}: {name} must hold one integer length in [0, {Tn}] per clip ([{B}])")
    return torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(device)


def sim_knn(X: torch.Tensor, Y: Optional[torch.Tensor] = None, k: Optional[int] = None, width: int = 1,
            metric: str = "euclidean", x_len=None, y_len=None):
    """The k nearest frames of every frame (syg_sim_knn_f32): X [B, T, D] float32 on the device (rows may be strided) ->
    (idx [B, T, k] int32, dist [B, T, k] float32, count [B, T] int32).  Row i keeps its min(k, candidates) nearest
    candidates ordered by distance, then by index; entries past count are idx = -1, dist = +inf.  Y [B, T', D] (or
    [1, T', D], one for every clip) are the frames searched, every one a candidate; without it X searches itself and
    the candidates of row i are the j with |i - j| >= width.  metric: euclidean | sqeuclidean | cosine
    (1 - x.y / max(|x| |y|, FLT_MIN): a zero frame is at distance 1 from everything).  k=None: sim_default_k(T, width),
    librosa's rule; k <= K_MAX.  x_len / y_len [B]: ragged batches; frames past a length are neither queries nor
    candidates.  The dense distance matrix is never written."""
    who = "sim_knn"
    code = _sim_metric(who, metric)
    # (_f32_in would copy a tensor whose last stride is not 1 and knows nothing of rows: the frames keep their row and
    # batch strides here, so the two stages of the input check are taken apart: _sim_frames, _on_device, _sim_strided)
    B, Tn, D = _sim_frames(who, X, "X")
    width = _sim_int(who, "width", width, 1, 1 << 30)
    Ty = Tn
    if Y is not None:
        By, Ty, Dy = _sim_frames(who, Y, "Y")
        if Dy != D or By not in (1, B):
            raise ValueError(f"{who}: Y {list(Y.shape)} must be [{B}, T', {D}] or [1, T', {D}] (X is {list(X.shape)})")
        if width != 1:
            raise ValueError(f"{who}: width applies to self-similarity; with Y every frame is a candidate (got width={width})")
    elif y_len is not None:
        raise ValueError(f"{who}: y_len needs Y (self-similarity takes x_len for both)")
    k = sim_default_k(Tn, width) if k is None else _sim_int(who, "k", k, 1, K_MAX)
    _on_device(X, f"{who}: X")
    if Y is not None and Y.device != X.device:
        raise ValueError(f"{who}: Y must be on the device of X ({X.device}; got {Y.device})")
    X, ldx, bsx = _sim_strided(X)
    ldy = bsy = 0
    if Y is not None:
        Y, ldy, bsy = _sim_strided(Y)
        if Y.shape[0] == 1:
            bsy = 0
    xl = _sim_lens(who, x_len, B, Tn, X.device, "x_len")
    yl = _sim_lens(who, y_len, B, Ty, X.device, "y_len")
    idx = torch.empty((B, Tn, k), dtype=torch.int32, device=X.device)
    dist = torch.empty((B, Tn, k), dtype=torch.float32, device=X.device)
    count = torch.empty((B, Tn), dtype=torch.int32, device=X.device)
    work = _workspace("syg_sim_knn_work_bytes", B, Tn, Ty, int(Y is not None), dtype=torch.float64, device=X.device)
    _call("syg_sim_knn_f32", _ptr(X), _ptr(Y), B, Tn, Ty, D, ldx, ldy, bsx, bsy, _ptr(xl), _ptr(yl), k, width, code, _ptr(idx),
          _ptr(dist), _ptr(count), _ptr(work))
    idx._syg_cols = count._syg_cols = Ty           # the library's own lists: _sim_check_lists has nothing to find in them
    return idx, dist, count


def _sim_lists(who, idx, dist, count):
    """The shape checks of a set of lists, without a device: (B, T, k)."""
    if not isinstance(idx, torch.Tensor) or idx.dim() != 3 or idx.dtype != torch.int32:
        raise ValueError(f"{who}: idx must be an int32 tensor [B, T, k]")
    B, Tn, k = (int(n) for n in idx.shape)
    if B < 1 or Tn < 1 or not 1 <= k <= K_MAX:
        raise ValueError(f"{who}: idx {list(idx.shape)} must be [B, T, k] with B, T >= 1 and k in [1, {K_MAX}]")
    if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or tuple(count.shape) != (B, Tn):
        raise ValueError(f"{who}: count must be an int32 tensor [{B}, {Tn}]")
    if dist is not None and (not isinstance(dist, torch.Tensor) or dist.dtype != torch.float32 or tuple(dist.shape) != (B, Tn, k)):
        raise ValueError(f"{who}: the distances / weights must be a float32 tensor [{B}, {Tn}, {k}]")
    return B, Tn, k


def _sim_check_lists(who, idx, count, n_cols):
    """The caller's lists hold what the kernels index with: counts in [0, k], the entries below a count in [0, n_cols).
    Lists that sim_knn made for n_cols columns are marked and pass without the two reductions and their host syncs (the
    kernels clamp what they index with in any case)."""
    if getattr(idx, "_syg_cols", None) == n_cols and getattr(count, "_syg_cols", None) == n_cols:
        return
    k = idx.shape[2]
    live = torch.arange(k, device=idx.device)[None, None, :] < count[:, :, None]
    bad = (count < 0) | (count > k)
    if bool(bad.any()) or bool((live & ((idx < 0) | (idx >= n_cols))).any()):
        raise ValueError(f"{who}: count must be in [0, {k}] and the entries of idx below it in [0, {n_cols})")


def sim_bandwidth(rowmax: torch.Tensor, who: str = "recurrence_matrix") -> torch.Tensor:
    """The default bandwidth of the affinities, per clip [B] float64: numpy's median, over the rows that kept a link, of
    the row's largest kept distance (rowmax [B, T], negative where a row kept nothing).  A clip without a link gets 1
    (it has no affinity to scale); a clip whose bandwidth comes out 0 raises ValueError."""
    r = rowmax.to(torch.float64)
    has = r >= 0
    n = has.sum(dim=1)
    s = torch.sort(torch.where(has, r, torch.full_like(r, float("inf"))), dim=1).values
    lo = torch.clamp((n - 1) // 2, min=0)[:, None]
    hi = torch.clamp(n // 2, max=r.shape[1] - 1)[:, None]
    bw = 0.5 * (torch.gather(s, 1, lo) + torch.gather(s, 1, hi))[:, 0]
    bw = torch.where(n > 0, bw, torch.ones_like(bw))
    if bool((bw == 0).any()):
        raise ValueError(f"{who}: the default bandwidth of a clip is 0 (its median nearest-neighbour distance); "
                         "pass bandwidth, or use mode='connectivity'")
    return bw


def _sim_bandwidth_arg(who, bandwidth, B, device):
    """A caller's bandwidth (a positive number, or one per clip) as a float64 device tensor [B]."""
    a = np.asarray(bandwidth.detach().cpu().numpy() if isinstance(bandwidth, torch.Tensor) else bandwidth, dtype=np.float64)
    if a.ndim == 0:
        a = np.full((B,), float(a))
    if a.shape != (B,) or not np.all(np.isfinite(a)) or np.any(a <= 0):
        raise ValueError(f"{who}: bandwidth must be a positive finite number, or one per clip ([{B}])")
    return torch.from_numpy(a).to(device)


def sim_dense(idx: torch.Tensor, dist: torch.Tensor, count: torch.Tensor, n_cols: Optional[int] = None, *,
              mode: str = "connectivity", sym: bool = False, bandwidth=None, self: bool = False, return_bandwidth: bool = False):
    """The dense recurrence matrix [B, T, n_cols] float32 of a set of lists (syg_sim_dense_f32): connectivity 1, distance
    the distance, affinity exp(-distance / bandwidth); 0 elsewhere.  sym keeps (i, j) only if each is in the other's
    list; self sets the diagonal to 1 (0 under distance).  bandwidth=None: sim_bandwidth of the rows' largest kept
    distances, taken after the sym pruning."""
    who = "recurrence_matrix"
    code = _sim_name(who, "mode", mode, SIM_MODES)
    B, Tn, k = _sim_lists(who, idx, dist, count)
    if dist is None:
        raise ValueError(f"{who}: the distances must be a float32 tensor [{B}, {Tn}, {k}]")
    n_cols = Tn if n_cols is None else _sim_int(who, "n_cols", n_cols, 1, 1 << 30)
    sym, self = bool(sym), bool(self)
    if (sym or self) and n_cols != Tn:
        raise ValueError(f"{who}: sym and self need a square matrix (T={Tn}, T'={n_cols})")
    if bandwidth is not None and code != 2:
        raise ValueError(f"{who}: bandwidth applies to mode='affinity' (got mode={mode!r})")
    _on_device(idx, f"{who}: idx")
    if dist.device != idx.device or count.device != idx.device:
        raise ValueError(f"{who}: idx, dist and count must be on one device")
    idx, dist, count = idx.contiguous(), dist.contiguous(), count.contiguous()
    _sim_check_lists(who, idx, count, n_cols)
    bw = None
    if code == 2:
        if bandwidth is None:
            rowmax = torch.empty((B, Tn), dtype=torch.float32, device=idx.device)
            _call("syg_sim_dense_f32", _ptr(idx), _ptr(dist), _ptr(count), B, Tn, n_cols, k, 1, int(sym), 0, None, None, _ptr(rowmax))
            bw = sim_bandwidth(rowmax)
        else:
            bw = _sim_bandwidth_arg(who, bandwidth, B, idx.device)
    out = torch.empty((B, Tn, n_cols), dtype=torch.float32, device=idx.device)
    _call("syg_sim_dense_f32", _ptr(idx), _ptr(dist), _ptr(count), B, Tn, n_cols, k, code, int(sym), int(self), _ptr(bw), _ptr(out), None)
    return (out, bw) if return_bandwidth else out


def recurrence_matrix(X: torch.Tensor, Y: Optional[torch.Tensor] = None, *, k: Optional[int] = None, width: int = 1,
                      metric: str = "euclidean", sym: bool = False, mode: str = "connectivity", bandwidth=None,
                      self: bool = False, x_len=None, y_len=None) -> torch.Tensor:
    """librosa.segment.recurrence_matrix (Y=None) / cross_similarity (Y given) of frame-major features X [B, T, D] ->
    [B, T, T'] float32, dense: sim_knn, then sim_dense.  Row i holds the links of frame i.  sym and self apply to
    self-similarity."""
    who = "recurrence_matrix"
    _sim_name(who, "mode", mode, SIM_MODES)
    if Y is not None and (sym or self):
        raise ValueError(f"{who}: sym and self apply to self-similarity, not to a cross-similarity with Y")
    if bandwidth is not None and mode != "affinity":
        raise ValueError(f"{who}: bandwidth applies to mode='affinity' (got mode={mode!r})")
    idx, dist, count = sim_knn(X, Y, k, width, metric, x_len, y_len)
    return sim_dense(idx, dist, count, int(Y.shape[1]) if Y is not None else None, mode=mode, sym=sym, bandwidth=bandwidth, self=self)


def nn_filter(S: torch.Tensor, idx: torch.Tensor, count: torch.Tensor, weights: Optional[torch.Tensor] = None,
              aggregate: str = "mean", bandwidth=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """librosa.decompose.nn_filter on frame-major S [B, T, F] (syg_nn_filter_f32): out[b, i] aggregates S[b, j] over row
    i's list (idx [B, T, k], count [B, T]; sim_knn's, or the caller's).  aggregate: mean | average (sum w S / sum w with
    w = weights [B, T, k]; with bandwidth the weights are distances and w = exp(-weights / bandwidth)) | median (numpy's:
    the mean of the two middle values at an even count, an input value bit for bit at an odd one).  A frame with an
    empty list keeps S[b, i]."""
    who = "nn_filter"
    code = _sim_name(who, "aggregate", aggregate, NN_AGGREGATES)
    B, Tn, F = _sim_frames(who, S, "S")
    lb, lt, k = _sim_lists(who, idx, weights, count)
    if (lb, lt) != (B, Tn):
        raise ValueError(f"{who}: idx {list(idx.shape)} must be [{B}, {Tn}, k] (S is {list(S.shape)})")
    if code == 1 and weights is None:
        raise ValueError(f"{who}: aggregate='average' needs weights [{B}, {Tn}, {k}] (the lists' affinities, or distances with bandwidth)")
    if code != 1 and (weights is not None or bandwidth is not None):
        raise ValueError(f"{who}: weights and bandwidth apply to aggregate='average' (got {aggregate!r})")
    _on_device(S, f"{who}: S")
    for name, t in (("idx", idx), ("count", count), ("weights", weights)):
        if t is not None and t.device != S.device:
            raise ValueError(f"{who}: {name} must be on the device of S ({S.device}; got {t.device})")
    S, lds, bss = _sim_strided(S)
    idx, count = idx.contiguous(), count.contiguous()
    weights = weights.contiguous() if weights is not None else None
    _sim_check_lists(who, idx, count, Tn)
    bw = _sim_bandwidth_arg(who, bandwidth, B, S.device) if bandwidth is not None else None
    o = _out(out, (B, Tn, F), S, contiguous=True)
    _call("syg_nn_filter_f32", _ptr(S), B, Tn, F, lds, bss, _ptr(idx), _ptr(count), k, _ptr(weights), _ptr(bw), code, _ptr(o))
    return o


def _repet_number(who, name, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v <= 0:
        raise ValueError(f"{who}: {name}={v!r} must be a positive finite number")
    return float(v)


def repet_masks(S: torch.Tensor, Sf: torch.Tensor, margin_b: float = 2.0, margin_f: float = 10.0, power: float = 2.0):
    """The two soft masks of REPET-SIM (syg_repet_masks_f32) from magnitudes S and their nn_filter Sf, same shape: with
    R = min(S, Sf), mask_b = softmask(R, margin_b (S - R), power) and mask_f = softmask(S - R, margin_f R, power)
    (librosa.util.softmask).  Returns (mask_f, mask_b)."""
    who = "repet_masks"
    mb, mf, pw = (_repet_number(who, n, v) for n, v in (("margin_b", margin_b), ("margin_f", margin_f), ("power", power)))
    if not isinstance(S, torch.Tensor) or S.dtype != torch.float32 or S.numel() < 1:
        raise ValueError(f"{who}: S must be a non-empty float32 tensor")
    if not isinstance(Sf, torch.Tensor) or Sf.dtype != torch.float32 or Sf.shape != S.shape:
        raise ValueError(f"{who}: Sf must be a float32 tensor {list(S.shape)}")
    _on_device(S, f"{who}: S")
    if Sf.device != S.device:
        raise ValueError(f"{who}: Sf must be on the device of S ({S.device}; got {Sf.device})")
    S, Sf = S.contiguous(), Sf.contiguous()
    Mf, Mb = torch.empty_like(S), torch.empty_like(S)
    _call("syg_repet_masks_f32", _ptr(S), _ptr(Sf), S.numel(), mb, mf, pw, _ptr(Mf), _ptr(Mb))
    return Mf, Mb


# ---------------------------------------------------------------------------------------------------------------------
# Viterbi decoding (csrc/sequence.hip; the host side -- builders, checks, log tables -- is _sequence.py)

VITERBI_FORMS = {None: 0, "wide": 1, "narrow": 2}
VITERBI_WORK_MAX = 256 << 20                      # bytes of back pointers a launch takes at most: the batch goes in pieces
_VITERBI_KEYS = ("s_max", "s_lds", "s_narrow", "tile")                                    # SYG_VITERBI_* of include/sygnals_hip.h
_VITERBI_DTYPES = {torch.float32: 0, torch.float64: 1}


def viterbi_constants() -> dict:
    """The figures syg_viterbi_f32 rests on (the library owns them): s_max the largest S, s_lds the largest S whose
    transition table lives in LDS, s_narrow the largest S of the narrow form, tile the frames of an emission tile; and
    work_max, the bytes of back pointers above which viterbi() decodes the batch in pieces."""
    return dict(_constants("syg_viterbi_constants", _VITERBI_KEYS), work_max=VITERBI_WORK_MAX)


def viterbi_work_bytes(B: int, S: int, T: int) -> int:
    """Bytes of the back-pointer workspace of B sequences of T frames over S states (syg_viterbi_work_bytes)."""
    return _work_bytes("syg_viterbi_work_bytes", int(B), int(S), int(T))


def viterbi_form(B: int, S: int) -> str:
    """The form the library's rule takes for B sequences over S states: 'wide' or 'narrow'."""
    f = int(lib().syg_viterbi_form(int(B), int(S)))
    if f < 0:
        raise ValueError(f"viterbi: B = {B}, S = {S} is not served ({SQ.SERVED})")
    return {1: "wide", 2: "narrow"}[f]


def _viterbi_host(v) -> np.ndarray:
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _viterbi_table_dev(a: np.ndarray) -> torch.Tensor:
    """A float64 table on the device; the small ones (shared transition matrices, initial rows) are kept."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size <= 4096:
        return _cached(("viterbi", a.shape, a.tobytes()), lambda: _dev(a), limit=64)
    return _dev(a)


def viterbi(prob: Optional[torch.Tensor] = None, transition=None, *, log_prob: Optional[torch.Tensor] = None, p_init=None,
            p_state=None, lengths=None, eps: Optional[float] = None, form: Optional[str] = None, return_logp: bool = False,
            out: Optional[torch.Tensor] = None, chunk: Optional[int] = None):
    """The most likely state path of every clip (syg_viterbi_f32; tests/sequence_ref.py is the definition).
    prob [B, S, T] float32 or float64 on the device, any strides (a [B, T, S] block is passed as its transpose(1, 2)
    view) -> states [B, T] int32, and logp [B] float64 with return_logp.
    transition [S, S] or one per clip [B, S, S], p_init [S] or [B, S] (default 1 / S) and p_state (None: the plain
    decoder; given: the discriminative one, log(prob + eps) - log(p_state + eps)) are host arrays or tensors of
    probabilities; their logs are taken on the host in float64 with eps, which defaults to the smallest normal number of
    prob's dtype.  Only log(prob + eps) is taken on the device, in float64.
    log_prob= instead of prob: the emissions are log-probabilities and so are transition, p_init (default log(1 / S)) and
    p_state: every table is used as given, no log is taken, eps plays no part.
    lengths [B] integers in 1 .. T: states past a clip's length are -1.  form: None (the library's rule), 'wide' or
    'narrow' (S <= s_narrow); both give the same bits.  out: an int32 [B, T] tensor for the states.  The batch is decoded
    in pieces of `chunk` clips (default: as many as keep the back pointers under work_max bytes), which changes no bit.
    Values outside [0, 1] or NaN in prob are not looked for (that would be a device reduction and a sync)."""
    who = "viterbi"
    if (prob is None) == (log_prob is None):
        raise ValueError(f"{who}: give either prob or log_prob=, not both and not neither")
    log_dom = log_prob is not None
    x = log_prob if log_dom else prob
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype not in _VITERBI_DTYPES or min(x.shape) < 1:
        raise ValueError(f"{who}: {'log_prob' if log_dom else 'prob'} must be a non-empty float32 or float64 tensor [B, S, T]")
    B, S, Tn = (int(n) for n in x.shape)
    K = viterbi_constants()
    if S > K["s_max"]:
        raise ValueError(f"{who}: S = {S} states is above the cap of {K['s_max']} ({SQ.SERVED})")
    if transition is None:
        raise ValueError(f"{who}: transition is required ({SQ.SERVED})")
    if form not in VITERBI_FORMS:
        raise ValueError(f"{who}: form={form!r} is not served; served: None, 'wide', 'narrow'")
    if form == "narrow" and S > K["s_narrow"]:
        raise ValueError(f"{who}: the narrow form serves S <= {K['s_narrow']}, not S = {S}")
    if log_dom:
        e = 0.0
    else:
        e = SQ.tiny(np.float32 if x.dtype == torch.float32 else np.float64) if eps is None else float(eps)
        if not np.isfinite(e) or e < 0:
            raise ValueError(f"{who}: eps={eps!r} must be finite and not negative")
    tr = SQ.check_transition(who, _viterbi_host(transition), S, B, stochastic=not log_dom)
    if p_init is None:
        pi = np.full(S, np.log(1.0 / S) if log_dom else 1.0 / S)
    else:
        pi = SQ.check_distribution(who, "p_init", _viterbi_host(p_init), S, B, stochastic=not log_dom)
    ps = None if p_state is None else SQ.check_distribution(who, "p_state", _viterbi_host(p_state), S, B, stochastic=not log_dom)
    lens = None
    if lengths is not None:
        lens = np.asarray(_viterbi_host(lengths))
        if lens.shape != (B,) or lens.dtype.kind not in "iu" or lens.min() < 1 or lens.max() > Tn:
            raise ValueError(f"{who}: lengths must hold one integer in [1, {Tn}] per clip ([{B}])")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1):
        raise ValueError(f"{who}: chunk={chunk!r} must be a positive integer")
    states = _out(out, (B, Tn), x, dtype=torch.int32, contiguous=True)
    _on_device(x, f"{who}: {'log_prob' if log_dom else 'prob'}")

    def table(a):
        return None if a is None else _viterbi_table_dev(a if log_dom else SQ.log_table(a, e))
    lt, li, lm = table(tr), table(pi), table(ps)
    ld = None if lens is None else torch.from_numpy(np.ascontiguousarray(lens.astype(np.int32))).to(x.device)
    logp = torch.empty(B, dtype=torch.float64, device=x.device)
    per = viterbi_work_bytes(1, S, Tn)
    Bc = min(B, int(chunk) if chunk is not None else max(1, VITERBI_WORK_MAX // per))
    work = _workspace("syg_viterbi_work_bytes", Bc, S, Tn, dtype=torch.float64, device=x.device)
    sb, ss, st = (int(v) for v in x.stride())
    for b0 in range(0, B, Bc):
        n = min(Bc, B - b0)

        def piece(t, per_clip):
            return None if t is None else _ptr(t[b0:b0 + n] if per_clip else t)
        _call("syg_viterbi_f32", _ptr(x[b0:b0 + n]), _VITERBI_DTYPES[x.dtype], int(log_dom), sb, ss, st, n, S, Tn,
              piece(ld, True), piece(lt, tr.ndim == 3), S * S if tr.ndim == 3 else 0, piece(li, pi.ndim == 2),
              S if pi.ndim == 2 else 0, piece(lm, ps is not None and ps.ndim == 2), S if ps is not None and ps.ndim == 2 else 0,
              e, _ptr(work), _nbytes(work), _ptr(states[b0:b0 + n]), _ptr(logp[b0:b0 + n]), VITERBI_FORMS[form])
    return (states, logp) if return_logp else states


# ---------------------------------------------------------------------------------------------------------------------
# Structure analysis (csrc/structure.hip; the filter bank and the frame fixing are _structure.py): what librosa.segment
# does with a recurrence matrix [B, T, T'] and the frame-major features [B, T, D] behind it.  tests/structure_ref.py is
# the contract.

_STRUCT_KEYS = ("agg_t_max", "median_w_max", "path_tile_rows", "path_tile_cols", "path_span_max", "shear_t_max")   # SYG_STRUCT_*


def structure_constants() -> dict:
    """The figures the structure kernels rest on (the library owns them): agg_t_max the frames of the longest span
    agglomerative serves, median_w_max the widest diagonal median, the path_enhance tile and the widest extent of its
    filters' offsets, shear_t_max the largest square matrix of the shear and the diagonal median; and the names served."""
    return dict(_constants("syg_structure_constants", _STRUCT_KEYS), modes=tuple(ST.BOUNDARY_MODES),
                aggregates=tuple(ST.SYNC_AGGREGATES))


def _struct_mats(who, R, name="R", square=False):
    """R [B, T, T'] checked without a device: its sizes."""
    _f32(R, f"{who}: {name}", 3, (), "[B, T, T']")
    if min(R.shape) < 1:
        raise ValueError(f"{who}: empty input ({name} has shape {list(R.shape)})")
    B, Tn, Tc = (int(n) for n in R.shape)
    if square and Tn != Tc:
        raise ValueError(f"{who}: {name} must be square [B, t, t] (got {list(R.shape)})")
    return B, Tn, Tc


def _struct_axis(who, axis) -> int:
    """librosa's axis of a matrix (-1 / 1: time along the columns, 0: along the rows) as the library's flag."""
    if isinstance(axis, bool) or axis not in (-1, 0, 1):
        raise ValueError(f"{who}: axis={axis!r} must be -1 (or 1) or 0")
    return 0 if axis == 0 else 1


def _struct_cval(who, cval) -> float:
    if isinstance(cval, bool) or not isinstance(cval, (int, float, np.integer, np.floating)) or not np.isfinite(cval):
        raise ValueError(f"{who}: cval={cval!r} must be a finite number")
    return float(cval)


def recurrence_to_lag(R: torch.Tensor, pad: bool = True, axis: int = -1) -> torch.Tensor:
    """librosa.segment.recurrence_to_lag of square matrices R [B, t, t] float32 on the device (rows may be strided) ->
    [B, 2 t, t] (pad) or [B, t, t]; axis=0: [B, t, 2 t].  lag[l, i] = R~[(l + i) mod n, i], R~ zero past row t."""
    who = "recurrence_to_lag"
    B, t, _ = _struct_mats(who, R, "rec", square=True)
    ax = _struct_axis(who, axis)
    if t > structure_constants()["shear_t_max"]:
        raise ValueError(f"{who}: t = {t} is above the served {structure_constants()['shear_t_max']}")
    _on_device(R, f"{who}: rec")
    R, ld, bs = _sim_strided(R)
    n = 2 * t if pad else t
    out = torch.empty((B, n, t) if ax == 1 else (B, t, n), dtype=torch.float32, device=R.device)
    _call("syg_lag_shear_f32", _ptr(R), B, t, ld, bs, 0, ax, int(bool(pad)), _ptr(out))
    return out


def lag_to_recurrence(lag: torch.Tensor, axis: int = -1) -> torch.Tensor:
    """librosa.segment.lag_to_recurrence: lag [B, 2 t, t] or [B, t, t] (axis=0: [B, t, 2 t]) -> [B, t, t]."""
    who = "lag_to_recurrence"
    B, rows, cols = _struct_mats(who, lag, "lag")
    ax = _struct_axis(who, axis)
    n, t = (rows, cols) if ax == 1 else (cols, rows)
    if n not in (t, 2 * t):
        raise ValueError(f"{who}: lag must be [t, t] or padded along axis={axis} to 2 t (got {[rows, cols]})")
    if t > structure_constants()["shear_t_max"]:
        raise ValueError(f"{who}: t = {t} is above the served {structure_constants()['shear_t_max']}")
    _on_device(lag, f"{who}: lag")
    lag, ld, bs = _sim_strided(lag)
    out = torch.empty((B, t, t), dtype=torch.float32, device=lag.device)
    _call("syg_lag_shear_f32", _ptr(lag), B, t, ld, bs, 1, ax, int(n == 2 * t), _ptr(out))
    return out


def _path_tables_dev(F: "ST.PathFilters"):
    return _cached(("path_filters", F.taps.shape, F.taps.tobytes()), lambda: (_dev(F.taps), _dev(F.fstart)), limit=16)


def path_enhance(R: torch.Tensor, n: int, window="hann", max_ratio: float = 2.0, min_ratio=None, n_filters: int = 7,
                 zero_mean: bool = False, clip: bool = True, mode: str = "reflect", cval: float = 0.0) -> torch.Tensor:
    """librosa.segment.path_enhance of R [B, T, T'] float32 on the device (rows may be strided) -> [B, T, T']: the maximum
    over a bank of n_filters diagonal smoothing filters of slopes min_ratio .. max_ratio (syg_path_enhance_f32 over the
    tap lists of _structure.path_filters), clipped at 0 with clip.  mode / cval: scipy.ndimage's boundary rule."""
    who = "path_enhance"
    B, Tn, Tc = _struct_mats(who, R)
    code = ST.boundary_code(who, mode)
    cv = _struct_cval(who, cval)
    F = ST.path_filters(n, window, max_ratio, min_ratio, n_filters, zero_mean)
    K = structure_constants()
    r0, r1, c0, c1 = F.span
    if max(r1 - r0, c1 - c0) > K["path_span_max"]:
        raise ValueError(f"{who}: the filters of n = {n} span {max(r1 - r0, c1 - c0) + 1} cells; served are up to "
                         f"{K['path_span_max'] + 1}")
    _on_device(R, f"{who}: R")
    R, ld, bs = _sim_strided(R)
    taps, fstart = _path_tables_dev(F)
    out = torch.empty((B, Tn, Tc), dtype=torch.float32, device=R.device)
    _call("syg_path_enhance_f32", _ptr(R), B, Tn, Tc, ld, bs, _ptr(taps), int(F.taps.shape[0]), _ptr(fstart), len(F.fstart) - 1, r0, r1,
          c0, c1, code, cv, int(bool(clip)), _ptr(out))
    return out


def diag_median(R: torch.Tensor, w: int, mode: str = "reflect", cval: float = 0.0, pad: bool = True, axis: int = -1) -> torch.Tensor:
    """timelag_filter(scipy.ndimage.median_filter, pad)(R, size=(1, w), mode, cval) of square R [B, t, t] float32 on the
    device, without the lag matrix (syg_diag_median_f32): the median along every diagonal, cyclic over 2 t (pad) or t rows.
    w odd, up to median_w_max; the result is an input value bit for bit."""
    who = "diag_median"
    B, t, _ = _struct_mats(who, R, square=True)
    K = structure_constants()
    if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or w < 1 or w > K["median_w_max"] or w % 2 == 0:
        raise ValueError(f"{who}: w={w!r} must be an odd integer in [1, {K['median_w_max']}]")
    ax = _struct_axis(who, axis)
    code = ST.boundary_code(who, mode)
    cv = _struct_cval(who, cval)
    if t > K["shear_t_max"]:
        raise ValueError(f"{who}: t = {t} is above the served {K['shear_t_max']}")
    _on_device(R, f"{who}: R")
    R, ld, bs = _sim_strided(R)
    out = torch.empty((B, t, t), dtype=torch.float32, device=R.device)
    _call("syg_diag_median_f32", _ptr(R), B, t, ld, bs, int(w), ax, int(bool(pad)), code, cv, _ptr(out))
    return out


def _struct_ints(who, name, v, n=None) -> np.ndarray:
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
    if a.ndim == 0 and n is not None:
        a = np.full((n,), a)
    if a.ndim != 1 or a.dtype.kind not in "iu" or a.size < 1 or (n is not None and a.size != n):
        raise ValueError(f"{who}: {name} must be " + ("an integer or " if n is not None else "")
                         + f"a one-dimensional array of integers{'' if n is None else f' [{n}]'}")
    return a.astype(np.int64)


def agglomerative(X: torch.Tensor, k, offset=None, length=None):
    """Temporally constrained Ward clustering (librosa.segment.agglomerative) of frame-major X [B, T, D] float32 on the
    device (frames may be strided): from singletons, the neighbouring pair with the least Ward cost (float64; the leftmost
    on ties) is merged until k segments remain.  Without offset / length every clip is one span and k is an integer or one
    per clip; with them span s covers length[s] frames from offset[s] of the flattened [B T] frame index (inside one clip,
    not overlapping) and k one per span.  A span holds up to agg_t_max frames and 1 <= k <= its length.
    -> (bounds [n_spans, max k] int32 on the device: the segment starts relative to the span, ascending, -1 past k;
    count [n_spans] int32)."""
    who = "agglomerative"
    B, Tn, D = _sim_frames(who, X, "X")
    if (offset is None) != (length is None):
        raise ValueError(f"{who}: offset and length come together")
    if offset is None:
        off, ln = np.arange(B, dtype=np.int64) * Tn, np.full((B,), Tn, dtype=np.int64)
    else:
        off = _struct_ints(who, "offset", offset)
        ln = _struct_ints(who, "length", length, off.size)
        if off.min() < 0 or ln.min() < 1 or np.any(off % Tn + ln > Tn) or off.max() >= B * Tn:
            raise ValueError(f"{who}: a span must hold at least one frame and lie inside one clip of {Tn} frames")
        o = np.argsort(off, kind="stable")
        if np.any(off[o][1:] < (off[o] + ln[o])[:-1]):
            raise ValueError(f"{who}: spans must not overlap")
    ks = _struct_ints(who, "k", k, off.size)
    if ks.min() < 1 or np.any(ks > ln):
        raise ValueError(f"{who}: k must be in [1, frames of the span] (got k in [{ks.min()}, {ks.max()}], spans of {ln.min()} to "
                         f"{ln.max()} frames)")
    cap = structure_constants()["agg_t_max"]
    if ln.max() > cap:
        raise ValueError(f"{who}: a span of {ln.max()} frames is above the served {cap} frames (the boundary costs and links of a "
                         "span live in LDS)")
    _on_device(X, f"{who}: X")
    X, ldx, bsx = _sim_strided(X)
    if B > 1 and bsx == 0:
        X, ldx, bsx = X.contiguous(), D, Tn * D
    n, kmax = int(off.size), int(ks.max())
    tab = torch.from_numpy(np.stack([off, ln, ks]).astype(np.int32)).to(X.device)
    bounds = torch.empty((n, kmax), dtype=torch.int32, device=X.device)
    count = torch.empty((n,), dtype=torch.int32, device=X.device)
    work = _workspace("syg_agglomerative_work_bytes", B, Tn, D, dtype=torch.float64, device=X.device)
    _call("syg_agglomerative_f32", _ptr(X), B, Tn, D, ldx, bsx, _ptr(tab[0]), _ptr(tab[1]), _ptr(tab[2]), n, int(ln.max()), kmax,
          _ptr(bounds), _ptr(count), _ptr(work), _nbytes(work))
    return bounds, count


def subsegment(X: torch.Tensor, frames, n_segments: int = 4):
    """librosa.segment.subsegment of frame-major X [B, T, D]: every clip is cut at `frames` (host integers, shared by the
    clips; unsorted, repeated or past T as librosa.util.fix_frames takes them) and each piece into min(n_segments, its
    frames) agglomerative segments.  -> (bounds [B, n] int32 on the device, frames of the clip, ascending, -1 past count;
    count [B])."""
    who = "subsegment"
    B, Tn, D = _sim_frames(who, X, "X")
    n_segments = _sim_int(who, "n_segments", n_segments, 1)
    edges = ST.fix_frames(_struct_ints(who, "frames", frames), Tn)
    starts, lens = edges[:-1], np.diff(edges)
    ks = np.minimum(lens, n_segments)
    P = starts.size
    off = (np.arange(B, dtype=np.int64)[:, None] * Tn + starts[None, :]).ravel()
    b, _ = agglomerative(X, np.tile(ks, B), off, np.tile(lens, B))
    b = b.reshape(B, P, -1)
    live = b >= 0
    b = torch.where(live, b + torch.from_numpy(starts.astype(np.int32)).to(b.device)[None, :, None], b)
    # the pieces are in ascending order and so are the starts inside one: the live entries, kept in place order
    n = int(ks.sum())
    keep = torch.from_numpy((np.arange(b.shape[2])[None, :] < ks[:, None]).ravel()).to(b.device)
    out = b.reshape(B, -1)[:, keep].contiguous()
    return out, torch.full((B,), n, dtype=torch.int32, device=out.device)


def segment_sync(X: torch.Tensor, edges, aggregate: str = "mean", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """librosa.util.sync of frame-major X [B, T, D] float32 on the device -> [B, n_seg, D]: the mean (summed in float64), max
    or min of the frames [edges[j], edges[j + 1]).  edges: integers [n_seg + 1] shared by the clips, or [B, n_seg + 1], not
    descending, in [0, T] (a host array, or an int32 device tensor that is used as it is); an empty segment gives 0.
    The median is not served."""
    who = "segment_sync"
    if aggregate == "median" or aggregate is np.median:
        raise ValueError(f"{who}: aggregate='median' is not served; served: 'mean', 'max', 'min'")
    code = _sim_name(who, "aggregate", aggregate, ST.SYNC_AGGREGATES)
    B, Tn, D = _sim_frames(who, X, "X")
    on_dev = isinstance(edges, torch.Tensor) and edges.is_cuda
    if on_dev:
        if edges.dtype != torch.int32 or edges.dim() not in (1, 2):
            raise ValueError(f"{who}: edges on the device must be an int32 tensor [n_seg + 1] or [{B}, n_seg + 1]")
        e = edges.contiguous()
        shape = tuple(e.shape)
    else:
        a = np.asarray(edges.numpy() if isinstance(edges, torch.Tensor) else edges)
        if a.dtype.kind not in "iu" or a.ndim not in (1, 2) or a.size < 1:
            raise ValueError(f"{who}: edges must be integers [n_seg + 1] or [{B}, n_seg + 1]")
        if a.min() < 0 or a.max() > Tn or np.any(np.diff(a, axis=-1) < 0):
            raise ValueError(f"{who}: edges must not descend and lie in [0, {Tn}]")
        shape = a.shape
    if shape[-1] < 2 or shape[-1] - 1 > Tn or (len(shape) == 2 and shape[0] != B):
        raise ValueError(f"{who}: edges {list(shape)} must be [n_seg + 1] or [{B}, n_seg + 1] with 1 <= n_seg <= {Tn}")
    n_seg = shape[-1] - 1
    _on_device(X, f"{who}: X")
    X, ldx, bsx = _sim_strided(X)
    if not on_dev:
        e = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(X.device)
    o = _out(out, (B, n_seg, D), X, contiguous=True)
    _call("syg_segment_sync_f32", _ptr(X), B, Tn, D, ldx, bsx, _ptr(e), n_seg, n_seg + 1 if len(shape) == 2 else 0, code, _ptr(o))
    return o


# ------------------------------------------------------------------ Kaldi-compatible front end: fbank and MFCC
_KALDI_KEYS = ("tile", "n_fft_min", "n_fft_max", "mel_min", "mel_max", "lds_max", "wgs_per_cu", "lds_worst")       # SYG_KALDI_*


def kaldi_constants() -> dict:
    """The figures the Kaldi front end rests on (the library owns them): the frames of a workgroup's tile, the smallest and
    largest padded frame length, the band counts served, the LDS a workgroup may take, the workgroups a CU of the capped
    grid, the LDS of the largest served shape."""
    return _constants("syg_kaldi_constants", _KALDI_KEYS)


def _kaldi_tables(s: "KD.Spec"):
    """(window, twiddle, padded mel banks, DCT x lifter | None) on the device."""
    win = _cached(("kaldi_win", s.window_type, s.wl, s.blackman_coeff),
                  lambda: _dev(KD.window(s.window_type, s.wl, s.blackman_coeff).astype(np.float32)))
    tw = _cached(("kaldi_tw", s.N), lambda: _dev(KD.twiddle_f32(s.N)))
    bp = _cached(("kaldi_mel", s.M, s.N, s.sr, s.low, s.high), lambda: _dev(KD.mel_padded_f32(s.M, s.N, s.sr, s.low, s.high)))
    dct = None
    if s.mfcc:
        dct = _cached(("kaldi_dct", s.num_ceps, s.M, s.lifter),
                      lambda: _dev(KD.dct_lifter(s.num_ceps, s.M, s.lifter).astype(np.float32)))
    return win, tw, bp, dct


def _kaldi_front(who, mfcc, y, sr, layout, seed, out, return_fbank, kw):
    s = KD.check(who, mfcc, sr, kw)
    layout = KD.check_layout(who, layout)
    seed = KD.check_seed(who, seed)
    _f32(y, f"{who}: y", 2, axes="[B, L]")
    B, L = y.shape
    if B < 1 or L < 1:
        raise ValueError(f"{who}: empty input (shape [{B}, {L}])")
    Tn = KD.frames_of(s, L)
    shape = lambda C: (B, C, Tn) if layout == "ct" else (B, Tn, C)            # noqa: E731
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape(s.C) or out.dtype != torch.float32
                            or out.device != y.device or not out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor {list(shape(s.C))} on the input's device")
    _on_device(y, f"{who}: y")
    y = _unit_stride(y)
    if Tn == 0:                                                              # too short a clip: torchaudio's empty result
        o = torch.empty(shape(s.C), dtype=torch.float32, device=y.device) if out is None else out
        return (o, torch.empty(shape(s.M), dtype=torch.float32, device=y.device)) if return_fbank else o
    win, tw, bp, dct = _kaldi_tables(s)
    # subtract_mean is a second launch of cmvn, which takes [B, C, T]: the first launch writes that layout
    direct = not (s.subtract_mean and layout == "tc")
    o = out if (out is not None and direct) else torch.empty(shape(s.C) if direct else (B, s.C, Tn), dtype=torch.float32,
                                                             device=y.device)
    ct = layout == "ct" or not direct
    so = (s.C * Tn, 1, Tn) if ct else (s.C * Tn, s.C, 1)
    fb, sf = None, (0, 0, 0)
    if return_fbank:
        fb = torch.empty(shape(s.M), dtype=torch.float32, device=y.device)
        sf = (s.M * Tn, 1, Tn) if layout == "ct" else (s.M * Tn, s.M, 1)
    _call("syg_kaldi_fbank_f32", _ptr(y), B, L, _ld(y), s.wl, s.hop, s.N, int(s.snip_edges), Tn, _ptr(win), _ptr(tw), _ptr(bp), s.M,
          s.preemph, int(s.remove_dc), int(s.raw_energy), int(s.use_power), int(s.use_log), KD.LOG_EPS, s.energy_floor, s.dither,
          seed, int(s.use_energy), int(s.htk_compat), _ptr(dct), s.num_ceps, _ptr(o), *so, _ptr(fb), *sf)
    if s.subtract_mean:
        cmvn(o, variance=False, out=o)
        if not direct:
            t = o.transpose(1, 2)
            o = out.copy_(t) if out is not None else t.contiguous()
    return (o, fb) if return_fbank else o


def kaldi_fbank(y: torch.Tensor, sr: float = 16000.0, layout: str = "ct", seed: int = 0, out: Optional[torch.Tensor] = None,
                **kw) -> torch.Tensor:
    """torchaudio.compliance.kaldi.fbank of y [B, L] float32 clips on the device, one launch: [B, C, T] (layout "ct", what
    cmvn / delta / spec_augment take) or [B, T, C] ("tc", Kaldi's own), C = num_mel_bins + use_energy.  **kw: torchaudio's
    keywords with its defaults (_kaldi.FBANK_DEFAULTS); the definition is tests/kaldi_ref.py.  Served: padded frame lengths
    256 ... 2048, 3 <= num_mel_bins <= 256; vtln_warp != 1 and round_to_power_of_two=False are refused.  seed keys the dither
    (Philox; used only with dither != 0).  subtract_mean is a second launch of cmvn(variance=False).  A clip shorter than
    a frame, or than min_duration, gives T = 0."""
    return _kaldi_front("kaldi_fbank", False, y, sr, layout, seed, out, False, kw)


def kaldi_mfcc(y: torch.Tensor, sr: float = 16000.0, layout: str = "ct", seed: int = 0, out: Optional[torch.Tensor] = None,
               return_fbank: bool = False, **kw):
    """torchaudio.compliance.kaldi.mfcc of y [B, L] in the same launch as the filterbank: the orthonormal DCT-II of the log
    mel energies, the first num_ceps coefficients, Kaldi's lifter; use_energy replaces coefficient 0 by the log-energy,
    htk_compat moves coefficient 0 to the end.  return_fbank=True returns (mfcc, log fbank [B, M, T] / [B, T, M]) from the one
    launch (the filterbank without subtract_mean).  **kw: _kaldi.MFCC_DEFAULTS."""
    return _kaldi_front("kaldi_mfcc", True, y, sr, layout, seed, out, bool(return_fbank), kw)
