"""Device-backed mirror of sygnals/core/dsp.py (FFT/IFFT, STFT, Welch, windowing).

Same signatures, dtypes (float64 / complex128 out) and error behaviour as the reference:
compute_fft :40-112, compute_ifft :114-162, compute_stft :167-229, apply_convolution :294-337,
compute_correlation :342-394, compute_autocorrelation :396-433, compute_psd_periodogram :438-498,
compute_psd_welch :495-560, amplitude_envelope :565-636, apply_window :641-691; `resample` is the `scipy` resampling
method of the reference's pipeline (scipy.signal.resample_poly) on the device.  Arithmetic runs in fp32 on the device (parity gate 1e-5, peak-relative).
"""
from __future__ import annotations

import logging
from typing import Optional, Tuple, Union

import numpy as np
from scipy.signal import get_window

from .. import _cepstrum, _resample, ops
from .._lib import SygnalsHipError

logger = logging.getLogger(__name__)


def _c128(t) -> np.ndarray:
    a = t.cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def _symmetric_window(window_type: str, n: int) -> np.ndarray:
    try:
        return get_window(window_type, n, fftbins=False)      # symmetric, dsp.py:676
    except ValueError as e:
        logger.error("Invalid window type '%s': %s", window_type, e)
        raise ValueError(f"Invalid window type '{window_type}'.") from e


def apply_window(data, window_type: str = "hann") -> np.ndarray:
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    w = _symmetric_window(window_type, data.shape[0])
    x = ops.to_device_f32(data[None, :])
    z = ops.pack_real(x, data.shape[0], ops._dev(w.astype(np.float32)))
    return z[0, :, 0].cpu().numpy().astype(np.float64)


def compute_fft(data, fs: Union[int, float] = 1.0, n: Optional[int] = None, window: Optional[str] = "hann"
                ) -> Tuple[np.ndarray, np.ndarray]:
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    wdev = None
    if window:
        try:
            wdev = ops._dev(_symmetric_window(window, data.shape[0]).astype(np.float32))
        except ValueError as e:
            raise ValueError(f"Invalid window type '{window}': {e}") from e
    if n is None:
        n = data.shape[0]
    z = ops.pack_real(ops.to_device_f32(data[None, :]), int(n), wdev)
    spectrum = _c128(ops.fft_any(z))[0]
    freqs = np.fft.fftfreq(int(n), d=1 / fs)
    return freqs.astype(np.float64, copy=False), spectrum.astype(np.complex128, copy=False)


def compute_ifft(spectrum, n: Optional[int] = None) -> np.ndarray:
    spectrum = np.asarray(spectrum)
    if spectrum.ndim != 1:
        raise ValueError("Input spectrum must be a 1D array.")
    if n is None:
        n = spectrum.shape[0]
    n = int(n)
    s = np.zeros(n, dtype=np.complex128)           # ifft(x, n) truncates / zero-pads the spectrum
    m = min(n, spectrum.shape[0])
    s[:m] = spectrum[:m]
    z = ops._dev(np.stack([s.real, s.imag], axis=-1).astype(np.float32)[None])
    t = _c128(ops.fft_any(z, inverse=True))[0]
    peak = float(np.max(np.abs(t))) if t.size else 0.0
    imag_max = float(np.max(np.abs(t.imag))) if t.size else 0.0
    # reference warns above 1e-9 absolute (float64); the fp32 device floor is ~1e-7 of the peak
    if imag_max > max(1e-9, 1e-5 * peak):
        logger.warning("Significant imaginary part found in IFFT result (max abs: %.2e). "
                       "Input spectrum might not have conjugate symmetry.", imag_max)
    return np.real(t).astype(np.float64, copy=False)


def compute_stft(y, n_fft: int = 2048, hop_length: Optional[int] = None, win_length: Optional[int] = None,
                 window: str = "hann", center: bool = True, pad_mode: str = "constant") -> np.ndarray:
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    if win_length is None:
        win_length = n_fft
    if hop_length is None:
        hop_length = win_length // 4
    if center and pad_mode != "constant":
        y = np.pad(y, n_fft // 2, mode=pad_mode)   # data movement only; zeros are padded on the device
        center = False
    if not center and y.shape[0] < n_fft:
        raise ValueError(f"n_fft={n_fft} is too large for input signal of length={y.shape[0]}")
    X = ops.stft_any(ops.to_device_f32(y[None, :]), n_fft, hop_length, center, window, win_length)
    return np.ascontiguousarray(_c128(X)[0].T).astype(np.complex128, copy=False)   # [F, T] like librosa


_cqt_warned = False


def compute_cqt(y, sr: int, hop_length: Optional[int] = 512, fmin: Optional[float] = None, n_bins: int = 84,
                bins_per_octave: int = 12, **kwargs) -> np.ndarray:
    """Constant-Q transform, complex128 [n_bins, 1 + len(y)//hop_length] (dsp.py:231-289).

    Accepted librosa keyword arguments: tuning (default 0.0), filter_scale (1), sparsity (0.01); the fixed choices
    norm=1, window='hann', scale=True, pad_mode='constant' may be passed but not changed.  The decimation filter
    differs from librosa's soxr_hq resampler (see sygnals_amd/_cqt.py).  Served: every combination of
    bins_per_octave and filter_scale whose octave frames (the power of two above the longest wavelet) are at most 1024
    samples -- with the default fmin at 48 kHz and hop 512, 60 bins per octave at filter_scale 1, 36 at 1.5, 24 at
    2.5 and 12 at 5 are served, 64 at 1 is not; what is not, ops.cqt refuses with a ValueError that names the two parameters
    (tests/cqt_cases.py: the tested settings).
    """
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    fixed = {"norm": 1, "window": "hann", "scale": True, "pad_mode": "constant"}
    for k, v in fixed.items():
        if k in kwargs and kwargs.pop(k) != v:
            raise SygnalsHipError(f"compute_cqt: only {k}={v!r} runs on the device")
    # APPROXIMATE ROW: librosa decimates between octaves with its default res_type='soxr_hq' (libsoxr:
    # stop band about -125 dB); the device (and this repository's oracle) use a 41-tap half-band FIR, Kaiser beta 10:
    # stop band <= -99 dB from 0.66 pi, pass band within 1.3e-5 up to 0.34 pi.  Measured against a -155 dB half-band:
    # 2e-5 ... 5e-5 of the transform's peak (tools/cqt_decimator_study.py).  librosa's default spelling is accepted
    # with that warning; a request for any OTHER resampler cannot be honoured and is refused rather than dropped.
    res_type = kwargs.pop("res_type", None)
    if res_type not in (None, "soxr_hq", "kaiser_halfband"):
        raise SygnalsHipError(f"compute_cqt: res_type={res_type!r} is not available on the device; the octave "
                              "decimator is a fixed 41-tap Kaiser half-band FIR (res_type='kaiser_halfband')")
    global _cqt_warned
    if res_type != "kaiser_halfband" and not _cqt_warned:
        _cqt_warned = True
        logger.warning("compute_cqt: the device path decimates with a 41-tap half-band FIR (Kaiser beta 10: stop band "
                       "<= -99 dB, pass band within 1.3e-5), not librosa's res_type='soxr_hq' (about -125 dB); values "
                       "differ from librosa.cqt by about 2e-5 ... 5e-5 of the transform's peak "
                       "(pass res_type='kaiser_halfband' to acknowledge)")
    tuning = kwargs.pop("tuning", 0.0)
    filter_scale = kwargs.pop("filter_scale", 1.0)
    sparsity = kwargs.pop("sparsity", 0.01)
    if kwargs:
        raise TypeError(f"compute_cqt: unsupported arguments {sorted(kwargs)}")
    if tuning is None:
        raise SygnalsHipError("compute_cqt: tuning estimation (tuning=None) is not offloaded; pass a number")
    out = ops.cqt(ops.to_device_f32(y[None, :]), sr, int(hop_length), fmin, n_bins, bins_per_octave, tuning,
                  filter_scale, sparsity)
    return _c128(out)[0].astype(np.complex128, copy=False)


def compute_psd_welch(x, fs: float = 1.0, window: str = "hann", nperseg: Optional[int] = None,
                      noverlap: Optional[int] = None, nfft: Optional[int] = None,
                      detrend: Union[str, bool] = "constant", scaling: str = "density"
                      ) -> Tuple[np.ndarray, np.ndarray]:
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    f, p = welch_batch(ops.to_device_f32(x[None, :]), fs, window, nperseg, noverlap, nfft, detrend, scaling)
    return f, p[0].cpu().numpy().astype(np.float64)


def _welch_args(L, fs, window, nperseg, noverlap, nfft, detrend, scaling):
    """scipy.signal.welch's defaults and argument checks for rows of L samples -> (nperseg, noverlap, nfft, window table, scale)"""
    if nperseg is None:
        nperseg = 256
    if nperseg > L:
        logger.warning("nperseg = %d is greater than input length = %d, using nperseg = %d", nperseg, L, L)
        nperseg = L
    nperseg = int(nperseg)
    if nfft is None:
        nfft = nperseg
    elif nfft < nperseg:
        raise ValueError("nfft must be greater than or equal to nperseg.")
    if noverlap is None:
        noverlap = nperseg // 2
    if noverlap >= nperseg:
        raise ValueError("noverlap must be less than nperseg.")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"Unknown scaling: {scaling!r}")
    ops.detrend_code(detrend)                                 # ValueError for anything but constant / linear / False
    w = get_window(window, nperseg)
    scale = 1.0 / (fs * (w * w).sum()) if scaling == "density" else 1.0 / w.sum() ** 2
    return nperseg, int(noverlap), int(nfft), w, scale


def welch_batch(x, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, detrend="constant",
                scaling="density"):
    """[B, L] device tensor -> (freqs float64 [F], Pxx device tensor [B, F]); scipy.signal.welch rules."""
    nperseg, noverlap, nfft, w, scale = _welch_args(x.shape[1], fs, window, nperseg, noverlap, nfft, detrend, scaling)
    p = ops.welch(x, nperseg, noverlap, nfft, w, detrend, scale)
    return np.fft.rfftfreq(nfft, 1 / fs).astype(np.float64), p


# ------------------------------------------------------------------ cross-spectral analysis (scipy.signal.csd / coherence;
# not in the reference's code: its specification lists correlation beside Welch, docs/dev_spec_v1.0.0.md 3.5, and
# multi-channel handling, 3.7).  Served: real float32 rows of one length, y with one row (a reference channel) or one per
# row of x, detrend False / 'constant' / 'linear', both scalings, any nperseg >= 1 and nfft >= nperseg, average='mean'.
_XSPEC_SERVED = ("served: real float32 rows x [B, L] and y [1 or B, L] of one length, average='mean', detrend False / "
                 "'constant' / 'linear', scaling 'density' / 'spectrum'")


def _xspec(x, y, fs, window, nperseg, noverlap, nfft, detrend, scaling, average, want, who, host=False):
    """the checks (all before any device work), then ops.cross_spectrum; host: x, y are host tensors still to be moved"""
    if average != "mean":
        raise ValueError(f"{who}: average={average!r} is not served ({_XSPEC_SERVED})")
    for t, name in ((x, "x"), (y, "y")):
        if not hasattr(t, "shape") or len(t.shape) != 2:
            raise ValueError(f"{who}: {name} must be a [rows, samples] device tensor ({_XSPEC_SERVED})")
        if getattr(t, "is_complex", lambda: False)():
            raise ValueError(f"{who}: complex input is not served ({_XSPEC_SERVED})")
        if t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{who}: {name} is empty, shape {tuple(t.shape)} ({_XSPEC_SERVED})")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"{who}: rows of unequal length are not served: x has {x.shape[1]} samples and y {y.shape[1]}; scipy "
                         f"zero-pads the shorter one, here the caller does ({_XSPEC_SERVED})")
    if y.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"{who}: y must have one row or one row per row of x ({x.shape[0]}), got {y.shape[0]} ({_XSPEC_SERVED})")
    nperseg, noverlap, nfft, w, scale = _welch_args(x.shape[1], fs, window, nperseg, noverlap, nfft, detrend, scaling)
    if host:
        x, y = ops.to_device_f32(x), ops.to_device_f32(y)
    r = ops.cross_spectrum(x, y, nperseg, noverlap, nfft, w, detrend, scale, want=want)
    return np.fft.rfftfreq(nfft, 1 / fs).astype(np.float64), r


def csd_batch(x, y, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, detrend="constant", scaling="density",
              average="mean"):
    """x [B, L], y [1 or B, L] device tensors -> (freqs float64 [F], Pxy device tensor [B, F, 2] = (Re, Im));
    scipy.signal.csd rules: Pxy = mean over segments of conj(X) Y."""
    f, r = _xspec(x, y, fs, window, nperseg, noverlap, nfft, detrend, scaling, average, ("pxy",), "csd_batch")
    return f, r["pxy"]


def coherence_batch(x, y, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, detrend="constant", average="mean"):
    """-> (freqs, Cxy device tensor [B, F]): scipy.signal.coherence, |Pxy|^2 / (Pxx Pyy) formed in float64 on the device;
    NaN where Pxx Pyy = 0, 1 with one segment."""
    f, r = _xspec(x, y, fs, window, nperseg, noverlap, nfft, detrend, "density", average, ("coherence",), "coherence_batch")
    return f, r["coherence"]


def cross_spectra_batch(x, y, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, detrend="constant",
                        scaling="density", average="mean"):
    """-> (freqs, Pxy [B, F, 2], Pxx [B, F], Pyy [B, F], Cxy [B, F]) from one pass over the two signals."""
    f, r = _xspec(x, y, fs, window, nperseg, noverlap, nfft, detrend, scaling, average, ops.CSD_WANTS, "cross_spectra_batch")
    return f, r["pxy"], r["pxx"], r["pyy"], r["coherence"]


def _xspec_rows(x, y, who):
    x, y = np.asarray(x), np.asarray(y)
    if x.ndim != 1 or y.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    if np.iscomplexobj(x) or np.iscomplexobj(y):
        raise ValueError(f"{who}: complex input is not served ({_XSPEC_SERVED})")
    if x.size == 0 or y.size == 0:
        raise ValueError(f"{who}: empty input ({_XSPEC_SERVED})")
    if x.shape != y.shape:
        raise ValueError(f"{who}: rows of unequal length are not served: x has {x.size} samples and y {y.size}; scipy "
                         f"zero-pads the shorter one, here the caller does ({_XSPEC_SERVED})")
    return x, y


def _host_row(v):
    return ops.torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))[None]


def compute_csd(x, y, fs: float = 1.0, window: str = "hann", nperseg: Optional[int] = None, noverlap: Optional[int] = None,
                nfft: Optional[int] = None, detrend: Union[str, bool] = "constant", scaling: str = "density",
                average: str = "mean") -> Tuple[np.ndarray, np.ndarray]:
    """scipy.signal.csd(x, y) of two 1-D arrays of one length -> (freqs float64, Pxy complex128)."""
    x, y = _xspec_rows(x, y, "compute_csd")
    f, r = _xspec(_host_row(x), _host_row(y), fs, window, nperseg, noverlap, nfft, detrend, scaling, average, ("pxy",),
                  "compute_csd", host=True)
    return f, _c128(r["pxy"])[0].astype(np.complex128, copy=False)


def compute_coherence(x, y, fs: float = 1.0, window: str = "hann", nperseg: Optional[int] = None,
                      noverlap: Optional[int] = None, nfft: Optional[int] = None, detrend: Union[str, bool] = "constant",
                      average: str = "mean") -> Tuple[np.ndarray, np.ndarray]:
    """scipy.signal.coherence(x, y) of two 1-D arrays of one length -> (freqs float64, Cxy float64)."""
    x, y = _xspec_rows(x, y, "compute_coherence")
    f, r = _xspec(_host_row(x), _host_row(y), fs, window, nperseg, noverlap, nfft, detrend, "density", average, ("coherence",),
                  "compute_coherence", host=True)
    return f, r["coherence"][0].cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------ convolution / correlation (dsp.py:294-433)
_MODES = ("full", "valid", "same")


def _conv_slice(n: int, m: int, mode: str) -> Tuple[int, int]:
    """(start, count) of scipy's 'full' / 'same' (centred on the first input) / 'valid' result inside the full
    linear convolution of n and m samples."""
    if mode == "full":
        return 0, n + m - 1
    if mode == "same":
        return (m - 1) // 2, n
    return min(n, m) - 1, max(n, m) - min(n, m) + 1


def convolve_batch(x, kernel, mode: str = "same", correlate: bool = False):
    """Rows of the device tensor x [B, n] convolved (correlate=True: cross-correlated) with kernel [m] or [B, m]
    -> device tensor [B, count]; the batched form of apply_convolution / compute_correlation."""
    if mode not in _MODES:
        raise ValueError("acceptable mode flags are 'valid', 'same', or 'full'")
    k = kernel if kernel.dim() == 2 else kernel[None, :]
    n, m = x.shape[1], k.shape[1]
    if n == 0 or m == 0:
        raise ValueError("convolve_batch: empty input")
    start, count = _conv_slice(n, m, mode)
    return ops.rfft_conv(x, k, reverse_k=correlate)[:, start:start + count]


def apply_convolution(data, kernel, mode: str = "same") -> np.ndarray:
    data, kernel = np.asarray(data), np.asarray(kernel)
    if data.ndim != 1 or kernel.ndim != 1:
        raise ValueError("Input data and kernel must be 1D arrays.")
    if data.size == 0 or kernel.size == 0:
        if mode not in _MODES:
            raise ValueError("acceptable mode flags are 'valid', 'same', or 'full'")
        return np.array([], dtype=np.float64)                  # scipy.signal.fftconvolve's empty-input rule
    out = convolve_batch(ops.to_device_f32(data[None, :]), ops.to_device_f32(kernel[None, :]), mode)
    return out[0].cpu().numpy().astype(np.float64)


def compute_correlation(x, y, mode: str = "full", method: str = "auto") -> np.ndarray:
    """scipy.signal.correlate(x, y): every `method` gives the same numbers up to rounding; the device always
    uses the FFT form (x convolved with the reversed y)."""
    x, y = np.asarray(x), np.asarray(y)
    if x.ndim != 1 or y.ndim != 1:
        raise ValueError("Input sequences for correlation must be 1D arrays.")
    if method not in ("auto", "direct", "fft"):
        raise ValueError("Acceptable method flags are 'auto', 'direct', or 'fft'.")
    if mode not in _MODES:
        raise ValueError("Acceptable mode flags are 'valid', 'same', or 'full'.")
    if x.size == 0 or y.size == 0:
        return np.array([], dtype=np.float64)
    out = convolve_batch(ops.to_device_f32(x[None, :]), ops.to_device_f32(y[None, :]), mode, correlate=True)
    return out[0].cpu().numpy().astype(np.float64)


def compute_autocorrelation(x, mode: str = "full", method: str = "auto") -> np.ndarray:
    return compute_correlation(x, x, mode=mode, method=method)


# ------------------------------------------------------------------ periodogram (dsp.py:438-498)
def periodogram_batch(x, fs=1.0, window="hann", nfft=None, detrend="constant", scaling="density"):
    """[B, L] device tensor -> (freqs float64 [F], Pxx device tensor [B, F]); scipy.signal.periodogram rules."""
    L = x.shape[1]
    if L == 0:
        raise ValueError("periodogram_batch: empty input")
    if nfft is None:
        nfft = L
    nfft = int(nfft)
    if nfft < 1:
        raise ValueError("nfft must be a positive integer")
    nperseg = min(L, nfft)                                    # nfft < L truncates x to nfft samples
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"Unknown scaling: {scaling!r}")
    ops.detrend_code(detrend)
    if isinstance(window, (str, tuple)):
        w = get_window(window, nperseg)
    else:
        w = np.asarray(window, dtype=np.float64)
        if w.ndim != 1:
            raise ValueError("window must be 1-D")
        if w.shape[0] != nperseg:
            raise ValueError("window must have length of nperseg")
    scale = 1.0 / (fs * (w * w).sum()) if scaling == "density" else 1.0 / w.sum() ** 2
    p = ops.periodogram(x, nfft, w, detrend, scale)
    return np.fft.rfftfreq(nfft, 1 / fs).astype(np.float64), p


def compute_psd_periodogram(x, fs: float = 1.0, window="hann", nfft: Optional[int] = None,
                            detrend: Union[str, bool] = "constant", scaling: str = "density"
                            ) -> Tuple[np.ndarray, np.ndarray]:
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    if x.size == 0:
        return np.empty(0, dtype=np.float64), np.empty(0, dtype=np.float64)
    f, p = periodogram_batch(ops.to_device_f32(x[None, :]), fs, window, nfft, detrend, scaling)
    return f, p[0].cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------ envelope (dsp.py:565-636)
def analytic_batch(x):
    """Rows of the device tensor x [B, n] -> analytic signal, complex [B, n, 2] (scipy.signal.hilbert)."""
    if x.shape[1] == 0:
        raise ValueError("analytic_batch: empty input")
    return ops.analytic_signal(x)


def envelope_batch(x):
    """Rows of the device tensor x [B, n] -> |analytic signal| [B, n] (the packing, masking and |.| passes folded into the
    transforms where the length has a two-kernel plan)."""
    if x.shape[1] == 0:
        raise ValueError("envelope_batch: empty input")
    env = ops.analytic_fused(x, True) if (x.dtype == ops.torch.float32 and x.is_cuda) else None
    return env if env is not None else ops.cabs_pow(ops.analytic_signal(x), 1)


def amplitude_envelope(y, method: str = "hilbert", frame_length: Optional[int] = None,
                       hop_length: Optional[int] = None) -> np.ndarray:
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    if method == "hilbert":
        if y.size == 0:
            raise ValueError("N must be positive.")
        env = envelope_batch(ops.to_device_f32(y[None, :]))
        return env[0].cpu().numpy().astype(np.float64)
    if method == "rms":
        if frame_length is None or hop_length is None:
            raise ValueError("frame_length and hop_length are required for 'rms' envelope method.")
        from .audio.features import rms_energy
        return rms_energy(y, frame_length=frame_length, hop_length=hop_length, center=True)
    raise ValueError(f"Unsupported envelope method: {method}. Choose 'hilbert' or 'rms'.")


# ------------------------------------------------------------------ resampling (scipy.signal.resample_poly)
def resample_poly_batch(y, up, down, window=("kaiser", 5.0), padtype: str = "constant", cval=None):
    """Rows of the device tensor y [B, L] (float32) resampled by up / down -> device tensor [B, ceil(L up / down)]
    (ops.resample_poly: scipy.signal.resample_poly's filter, alignment and pad types constant, mean, minimum, maximum,
    edge, wrap, symmetric and reflect)."""
    return ops.resample_poly(y, up, down, window, padtype, cval)


def resample_batch(y, orig_sr, target_sr, window=("kaiser", 5.0), padtype: str = "constant", cval=None):
    """Rows of the device tensor y [B, L] from orig_sr to target_sr (positive, integer-valued rates): up / down is
    target_sr / orig_sr reduced."""
    up, down = _resample.ratio_of_rates(orig_sr, target_sr)
    return ops.resample_poly(y, up, down, window, padtype, cval)


def resample(data, orig_sr, target_sr, window=("kaiser", 5.0), padtype: str = "constant", cval=None) -> np.ndarray:
    """1-D data from orig_sr to target_sr, float64 out: scipy.signal.resample_poly(data, up, down) with up / down =
    target_sr / orig_sr reduced; the data is rounded to float32 and the arithmetic is float32 on the device."""
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    up, down = _resample.ratio_of_rates(orig_sr, target_sr)
    _resample.check_padtype(padtype, data.size if data.size else None)
    if data.size == 0:
        return np.array([], dtype=np.float64)
    out = ops.resample_poly(ops.to_device_f32(data[None, :]), up, down, window, padtype, cval)
    return out[0].cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------ cepstral analysis (not in the reference's code: its
# specification lists it, docs/dev_spec_v1.0.0.md 3.5; the float64 restatement tests/cepstrum_ref.py is the contract)
def real_cepstrum_batch(x, n: Optional[int] = None, amin: float = _cepstrum.AMIN):
    """Rows of the device tensor x [B, L] (float32) -> their real cepstra [B, n] (ops.real_cepstrum)."""
    return ops.real_cepstrum(x, n, amin)


def complex_cepstrum_batch(x, n: Optional[int] = None, amin: float = _cepstrum.AMIN):
    """Rows of the device tensor x [B, L] (float32) -> (complex cepstra [B, n], ndelay [B] int32) (ops.complex_cepstrum)."""
    return ops.complex_cepstrum(x, n, amin)


def inverse_complex_cepstrum_batch(ceps, ndelay):
    """(complex cepstra [B, n] on the device, ndelay [B]) -> the rows [B, n] (ops.inverse_complex_cepstrum)."""
    return ops.inverse_complex_cepstrum(ceps, ndelay)


def cepstrogram_batch(y, n_fft: int = 2048, hop_length: int = 512, center: bool = True, window="hann",
                      win_length: Optional[int] = None, n_ceps: Optional[int] = None, amin: float = _cepstrum.AMIN):
    """Clips y [B, L] on the device (float32) -> the real cepstrum of every frame, [B, Q, T] (ops.cepstrogram): compute_stft's
    framing, Q = n_ceps or n_fft // 2 + 1 quefrencies."""
    return ops.cepstrogram(y, n_fft, hop_length, center, window, win_length, n_ceps, amin)


def _cepstrum_row(data, n, n_min: int = 1):
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    if data.size == 0:
        raise ValueError("Input data must hold at least one sample.")
    return data, _cepstrum.row_length(n, data.shape[0], n_min)


def real_cepstrum(data, n: Optional[int] = None, amin: float = _cepstrum.AMIN) -> np.ndarray:
    """ifft(log(max(|fft(data, n)|, amin))).real, float64 [n]; data is rounded to float32 and the arithmetic is float32 on
    the device.  amin must be finite and >= 0 (at 0 a zero bin gives -inf)."""
    data, n = _cepstrum_row(data, n)
    amin = _cepstrum.check_amin(amin)
    return ops.real_cepstrum(ops.to_device_f32(data[None, :]), n, amin)[0].cpu().numpy().astype(np.float64)


def complex_cepstrum(data, n: Optional[int] = None, amin: float = _cepstrum.AMIN) -> Tuple[np.ndarray, int]:
    """(c float64 [n], ndelay): ifft(log(max(|X|, amin)) + i phi).real with phi the unwrapped phase of X = fft(data, n)
    (np.unwrap's rule; bin 0 counts as 0 or +pi by the sign of Re X[0]) less its linear term pi ndelay k / center,
    center = (n + 1) // 2, ndelay = rint(phi[center] / pi).  A right shift of a minimum-phase row by d samples gives
    ndelay = -d."""
    data, n = _cepstrum_row(data, n, 2)
    amin = _cepstrum.check_amin(amin)
    c, nd = ops.complex_cepstrum(ops.to_device_f32(data[None, :]), n, amin)
    return c[0].cpu().numpy().astype(np.float64), int(nd[0].item())


def inverse_complex_cepstrum(ceps, ndelay: int) -> np.ndarray:
    """The row whose complex cepstrum is (ceps, ndelay), float64.  Exact for even n at any ndelay; for odd n only at
    ndelay = 0 (the linear term is then no circular shift: errors of 1e-2 at n = 255 and ndelay = -31).  The sign of the
    row's sum is not part of (ceps, ndelay): a row with a negative sum comes back with its sum's sign turned, x - 2 mean(x)."""
    ceps, _ = _cepstrum_row(ceps, None, 2)
    if isinstance(ndelay, bool) or int(ndelay) != ndelay:
        raise ValueError(f"ndelay must be an integer, got {ndelay}")
    x = ops.inverse_complex_cepstrum(ops.to_device_f32(ceps[None, :]), [int(ndelay)])
    return x[0].cpu().numpy().astype(np.float64)
