"""Device-backed mirror of sygnals/core/transforms.py: discrete_wavelet_transform :22-79,
inverse_discrete_wavelet_transform :81-115 (pywt.wavedec / waverec: the Daubechies family haar, db1 ... db10 and the modes
symmetric, reflect, periodic, constant and zero; sygnals_amd/_wavelets.py, csrc/dwt.hip), hilbert_transform :119-151 and
laplace_transform_numerical :159-199 (sygnals_amd/_laplace.py, csrc/laplace.hip).  continuous_wavelet_transform is the
pywt.cwt call of sygnals/utils/visualizations.py plot_scalogram (morl, mexh, gaus1 and cmorB-C; sygnals_amd/_cwt.py,
csrc/cwt.hip).

`dwt_batch` / `idwt_batch` are the batched forms that keep the coefficients on the device, `laplace_batch` the one that
keeps the transform there, `cwt_batch` the one that keeps the scalogram there.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from .. import _cwt, _laplace, _wavelets, ops
from .dsp import _c128, analytic_batch


def hilbert_transform(data) -> np.ndarray:
    """Analytic signal x + i*H(x) (scipy.signal.hilbert), complex128."""
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    if data.size == 0:
        raise ValueError("N must be positive.")
    return _c128(analytic_batch(ops.to_device_f32(data[None, :])))[0].astype(np.complex128, copy=False)


def dwt_batch(y: torch.Tensor, wavelet: str = "db4", level: Optional[int] = None, mode: str = "symmetric"):
    """Multi-level DWT of every clip of y [B, L] (float32, on the device) -> (packed [B, total] device tensor, lens):
    row b is [cA_n | cD_n | ... | cD_1] of clip b and `lens` the lengths of those arrays (ops.dwt)."""
    return ops.dwt(y, wavelet, level, mode)


def idwt_batch(packed: torch.Tensor, lens, wavelet: str = "db4", mode: str = "symmetric") -> torch.Tensor:
    """Inverse of dwt_batch: packed [B, sum(lens)] -> [B, L'] on the device (ops.idwt)."""
    return ops.idwt(packed, lens, wavelet, mode)


def discrete_wavelet_transform(data, wavelet: str = "db4", level: Optional[int] = None,
                               mode: str = "symmetric") -> List[np.ndarray]:
    """pywt.wavedec: [cA_n, cD_n, ..., cD_1], float64 arrays."""
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    if data.size == 0:
        raise ValueError("Input data must hold at least one sample.")
    if level is None:
        try:
            level = max(1, _wavelets.dwt_max_level(data.size, _wavelets.filter_length(wavelet)))
        except ValueError as e:
            raise ValueError(f"Invalid wavelet name '{wavelet}' or error calculating max level.") from e
    elif isinstance(level, bool) or not isinstance(level, int) or level < 1:
        raise ValueError(f"Decomposition level must be an integer >= 1, got {level}.")
    packed, lens = ops.dwt(ops.to_device_f32(data[None, :]), wavelet, level, mode)
    row = packed[0].cpu().numpy().astype(np.float64)
    return [c.copy() for c in np.split(row, np.cumsum(lens)[:-1])]


def inverse_discrete_wavelet_transform(coeffs, wavelet: str, mode: str = "symmetric") -> np.ndarray:
    """pywt.waverec of [cA_n, cD_n, ..., cD_1] -> float64 signal."""
    if not isinstance(coeffs, list) or len(coeffs) < 2:
        raise ValueError("Input 'coeffs' must be a list containing at least cA and cD coefficients.")
    arrs = [np.asarray(c, dtype=np.float32) for c in coeffs]
    if any(a.ndim != 1 for a in arrs):
        raise ValueError("Every coefficient array must be 1D.")
    lens = [a.size for a in arrs]
    _wavelets.waverec_length(lens, _wavelets.filter_length(wavelet))         # refuses mismatched lengths before a copy
    y = ops.idwt(ops.to_device_f32(np.concatenate(arrs)[None, :]), lens, wavelet, mode)
    return y[0].cpu().numpy().astype(np.float64)


def laplace_batch(y: torch.Tensor, s_values, t_step: float = 1.0) -> torch.Tensor:
    """Numerical Laplace transform of every clip of y [B, L] (float32, on the device) at the complex s_values [S] ->
    [B, S] complex128 on the device: F[b, i] = t_step sum_n y[b, n] exp(-s_i n t_step) (ops.laplace)."""
    return ops.laplace(y, s_values, t_step)


def laplace_transform_numerical(data, s_values, t_step: float = 1.0) -> np.ndarray:
    """sum_n data[n] exp(-s n t_step) t_step for each s in s_values, complex128.  Served: finite t_step and s-values with
    -Re(s) t_step (len(data) - 1) <= 700 (beyond that the reference's own exp overflows); the data is rounded to float32."""
    data, s_values = np.asarray(data), np.asarray(s_values)
    if data.ndim != 1:
        raise ValueError("Input data must be 1D.")
    if s_values.ndim != 1:
        raise ValueError("s_values must be 1D.")
    s = _laplace.check_s_values(s_values, t_step)
    if s.size == 0 or data.size == 0:                                # an empty list gives an empty result, no data zeros
        return np.zeros(s.size, dtype=np.complex128)
    _laplace.check_domain(s, t_step, data.size)
    return ops.laplace(ops.to_device_f32(data[None, :]), s, t_step)[0].cpu().numpy()


def scalogram_scales(num, L) -> np.ndarray:
    """The scale grid plot_scalogram makes from a count: geomspace(1, max(2, L / 8), max(1, num))."""
    return _cwt.scalogram_scales(num, L)


def central_frequency(wavelet, precision: int = 8) -> float:
    """pywt.central_frequency of a served wavelet, in cycles per unit of its own axis."""
    return _cwt.central_frequency(wavelet, precision)


def scale2frequency(wavelet, scales, precision: int = 8) -> np.ndarray:
    """pywt.scale2frequency: central_frequency(wavelet) / scales."""
    return _cwt.scale2frequency(wavelet, _cwt.check_scales(scales), precision)


def cwt_batch(y: torch.Tensor, scales, wavelet: str = "morl", output: str = "magnitude", stride: int = 1) -> torch.Tensor:
    """Scalograms of every clip of y [B, L] (float32, on the device) -> [B, S, ceil(L / stride)] float32 on the device
    ([..., 2] for the `coef` of a complex wavelet): the image-like feature format_features_as_image / image_device take
    (ops.cwt)."""
    return ops.cwt(y, scales, wavelet, output, stride)


def continuous_wavelet_transform(data, scales, wavelet: str = "morl", sampling_period: float = 1.0, method: str = "conv"):
    """pywt.cwt without `axis`: (coefs [S, L], frequencies [S]); coefs float64 for a real wavelet, complex128 for a complex
    one.  method: 'conv' (the library's rule picks the path per scale) | 'fft' (every scale through the transforms).  The
    data is rounded to float32."""
    data = np.asarray(data)
    if data.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    if data.size == 0:
        raise ValueError("Input data must hold at least one sample.")
    if method not in ("conv", "fft"):
        raise ValueError("method must be 'conv' or 'fft'.")
    w = _cwt.parse_wavelet(wavelet)
    s = _cwt.check_scales(scales)
    _cwt.cwt_plan(s, wavelet)                                        # a scale too small is refused before a copy
    W = ops.cwt(ops.to_device_f32(data[None, :]), s, wavelet, "coef", 1, form="spectral" if method == "fft" else None)[0]
    W = W.cpu().numpy().astype(np.float64)
    coefs = W[..., 0] + 1j * W[..., 1] if w.complex else W
    return coefs, _cwt.scale2frequency(wavelet, s) / sampling_period
