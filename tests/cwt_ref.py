"""PyWavelets 1.x `pywt.cwt`, `integrate_wavelet`, `central_frequency`, restated in float64 NumPy for the four wavelets
the project serves (morl, mexh, gaus1, cmorB-C).  PyWavelets is not installed where these tests run, so this restatement
is the contract the device is held to; parity with PyWavelets itself is unpinned (the restatement was checked only through
the central frequencies it yields: 0.8125, 0.25, 0.2 and C, PyWavelets' documented values).

This file computes step 3 as pywt does, diff(convolve(data, k_s)); the package's plan (sygnals_amd/_cwt.py) differences
the filter instead.  tests/test_cwt_ref.py holds the two against each other."""
import re

import numpy as np


def wavelet_def(name):
    """(psi, lo, hi, is_complex)"""
    if name == "morl":
        return (lambda x: np.exp(-x ** 2 / 2) * np.cos(5 * x)), -8.0, 8.0, False
    if name == "mexh":
        return (lambda x: 2 / (np.sqrt(3) * np.pi ** 0.25) * (1 - x ** 2) * np.exp(-x ** 2 / 2)), -8.0, 8.0, False
    if name == "gaus1":
        return (lambda x: -2 * x * np.exp(-x ** 2) / (np.pi / 2) ** 0.25), -5.0, 5.0, False
    m = re.fullmatch(r"cmor([0-9.]+)-([0-9.]+)", name)
    if not m:
        raise ValueError(name)
    B, C = float(m.group(1)), float(m.group(2))
    return (lambda x: (np.pi * B) ** -0.5 * np.exp(-x ** 2 / B) * np.exp(2j * np.pi * C * x)), -8.0, 8.0, True


def integrate_wavelet(name, precision=10):
    psi, lo, hi, cplx = wavelet_def(name)
    x = np.linspace(lo, hi, 2 ** precision)
    step = x[1] - x[0]
    return np.cumsum(psi(x)) * step, x


def kernel(name, s):
    """k_s: the integrated wavelet (conjugated when complex) resampled to scale s and reversed."""
    int_psi, x = integrate_wavelet(name)
    if wavelet_def(name)[3]:
        int_psi = np.conj(int_psi)
    step = x[1] - x[0]
    j = (np.arange(s * (x[-1] - x[0]) + 1) / (s * step)).astype(int)
    if j[-1] >= int_psi.size:
        j = np.extract(j < int_psi.size, j)
    return int_psi[j][::-1]


def cwt_scale(data, name, s):
    """One row of pywt.cwt(data, [s], name)[0], conv method."""
    data = np.asarray(data, dtype=np.float64)
    conv = np.convolve(data, kernel(name, s))
    coef = -np.sqrt(s) * np.diff(conv)
    d = (coef.shape[-1] - data.shape[-1]) / 2.0
    if d > 0:
        coef = coef[int(np.floor(d)):coef.shape[-1] - int(np.ceil(d))]
    elif d < 0:
        raise ValueError(f"Selected scale of {s} too small.")
    return coef


def central_frequency(name, precision=8):
    psi, lo, hi, _ = wavelet_def(name)
    x = np.linspace(lo, hi, 2 ** precision)
    p = psi(x)
    domain = float(x[-1] - x[0])
    index = int(np.argmax(np.abs(np.fft.fft(p)[1:]))) + 2
    if index > len(p) / 2:
        index = len(p) - index + 2
    return 1.0 / (domain / (index - 1))


def cwt(data, scales, name, sampling_period=1.0):
    """(coefs [S, L] float64 or complex128, frequencies [S])"""
    scales = np.asarray(scales, dtype=np.float64)
    cplx = wavelet_def(name)[3]
    out = np.empty((scales.size, np.asarray(data).shape[-1]), dtype=np.complex128 if cplx else np.float64)
    for i, s in enumerate(scales):
        out[i] = cwt_scale(data, name, float(s))
    return out, central_frequency(name) / scales / sampling_period


def h_filter(name, s):
    """(h_s, floor(d)): the differenced filter of the issue's identity, from this file's own kernel."""
    k = kernel(name, s)
    n = k.size
    if n < 2:
        raise ValueError(f"Selected scale of {s} too small.")
    dk = np.concatenate([k[:1], np.diff(k), -k[-1:]])
    return -np.sqrt(s) * dk, int(np.floor((n - 2) / 2.0))


def cwt_rows(x, scales, name):
    """Float64 reference for a batch x [B, L] (the float32 input's values): [B, S, L], via FFT convolution per scale (the
    conv-then-diff form in float64 costs O(L taps) per row; scipy's fftconvolve in float64 is good to ~1e-15 of
    ||h||_1 max|x|, ten orders below the gate)."""
    from scipy.signal import fftconvolve
    x = np.asarray(x, dtype=np.float64)
    B, L = x.shape
    cplx = wavelet_def(name)[3]
    out = np.empty((B, len(scales), L), dtype=np.complex128 if cplx else np.float64)
    for i, s in enumerate(scales):
        k = kernel(name, float(s))
        n = k.size
        if n < 2:
            raise ValueError(f"Selected scale of {s} too small.")
        conv = fftconvolve(x, k[None, :], mode="full", axes=1) if L * n > 1 << 16 else np.stack([np.convolve(r, k) for r in x])
        coef = -np.sqrt(s) * np.diff(conv, axis=1)
        d = (coef.shape[1] - L) / 2.0
        if d > 0:
            coef = coef[:, int(np.floor(d)):coef.shape[1] - int(np.ceil(d))]
        out[:, i] = coef
    return out
