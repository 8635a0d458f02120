"""tests/hpss_cases.py held to its purpose, on the CPU with the float64 restatement alone: the inputs reach the rules the
GPU tests of tests/test_gpu_hpss_params.py are about, whatever a kernel does with them."""
import functools

import numpy as np
import pytest

from sygnals_amd import ops
from tests import hpss_cases as K
from tests import hpss_ref as R

TIE_INPUTS = tuple((3, T) for T in K.MEDIAN_T) + ((2, 33),)


@functools.lru_cache(maxsize=None)
def _tie_mag(B, T):
    S = K.mag32(K.tie_spectrum(B, T))
    S.setflags(write=False)
    return S


def _medians(S, win):
    return R.median_filter_axis(S, win[0], axis=1), R.median_filter_axis(S, win[1], axis=2)


def _lower_median(X, k, axis):
    """median_filter_axis with the rank (k - 1) // 2: what a kernel off by one at an even window would compute."""
    X = np.moveaxis(np.asarray(X), axis, -1)
    n = X.shape[-1]
    idx = R.reflect_index(np.arange(n)[:, None] - k // 2 + np.arange(k)[None, :], n)
    return np.moveaxis(np.sort(X[..., idx], axis=-1)[..., (k - 1) // 2], -1, axis)


def test_tie_spectrum_values():
    S = _tie_mag(3, 40)
    want = np.float32([0, 3, 4, 5, 6, np.sqrt(52), 8, np.sqrt(73), 10])
    assert np.array_equal(np.unique(S), want)
    assert np.array_equal(K.tie_spectrum(3, 40), K.tie_spectrum(3, 40))              # seeded
    D = K.tie_spectrum(3, 40)
    assert not np.array_equal(D[0], D[1]) and not np.array_equal(D[1], D[2])         # the clips of a batch differ


@pytest.mark.parametrize("B,T", TIE_INPUTS)
def test_tie_spectrum_ties_and_zeros(B, T):
    S = _tie_mag(B, T)
    for win in K.MEDIAN_WINDOWS + (K.SOFTMASK_WINDOWS,):
        H, P = _medians(S, win)
        assert np.mean(H == P) >= 0.20, (win, np.mean(H == P))
        if max(win) <= 17:
            assert np.sum((H == 0) & (P == 0)) >= 1000, (win, np.sum((H == 0) & (P == 0)))


def test_softmask_input_has_both_kinds():
    H, P = _medians(_tie_mag(2, 33), K.SOFTMASK_WINDOWS)
    assert np.sum((H == 0) & (P == 0)) >= 1000
    assert np.sum((H == P) & (H > 0)) >= 1000


@pytest.mark.parametrize("T", (17, 40))
def test_tie_spectrum_tells_the_rank_of_an_even_window(T):
    S = _tie_mag(3, T)
    for k in sorted({k for win in K.MEDIAN_WINDOWS for k in win if k % 2 == 0}):
        for axis in (1, 2):
            assert np.mean(R.median_filter_axis(S, k, axis) != _lower_median(S, k, axis)) >= 0.05, (k, axis)
    for k in (3, 31, 63):                                                            # (an odd window has one median)
        assert np.array_equal(R.median_filter_axis(S, k, 1), _lower_median(S, k, 1))


def test_edge_spectrum_kinds():
    D = K.edge_spectrum(K.EDGE_T)
    assert D.shape == (1, K.EDGE_T, K.NB, 2) and D.dtype == np.float32
    S = K.mag32(D)[0]
    cells = K.edge_cells(K.EDGE_T)
    tiny32 = np.finfo(np.float32).tiny
    t, f = cells["tiny"]
    with np.errstate(under="ignore"):
        sq = D[0, t, f] ** 2
    assert np.all((sq > 0) & (sq < tiny32))                                          # both squares denormal, neither flushed
    assert np.all(S[t, f] >= 1e-21) and np.all(S[t, f] < 2e-19)                      # and the magnitude normal
    t, f = cells["huge"]
    assert np.all(np.isposinf(S[t, f])) and np.all(np.isfinite(D[0, t, f]))
    t, f = cells["zero"]
    assert not S[t, f].any()
    assert np.isinf(S).sum() <= 80 and np.isfinite(S).sum() == S.size - np.isinf(S).sum()
    # every kind is the median of some window at every pair of windows the GPU test runs: it is in the output, where a
    # wrong bit shows, and +inf stays rare
    tiny_values = set(S[cells["tiny"]].tolist())
    for win in K.EDGE_WINDOWS:
        H = R.median_filter_axis(S, win[0], axis=0)
        P = R.median_filter_axis(S, win[1], axis=1)
        for M in (H, P):
            assert np.mean(np.isinf(M)) <= 0.01, win
        both = np.concatenate([H.ravel(), P.ravel()])
        assert np.isposinf(both).sum() >= 5 and (both == 0).sum() >= 5, win
        assert sum(v in tiny_values for v in both[(both > 0) & (both < 1e-18)].tolist()) >= 5, win


def test_edge_spectrum_shows_flushed_denormal_squares():
    # a magnitude whose denormal squares were flushed to zero is 0 on the tiny cells, and that reaches the medians
    D = K.edge_spectrum(K.EDGE_T)
    S = K.mag32(D)[0]
    with np.errstate(under="ignore", over="ignore"):
        sq = D[0] * D[0]
    sq[sq < np.finfo(np.float32).tiny] = 0.0
    F = np.sqrt(sq[..., 0] + sq[..., 1], dtype=np.float32)
    t, f = K.edge_cells(K.EDGE_T)["tiny"]
    assert not F[t, f].any() and np.array_equal(np.delete(F.ravel(), t * K.NB + f), np.delete(S.ravel(), t * K.NB + f))
    for win in K.EDGE_WINDOWS:
        for k, axis in zip(win, (0, 1)):
            assert np.sum(R.median_filter_axis(S, k, axis) != R.median_filter_axis(F, k, axis)) >= 5, (win, axis)


def _split_inverse(X, drop_imag):
    """irfft of X [1025] by the real-split form of the kernel (the even / odd samples as one 1024-point complex inverse),
    with or without discarding Im X[0] and Im X[1024] first."""
    X = np.array(X, dtype=np.complex128)
    if drop_imag:
        X[0], X[1024] = X[0].real, X[1024].real
    k = np.arange(1024)
    xk, xm = X[k], np.conj(X[1024 - k])
    Z = (xk + xm) / 2 + 1j * ((xk - xm) / 2 * np.exp(2j * np.pi * k / 2048))
    z = np.fft.ifft(Z)
    return np.stack([z.real, z.imag], axis=-1).ravel()


def test_noise_spectrum_shows_a_split_inverse_that_keeps_the_real_bins_imaginary_parts():
    X = K.to_complex(K.noise_spectrum(1, 2))[0, :, 0]
    want = np.fft.irfft(X, n=2048)
    assert np.abs(_split_inverse(X, True) - want).max() <= 1e-14 * np.abs(want).max()
    assert np.abs(_split_inverse(X, False) - want).max() >= 1e-4 * np.abs(want).max()   # ten times the GPU test's gate


def test_istft_seams_step_the_segment_count():
    # derived from the kernel's rule, not copied: the first lengths at which a clip takes two and three waves
    first = {n: next(L for L in range(1, 40000) if K.istft_segments(L) == n) for n in (2, 3)}
    assert K.ISTFT_SEAMS == (first[2] - 1, first[2], first[3] - 1, first[3])
    assert [K.istft_segments(L) for L in K.ISTFT_SEAMS] == [1, 2, 2, 3]
    for L in (1, 511, 512, 1023, 1535, 7679, 7680):                                  # the lengths of tests/test_gpu_hpss.py
        assert K.istft_segments(L) == 1


def test_hnr_cases_have_frames():
    for c in K.HNR_CASES:
        T = ops.num_frames_padded(c.L, c.fl, c.hop, bool(c.center))
        assert T >= 1, c
        yh, yp = K.hnr_rows_input(c)
        assert yh.shape == yp.shape == (c.B, c.L) and yh.dtype == yp.dtype == np.float32
        hnr, ph, pp = R.hnr_from_components(yh[0], yp[0], c.fl, c.hop, bool(c.center))
        assert hnr.shape == ph.shape == pp.shape == (T,), c
    odd = K.HNR_CASES[3]
    assert ops.num_frames_padded(odd.L, odd.fl, odd.hop, True) == ops.num_frames(odd.L, odd.fl, odd.hop, True) - 1
    assert ops.num_frames_padded(4096, 4096, 1024, False) == 1 == ops.num_frames_padded(100, 4096, 1024, True)
    last = K.HNR_CASES[-1]
    assert last.ld > last.L and (last.B * ops.num_frames_padded(last.L, last.fl, last.hop, True)) % 4 != 0


def test_hnr_constant_rows_are_determinate():
    # the constants' interior powers sit 21 % above and 19 % below the threshold, and over every case at most 2 % of the
    # frames have a power within 1 % of it
    ch, cp = np.float64(np.float32(K.HNR_CONSTANTS[0])), np.float64(np.float32(K.HNR_CONSTANTS[1]))
    assert ch * ch > 1.2 * R.EPSILON and cp * cp < 0.82 * R.EPSILON
    for c in K.HNR_CASES:
        yh, yp = K.hnr_rows_input(c)
        near = total = 0
        for r in range(c.B):
            _, ph, pp = R.hnr_from_components(yh[r], yp[r], c.fl, c.hop, bool(c.center))
            near += int(np.sum((np.abs(ph / R.EPSILON - 1) < 0.01) | (np.abs(pp / R.EPSILON - 1) < 0.01)))
            total += ph.size
        assert near <= 0.02 * total, c
