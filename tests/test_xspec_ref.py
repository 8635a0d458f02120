"""The float64 restatement tests/xspec_ref.py against SciPy (scipy.signal.csd / coherence / welch / correlate), and the
conditions on the inputs of the GPU tests, asserted here so that a GPU failure cannot be blamed on the input.  CPU only."""
import numpy as np
import pytest
import scipy.fft
import scipy.signal

from tests import xspec_ref as R

FS = 48000.0


@pytest.fixture(scope="module")
def refs():
    """(inputs, restatement of row 0) per case, computed once"""
    out = {}
    for c in R.ALL_CASES:
        x, y = R.case_inputs(c)
        out[c["name"]] = (x, y, R.cross_spectra(x[0], y[0], fs=FS, **R.case_kw(c)))
    return out


@pytest.mark.parametrize("c", R.ALL_CASES, ids=lambda c: c["name"])
def test_restatement_equals_scipy(c, refs):
    x, y, (f, pxy, pxx, pyy, coh, _) = refs[c["name"]]
    kw = dict(R.case_kw(c), fs=FS)
    x0, y0 = x[0].astype(np.float64), y[0].astype(np.float64)
    fs_, sxy = scipy.signal.csd(x0, y0, **kw)
    S = np.sqrt(pxx * pyy)
    tol = 1e-12 * S.max()
    assert np.array_equal(f, fs_)
    assert np.abs(pxy - sxy).max() <= tol
    assert np.abs(pxx - scipy.signal.welch(x0, **kw)[1]).max() <= 1e-12 * pxx.max()
    assert np.abs(pyy - scipy.signal.welch(y0, **kw)[1]).max() <= 1e-12 * pyy.max()
    kc = {k: v for k, v in kw.items() if k != "scaling"}
    with np.errstate(invalid="ignore", divide="ignore"):
        sc = scipy.signal.coherence(x0, y0, **kc)[1]
    ok = np.isfinite(coh) & np.isfinite(sc) & (S > 0)
    assert np.array_equal(np.isnan(coh), np.isnan(sc))
    # an error of 1e-12 max S in each of Pxy, Pxx, Pyy moves |Pxy|^2 / (Pxx Pyy) by at most 4e-12 max S / S_k
    assert (np.abs(coh - sc)[ok] <= 4e-12 * S.max() / S[ok]).all()


@pytest.mark.parametrize("c", [c for c in R.ALL_CASES if c["coh"]], ids=lambda c: c["name"])
def test_condition_a_on_the_coherence_inputs(c):
    """every row on which the coherence is gated: min_k S_k >= 1e-3 max_k S_k, S = sqrt(Pxx Pyy) in float64"""
    x, y = R.case_inputs(c)
    for b in range(c["B"]):
        _, _, pxx, pyy, _, _ = R.cross_spectra(x[b], y[0 if y.shape[0] == 1 else b], fs=FS, **R.case_kw(c))
        S = np.sqrt(pxx * pyy)
        assert S.min() >= 1e-3 * S.max(), (c["name"], b, S.min() / S.max())


def test_one_segment_coherence_is_one():
    x, y = R.noise_pair(1, 256, 5)
    coh = R.cross_spectra(x[0], y[0], nperseg=256)[4]
    assert np.abs(coh - 1.0).max() <= 1e-12


def test_zero_row_gives_nan_coherence_and_zero_pxy():
    x, y = R.noise_pair(1, 600, 6)
    _, pxy, pxx, _, coh, _ = R.cross_spectra(np.zeros(600), y[0], nperseg=128)
    assert not pxy.any() and not pxx.any() and np.isnan(coh).all()


@pytest.mark.parametrize("c", R.GCC_CASES, ids=lambda c: c["name"])
def test_gcc_none_equals_scipy_correlate(c):
    x, y = R.gcc_inputs(c)
    for b in (0, c["B"] - 1):
        xb, yb = x[b].astype(np.float64), y[0 if y.shape[0] == 1 else b].astype(np.float64)
        lags, r = R.gcc(xb, yb, c["max_lag"], "none")
        full = scipy.signal.correlate(xb, yb, "full", method="direct" if xb.size <= 1000 else "fft")
        fl = scipy.signal.correlation_lags(xb.size, yb.size, "full")
        ref = full[np.searchsorted(fl, lags)]
        assert np.array_equal(fl[np.searchsorted(fl, lags)], lags)
        assert np.abs(r - ref).max() <= 1e-12 * np.abs(full).max()
        # the sign convention: x[n] = y[n - d] peaks at lag +d
        d = c["delays"][b % len(c["delays"])]
        if abs(d) <= lags[-1]:
            assert lags[int(np.argmax(r))] == d


def test_phat_by_construction():
    g = np.random.default_rng(3)
    L = 300
    y = g.standard_normal(L)
    for d in (0, 7, -33, 250):
        x = np.roll(y, d)
        X, Y = np.fft.rfft(x), np.fft.rfft(y)
        G = X * np.conj(Y)
        a = np.abs(G)
        assert (a > 0).all() and np.abs(np.abs(G / a) - 1.0).max() <= 1e-12          # |W G| = 1 on every non-zero bin
        full = R.gcc(x, y, None, "phat", n=L)[1]
        imp = np.zeros(L)
        imp[d % L] = 1.0
        circ = np.array([full[(L - 1) + t] for t in range(0, L)])                   # lags 0 .. L - 1: one full period
        assert np.abs(circ - imp).max() <= 1e-12                                     # a unit impulse at the shift
    # a bin that is exactly 0 gets W = 0
    x0 = np.zeros(L)
    assert not R.gcc(x0, y, 10, "phat")[1].any()


@pytest.mark.parametrize("w", ["none", "phat"])
@pytest.mark.parametrize("c", R.GCC_CASES, ids=lambda c: c["name"])
def test_condition_b_on_the_gcc_inputs(c, w):
    """a float32 scipy.fft evaluation of the same definition is within 1e-6 of the peak of the float64 one, and the
    runner-up lag is below half the peak"""
    x, y = R.gcc_inputs(c)
    for b in range(min(c["B"], 4)):
        xb, yb = x[b], y[0 if y.shape[0] == 1 else b]
        lags, r64 = R.gcc(xb, yb, c["max_lag"], w)
        _, r32 = R.gcc(xb, yb, c["max_lag"], w, dtype=np.float32)
        assert r32.dtype == np.float32
        pk = np.abs(r64).max()
        assert np.abs(r32 - r64).max() <= 1e-6 * pk, (c["name"], b, np.abs(r32 - r64).max() / pk)
        d = c["delays"][b % len(c["delays"])]
        if abs(d) <= lags[-1]:
            i = int(np.argmax(r64))
            assert lags[i] == d
            rest = np.delete(r64, i)
            assert rest.size == 0 or rest.max() < 0.5 * r64[i], (c["name"], b, rest.max() / r64[i])


def test_pick_rule():
    r = np.array([0.0, 1.0, 3.0, 3.0, 1.0])
    d, lag, pk = R.pick(r, -2, fs=2.0)                   # first maximum at index 2; parabola through (1, 3, 3)
    assert lag == 0 and d == pytest.approx(0.5 / 2.0) and pk == pytest.approx(3.25)
    assert R.pick(np.array([5.0, 1.0, 2.0]), -1) == (-1.0, -1, 5.0)      # a maximum on the edge is not refined
    assert R.pick(np.array([1.0, 1.0, 1.0]), 0) == (0.0, 0, 1.0)         # flat: the parabola does not open downwards


def test_half_sample_delay_input():
    """x = the mean of y delayed by 6 and by 7 samples: the refined estimate is within 0.5 sample of 6.5"""
    g = np.random.default_rng(11)
    y = g.standard_normal(1000)
    x = 0.5 * (np.concatenate([np.zeros(6), y[:-6]]) + np.concatenate([np.zeros(7), y[:-7]]))
    for w in ("none", "phat"):
        lags, r = R.gcc(x, y, 64, w)
        d, lag, _ = R.pick(r, int(lags[0]))
        assert lag in (6, 7) and abs(d - 6.5) <= 0.5
