"""The float64 index-form restatement (tests/resample_ref.py) equals scipy.signal.resample_poly within 1e-12 of the peak,
and the host plan (sygnals_amd/_resample.py) is that restatement's plan with a float32 table.  No device.
A one-sample row with padtype='reflect' is never handed to scipy (scipy itself dies on it)."""
import numpy as np
import pytest
from scipy.signal import resample_poly as sp_resample_poly

from sygnals_amd import _resample as RS
from tests import resample_ref as R

# (L, up, down): the shapes the arithmetic was checked on
SHAPES = [(1, 3, 2), (5, 160, 147), (37, 2, 1), (64, 1, 2), (101, 3, 7), (200, 147, 160), (333, 160, 441), (257, 320, 441)]
TAPS = [1, 2, 30, 31, 64]
TAP_RATIOS = [(3, 4), (5, 3), (2, 7)]
PAD_SHAPES = [(2, 160, 147), (5, 160, 147), (7, 3, 2), (37, 2, 3), (64, 160, 441), (101, 5, 3), (200, 147, 160)]


def _row(L, seed=0):
    rng = np.random.default_rng(1000 * L + seed)
    return rng.standard_normal(L) + 0.7                 # an offset: the statistic pad types must carry it


def _close(got, want):
    assert got.shape == want.shape
    peak = max(float(np.max(np.abs(want))), 1e-300)
    err = float(np.max(np.abs(got - want))) / peak
    assert err <= 1e-12, err


@pytest.mark.parametrize("L,up,down", SHAPES)
def test_defaults_equal_scipy(L, up, down):
    x = _row(L)
    _close(R.resample_poly(x, up, down), sp_resample_poly(x, up, down))


def test_kp_of_the_listed_shapes():
    want = {(5, 160, 147): 21, (64, 1, 2): 43, (200, 147, 160): 23, (333, 160, 441): 58, (257, 320, 441): 29}
    for (L, up, down), Kp in want.items():
        assert R.plan(L, up, down)[4] == Kp


@pytest.mark.parametrize("padtype", R.SERVED)
@pytest.mark.parametrize("L,up,down", PAD_SHAPES)
def test_padtypes_equal_scipy(padtype, L, up, down):
    x = _row(L, 1)
    _close(R.resample_poly(x, up, down, padtype=padtype), sp_resample_poly(x, up, down, padtype=padtype))


@pytest.mark.parametrize("L,up,down", PAD_SHAPES + [(1, 3, 2)])
def test_cval_equals_scipy(L, up, down):
    x = _row(L, 2)
    _close(R.resample_poly(x, up, down, padtype="constant", cval=2.5), sp_resample_poly(x, up, down, padtype="constant", cval=2.5))


@pytest.mark.parametrize("padtype", [p for p in R.SERVED if p != "reflect"])
def test_one_sample_rows(padtype):
    x = np.array([1.25])
    _close(R.resample_poly(x, 3, 2, padtype=padtype), sp_resample_poly(x, 3, 2, padtype=padtype))


@pytest.mark.parametrize("ntaps", TAPS)
@pytest.mark.parametrize("up,down", TAP_RATIOS)
def test_caller_taps_equal_scipy(ntaps, up, down):
    h = np.random.default_rng(ntaps).standard_normal(ntaps)
    for L in (1, 9, 150):
        x = _row(L, 3)
        _close(R.resample_poly(x, up, down, window=h), sp_resample_poly(x, up, down, window=h))


def test_identity_and_reduction():
    x = _row(50)
    assert np.array_equal(R.resample_poly(x, 4, 4), x)
    _close(R.resample_poly(x, 6, 4), sp_resample_poly(x, 3, 2))


@pytest.mark.parametrize("L,up,down", SHAPES + [(2, 160, 147), (4097, 441, 160), (1 << 20, 160, 441), (33554432, 160, 441)])
def test_plan_is_the_restatements(L, up, down):
    u, d, n_out, npr, Kp, tab = R.plan(L, up, down)
    p = RS.resample_plan(up, down, L)
    assert (p.up, p.down, p.n_out, p.n_pre_remove, p.Kp) == (u, d, n_out, npr, Kp)
    assert p.table.dtype == np.float32 and p.table.shape == (u, Kp) and p.table.flags.c_contiguous
    assert np.array_equal(p.table, tab.astype(np.float32))


@pytest.mark.parametrize("ntaps", TAPS)
def test_plan_with_caller_taps(ntaps):
    h = np.random.default_rng(ntaps).standard_normal(ntaps)
    for (up, down) in TAP_RATIOS:
        for L in (1, 9, 150):
            u, d, n_out, npr, Kp, tab = R.plan(L, up, down, h)
            for w in (h, list(h)):
                p = RS.resample_plan(up, down, L, w)
                assert (p.n_out, p.n_pre_remove, p.Kp) == (n_out, npr, Kp) and np.array_equal(p.table, tab.astype(np.float32))


def test_plan_reduces_caches_and_refuses():
    a, b = RS.resample_plan(48000, 44100, 300), RS.resample_plan(160, 147, 300)
    assert a is b and (a.up, a.down) == (160, 147)
    one = RS.resample_plan(4, 4, 17)
    assert (one.up, one.down, one.n_out, one.table) == (1, 1, 17, None)
    assert RS.ratio_of_rates(44100, 16000) == (160, 441) and RS.ratio_of_rates(16000.0, 48000) == (3, 1)
    for bad in ((0, 1), (1, 0), (1.5, 2), (-2, 3)):
        with pytest.raises(ValueError):
            RS.resample_plan(bad[0], bad[1], 10)
    with pytest.raises(ValueError):
        RS.resample_plan(2, 1, 0)
    for w in (np.zeros((2, 2)), np.zeros(0)):
        with pytest.raises(ValueError):
            RS.resample_plan(2, 1, 10, w)
