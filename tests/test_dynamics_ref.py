"""The float64 restatement of the feature dynamics (tests/dynamics_ref.py) against SciPy, its own definitions and, where
it imports, librosa; the host tables of sygnals_amd/_dynamics.py against the restatement's.  No device."""
import numpy as np
import pytest
from scipy.signal import savgol_filter

from sygnals_amd import _dynamics as DY
from tests import dynamics_cases as DC
from tests import dynamics_ref as R


def scipy_delta(x, width, order, mode, cval=0.0):
    return savgol_filter(x, width, deriv=order, polyorder=order, axis=-1, mode=mode, cval=cval)


def close_to_scipy(x, width, order, mode, cval=0.0):
    got = R.delta(x, width, order, mode, cval)
    want = scipy_delta(x.astype(np.float64), width, order, mode, cval)
    peak = max(float(np.max(np.abs(x))), abs(cval) if mode == "constant" else 0.0)
    err = float(np.max(np.abs(got - want)))                         # zeros compare by value: SciPy returns -0.0
    assert err <= 1e-12 * R.norm1(width, order) * peak, (width, order, mode, x.shape, err)
    return err / (R.norm1(width, order) * peak)


@pytest.mark.parametrize("width,order", DC.DELTA_WO)
def test_restatement_equals_savgol_filter_interp(width, order):
    worst = 0.0
    for i, T in enumerate(DC.delta_T(width)):
        B, K = DC.bk_for(i + width + order, T)
        worst = max(worst, close_to_scipy(DC.delta_input(B, K, T, seed=1000 * width + 10 * order + i), width, order, "interp"))
    print(f"width={width} order={order}: {worst:.2e} of ||c||_1 max|x|")


@pytest.mark.parametrize("mode", DC.EDGE_MODES)
def test_restatement_equals_savgol_filter_edge_modes(mode):
    for width, order in ((9, 1), (9, 2), (5, 2), (31, 1)):
        for i, T in enumerate(sorted(set(DC.mode_T(width) + [1, 2, 3, 4, 5, DC.TILE + 1]))):
            B, K = DC.bk_for(i, T)
            close_to_scipy(DC.delta_input(B, K, T, seed=77 + i), width, order, mode, DC.CVAL)


def test_interp_refuses_short_rows_in_scipys_words():
    with pytest.raises(ValueError, match="window_length must be less than or equal to the size of x"):
        R.delta(np.zeros((1, 8)), 9, 1)
    with pytest.raises(ValueError, match="window_length must be less than or equal to the size of x"):
        DY.check_interp(9, 8, "interp")
    DY.check_interp(9, 9, "interp")
    DY.check_interp(9, 1, "nearest")


@pytest.mark.parametrize("width", [3, 5, 9, 31, 101, 255])
def test_host_tables(width):
    for order in range(1, min(4, width - 1) + 1):
        c, E = R.tables(width, order)
        c32, E32 = DY.delta_tables(width, order)
        assert c32.dtype == E32.dtype == np.float32
        assert np.array_equal(c32.view(np.uint32), c.astype(np.float32).view(np.uint32))
        assert np.array_equal(E32.view(np.uint32), E.astype(np.float32).view(np.uint32))
        assert DY.delta_tables(width, order)[0] is c32                            # cached per (width, order)
        h = width // 2
        tab = DY.pack_table(width, order)
        assert tab.shape == (width * width,) and tab.dtype == np.float32
        assert np.array_equal(tab[:width], c32[::-1])
        assert np.array_equal(tab[width:width + h * width].reshape(h, width), E32[:, :h].T)
        assert np.array_equal(tab[width + h * width:].reshape(h, width), E32[:, width - h:].T)


def test_argument_rules():
    for w in (2, 4, 1, 0, -3, 257, 9.0, True):
        with pytest.raises(ValueError, match="width must be an odd integer"):
            DY.check_width_order(w, 1)
    for w, o in ((9, 0), (9, 5), (3, 3), (5, -1)):
        with pytest.raises(ValueError, match="order must be an integer in"):
            DY.check_width_order(w, o)
    assert DY.check_width_order(3, 2) == (3, 2) and DY.check_width_order(255, 4) == (255, 4)
    with pytest.raises(ValueError, match="unknown mode 'reflect'"):
        DY.check_mode("reflect")
    for W in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="window must be None"):
            DY.check_window(W)
    assert DY.check_window(None) == 0 and DY.check_window(600) == 600
    for n, d in ((0, 1), (2, 0), (2.0, 1), (2, 1.5)):
        with pytest.raises(ValueError):
            DY.check_stack(n, d)
    with pytest.raises(ValueError, match="above 2\\^31"):
        DY.check_size("delta", 1 << 11, 1 << 10, (1 << 10) + 1)
    with pytest.raises(ValueError, match="empty input"):
        DY.check_size("delta", 1, 0, 5)


def test_edge_columns_are_no_heavier_than_the_interior():
    """||E[:, t]||_1 <= ||c||_1 (1 + 1e-12) for every table the device tests use: one scale, ||c||_1 max|x|, serves the whole
    row.  With deriv = polyorder the fitted derivative is a constant, so the two are equal but for the rounding of SciPy's
    least-squares fit.  That rounding alone passes 1e-12 at some larger tables no test uses (1.2e-12 at width 43 order 4,
    6.8e-11 at width 89 order 4, with SciPy 1.15): the survey over all odd widths 3 ... 101 and 255 is printed, not
    asserted; against a gate of 1e-5 of the same scale such an excess is nothing."""
    def excess(width, order):
        c, E = R.tables(width, order)
        return float(np.max(np.sum(np.abs(E), axis=0)) / np.sum(np.abs(c))) - 1
    used = sorted(set(DC.DELTA_WO) | {(9, 1), (9, 2), (5, 2), (31, 1), (5, 1), (31, 2)})
    for width, order in used:
        assert excess(width, order) <= 1e-12, (width, order)
    survey = {(w, o): excess(w, o) for w in list(range(3, 102, 2)) + [255] for o in range(1, min(4, w - 1) + 1)}
    at = max(survey, key=survey.get)
    print(f"tables in use: within 1e-12; widths 3 ... 101 and 255: worst excess {survey[at]:.2e} at (width, order) = {at}")


# ---------------------------------------------------------------- cmvn
@pytest.mark.parametrize("T", DC.CMVN_T)
def test_cmvn_loop_equals_prefix_form(T):
    B, K = (3, 13) if T <= 601 else (2, 4)
    x = DC.cmvn_input(B, K, T, seed=T)
    assert DC.cmvn_input_ok(x)
    worst = 0.0
    for W in DC.cmvn_windows(T):
        for variance in (True, False):
            a, b = R.cmvn_loop(x, W, variance), R.cmvn_prefix(x, W, variance)
            peak = max(1.0, float(np.max(np.abs(a))))
            worst = max(worst, float(np.max(np.abs(a - b))) / peak)
            assert np.max(np.abs(a - b)) <= 1e-9 * peak, (T, W, variance)
            if W is not None and W >= T:
                assert np.array_equal(a, R.cmvn_loop(x, None, variance))         # W >= T is the global form
    print(f"T={T}: loop against prefix sums {worst:.2e} of the peak")


def test_cmvn_long_c0_row_prefix_form():
    rng = np.random.default_rng(1)
    x = (-400.0 + 50.0 * rng.standard_normal((1, 100000))).astype(np.float32)
    T = x.shape[-1]
    y = R.cmvn_prefix(x, 600)
    for t in (0, 1, 299, 300, 301, 50000, T - 301, T - 300, T - 1):
        s, e = R.window_of(t, 600, T)
        seg = x[0, s:e].astype(np.float64)
        want = (x[0, t] - seg.mean()) / np.sqrt(max(np.mean((seg - seg.mean()) ** 2), R.VAR_FLOOR))
        assert abs(y[0, t] - want) <= 1e-9 * np.max(np.abs(y))


def test_cmvn_windows_and_exact_cases():
    assert R.window_of(0, 600, 1000) == (0, 600) and R.window_of(999, 600, 1000) == (400, 1000)
    assert R.window_of(500, 600, 1000) == (200, 800) and R.window_of(3, 601, 10) == (0, 10)
    assert R.window_of(5, 3, 10) == (4, 7) and R.window_of(5, 2, 10) == (4, 6) and R.window_of(0, 1, 1) == (0, 1)
    for T, W in ((10, 3), (10, 2), (1000, 600), (1000, 601), (5, 9), (1, 1)):
        s, e = R.windows(T, W)
        assert [tuple(v) for v in zip(s, e)] == [R.window_of(t, W, T) for t in range(T)]
    const = np.full((2, 50), np.float32(-412.3371))
    for W in (None, 1, 7, 50):
        for f in (R.cmvn_loop, R.cmvn_prefix):
            assert np.all(f(const, W) == 0.0) and np.all(f(const, W, False) == 0.0)
    one = np.array([[3.25]], dtype=np.float32)
    assert np.all(R.cmvn_loop(one) == 0.0) and np.all(R.cmvn_loop(one, 1) == 0.0)
    x = DC.cmvn_input(1, 3, 40, seed=2)
    assert np.all(R.cmvn_loop(x, 1) == 0.0) and np.all(R.cmvn_prefix(x, 1) == 0.0)


# ---------------------------------------------------------------- stack_memory
@pytest.mark.parametrize("T", [1, 65])
def test_stack_memory_formula_equals_pad_and_slice(T):
    x = DC.delta_input(3, 13, T, seed=T)
    for n_steps, delay in DC.STACK:
        d = T + 1 if delay == "T+1" else delay
        got = R.stack_memory(x, n_steps, d)
        pad = (n_steps - 1) * abs(d)
        blocks = []
        for i in range(n_steps):
            if d > 0:
                p = np.pad(x, [(0, 0), (0, 0), (pad, 0)])
                blocks.append(p[:, :, pad - i * d: pad - i * d + T])
            else:
                p = np.pad(x, [(0, 0), (0, 0), (0, pad)])
                blocks.append(p[:, :, -i * d: -i * d + T])
        assert np.array_equal(got, np.concatenate(blocks, axis=1)), (n_steps, d)
        for b, i, k, t in ((0, n_steps - 1, 12, T - 1), (2, 0, 0, 0)):
            src = t - i * d
            assert got[b, i * 13 + k, t] == (x[b, k, src] if 0 <= src < T else 0.0)


# ---------------------------------------------------------------- librosa, where it imports
def test_against_librosa():
    librosa = pytest.importorskip("librosa")
    x = DC.delta_input(1, 13, 65, seed=4)[0]
    for order in (1, 2):
        assert np.allclose(R.delta(x, 9, order), librosa.feature.delta(x.astype(np.float64), width=9, order=order), atol=1e-10)
    for n_steps, d in ((2, 1), (5, 3), (2, -1)):
        assert np.array_equal(R.stack_memory(x, n_steps, d), librosa.feature.stack_memory(x, n_steps=n_steps, delay=d))
