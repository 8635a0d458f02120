"""Device deltas, CMVN, context stacking and their fusion (syg_dynamics_f32, syg_stack_memory_f32; ops.delta / cmvn /
stack_memory / feature_post, mfcc_deltas_batch) against SciPy and the float64 restatement of tests/dynamics_ref.py.

Gates: delta |y - savgol_filter in float64| <= 1e-5 ||c||_1 max|x_row|; cmvn 1e-5 max(1, max|y_ref|) per row with the
variance and 1e-5 max|x_row| without; everything else bit for bit.  Every call writes into an `out` filled with NaN, and
every test prints its worst fraction of the gate."""
import numpy as np
import pytest
import torch
from scipy.signal import savgol_filter

from sygnals_amd import ops
from tests import dynamics_cases as DC
from tests import dynamics_ref as R

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cpu(t):
    return t.cpu().numpy()


def nan_out(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def forms_for(T, sliding=False):
    """The forms a row of T frames fits: tiled always, resident while its LDS does."""
    k = ops.dynamics_constants()
    fits = (20 * T + 16 if sliding else 4 * T) <= k["lds_max"]
    return ("resident", "tiled") if fits else ("tiled",)


def delta_fraction(got, x, width, order, mode="interp", cval=0.0):
    want = savgol_filter(x.astype(np.float64), width, deriv=order, polyorder=order, axis=-1, mode=mode, cval=cval)
    assert np.isfinite(got).all()
    peak = np.max(np.abs(x.astype(np.float64)), axis=-1, keepdims=True)
    if mode == "constant":
        peak = np.maximum(peak, abs(cval))
    bound = 1e-5 * R.norm1(width, order) * peak
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), f"worst {float(np.max(err / np.maximum(bound, 1e-300))):.3e} of the gate"
    return float(np.max(err / np.maximum(bound, 1e-300)))


def test_constants_are_the_cases():
    k = ops.dynamics_constants()
    assert k["tile"] == DC.TILE and k["resident_max_t"] == DC.RESIDENT_T and k["resident_max_t_sliding"] == DC.RESIDENT_T_SLIDING
    assert k["direct_window"] == DC.DIRECT_WINDOW == R.DIRECT_WINDOW and k["width_max"] == 255 and k["order_max"] == 4
    assert ops.dynamics_form(DC.RESIDENT_T) == "resident" and ops.dynamics_form(DC.RESIDENT_T + 1) == "tiled"
    assert ops.dynamics_form(DC.RESIDENT_T_SLIDING + 1, 600) == "tiled" and ops.dynamics_form(600, 600) == "resident"


# ---------------------------------------------------------------- delta
@pytest.mark.parametrize("width,order", DC.DELTA_WO)
def test_delta_against_scipy_both_forms(width, order):
    worst = 0.0
    for i, T in enumerate(DC.delta_T(width)):
        B, K = DC.bk_for(i + width + order, T)
        x = DC.delta_input(B, K, T, seed=1000 * width + 10 * order + i)
        xd = dev(x)
        outs = []
        for form in (None,) + forms_for(T):
            got = cpu(ops.delta(xd, width, order, out=nan_out(B, K, T), form=form))
            worst = max(worst, delta_fraction(got, x, width, order))
            outs.append(got)
        assert all(bits_equal(outs[0], o) for o in outs[1:]), f"forms differ at T={T}"
        if B > 1:                                      # a batch equals its rows
            one = cpu(ops.delta(xd[B - 1:, K - 1:], width, order))
            assert bits_equal(one, outs[0][B - 1:, K - 1:])
    print(f"delta width={width} order={order}: worst fraction of the gate {worst:.3e}")


@pytest.mark.parametrize("mode", DC.EDGE_MODES)
def test_delta_edge_modes(mode):
    worst = 0.0
    for width, order in ((9, 1), (9, 2), (5, 2), (31, 1)):
        for i, T in enumerate(DC.mode_T(width) + [DC.TILE + 1]):
            B, K = DC.bk_for(i, T)
            x = DC.delta_input(B, K, T, seed=77 + i)
            outs = []
            for form in forms_for(T):
                got = cpu(ops.delta(dev(x), width, order, mode=mode, cval=DC.CVAL, out=nan_out(B, K, T), form=form))
                worst = max(worst, delta_fraction(got, x, width, order, mode, DC.CVAL))
                outs.append(got)
            assert bits_equal(outs[0], outs[-1])
    print(f"delta mode={mode}: worst fraction of the gate {worst:.3e}")


def test_delta_strided_rows_equal_contiguous():
    B, K, T = 3, 13, 94
    x = DC.delta_input(B, K + 1, T + 7, seed=5)
    buf = nan_out(B, K + 1, T + 7)
    buf[:, 1:, :T] = dev(x)[:, 1:, :T]
    view = buf[:, 1:, :T]
    assert not view.is_contiguous()
    for form in ("resident", "tiled"):
        a = cpu(ops.delta(view, 9, 1, out=nan_out(B, K, T), form=form))
        b = cpu(ops.delta(view.contiguous(), 9, 1, out=nan_out(B, K, T), form=form))
        assert np.isfinite(a).all() and bits_equal(a, b)
    big = nan_out(B, 2 * K, T + 3)                       # a strided out
    ops.delta(view, 9, 2, out=big[:, K:, :T])
    assert bits_equal(cpu(big[:, K:, :T]), cpu(ops.delta(view, 9, 2)))
    assert torch.isnan(big[:, :K]).all() and torch.isnan(big[:, :, T:]).all()
    print("delta strided: 0 of the gate (bit for bit)")


@pytest.mark.parametrize("width,order", [(9, 1), (9, 2), (5, 1), (31, 2)])
def test_delta_impulses_give_the_tables(width, order):
    c, E = ops.delta_tables(width, order)
    h = width // 2
    T = 2 * width + 5
    pos = list(range(width)) + list(range(T - width, T))
    x = np.zeros((1, len(pos) + 1, T), dtype=np.float32)           # the last row stays all zero
    for r, p in enumerate(pos):
        x[0, r, p] = 1.0
    want = np.zeros_like(x)
    w = c[::-1]
    for r, p in enumerate(pos):
        for t in range(T):
            if t < h:
                want[0, r, t] = E[p, t] if p < width else 0.0
            elif t >= T - h:
                want[0, r, t] = E[p - (T - width), width - (T - t)] if p >= T - width else 0.0
            else:
                j = p - t + h
                want[0, r, t] = w[j] if 0 <= j < width else 0.0
    for form in ("resident", "tiled"):
        got = cpu(ops.delta(dev(x), width, order, out=nan_out(*x.shape), form=form))
        assert np.array_equal(got, want)                             # by value: -0.0 equals 0.0
        assert np.all(got[0, -1] == 0.0)
    print("delta impulses: 0 of the gate (the float32 tables' entries)")


def test_delta_long_row():
    T = 1 << 20
    x = DC.delta_input(1, 1, T, seed=9)
    got = cpu(ops.delta(dev(x), 9, 1, out=nan_out(1, 1, T)))
    f1 = delta_fraction(got, x, 9, 1)
    got2 = cpu(ops.delta(dev(x), 9, 2, out=nan_out(1, 1, T)))
    print(f"delta 2^20 frames: worst fraction of the gate {max(f1, delta_fraction(got2, x, 9, 2)):.3e}")


# ---------------------------------------------------------------- cmvn
def cmvn_fraction(got, x, W, variance):
    want = R.cmvn_prefix(x, W, variance)
    assert np.isfinite(got).all()
    if variance:
        bound = 1e-5 * np.maximum(1.0, np.max(np.abs(want), axis=-1, keepdims=True))
    else:
        bound = 1e-5 * np.max(np.abs(x.astype(np.float64)), axis=-1, keepdims=True)
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), f"worst {float(np.max(err / bound)):.3e} of the gate (W={W}, variance={variance})"
    return float(np.max(err / bound))


def ulp_distance(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.max(np.abs(ia - ib)))


@pytest.mark.parametrize("T", DC.CMVN_T)
def test_cmvn_against_restatement(T):
    B, K = (3, 13) if T <= 601 else (2, 4)
    x = DC.cmvn_input(B, K, T, seed=T)
    assert DC.cmvn_input_ok(x)
    xd = dev(x)
    worst, worst_ulp = 0.0, 0
    for W in DC.cmvn_windows(T):
        sliding = W is not None and W < T
        for variance in (True, False):
            outs = []
            for form in forms_for(T, sliding):
                got = cpu(ops.cmvn(xd, W, variance, out=nan_out(B, K, T), form=form))
                if T == 1 or W == 1:
                    assert np.all(got == 0.0)                        # the exact cases, by value
                else:
                    worst = max(worst, cmvn_fraction(got, x, W, variance))
                outs.append(got)
            d = ulp_distance(outs[0], outs[-1])
            worst_ulp = max(worst_ulp, d)
            assert d <= 2, f"forms differ by {d} ulp (T={T}, W={W})"
            if not sliding:
                assert bits_equal(outs[0], outs[-1])                 # the global sums are cut by frame index alone
            auto = ops.cmvn(xd, W, variance)
            inplace = xd.clone()
            assert ops.cmvn(inplace, W, variance, out=inplace) is inplace
            assert bits_equal(cpu(auto), cpu(inplace))
    print(f"cmvn T={T}: worst fraction of the gate {worst:.3e}; forms within {worst_ulp} ulp")


def test_cmvn_exact_cases_and_batch_rows():
    x = np.full((2, 3, 700), np.float32(-412.3371), dtype=np.float32)
    x[1] = np.float32(0.1)
    for W in (None, 1, 31, 300, 699, 700):
        for form in forms_for(700, W is not None and W < 700):
            for variance in (True, False):
                assert np.all(cpu(ops.cmvn(dev(x), W, variance, out=nan_out(2, 3, 700), form=form)) == 0.0)
    y = DC.cmvn_input(5, 13, 1201, seed=3)
    yd = dev(y)
    for W in (None, 300):
        full = cpu(ops.cmvn(yd, W))
        assert bits_equal(cpu(ops.cmvn(yd[4:, 12:], W)), full[4:, 12:])
        assert bits_equal(cpu(ops.cmvn(yd[:, 1::2], W)), full[:, 1::2])   # rows strided over K
    print("cmvn exact cases: 0 by value")


def test_cmvn_long_row():
    T = 1 << 20
    x = DC.cmvn_input(1, 2, T, seed=11)
    assert DC.cmvn_input_ok(x)
    xd = dev(x)
    f = [cmvn_fraction(cpu(ops.cmvn(xd, W, True, out=nan_out(1, 2, T))), x, W, True) for W in (600, None)]
    inplace = xd.clone()
    ops.cmvn(inplace, 600, out=inplace)
    assert bits_equal(cpu(inplace), cpu(ops.cmvn(xd, 600)))
    print(f"cmvn 2^20 frames: worst fraction of the gate {max(f):.3e}")


# ---------------------------------------------------------------- feature_post
@pytest.mark.parametrize("shape", DC.POST_SHAPES)
def test_feature_post_is_the_composition(shape):
    B, K, T = shape
    x = DC.cmvn_input(B, K, T, seed=T + K)
    xd = dev(x)
    worst = 0.0
    for cm in (None, "global", 300):
        sliding = cm == 300 and T > 300
        W = None if cm == "global" else cm
        for form in (None,) + forms_for(T, sliding):
            s = ops.cmvn(xd, W, form=form) if cm is not None else xd
            for deltas in (0, 1, 2):
                want = torch.cat([s] + [ops.delta(s, 9, d, form=form) for d in range(1, deltas + 1)], dim=1)
                got = ops.feature_post(xd, cmvn=cm, deltas=deltas, out=nan_out(B, (deltas + 1) * K, T), form=form)
                assert bits_equal(cpu(got), cpu(want)), f"cmvn={cm} deltas={deltas} form={form}"
        ref = R.feature_post(x, cm, True, 2)
        got = cpu(ops.feature_post(xd, cmvn=cm, deltas=2)).astype(np.float64)
        scale = np.maximum(1.0, np.max(np.abs(ref), axis=-1, keepdims=True))
        worst = max(worst, float(np.max(np.abs(got - ref) / (1e-5 * R.norm1(9, 1) * scale))))
    for mode in DC.EDGE_MODES:                            # wrap over several tiles goes through the statics
        s = ops.cmvn(xd)
        want = torch.cat([s, ops.delta(s, 9, 1, mode=mode), ops.delta(s, 9, 2, mode=mode)], dim=1)
        for form in forms_for(T):
            got = ops.feature_post(xd, cmvn="global", deltas=2, mode=mode, out=nan_out(B, 3 * K, T), form=form)
            assert bits_equal(cpu(got), cpu(want)), mode
    assert worst <= 1.0
    print(f"feature_post {shape}: the composition bit for bit; {worst:.3e} of the delta gate from the float64 restatement")


# ---------------------------------------------------------------- stack_memory
@pytest.mark.parametrize("T", [1, 65])
def test_stack_memory_bit_for_bit(T):
    x = DC.delta_input(3, 13, T + 4, seed=T)[:, :, :T]
    buf = nan_out(3, 14, T + 4)
    buf[:, 1:, :T] = dev(x)
    for n_steps, delay in DC.STACK:
        d = T + 1 if delay == "T+1" else delay
        want = R.stack_memory(x, n_steps, d)
        got = cpu(ops.stack_memory(buf[:, 1:, :T], n_steps, d, out=nan_out(3, n_steps * 13, T)))
        assert bits_equal(got, want), (n_steps, d)
    print("stack_memory: bit for bit")


# ---------------------------------------------------------------- mfcc_deltas_batch
def test_mfcc_deltas_batch():
    from oracle import cpu_ref as O
    from sygnals_amd.core.features.cepstral import mfcc_deltas_batch
    sr = 22050
    y = ops.to_device_f32(O.synth_clips(3, 32768, sr, seed=3))
    base = cpu(ops.mfcc_batch(y, sr, n_mfcc=13))
    got = cpu(mfcc_deltas_batch(y, sr, n_mfcc=13, deltas=2, width=9))
    K, T = base.shape[1:]
    assert got.shape == (3, 3 * K, T) and bits_equal(got[:, :K], base)
    f = max(delta_fraction(got[:, d * K:(d + 1) * K], base, 9, d) for d in (1, 2))
    norm = cpu(mfcc_deltas_batch(y, sr, n_mfcc=13, deltas=1, cmvn="global"))
    assert np.all(np.abs(norm[:, :K].mean(axis=-1)) < 1e-4) and np.allclose(norm[:, :K].std(axis=-1), 1.0, atol=1e-4)
    print(f"mfcc_deltas_batch: statics are mfcc_batch's bits; deltas {f:.3e} of the gate")
