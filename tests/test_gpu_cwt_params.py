"""GPU tests of the continuous wavelet transform across what tests/test_gpu_cwt.py leaves alone: the three inner forms of
the direct kernel (tests/cwt_cases.py names the form every case reaches; tests/test_cwt_cases.py holds the table to it),
scale lists in any order and with repeats, strides over several tiles, strided and overlapping input rows, the smallest
filters, transform lengths without slack, pairing at its bound and the two chunking loops.

Reference and gate are those of tests/test_gpu_cwt.py: tests/cwt_ref.py in float64 on the float32 input,
|W_dev - W_ref64| <= 1e-5 A_s per clip and scale, A_s = ||h_s||_1 max|x|.  Every parity call writes into an `out=` filled
with NaN and must leave it finite: a cell the kernels never wrote fails.  Each group prints its worst ratio.

Worst ratios measured on MI355X: see README.md, "Continuous wavelet transform"."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from sygnals_amd import _cwt as CW
from tests import cwt_cases as K
from tests import cwt_ref as R
from tests.test_gpu_cwt import GATE, _np, _rows, _worst

FORMS = ("direct", "spectral")
OUTPUTS = ("coef", "magnitude", "power")


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    ops.require_gpu()
    return ops


@functools.lru_cache(maxsize=None)
def _case(name, scales, L, B=3, seed=0):
    """(x [B, L] float32, the float64 reference [B, S, L]): computed once, shared, never written to."""
    x = _rows(B, L, 7 * L + 13 * len(name) + seed)
    want = R.cwt_rows(x, scales, name)
    want.setflags(write=False)
    return x, want


def _cwt(ops, xd, scales, name, output="coef", stride=1, form=None):
    """ops.cwt into a result filled with NaN: every cell must have been written."""
    plan = CW.cwt_plan(scales, name)
    shape = ops.cwt_out_shape(xd.shape[0], plan.S, xd.shape[1], stride, plan.wavelet.complex, output)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=xd.device)
    assert ops.cwt(xd, scales, name, output, stride=stride, form=form, out=out) is out
    assert bool(torch.isfinite(out).all())
    return out


def _forms_agree(c, mag, powr, cplx):
    """|.| and |.|^2 within 2 ulp of the float64 value of the device's own coefficients (the rule and the floors of
    test_gpu_cwt.py::test_output_forms_strides_and_determinism)."""
    a = np.abs(_np(c, cplx))
    for got, ref, floor in ((mag, a, 1e-19), (powr, a * a, 1e-37)):
        g = got.cpu().numpy().astype(np.float64)
        assert g.shape == ref.shape
        assert np.all(np.abs(g - ref) <= 2 * np.spacing(ref.astype(np.float32)).astype(np.float64) + floor)


# ---------------------------------------------------------------------------- 1. the direct form's table
@pytest.mark.parametrize("c", K.direct_cases(), ids=K.case_id)
def test_direct_cases(ops, c):
    plan = CW.cwt_plan(c.scales, c.wavelet)
    cplx = plan.wavelet.complex
    x, want = _case(c.wavelet, tuple(c.scales), c.L, c.B)
    xd = ops.to_device_f32(x)
    got = {o: _cwt(ops, xd, c.scales, c.wavelet, o, c.stride, "direct") for o in OUTPUTS}
    assert got["coef"].shape[2] == -(-c.L // c.stride)
    worst = _worst(_np(got["coef"], cplx), want[:, :, ::c.stride], x, plan)
    _forms_agree(got["coef"], got["magnitude"], got["power"], cplx)
    if c.stride > 1:                                     # a strided call equals the columns it keeps, whatever form ran them
        for o in OUTPUTS:
            full = _cwt(ops, xd, c.scales, c.wavelet, o, 1, "direct")
            assert torch.equal(got[o], full[:, :, ::c.stride].contiguous())
    assert torch.equal(got["coef"], _cwt(ops, xd, c.scales, c.wavelet, "coef", c.stride, "direct"))     # the same bits
    for b in range(c.B):                                                                              # a batch equals its rows
        assert torch.equal(got["coef"][b:b + 1], _cwt(ops, xd[b:b + 1], c.scales, c.wavelet, "coef", c.stride, "direct"))
    print(f"cwt direct {c.name}: worst {worst:.2e} of A_s")


# ---------------------------------------------------------------------------- 2. scale order
@pytest.mark.parametrize("form", (None,) + FORMS)
@pytest.mark.parametrize("name", ("morl", K.CMOR))
def test_scale_order_and_repeats(ops, name, form):
    scales = np.asarray(K.MIXED_ORDER, dtype=np.float64)
    cplx = CW.parse_wavelet(name).complex
    x, want = _case(name, K.MIXED_ORDER, K.MIXED_L)
    xd = ops.to_device_f32(x)
    up = np.argsort(scales, kind="stable")
    direct_rows = set(int(i) for i in CW.split_forms(CW.cwt_plan(scales, name), ops.cwt_constants()["direct_taps_max"], form)[0])
    W = {}
    worst = 0.0
    for tag, perm in (("caller", np.arange(scales.size)), ("ascending", up), ("descending", up[::-1])):
        W[tag] = _cwt(ops, xd, scales[perm], name, form=form)
        worst = max(worst, _worst(_np(W[tag], cplx), want[:, perm], x, CW.cwt_plan(scales[perm], name)))
    # the filter of a scale does not depend on its place in the list, nor does the chain of fmaf of a direct row: the same
    # bits wherever the caller put it.  (A spectral row of a real wavelet is the real or the imaginary part of one inverse
    # transform, by which place it has in its pair: parity only.)
    for k, i in enumerate(up):
        if int(i) in direct_rows:
            assert torch.equal(W["caller"][:, i], W["ascending"][:, k])
            assert torch.equal(W["caller"][:, i], W["descending"][:, scales.size - 1 - k])
    a, b = (i for i in range(scales.size) if scales[i] == 2.0)
    if a in direct_rows:
        assert b in direct_rows and torch.equal(W["caller"][:, a], W["caller"][:, b])
    print(f"cwt {name} form={form}, ten scales in three orders, one twice: worst {worst:.2e} of A_s")


# ---------------------------------------------------------------------------- 3. spectral lengths
@pytest.mark.parametrize("name", ("morl", K.CMOR))
@pytest.mark.parametrize("c", K.SPECTRAL_CASES, ids=lambda c: c.name)
def test_spectral_lengths(ops, c, name):
    scales = K.spectral_scales(c)
    plan = CW.cwt_plan(scales, name)
    assert ops.cwt_fft_len(c.L, int(plan.taps.max())) == c.M and ops.fft_plan(c.M) == c.plan
    x, want = _case(name, scales, c.L, c.B)
    got = _np(_cwt(ops, ops.to_device_f32(x), scales, name, form="spectral"), plan.wavelet.complex)
    worst = _worst(got, want, x, plan)
    # the last taps - 1 columns of the row of the longest filter: where a transform one point too short would wrap into
    tail = slice(max(0, c.L - (c.taps - 1)), c.L)
    A = plan.l1[None, :] * np.max(np.abs(x.astype(np.float64)), axis=1)[:, None]
    end = float(np.max(np.max(np.abs(got - want)[:, :, tail], axis=2) / A))
    print(f"cwt {name} spectral {c.name} (M = {c.M}): worst {worst:.2e} of A_s, over the last {c.taps - 1} columns {end:.2e}")


# ---------------------------------------------------------------------------- 4. pairing at its bound
def test_pairing_at_the_bound(ops):
    s, L = float(K.PAIR_S), K.PAIR_L
    both = (s, CW.PAIR_RATIO * s)
    plan = CW.cwt_plan(both, "morl")
    assert CW.spectral_rows(plan, [0, 1]) == [(0, 1)]
    # a tone at the large scale's centre frequency: its row is large where the small scale's is nearly null, and the small
    # scale is still held to its own A_s
    rng = np.random.default_rng(80)
    n = np.arange(L)[None, :]
    x = (np.cos(2 * np.pi * (0.8125 / both[1]) * n + rng.uniform(0, 6, size=(3, 1))) + 0.01 * rng.standard_normal((3, L))).astype(np.float32)
    want = R.cwt_rows(x, both, "morl")
    assert np.abs(want[:, 1]).max() > 10 * np.abs(want[:, 0]).max()
    xd = ops.to_device_f32(x)
    worst = _worst(_np(_cwt(ops, xd, both, "morl", form="spectral"), False), want, x, plan)
    worst = max(worst, _worst(_np(_cwt(ops, xd, both[::-1], "morl", form="spectral"), False), want[:, ::-1], x,
                              CW.cwt_plan(both[::-1], "morl")))
    alone = 0.0
    for i in (0, 1):
        alone = max(alone, _worst(_np(_cwt(ops, xd, both[i:i + 1], "morl", form="spectral"), False), want[:, i:i + 1], x,
                                  CW.cwt_plan(both[i:i + 1], "morl")))
    print(f"cwt morl spectral, scales {both} in one filter row: worst {worst:.2e} of A_s, each alone {alone:.2e}")


# ---------------------------------------------------------------------------- 5. row layout and the zero rule
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ("morl", K.CMOR))
def test_strided_rows_among_nan(ops, name, form):
    L, scales = K.LAYOUT_L, K.LAYOUT_SCALES
    plan = CW.cwt_plan(scales, name)
    cplx = plan.wavelet.complex
    assert int(plan.taps.max()) > 2 * L                                  # the longest filter reaches past both ends of the row
    x = np.array(_case(name, scales, L)[0])
    x[1] = 0.0
    x[2] = 0.75
    want = R.cwt_rows(x, scales, name)
    # rows L + 40 apart that start 7 floats into the buffer, every other float of it NaN (a fourth row behind them): a read
    # outside [0, L) that the zero rule did not replace shows
    buf = torch.full((4, L + 40), float("nan"), dtype=torch.float32, device=ops.require_gpu())
    view = buf[:3, 7:7 + L]
    view.copy_(ops.to_device_f32(x))
    assert view.stride(0) == L + 40 and view.data_ptr() % 16 != 0 and not view.is_contiguous()
    dense = view.contiguous()
    worst = 0.0
    for stride in (1, 5):
        got = {o: _cwt(ops, view, scales, name, o, stride, form) for o in OUTPUTS}
        for o in OUTPUTS:
            assert torch.equal(got[o], _cwt(ops, dense, scales, name, o, stride, form))
            assert not bool(got[o][1].any())                             # the all-zero row: exactly zero in every form
        c = _np(got["coef"], cplx)
        keep = [0, 2]
        worst = max(worst, _worst(c[keep], want[keep][:, :, ::stride], x[keep], plan))
        _forms_agree(got["coef"], got["magnitude"], got["power"], cplx)
        if stride == 1:                                                  # the constant row: sum h = 0 away from the ends
            A = plan.l1 * 0.75
            for i in range(plan.S):
                t = int(plan.taps[i])
                if 2 * t < L:
                    assert np.abs(c[2, i, t:L - t]).max() <= GATE * A[i]
    assert bool(torch.isnan(buf[:, :7]).all()) and bool(torch.isnan(buf[:, 7 + L:]).all()) and bool(torch.isnan(buf[3]).all())
    print(f"cwt {name} form={form}, rows of {L} in a buffer of NaN, strides 1 and 5: worst {worst:.2e} of A_s")


# ---------------------------------------------------------------------------- 6. rows that overlap
@pytest.mark.parametrize("name", ("morl", K.CMOR))
def test_rows_closer_than_their_length(ops, name):
    L, scales = K.LAYOUT_L, K.LAYOUT_SCALES
    xd = ops.to_device_f32(_rows(1, L + 200, 21))
    views = (xd[:, :L].expand(3, L), xd[0].unfold(0, L, 100))
    assert [tuple(v.shape) for v in views] == [(3, L)] * 2 and [v.stride(0) for v in views] == [0, 100]
    for v in views:
        for form in (None,) + FORMS:
            for stride in (1, 5):
                assert torch.equal(_cwt(ops, v, scales, name, stride=stride, form=form),
                                   _cwt(ops, v.contiguous(), scales, name, stride=stride, form=form))


# ---------------------------------------------------------------------------- 7. the two chunking loops
@pytest.mark.parametrize("name", ("morl", K.CMOR))
def test_clip_blocks_of_the_spectral_form(ops, name, monkeypatch):
    L, B, scales = 700, 5, (40, 100, 300)
    plan = CW.cwt_plan(scales, name)
    x, want = _case(name, scales, L, B)
    xd = ops.to_device_f32(x)
    whole = _cwt(ops, xd, scales, name, form="spectral")
    R_ = len(CW.spectral_rows(plan, range(3)))
    per_clip = ops.lib().syg_cwt_work_bytes(1, R_, ops.cwt_fft_len(L, int(plan.taps.max())))
    assert per_clip > 0 and ops.CWT_WORK_BYTES // per_clip >= B                  # one block as it stands
    monkeypatch.setattr(ops, "CWT_WORK_BYTES", 2 * per_clip + per_clip // 2)     # blocks of 2, 2 and 1 clips
    assert torch.equal(_cwt(ops, xd, scales, name, form="spectral"), whole)
    print(f"cwt {name} spectral in clip blocks of two: worst {_worst(_np(whole, plan.wavelet.complex), want, x, plan):.2e} of A_s")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ("morl", K.CMOR))
def test_more_clips_than_a_launch_takes(ops, name, form):
    B, L = 65537, 4
    scales = (K.first_scale(name, 3),)
    plan = CW.cwt_plan(scales, name)
    assert int(plan.taps[0]) == 3
    x7, want = _case(name, scales, L, 7)
    xd = ops.to_device_f32(x7)[torch.arange(B, device=ops.require_gpu()) % 7]
    got = _cwt(ops, xd, scales, name, form=form)
    assert got.shape[0] == B and torch.equal(got, got[:7][torch.arange(B, device=got.device) % 7])
    print(f"cwt {name} form={form}, {B} clips of {L} samples under 3 taps: worst "
          f"{_worst(_np(got[:7], plan.wavelet.complex), want, x7, plan):.2e} of A_s")


# ---------------------------------------------------------------------------- 8. other cmor parameters
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", K.OTHER_CMOR)
def test_other_cmor_parameters(ops, name, form):
    plan = CW.cwt_plan(K.OTHER_CMOR_SCALES, name)
    x, want = _case(name, K.OTHER_CMOR_SCALES, K.OTHER_CMOR_L)
    got = _cwt(ops, ops.to_device_f32(x), K.OTHER_CMOR_SCALES, name, form=form)
    print(f"cwt {name} form={form}: worst {_worst(_np(got, True), want, x, plan):.2e} of A_s")
