"""GPU tests of the continuous wavelet transform (csrc/cwt.hip, ops.cwt) against tests/cwt_ref.py run in float64 on the
float32 input.  Gate: |W_dev - W_ref64| <= 1e-5 A_s per clip and scale, A_s = ||h_s||_1 max|x| (a scale far from the
signal's band is a null: a gate on the output's own peak would be wrong there).  Each group prints its worst ratio.

Worst ratios measured on MI355X (fraction of A_s, gate 1e-5): see README.md, "Continuous wavelet transform"."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from sygnals_amd import _cwt as CW
from tests import cwt_ref as R

GATE = 1e-5
WAVELETS = ("morl", "mexh", "gaus1", "cmor1.5-1.0")
SCALES = (1, 1.5, 2, 7.3, 32, 64.5, 512)
FORMS = ("direct", "spectral")


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    ops.require_gpu()
    return ops


def _rows(B, L, seed):
    """Tone plus noise, a different tone per row."""
    rng = np.random.default_rng(seed)
    n = np.arange(L)[None, :]
    f = rng.uniform(0.002, 0.2, size=(B, 1))
    return (np.cos(2 * np.pi * f * n + rng.uniform(0, 6, size=(B, 1))) + 0.5 * rng.standard_normal((B, L))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name, L, scales=SCALES, B=33):
    """(x [B, L] float32, the float64 reference [B, S, L]): computed once, shared by the forms, never written to."""
    x = _rows(B, L, 11 * L + len(name))
    want = R.cwt_rows(x, scales, name)
    want.setflags(write=False)
    return x, want


def _np(t, cplx):
    a = t.cpu().numpy()
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64) if cplx else a.astype(np.float64)


def _worst(got, want, x, plan):
    """Worst ratio of the error to A_s over clips and scales; asserts the gate on every one of them."""
    assert got.shape == want.shape and np.isfinite(got).all()
    A = plan.l1[None, :] * np.max(np.abs(x.astype(np.float64)), axis=1)[:, None]
    err = np.max(np.abs(got - want), axis=2)
    ratio = float(np.max(err / A))
    assert np.all(err <= GATE * A), ratio
    return ratio


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", WAVELETS)
def test_wavelets_forms_lengths_batches(ops, name, form):
    tile = ops.cwt_constants()["tile"]
    plan = CW.cwt_plan(SCALES, name)
    cplx = plan.wavelet.complex
    worst = 0.0
    for L in (1, 2, 17, tile - 1, tile, tile + 1, 4097):
        x, want = _case(name, L)
        xd = ops.to_device_f32(x)
        for B in (1, 3, 33):
            got = ops.cwt(xd[:B], SCALES, name, form=form)
            assert tuple(got.shape) == ((B, len(SCALES), L, 2) if cplx else (B, len(SCALES), L)) and got.dtype == torch.float32
            worst = max(worst, _worst(_np(got, cplx), want[:B], x[:B], plan))
    print(f"cwt {name} form={form}: worst {worst:.2e} of A_s")


@pytest.mark.parametrize("name", ("morl", "gaus1", "cmor1.5-1.0"))
def test_automatic_form_straddles_the_threshold(ops, name):
    mx = ops.cwt_constants()["direct_taps_max"]
    support = 10.0 if name == "gaus1" else 16.0
    # taps = s (hi - lo) + 2: tap counts max - 1, max and max + 1, then two more spectral scales: three in all, so the two
    # smallest pair (within a factor 4) and the largest runs alone
    scales = tuple((T - 2) / support for T in (mx - 1, mx, mx + 1)) + (2.5 * mx / support, 3.0 * mx / support)
    plan = CW.cwt_plan(scales, name)
    assert list(plan.taps[:3]) == [mx - 1, mx, mx + 1]
    direct, spec = CW.split_forms(plan, mx, None)
    assert list(direct) == [0, 1] and list(spec) == [2, 3, 4]
    rows = CW.spectral_rows(plan, spec)
    assert rows == ([(2, -1), (3, -1), (4, -1)] if plan.wavelet.complex else [(2, 3), (4, -1)])
    worst = 0.0
    for L in (700, 2 * mx + 301):
        x, want = _case(name, L, scales, 3)
        xd = ops.to_device_f32(x)
        auto = _np(ops.cwt(xd, scales, name), plan.wavelet.complex)
        worst = max(worst, _worst(auto, want, x, plan))
        for form in FORMS:
            forced = _np(ops.cwt(xd, scales, name, form=form), plan.wavelet.complex)
            worst = max(worst, _worst(forced, want, x, plan), _worst(auto, forced, x, plan))
        # the rule took the direct form for the short filters and the spectral one for the rest: the same bits
        d = ops.cwt(xd, scales, name, form="direct")
        s = ops.cwt(xd, scales, name, form="spectral")
        a = ops.cwt(xd, scales, name)
        assert torch.equal(a[:, :2], d[:, :2]) and torch.equal(a[:, 2:], s[:, 2:])
    print(f"cwt {name} automatic form around {mx} taps: worst {worst:.2e} of A_s")


@pytest.mark.parametrize("name", ("morl", "cmor1.5-1.0"))
def test_far_apart_scales_are_not_paired(ops, name):
    scales = (1, 4096)
    plan = CW.cwt_plan(scales, name)
    assert CW.spectral_rows(plan, [0, 1]) == [(0, -1), (1, -1)]
    x, want = _case(name, 600, scales, 3)
    xd = ops.to_device_f32(x)
    worst = 0.0
    for form in (None,) + FORMS:                 # direct: 65538 taps over 600 samples, a span that is not staged
        worst = max(worst, _worst(_np(ops.cwt(xd, scales, name, form=form), plan.wavelet.complex), want, x, plan))
    print(f"cwt {name} scales [1, 4096]: worst {worst:.2e} of A_s")


@pytest.mark.parametrize("name", ("morl", "gaus1", "cmor1.5-1.0"))
def test_unit_impulses_give_the_table(ops, name):
    """An impulse at p gives W[s, t] = h_s[t + shift_s - p], the float32 table's own entries, and zero where the filter does
    not reach: offsets, reversal and crop, for odd and even len(coef) - L."""
    tile = ops.cwt_constants()["tile"]
    L = tile + 100
    scales = (1, 2, 7.3, 7.35, 40)
    plan = CW.cwt_plan(scales, name)
    assert {int(t) % 2 for t in plan.taps} == {0, 1}
    pos = list(range(40)) + list(range(L - 40, L))
    x = np.zeros((len(pos), L), dtype=np.float32)
    x[np.arange(len(pos)), pos] = 1.0
    got = _np(ops.cwt(ops.to_device_f32(x), scales, name, form="direct"), plan.wavelet.complex)
    want = np.zeros(got.shape, dtype=got.dtype)
    t = np.arange(L)
    for i in range(plan.S):
        h = plan.filter32(i)
        shift = int(plan.offset[i]) + 1
        for b, p in enumerate(pos):
            j = t + shift - p
            ok = (j >= 0) & (j < h.size)
            want[b, i, ok] = h[j[ok]]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ("morl", "cmor1.5-1.0"))
def test_output_forms_strides_and_determinism(ops, name, form):
    L, B = 1500, 5
    scales = (1, 2, 7.3, 32, 64.5, 200)
    plan = CW.cwt_plan(scales, name)
    cplx = plan.wavelet.complex
    xd = ops.to_device_f32(_rows(B, L, 5))
    c = ops.cwt(xd, scales, name, "coef", form=form)
    assert torch.equal(c, ops.cwt(xd, scales, name, "coef", form=form))                  # the same call, the same bits
    for b in range(B):                                                                    # a batch equals its rows
        assert torch.equal(c[b:b + 1], ops.cwt(xd[b:b + 1], scales, name, "coef", form=form))
    mag = ops.cwt(xd, scales, name, "magnitude", form=form)
    powr = ops.cwt(xd, scales, name, "power", form=form)
    assert tuple(mag.shape) == tuple(powr.shape) == (B, len(scales), L)
    a = np.abs(_np(c, cplx))
    # |.| and |.|^2 of the same coefficients, formed in float32 in the epilogue: within 2 ulp of the float64 value of the
    # float32 coefficients (float32 squares of values below 1e-19 are flushed: absolute floors of that size and of its square)
    for got, ref, floor in ((mag, a, 1e-19), (powr, a * a, 1e-37)):
        g = got.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(g - ref) <= 2 * np.spacing(ref.astype(np.float32)).astype(np.float64) + floor)
    out = torch.empty_like(c)
    assert ops.cwt(xd, scales, name, "coef", form=form, out=out) is out and torch.equal(out, c)
    for stride in (1, 3, 512, L + 1):
        for output, full in (("coef", c), ("magnitude", mag), ("power", powr)):
            got = ops.cwt(xd, scales, name, output, stride=stride, form=form)
            assert got.shape[2] == -(-L // stride) and torch.equal(got, full[:, :, ::stride].contiguous())


def test_continuous_wavelet_transform_mirror(ops):
    import sygnals_amd.core.transforms as TR
    sr, L = 8000, 2048
    t = np.arange(L) / sr
    x = np.sin(2 * np.pi * (100.0 * t + 0.5 * 12000.0 * t * t))                           # chirp 100 Hz -> 3172 Hz
    scales = TR.scalogram_scales(64, L)
    assert np.array_equal(scales, np.geomspace(1.0, 256.0, 64))
    x32 = x.astype(np.float32)[None, :]
    worst = 0.0
    for name, dtype in (("morl", np.float64), ("cmor1.5-1.0", np.complex128)):
        plan = CW.cwt_plan(scales, name)
        want, fwant = R.cwt(x32[0].astype(np.float64), scales, name, sampling_period=1.0 / sr)
        for method in ("conv", "fft"):
            W, f = TR.continuous_wavelet_transform(x, scales, name, sampling_period=1.0 / sr, method=method)
            assert W.shape == (64, L) and W.dtype == dtype and f.shape == (64,) and f.dtype == np.float64
            assert np.all(np.abs(f - fwant) <= 1e-12 * np.abs(fwant))
            worst = max(worst, _worst(W[None], want[None], x32, plan))
    print(f"continuous_wavelet_transform, chirp of 2048 samples x 64 scales: worst {worst:.2e} of A_s")


def test_cwt_batch_into_image_device(ops):
    import sygnals_amd.core.transforms as TR
    from sygnals_amd.core.ml_utils.formatters import image_device
    x = _rows(3, 2048, 9)
    scales = TR.scalogram_scales(16, 2048)
    plan = CW.cwt_plan(scales, "morl")
    S = TR.cwt_batch(ops.to_device_f32(x), scales, "morl", stride=8)
    assert tuple(S.shape) == (3, 16, 256) and S.dtype == torch.float32 and S.is_cuda
    want = np.abs(R.cwt_rows(x, scales, "morl"))[:, :, ::8]
    A = plan.l1[None, :, None] * np.max(np.abs(x.astype(np.float64)), axis=1)[:, None, None]
    assert np.all(np.abs(S.cpu().numpy() - want) <= GATE * A)
    img = image_device(S[0].contiguous())
    s0 = S[0].cpu().numpy().astype(np.float64)
    assert tuple(img.shape) == (16, 256) and np.allclose(img.cpu().numpy(), (s0 - s0.min()) / (s0.max() - s0.min()), atol=1e-6)
    small = image_device(S[1].contiguous(), output_shape=(32, 64))
    assert tuple(small.shape) == (32, 64) and float(small.min()) >= 0.0 and float(small.max()) <= 1.0


def test_dsp_cwt_on_a_wav(ops, tmp_path):
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli.main import cli
    sr, L = 8000, 1200
    pcm = np.round(12000 * np.sin(2 * np.pi * 440.0 * np.arange(L) / sr)).astype(np.int16)
    wavfile.write(tmp_path / "a.wav", sr, pcm)
    x32 = (pcm / 32768.0).astype(np.float32)[None, :]
    r = CliRunner().invoke(cli, ["dsp", "cwt", str(tmp_path / "a.wav"), "-o", str(tmp_path / "w.npz"), "--scales", "8"])
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "w.npz")
    scales = np.geomspace(1.0, L / 8.0, 8)
    assert sorted(z.files) == ["coefficients", "frequencies", "scales", "wavelet"] and str(z["wavelet"]) == "morl"
    assert np.array_equal(z["scales"], scales) and np.allclose(z["frequencies"], 0.8125 / scales * sr, rtol=1e-12)
    want = R.cwt_rows(x32, scales, "morl")
    worst = _worst(z["coefficients"][None], want, x32, CW.cwt_plan(scales, "morl"))
    r = CliRunner().invoke(cli, ["dsp", "cwt", str(tmp_path / "a.wav"), "-o", str(tmp_path / "w.csv"), "--scale-values", "2,9.5",
                                 "--wavelet", "cmor1.5-1.0", "--stride", "64"])
    assert r.exit_code == 0, r.output
    import pandas as pd
    df = pd.read_csv(tmp_path / "w.csv")
    n = -(-L // 64)
    assert list(df.columns) == ["scale", "frequency", "time", "real", "imag"] and len(df) == 2 * n
    assert np.allclose(df["time"].to_numpy()[:n], np.arange(n) * 64 / sr) and set(df["scale"]) == {2.0, 9.5}
    wantc = R.cwt_rows(x32, [2, 9.5], "cmor1.5-1.0")[:, :, ::64]
    got = (df["real"].to_numpy() + 1j * df["imag"].to_numpy()).reshape(1, 2, n)
    worst = max(worst, _worst(got, wantc, x32, CW.cwt_plan([2, 9.5], "cmor1.5-1.0")))
    r = CliRunner().invoke(cli, ["dsp", "cwt", str(tmp_path / "a.wav"), "-o", str(tmp_path / "m.csv"), "--scales", "3", "--magnitude"])
    assert r.exit_code == 0, r.output
    df = pd.read_csv(tmp_path / "m.csv")
    assert list(df.columns) == ["scale", "frequency", "time", "value"] and len(df) == 3 * L and (df["value"] >= 0).all()
    print(f"dsp cwt on a WAV: worst {worst:.2e} of A_s")
