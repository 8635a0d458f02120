"""Causal SOS filtering on the device (ops.sosfilt, syg_sosfilt_f32) against scipy.signal.sosfilt in float64 on the
float32 input, the FIR and equalizer paths built on it, the CLI, and the zero-phase path through the new designers.

Gates, per row: |y - y_ref| <= 1e-5 max|y_ref| and |zf - zf_ref| <= 1e-5 max|zf_ref| over the row's states.  Every
result of the sweep goes into an out= buffer filled with NaN.  The references are held to long double by
tests/test_iir_ref.py on these very inputs (tests/iir_cases.py)."""
import numpy as np
import pytest
import torch
from scipy import signal

from tests import iir_cases as IC

pytestmark = pytest.mark.gpu
GATE = IC.GATE
NAN = float("nan")


@pytest.fixture(scope="module")
def k():
    from sygnals_amd import ops
    return ops.sosfilt_constants()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fractions(y, zf, y_ref, zf_ref):
    """Worst per-row error as a fraction of the row's reference peak: (y, zf)."""
    y, zf = np.asarray(y, dtype=np.float64), np.asarray(zf, dtype=np.float64)
    assert y.shape == y_ref.shape and zf.shape == zf_ref.shape
    assert np.isfinite(y).all() and np.isfinite(zf).all(), "non-finite output (an element of the NaN buffer not written?)"
    B = y.shape[0]
    ypk = np.max(np.abs(y_ref), axis=1)
    zpk = np.max(np.abs(zf_ref.reshape(B, -1)), axis=1)
    ey = np.max(np.abs(y - y_ref), axis=1)
    ez = np.max(np.abs(zf - zf_ref).reshape(B, -1), axis=1)
    assert (ey[ypk == 0] == 0).all() and (ez[zpk == 0] == 0).all()
    return float(np.max(ey / np.where(ypk > 0, ypk, 1.0))), float(np.max(ez / np.where(zpk > 0, zpk, 1.0)))


def run(design, x, zi, **kw):
    """ops.sosfilt into a NaN-filled out= buffer -> (y, zf) on the host."""
    from sygnals_amd import ops
    out = torch.full(x.shape, NAN, dtype=torch.float32, device="cuda")
    y, zf = ops.sosfilt(dev(x), IC.DESIGNS[design], zi=dev(zi), return_state=True, out=out, **kw)
    assert y is out and zf.dtype == torch.float64 and tuple(zf.shape) == (x.shape[0], IC.SECTIONS[design], 2)
    return y.cpu().numpy(), zf.cpu().numpy()


def check_cases(cases, what):
    worst = [0.0, 0.0]
    for c in cases:
        x, zi = IC.make_input(c)
        y_ref, zf_ref = IC.scipy_ref(IC.DESIGNS[c.design], x, zi)
        fy, fz = fractions(*run(c.design, x, zi), y_ref, zf_ref)
        print(f"{IC.case_id(c)}: y {fy:.2e} zf {fz:.2e}")
        assert fy <= GATE and fz <= GATE, (IC.case_id(c), fy, fz)
        worst = [max(worst[0], fy), max(worst[1], fz)]
    print(f"worst of {what}: y {worst[0]:.2e} of the row's peak, zf {worst[1]:.2e}")


def test_sweep_lengths(k):
    """1, 2, 3; one chunk, the scan's look-ahead, one wave of chunks and the longest one-launch scan, each +- 1 (from the
    library's constants)."""
    assert IC.boundary_lengths(k) == [1, 2, 3, 255, 256, 257, 8191, 8192, 8193, 16383, 16384, 16385, 65535, 65536, 65537]
    check_cases(IC.sweep_cases(k)["lengths"], "lengths")


@pytest.mark.parametrize("design", list(IC.DESIGNS))
def test_sweep_designs(k, design):
    """1, 2, 3, 4, 8, 10, 17 and 32 sections (groups 8 | 2, 8 | 8 | 1, four full), zi absent, zero, steady and random."""
    cases = [c for c in IC.sweep_cases(k)["designs"] if c.design == design]
    assert [c.zi for c in cases] == list(IC.ZI_MODES)
    check_cases(cases, design)


def test_sweep_batches(k):
    cases = IC.sweep_cases(k)["batches"]
    assert sorted({c.B for c in cases}) == [1, 3, 16, 17, 33]
    check_cases(cases, "batches")


def test_long_row(k):
    (c,) = IC.sweep_cases(k)["long"]
    assert c.L == 1 << 20 and c.B == 1
    check_cases([c], "one row of 2^20")


def test_strided_rows_in_nan_buffers():
    """Rows 1540 floats apart that start 7 floats into a NaN buffer, in and out: nothing outside the rows is touched."""
    from sygnals_amd import ops
    c = IC.STRIDED
    x, zi = IC.make_input(c)
    y_ref, zf_ref = IC.scipy_ref(IC.DESIGNS[c.design], x, zi)
    n = 7 + c.B * 1540
    xin = torch.full((n,), NAN, dtype=torch.float32, device="cuda")
    yout = torch.full((n,), NAN, dtype=torch.float32, device="cuda")
    xv, yv = xin.as_strided((c.B, c.L), (1540, 1), 7), yout.as_strided((c.B, c.L), (1540, 1), 7)
    xv.copy_(dev(x))
    before = xin.clone()
    y, zf = ops.sosfilt(xv, IC.DESIGNS[c.design], zi=dev(zi), return_state=True, out=yv)
    assert y.data_ptr() == yv.data_ptr()
    fy, fz = fractions(yv.cpu().numpy(), zf.cpu().numpy(), y_ref, zf_ref)
    print(f"strided: y {fy:.2e} zf {fz:.2e}")
    assert fy <= GATE and fz <= GATE
    assert torch.equal(torch.isnan(xin), torch.isnan(before)) and torch.equal(xv, dev(x))
    mask = torch.ones(n, dtype=torch.bool, device="cuda")
    mask.as_strided((c.B, c.L), (1540, 1), 7).fill_(False)
    assert torch.isnan(yout[mask]).all() and int(mask.sum()) == n - c.B * c.L


def test_y_aliasing_x():
    from sygnals_amd import ops
    c = IC.ALIAS                                         # 17 sections: three groups, the later ones in place anyway
    x, zi = IC.make_input(c)
    y_ref, zf_ref = IC.scipy_ref(IC.DESIGNS[c.design], x, zi)
    sep, zsep = run(c.design, x, zi)
    xd = dev(x)
    y, zf = ops.sosfilt(xd, IC.DESIGNS[c.design], zi=dev(zi), return_state=True, out=xd)
    assert y is xd
    fy, fz = fractions(y.cpu().numpy(), zf.cpu().numpy(), y_ref, zf_ref)
    assert fy <= GATE and fz <= GATE
    assert np.array_equal(y.cpu().numpy(), sep) and np.array_equal(zf.cpu().numpy(), zsep)      # and the same bits as apart


def test_zero_row_and_constant_row():
    for name in ("butter4_bp", "cat17"):
        x = np.zeros((2, 1283), dtype=np.float32)
        for zi in (None, np.zeros((2, IC.SECTIONS[name], 2))):
            y, zf = run(name, x, zi)
            assert not y.any() and not zf.any()
    for name in IC.CONSTANT_DESIGNS:
        x, zi = IC.make_input(IC.constant_case(name), constant=True)
        sos = IC.DESIGNS[name]
        y_ref, zf_ref = IC.scipy_ref(sos, x, zi)
        y, zf = run(name, x, zi)
        fy, fz = fractions(y, zf, y_ref, zf_ref)
        dc = np.prod(sos[:, :3].sum(axis=1) / sos[:, 3:].sum(axis=1))
        steady = dc * x[:, :1].astype(np.float64)
        off = float(np.max(np.abs(y - steady) / np.abs(steady)))
        print(f"constant row, {name}: y {fy:.2e} zf {fz:.2e}, off the steady output by {off:.2e} from the first sample")
        assert fy <= GATE and fz <= GATE and off <= GATE


def test_identity_is_exact():
    from sygnals_amd import ops
    x = np.random.default_rng(3).standard_normal((3, 1000)).astype(np.float32)
    for n in (1, 9):
        sos = np.tile(np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]), (n, 1))
        y, zf = ops.sosfilt(dev(x), sos, return_state=True)
        assert np.array_equal(y.cpu().numpy(), x) and not zf.cpu().numpy().any()
    y = ops.sosfilt(dev(x), np.array([[2.0, 0.0, 0.0, 2.0, 0.0, 0.0]]))                  # a0 = 2 is divided out
    assert np.array_equal(y.cpu().numpy(), x)


@pytest.mark.parametrize("design", IC.IMPULSE_DESIGNS)
def test_unit_impulses(design):
    x = IC.impulses()
    y_ref, zf_ref = IC.scipy_ref(IC.DESIGNS[design], x, None)
    y, zf = run(design, x, None)
    fy, fz = fractions(y, zf, y_ref, zf_ref)
    print(f"impulses, {design}: y {fy:.2e} zf {fz:.2e}")
    assert fy <= GATE and fz <= GATE
    for r, n in enumerate(IC.IMPULSE_AT):
        assert not y[r, :n].any()                                       # exactly 0 in front of the impulse


def test_same_bits_twice_and_batch_equals_rows():
    from sygnals_amd import ops
    for c in (IC.Case("ellip8_bp", 17, 777, "random"), IC.Case("cat17", 5, 4099, "random"), IC.Case("eq10", 3, 16385, "steady")):
        x, zi = IC.make_input(c)
        sos = IC.DESIGNS[c.design]
        xd, zd = dev(x), dev(zi)
        y1, z1 = ops.sosfilt(xd, sos, zi=zd, return_state=True)
        y2, z2 = ops.sosfilt(xd, sos, zi=zd, return_state=True)
        assert torch.equal(y1, y2) and torch.equal(z1, z2)
        for r in range(c.B):
            # the row where it lies in the batch (L odd: mostly off 16-byte boundaries), and a copy of it on one
            for xr in (xd[r:r + 1], xd[r:r + 1].clone()):
                yr, zr = ops.sosfilt(xr, sos, zi=zd[r:r + 1], return_state=True)
                assert torch.equal(yr[0], y1[r]) and torch.equal(zr[0], z1[r]), (IC.case_id(c), r)


@pytest.mark.parametrize("design", IC.STREAM_DESIGNS)
def test_streaming_in_pieces(design):
    """Pieces cut at 1, 2, 257, 1000 and 16385 with zf carried into zi on the device: the float64 recurrences differ only
    in where the scan is cut, so a float32 output may differ by one rounding (2^-23 of the peak); the final state within
    1e-9 relative."""
    from sygnals_amd import ops
    x = IC.stream_input(design)
    sos = IC.DESIGNS[design]
    xd = dev(x)
    whole, zf_whole = ops.sosfilt(xd, sos, return_state=True)
    cuts = (0,) + IC.STREAM_CUTS + (IC.STREAM_L,)
    zi, parts = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        yp, zi = ops.sosfilt(xd[:, a:b], sos, zi=zi, return_state=True)
        parts.append(yp)
    y = torch.cat(parts, dim=1).cpu().numpy().astype(np.float64)
    w = whole.cpu().numpy().astype(np.float64)
    d = float(np.max(np.abs(y - w)) / np.max(np.abs(w)))
    zw = zf_whole.cpu().numpy()
    dz = float(np.max(np.abs(zi.cpu().numpy() - zw)) / np.max(np.abs(zw)))
    print(f"streaming, {design}: pieces vs whole {d:.2e} of the peak (2^-23 = {2.0 ** -23:.2e}), final state {dz:.2e}")
    assert d <= 2.0 ** -23 and dz <= 1e-9
    y_ref, zf_ref = IC.scipy_ref(sos, x, None)
    fy, fz = fractions(y, zi.cpu().numpy(), y_ref, zf_ref)
    assert fy <= GATE and fz <= GATE


# ---------------------------------------------------------------- end to end
E2E = {"cheby1_5_lp": dict(cutoff=3000.0, order=5, filter_type="lowpass", family="cheby1", rp=1.0),
       "ellip8_bp": dict(cutoff=(300.0, 3400.0), order=8, filter_type="bandpass", family="ellip", rp=0.5, rs=60.0),
       "bessel4_lp": dict(cutoff=2000.0, order=4, filter_type="lowpass", family="bessel")}


def peak_fraction(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape and np.isfinite(a).all()
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("design", IC.E2E_DESIGNS)
def test_apply_sos_filter_causal(design):
    from sygnals_amd.core import filters as F
    kw = dict(E2E[design])
    sos = F.design_iir_sos(kw.pop("cutoff"), IC.FS, kw.pop("order"), kw.pop("filter_type"), **kw)
    assert np.array_equal(sos, IC.DESIGNS[design])
    x = IC.e2e_input(design)
    y_ref, zf_ref = IC.scipy_ref(sos, x, None)
    y1 = F.apply_sos_filter_causal(sos, x[0].astype(np.float64))
    assert y1.dtype == np.float64 and peak_fraction(y1, y_ref[0]) <= GATE
    yb = F.apply_sos_filter_causal_batch(sos, dev(x))
    assert yb.is_cuda and peak_fraction(yb.cpu().numpy(), y_ref) <= GATE
    # from a host array, one [S, 2] state for every row, and the state handed on
    zi = 0.25 * signal.sosfilt_zi(sos)
    y2, zf2 = F.apply_sos_filter_causal_batch(sos, x, zi=zi, return_state=True)
    r2, rz2 = IC.scipy_ref(sos, x, np.broadcast_to(zi[None], (2,) + zi.shape))
    fy, fz = fractions(y2.cpu().numpy(), zf2.cpu().numpy(), r2, rz2)
    assert fy <= GATE and fz <= GATE


def test_fir_filter():
    from sygnals_amd.core import filters as F
    x = IC.e2e_input("ellip8_bp")
    taps = F.design_fir(101, 3000.0, 48000.0)
    ref = signal.lfilter(signal.firwin(101, 3000, fs=48000), 1, x.astype(np.float64), axis=-1)
    y = F.apply_fir_filter_batch(taps, dev(x))
    assert tuple(y.shape) == x.shape
    f = max(peak_fraction(y[r].cpu().numpy(), ref[r]) for r in range(x.shape[0]))
    print(f"fir 101 taps: {f:.2e} of the row's peak")
    assert f <= GATE


def test_equalizers():
    from sygnals_amd.core.audio import effects as FX
    from sygnals_amd.core.audio.effects import equalizer as EQ
    x = IC.e2e_input("ellip8_bp")
    x64 = x.astype(np.float64)
    ref = signal.sosfilt(IC.DESIGNS["eq10"], x64, axis=-1)
    y = FX.apply_graphic_eq(x64[0], 48000, IC.GRAPHIC_BANDS, IC.GRAPHIC_Q)
    assert y.dtype == np.float64 and peak_fraction(y, ref[0]) <= GATE
    yb = FX.apply_graphic_eq_batch(dev(x), 48000, IC.GRAPHIC_BANDS, IC.GRAPHIC_Q)
    assert max(peak_fraction(yb[r].cpu().numpy(), ref[r]) for r in range(2)) <= GATE
    params = [{"type": "peak", "freq": 1000.0, "gain_db": 4.0, "q": 2.0}, {"type": "low_shelf", "freq": 120.0, "gain_db": -3.0},
              {"type": "high_shelf", "freq": 8000.0, "gain_db": 5.0, "q": 0.9}, {"type": "notch", "freq": 50.0, "q": 30.0}]
    sos = EQ.parametric_eq_sos(48000, params)
    assert sos.shape == (4, 6)
    ref = signal.sosfilt(sos, x64, axis=-1)
    y = FX.apply_parametric_eq(x64[1], 48000, params)
    assert peak_fraction(y, ref[1]) <= GATE
    yb = FX.apply_parametric_eq_batch(dev(x), 48000, params)
    f = max(peak_fraction(yb[r].cpu().numpy(), ref[r]) for r in range(2))
    print(f"parametric eq (peak + shelves + notch): {f:.2e} of the row's peak")
    assert f <= GATE
    # gains below 0.1 dB: the input, unchanged, as a copy
    xd = dev(x)
    for yb in (FX.apply_graphic_eq_batch(xd, 48000, [(100.0, 0.05), (1000.0, -0.09)]),
               FX.apply_parametric_eq_batch(xd, 48000, [{"type": "peak", "freq": 1000.0, "gain_db": 0.05}])):
        assert torch.equal(yb, xd) and yb.data_ptr() != xd.data_ptr()
    assert np.array_equal(FX.apply_graphic_eq(x64[0], 48000, [(100.0, 0.05)]), x64[0])


def test_cli_on_a_small_wav(tmp_path):
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli.main import cli
    sr = 16000
    x = (0.2 * np.random.default_rng(11).standard_normal(3000)).astype(np.float32)
    wavfile.write(tmp_path / "x.wav", sr, x)
    x64 = x.astype(np.float64)
    src, out = str(tmp_path / "x.wav"), str(tmp_path / "y.npz")
    r = CliRunner()
    res = r.invoke(cli, ["filter", "apply", src, "-o", out, "--type", "bandpass", "--cutoff", "300,3400", "--order", "4", "--family",
                         "ellip", "--rp", "0.5", "--rs", "60", "--causal"])
    assert res.exit_code == 0, res.output
    sos = signal.ellip(4, 0.5, 60.0, (300.0, 3400.0), "bandpass", fs=sr, output="sos")
    assert peak_fraction(np.load(out)["data"], signal.sosfilt(sos, x64)) <= GATE
    res = r.invoke(cli, ["filter", "eq", src, "-o", out, "--band", "peak:1000:-6:1.4", "--band", "low_shelf:120:3", "--band", "notch:50:0:30"])
    assert res.exit_code == 0 and "3 stages" in res.output, res.output
    from sygnals_amd.core.audio.effects import equalizer as EQ
    sos = np.concatenate([EQ.design_eq_sos("peak", sr, 1000.0, -6.0, 1.4), EQ.design_eq_sos("low_shelf", sr, 120.0, 3.0),
                          EQ.design_eq_sos("notch", sr, 50.0, 0.0, 30.0)])
    assert peak_fraction(np.load(out)["data"], signal.sosfilt(sos, x64)) <= GATE
    res = r.invoke(cli, ["filter", "fir", src, "-o", out, "--numtaps", "63", "--cutoff", "300,3400", "--window", "kaiser:6.0", "--no-pass-zero"])
    assert res.exit_code == 0, res.output
    taps = signal.firwin(63, [300.0, 3400.0], window=("kaiser", 6.0), pass_zero=False, fs=sr)
    assert peak_fraction(np.load(out)["data"], signal.lfilter(taps, 1, x64)) <= GATE


@pytest.mark.parametrize("family,kw", [("ellip", dict(rp=0.5, rs=60.0)), ("cheby1", dict(rp=1.0)), ("cheby2", dict(rs=40.0)),
                                       ("bessel", {})])
def test_zero_phase_path_through_the_designers(family, kw):
    """apply_sos_filter_batch, unchanged, with the other families (at most 8 sections) against scipy.signal.sosfiltfilt."""
    from sygnals_amd.core import filters as F
    x = IC.e2e_input("ellip8_bp")
    worst = 0.0
    for cutoff, order, ftype in ((3000.0, 5, "lowpass"), ((300.0, 3400.0), 8, "bandpass"), (500.0, 6, "highpass")):
        sos = F.design_iir_sos(cutoff, IC.FS, order, ftype, family=family, **kw)
        assert sos.shape[0] <= 8
        ref = signal.sosfiltfilt(sos, x.astype(np.float64), axis=-1)
        y = F.apply_sos_filter_batch(sos, dev(x)).cpu().numpy()
        worst = max(worst, max(peak_fraction(y[r], ref[r]) for r in range(x.shape[0])))
    print(f"zero-phase, {family}: {worst:.2e} of the row's peak")
    assert worst <= GATE
