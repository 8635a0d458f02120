"""The continuous-wavelet entries of the C ABI are declared, bound and exported and reject bad arguments before device work;
the host plan's float32 table is the restatement's differenced filter bit for bit; the mirrors keep their signatures; what
is not served is refused without a device; the CLI reports its usage errors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from sygnals_amd import _cwt as CW
from tests import cwt_ref as R
from tests.test_cabi_symbols import declared_functions

NEW = ["syg_cwt_tile", "syg_cwt_direct_taps_max", "syg_cwt_scales_per_group", "syg_cwt_span_max", "syg_cwt_taps_lds_max",
       "syg_cwt_work_bytes", "syg_cwt_f32", "syg_cwt_spectrum_c64", "syg_cwt_crop_f32"]
WAVELETS = ("morl", "mexh", "gaus1", "cmor1.5-1.0")
REFUSED = ("gaus2", "gaus8", "cgau1", "shan1.5-1.0", "fbsp2-1.5-1.0", "db4", "haar", "cmor", "cmor0-1.0", "cmor1.5", "cmor-1-1", "", 7)


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_double * 64)()                       # never dereferenced: every call is rejected
    return C.cast(buf, C.c_void_p)


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)
    assert h.syg_abi_version() == 1


def test_constants(h):
    from sygnals_amd import ops
    k = ops.cwt_constants()
    assert k == dict(tile=h.syg_cwt_tile(), direct_taps_max=h.syg_cwt_direct_taps_max(),
                     scales_per_group=h.syg_cwt_scales_per_group(), span_max=h.syg_cwt_span_max(),
                     taps_lds_max=h.syg_cwt_taps_lds_max())
    assert k["tile"] % 256 == 0 and 256 <= k["tile"] <= 4096
    assert 1 <= k["scales_per_group"] <= 64
    assert 4 * k["span_max"] <= 160 * 1024                                # the staged span fits the 160 KiB of LDS
    # a full tile at stride 1 under filters of the rule's length is staged (and two such blocks fit a CU)
    assert 16 <= k["direct_taps_max"] and 2 * 4 * (k["tile"] + 2 * k["direct_taps_max"]) <= 160 * 1024
    assert k["tile"] + 2 * k["direct_taps_max"] <= k["span_max"]
    # padded rows 4, their transform 8, products + inverse + four-step temporary 3 x 8 R
    assert h.syg_cwt_work_bytes(3, 5, 1024) == 3 * 1024 * (12 + 24 * 5)
    for bad in ((0, 1, 16), (1, 0, 16), (1, 1, 1), (65536, 1, 16), (1, 1, (1 << 27) + 1)):
        assert h.syg_cwt_work_bytes(*bad) == -1 and b"bad B / R / M" in h.syg_last_error()


def _cw(h, p, x=True, B=2, L=100, ldx=100, table=True, meta=True, S=3, S_out=3, cplx=0, reach=40, output=0, stride=1, n_out=100, y=True):
    a = lambda on: p if on else None                                 # noqa: E731
    return h.syg_cwt_f32(a(x), B, L, ldx, a(table), a(meta), S, S_out, cplx, reach, output, stride, n_out, a(y), None)


def test_rejects(h, p):
    for kw in ({"x": False}, {"table": False}, {"meta": False}, {"y": False}):
        assert _cw(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"B": -1}, {"B": 65536}, {"L": 0, "n_out": 0}, {"L": -4}):
        assert _cw(h, p, **kw) == -1 and b"bad B / L" in h.syg_last_error()
    for kw in ({"S": 0}, {"S": -2}, {"S": 4}, {"S_out": 0, "S": 0}, {"S_out": -1}):
        assert _cw(h, p, **kw) == -1 and b"bad S" in h.syg_last_error()
    for stride in (0, -1):
        assert _cw(h, p, stride=stride) == -1 and b"stride must be at least 1" in h.syg_last_error()
    for output in (-1, 3, 99):
        assert _cw(h, p, output=output) == -1 and b"unknown output code" in h.syg_last_error()
    for cplx in (-1, 2):
        assert _cw(h, p, cplx=cplx) == -1 and b"cplx must be" in h.syg_last_error()
    for n_out in (99, 101, 0):
        assert _cw(h, p, n_out=n_out) == -1 and b"is not ceil(L / stride) = 100" in h.syg_last_error()
    assert _cw(h, p, stride=3, n_out=33) == -1 and b"= 34" in h.syg_last_error()                    # ceil, not floor
    assert _cw(h, p, ldx=99) == -1 and b"ldx=99 is less than L=100" in h.syg_last_error()
    for reach in (0, -5, 1 << 31):
        assert _cw(h, p, reach=reach) == -1 and b"reach must be" in h.syg_last_error()
    # the two ends of the spectral form
    assert h.syg_cwt_spectrum_c64(None, p, 1, 1, 16, p, None) == -1 and b"null pointer" in h.syg_last_error()
    assert h.syg_cwt_spectrum_c64(p, p, 0, 1, 16, p, None) == -1 and b"bad B / R / M" in h.syg_last_error()
    q = C.cast((C.c_double * 8)(), C.c_void_p)
    assert h.syg_cwt_spectrum_c64(p, q, 1, 1, 16, p, None) == -1 and b"in-place" in h.syg_last_error()
    crop = lambda Z=p, B=1, R=1, M=128, rm=p, L=100, S=2, cplx=0, output=0, stride=1, n_out=100, y=q: \
        h.syg_cwt_crop_f32(Z, B, R, M, rm, L, S, cplx, output, stride, n_out, y, None)            # noqa: E731
    assert crop(Z=None) == -1 and b"null pointer" in h.syg_last_error()
    assert crop(rm=None) == -1 and crop(y=None) == -1
    assert crop(B=0) == -1 and b"bad B / L" in h.syg_last_error()
    assert crop(output=3) == -1 and b"unknown output code" in h.syg_last_error()
    assert crop(stride=0) == -1 and b"stride must be at least 1" in h.syg_last_error()
    assert crop(n_out=50) == -1 and b"is not ceil(L / stride)" in h.syg_last_error()
    for kw in ({"R": 0}, {"R": 3}, {"M": 99}):
        assert crop(**kw) == -1 and b"bad R / M" in h.syg_last_error()


@pytest.mark.parametrize("name", WAVELETS)
def test_plan_table_is_the_restatement_rounded_once(name):
    scales = [1, 1.5, 2, 7.3, 32, 64.5, 512]
    plan = CW.cwt_plan(scales, name)
    assert plan.S == len(scales) and plan.table.dtype == np.float32 and plan.planes == (2 if name.startswith("cmor") else 1)
    # scale 512: 512 (hi - lo) + 1 samples of the kernel, one more of its difference
    assert int(plan.taps.max()) == (512 * 10 + 2 if name == "gaus1" else 512 * 16 + 2)
    for i, s in enumerate(scales):
        hs, off = R.h_filter(name, s)
        o, n = int(plan.tab_off[i]), int(plan.taps[i])
        assert n == hs.size and plan.offset[i] == off == int(np.floor((n - 3) / 2.0))
        if plan.planes == 2:
            assert np.array_equal(plan.table[o:o + n], hs.real.astype(np.float32))
            assert np.array_equal(plan.table[o + n:o + 2 * n], hs.imag.astype(np.float32))
        else:
            assert np.array_equal(plan.table[o:o + n], hs.astype(np.float32))
        assert plan.l1[i] == pytest.approx(np.abs(hs).sum(), rel=1e-15)
    assert plan.table.size == int(plan.taps.sum()) * plan.planes
    m = plan.meta(np.arange(plan.S))
    assert m.dtype == np.int32 and m.shape == (plan.S, 4)
    assert np.array_equal(m[:, 0], plan.tab_off) and np.array_equal(m[:, 2], plan.offset + 1) and np.array_equal(m[:, 3], np.arange(plan.S))
    assert CW.cwt_plan(np.asarray(scales, dtype=np.float64), name) is plan            # cached per wavelet and scale list


def test_split_and_pairing():
    plan = CW.cwt_plan([1, 4096, 40, 100, 150, 700], "morl")
    d, s = CW.split_forms(plan, 1024, None)
    assert list(d) == [0, 2] and list(s) == [1, 3, 4, 5]
    assert [len(v) for v in CW.split_forms(plan, 1024, "direct")] == [6, 0]
    assert [len(v) for v in CW.split_forms(plan, 1024, "spectral")] == [0, 6]
    # neighbours in sorted order, within a factor 4: (100, 150), then 700 alone (4096 is 5.9 times it), 4096 alone
    assert CW.spectral_rows(plan, s) == [(3, 4), (5, -1), (1, -1)]
    assert CW.spectral_rows(CW.cwt_plan([1, 4096], "morl"), [0, 1]) == [(0, -1), (1, -1)]
    assert CW.spectral_rows(CW.cwt_plan([1, 4], "morl"), [0, 1]) == [(0, 1)]
    assert CW.spectral_rows(CW.cwt_plan([1, 2, 3], "cmor1.5-1.0"), [0, 1, 2]) == [(0, -1), (1, -1), (2, -1)]
    rows = CW.spectral_rows(plan, s)
    hh, rmeta = CW.spectral_tables(plan, rows, 70000)
    assert hh.shape == (3, 70000, 2) and rmeta.tolist()[0] == [plan.offset[3] + 1, 3, plan.offset[4] + 1, 4]
    assert rmeta.tolist()[1] == [plan.offset[5] + 1, 5, 0, -1]
    assert np.array_equal(hh[0, :plan.taps[3], 0], plan.filter32(3)) and np.array_equal(hh[0, :plan.taps[4], 1], plan.filter32(4))
    assert not hh[0, plan.taps[4]:].any() and not hh[1, :, 1].any()
    # the widest span of a group at one column
    assert plan.reach([0], 8) == plan.taps[0] and plan.reach([0, 2], 8) == plan.taps[2]


def test_mirror_signatures():
    import sygnals_amd.core.transforms as TR
    from sygnals_amd import ops
    sig = inspect.signature(TR.continuous_wavelet_transform)
    assert list(sig.parameters) == ["data", "scales", "wavelet", "sampling_period", "method"]
    assert [sig.parameters[k].default for k in ("wavelet", "sampling_period", "method")] == ["morl", 1.0, "conv"]
    sig = inspect.signature(TR.cwt_batch)
    assert list(sig.parameters) == ["y", "scales", "wavelet", "output", "stride"]
    assert [sig.parameters[k].default for k in ("wavelet", "output", "stride")] == ["morl", "magnitude", 1]
    sig = inspect.signature(ops.cwt)
    assert list(sig.parameters) == ["y", "scales", "wavelet", "output", "stride", "form", "out"]
    assert [sig.parameters[k].default for k in ("wavelet", "output", "stride", "form", "out")] == ["morl", "coef", 1, None, None]
    assert list(inspect.signature(ops.cwt_plan).parameters) == ["scales", "wavelet", "L"]
    assert list(inspect.signature(TR.scalogram_scales).parameters) == ["num", "L"]
    assert list(inspect.signature(TR.central_frequency).parameters)[0] == "wavelet"
    assert list(inspect.signature(TR.scale2frequency).parameters)[:2] == ["wavelet", "scales"]
    assert np.array_equal(TR.scalogram_scales(64, 2048), np.geomspace(1.0, 256.0, 64))
    assert TR.central_frequency("morl") == 0.8125 and np.array_equal(TR.scale2frequency("mexh", [1, 2]), [0.25, 0.125])


def test_refusals_need_no_device():
    import sygnals_amd.core.transforms as TR
    from sygnals_amd import ops
    y = torch.zeros((2, 40), dtype=torch.float32)                   # a host tensor: anything that got further would fail on it
    x = np.zeros(40)
    for name in REFUSED:
        for call in (lambda: ops.cwt(y, [1, 2], name), lambda: TR.cwt_batch(y, [1, 2], name),
                     lambda: TR.continuous_wavelet_transform(x, [1, 2], name), lambda: TR.central_frequency(name),
                     lambda: TR.scale2frequency(name, [1.0])):
            with pytest.raises(ValueError) as e:
                call()
            assert "not served" in str(e.value) and all(s in str(e.value) for s in ("morl", "mexh", "gaus1", "cmorB-C"))
    for data in (np.zeros(0), []):
        with pytest.raises(ValueError) as e:
            TR.continuous_wavelet_transform(data, [1, 2])
        assert "at least one sample" in str(e.value)
    with pytest.raises(ValueError) as e:
        TR.continuous_wavelet_transform(np.zeros((2, 8)), [1, 2])
    assert "1D" in str(e.value)
    for call in (lambda: ops.cwt(torch.zeros((0, 8)), [1]), lambda: ops.cwt(torch.zeros((2, 0)), [1]), lambda: ops.cwt(x, [1]),
                 lambda: ops.cwt(torch.zeros(8), [1]), lambda: ops.cwt(torch.zeros((2, 8), dtype=torch.float64), [1])):
        with pytest.raises(ValueError):
            call()
    for scales in ([], [1, 0], [2, -1], [np.nan], np.zeros((2, 2))):
        for call in (lambda: ops.cwt(y, scales), lambda: TR.continuous_wavelet_transform(x, scales), lambda: ops.cwt_plan(scales)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == "Scales array must not be empty and contain only positive values."
    for call in (lambda: ops.cwt(y, [4, 0.01]), lambda: TR.continuous_wavelet_transform(x, [4, 0.01]), lambda: TR.cwt_batch(y, [0.01])):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "Selected scale of 0.01 too small."
    with pytest.raises(ValueError) as e:
        TR.continuous_wavelet_transform(x, [1, 2], method="direct")
    assert "method must be 'conv' or 'fft'" in str(e.value)
    for kw in ({"output": "phase"}, {"form": "lds"}, {"stride": 0}, {"stride": 1.5}, {"stride": -2}):
        with pytest.raises(ValueError):
            ops.cwt(y, [1, 2], **kw)
    # a step matrix above 2^31 elements: 2 x 1100 x 2^20 = 2.3e9; the message names the size.  (An expanded view: no memory.)
    big = torch.zeros((1, 1), dtype=torch.float32).expand(2, 1 << 20)
    with pytest.raises(ValueError) as e:
        ops.cwt(big, np.linspace(1, 2, 1100))
    assert str(2 * 1100 * (1 << 20)) in str(e.value) and "2^31" in str(e.value)


def test_plugin_registers_the_transform():
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin
    names = []

    class Reg:
        def add_transform(self, name, fn):
            names.append(name)
    SygnalsAmdPlugin().register_transforms(Reg())
    assert "continuous_wavelet_transform" in names and "hilbert_transform" in names


def test_cli_usage_errors(tmp_path):
    import click
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli, parse_scale_values
    assert np.array_equal(parse_scale_values("1, 2.5,8"), [1.0, 2.5, 8.0])
    for bad in ("1,x", "", "1,,2"):
        with pytest.raises(click.UsageError):
            parse_scale_values(bad)
    pd.DataFrame({"value": np.arange(8.0)}).to_csv(tmp_path / "x.csv", index=False)
    run = lambda *a: CliRunner().invoke(cli, ["dsp", "cwt", str(tmp_path / "x.csv"), "-o", str(tmp_path / "y.npz"), *a])   # noqa: E731
    r = run()
    assert r.exit_code == 2 and "exactly one of --scales" in r.output
    r = run("--scales", "4", "--scale-values", "1,2")
    assert r.exit_code == 2 and "exactly one of --scales" in r.output
    r = run("--scales", "0")
    assert r.exit_code == 2 and "--scales must be at least 1" in r.output
    r = run("--scales", "4", "--stride", "0")
    assert r.exit_code == 2 and "--stride must be at least 1" in r.output
    r = run("--scale-values", "1,abc")
    assert r.exit_code == 2 and "--scale-values" in r.output
    r = run("--scale-values", "1,-2")
    assert r.exit_code == 2 and "only positive values" in r.output
    r = run("--scale-values", "0.01")
    assert r.exit_code == 2 and "Selected scale of 0.01 too small." in r.output
    r = run("--scales", "4", "--wavelet", "gaus2")
    assert r.exit_code == 2 and "not served" in r.output
    r = CliRunner().invoke(cli, ["dsp", "--help"])
    assert r.exit_code == 0 and "cwt" in r.output
