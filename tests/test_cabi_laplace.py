"""The Laplace entries of the C ABI are declared, bound and exported and reject bad arguments before device work; the
host table builder (sygnals_amd/_laplace.py) means what include/sygnals_hip.h says; the mirrors keep the reference's
signature, messages and empty-input behaviour; the CLI reads its s-values."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from sygnals_amd import _laplace as LP
from tests import laplace_emul as E
from tests import laplace_ref as R
from tests.test_cabi_symbols import declared_functions

NEW = ["syg_laplace_chunk", "syg_laplace_tile_rows", "syg_laplace_tile_cols", "syg_laplace_segment", "syg_laplace_steep",
       "syg_laplace_fac_stride", "syg_laplace_work_bytes", "syg_laplace_f32"]


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def K(h):
    return dict(C=h.syg_laplace_chunk(), tile_cols=h.syg_laplace_tile_cols(), segment=h.syg_laplace_segment(),
                steep=h.syg_laplace_steep(), fac_stride=h.syg_laplace_fac_stride())


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
    Cc, Rr, N = h.syg_laplace_chunk(), h.syg_laplace_tile_rows(), h.syg_laplace_tile_cols()
    assert Cc in (64, 128) and Rr >= 4 and N >= 4
    assert h.syg_laplace_segment() % (Cc * Rr) == 0                 # a segment is whole tiles
    assert LP.STEEP_LOG / (Cc - 1) * h.syg_laplace_steep() >= 746.0  # what a steep column skips is below float64
    assert np.exp(-LP.STEEP_LOG) > 1e3 * np.finfo(np.float32).tiny  # and the table of any other column stays normal


def _lp(h, p, x=True, B=2, L=100, ldx=100, table=True, fac=True, anchor=True, col=True, Sf=16, Sr=0, ssf=0, ssr=0, S=3, t=1.0,
        out=True, work=None, form=-1):
    a = lambda on: p if on else None                                 # noqa: E731
    return h.syg_laplace_f32(a(x), B, L, ldx, a(table), a(fac), a(anchor), a(col), Sf, Sr, ssf, ssr, S, t, a(out), work, form,
                             None)


def test_rejects(h, p):
    for kw in ({"x": False}, {"fac": False}, {"anchor": False}, {"col": False}, {"out": False}, {"table": False}):
        assert _lp(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    assert _lp(h, p, table=False, Sf=0, ssf=3, L=0) == -1 and b"bad B / L" in h.syg_last_error()   # a NULL table is fine there
    for kw in ({"B": 0}, {"B": -1}, {"L": 0}, {"L": -5}, {"B": 1 << 31}, {"L": 1 << 40, "ldx": 1 << 40}, {"B": 1 << 20, "L": 1 << 30, "ldx": 1 << 30}):
        assert _lp(h, p, **kw) == -1 and b"bad B / L" in h.syg_last_error()
    for kw in ({"Sf": 15}, {"Sf": -16}, {"Sr": 8}, {"Sf": 1 << 25}):
        assert _lp(h, p, **kw) == -1 and b"must be multiples of" in h.syg_last_error()
    for kw in ({"S": 0}, {"S": -1}, {"S": 1 << 25}, {"S": 17}, {"S": 3, "Sf": 32, "Sr": 16}, {"ssf": -1}, {"ssr": 4}):
        assert _lp(h, p, **kw) == -1 and b"bad S" in h.syg_last_error()
    assert _lp(h, p, ldx=99) == -1 and b"ldx=99 is less than L=100" in h.syg_last_error()
    for t in (float("nan"), float("inf")):
        assert _lp(h, p, t=t) == -1 and b"t_step must be finite" in h.syg_last_error()
    for form in (-2, 2):
        assert _lp(h, p, form=form) == -1 and b"form must be" in h.syg_last_error()
    assert _lp(h, p, form=1) == -1 and b"needs `work`" in h.syg_last_error()
    seg = h.syg_laplace_segment()
    assert _lp(h, p, B=1, L=seg + 1, ldx=seg + 1) == -1 and b"needs `work`" in h.syg_last_error()   # the rule: one long row
    odd = C.c_void_p(p.value + 8)
    assert _lp(h, p, form=1, work=odd) == -1 and b"16-byte aligned" in h.syg_last_error()


def test_work_bytes_on_both_sides_of_the_switch(h):
    wb, seg, N = h.syg_laplace_work_bytes, h.syg_laplace_segment(), h.syg_laplace_tile_cols()
    assert wb(1, seg, N, -1) == 0                                    # one segment: nothing to split
    assert wb(1, seg + 1, N, -1) == 16 * 2 * N                      # two segments of a long row, a complex float64 per column
    assert wb(3, 5 * seg, 2 * N, -1) == 16 * 3 * 5 * 2 * N
    assert wb(1, 1 << 24, 4 * N, -1) == 16 * ((1 << 24) // seg) * 4 * N
    assert wb(1 << 14, 2 * seg, N, -1) == 0                          # a batch fills the device with whole rows
    assert wb(1 << 14, 2 * seg, N, 1) == 16 * (1 << 14) * 2 * N and wb(1, 1 << 24, N, 0) == 0      # the explicit forms
    assert wb(1, 1 << 24, 0, -1) == 0                                # steep columns only
    assert wb(0, 10, N, -1) == -1 and wb(1, 0, N, -1) == -1 and wb(1, 10, N + 1, -1) == -1 and wb(1, 10, N, 2) == -1


S_MIX = np.array([0.0, 0.3j, 1e-3 + 3.1j, -1e-3 - 2j, 0.5, -0.5 + 1j, 0.634 + 0.1j, 0.636, -0.636 + 2j, 5 + 1j, -11.0, 100.0,
                  -0.0 + 1j, 2e-4 - 5.3j, -3e-2])


def test_plan_layout(K):
    t = 0.5
    s = S_MIX / t
    pl = LP.plan(s, t, **K)
    Cc, N = K["C"], K["tile_cols"]
    assert pl.S == 15 and pl.S_fwd == 16 and pl.S_rev == 16 and pl.S_steep_fwd == 3 and pl.S_steep_rev == 2
    assert pl.table.shape == (Cc, 2, 32) and pl.table.dtype == np.float32 and pl.fac.shape == (37, K["fac_stride"])
    assert pl.col.dtype == np.int32 and sorted(pl.col[pl.col >= 0]) == list(range(15)) and np.sum(pl.col < 0) == 37 - 15
    a = (s * t).real
    for c, o in enumerate(pl.col):
        if o < 0:
            assert not pl.table[:, :, c].any() if c < 32 else True
            assert not pl.fac[c].any()
            continue
        steep, rev = abs(a[o]) * (Cc - 1) > LP.STEEP_LOG, a[o] < 0
        assert steep == (c >= 32) and rev == bool(pl.rev[c])
        assert rev == (16 <= c < 32 or c >= 35)
        z = np.exp(s[o] * t if rev else -s[o] * t)                  # direct float64 exp
        if c < 32:
            i = np.arange(Cc)
            want = np.exp((s[o] * t if rev else -s[o] * t) * (Cc - 1 - i if rev else i))
            assert np.array_equal(pl.table[:, 0, c], want.real.astype(np.float32))
            assert np.array_equal(pl.table[:, 1, c], want.imag.astype(np.float32))
        f = pl.fac[c, 0::2] + 1j * pl.fac[c, 1::2]
        e = np.concatenate([np.arange(16) * Cc, [16 * Cc, K["segment"], 1]])
        assert np.allclose(f, z ** e, rtol=1e-10, atol=0) or steep       # z ** 16384 itself carries 2e-12
        assert f[18] == z
    assert np.all(np.hypot(pl.table[:, 0], pl.table[:, 1]) <= 1.0)                 # both sign groups decay
    assert np.all(np.hypot(pl.fac[:, 0::2], pl.fac[:, 1::2]) <= 1.0 + 1e-15)
    nz = np.abs(pl.table[:, 0, pl.col[:32] >= 0]) + np.abs(pl.table[:, 1, pl.col[:32] >= 0])
    assert nz.min() > 1e3 * np.finfo(np.float32).tiny               # no entry of a table column leaves the normal range
    an = LP.anchors(pl, 64)
    assert np.all(np.isfinite(an)) and np.array_equal(an[~pl.rev & (pl.col >= 0)], np.tile([1.0, 0.0], (np.sum(~pl.rev & (pl.col >= 0)), 1)))
    c = int(np.flatnonzero(pl.col == 10)[0])                        # sigma t = -11: 693 at L = 64
    assert np.isclose(an[c, 0], np.exp(11.0 * 63), rtol=1e-12)


@pytest.mark.parametrize("L", [1, 2, 63, 65, 1025, 16385 + 64])
def test_tables_walked_in_numpy_meet_the_gate(K, L):
    """The whole arithmetic of the kernel from the tables alone, both launch forms: impulses, a row that starts with
    zeros (where an underflowed table would lose the sum) and noise, s out to the domain's edge."""
    rng = np.random.default_rng(L)
    t = 1.0 / 8000.0
    T = max(L - 1, 1) * t
    s = np.concatenate([S_MIX / t * (1 if 11.0 * (L - 1) <= 700 else 0.0), [-700.0 / T + 0.3j / t, 30 / T, -30 / T - 1j / t]])
    pl, Cc = LP.plan(s, t, **K), K["C"]
    an = LP.anchors(pl, L)
    n = np.arange(L)
    rows = [rng.standard_normal(L), 1.0 * (n == L - 1), 1.0 * (n == min(L - 1, Cc + 1)), 1.0 * (n >= L // 2)]
    for x in rows:
        x = x.astype(np.float32)
        ref, A = R.laplace(x, s, t), R.scale(x, s, t)
        for segmented in (False, True):
            got = E.run(x, pl, an, t, Cc, 16, K["segment"], K["steep"], segmented)
            assert np.all(np.abs(got - ref) <= 1e-5 * A)


def test_plan_rejects(K):
    for s, t in ((np.zeros((2, 2)), 1.0), ([1.0, np.nan], 1.0), ([1.0, np.inf + 1j], 1.0), ([1.0], np.nan), ([1.0], np.inf)):
        with pytest.raises(ValueError):
            LP.plan(s, t, **K)
    with pytest.raises(ValueError):
        LP.plan([1.0], 1.0, **dict(K, steep=100))                    # constants the builder cannot serve


def test_mirror_signature_messages_and_empty_inputs():
    import sygnals_amd.core.transforms as TR
    sig = inspect.signature(TR.laplace_transform_numerical)
    assert list(sig.parameters) == ["data", "s_values", "t_step"] and sig.parameters["t_step"].default == 1.0
    assert list(inspect.signature(TR.laplace_batch).parameters) == ["y", "s_values", "t_step"]

    def raises(text, *a):
        with pytest.raises(ValueError) as e:
            TR.laplace_transform_numerical(*a)
        assert text in str(e.value)
        return str(e.value)

    assert raises("", np.zeros((2, 3)), np.zeros(2, dtype=complex)) == "Input data must be 1D."
    assert raises("", np.zeros(3), np.zeros((2, 2), dtype=complex)) == "s_values must be 1D."
    out = TR.laplace_transform_numerical(np.ones(5), np.zeros(0, dtype=np.complex128))
    assert out.shape == (0,) and out.dtype == np.complex128
    out = TR.laplace_transform_numerical(np.zeros(0), np.array([1.0, 2j]), 0.5)
    assert np.array_equal(out, np.zeros(2, dtype=np.complex128)) and out.dtype == np.complex128
    # the domain: -sigma t_step (L - 1) = 700.001 is refused (before any device call), naming the value and the bound
    L, t = 101, 0.5
    msg = raises("outside the served domain", np.ones(L), np.array([0.0, -700.001 / (t * (L - 1)) + 2j]), t)
    assert "s_values[1]" in msg and "700" in msg and "-14.00002" in msg
    raises("not finite", np.ones(4), np.array([np.nan + 0j]))
    raises("t_step must be finite", np.ones(4), np.array([1.0 + 0j]), np.inf)
    LP.check_domain(np.array([-700.0 / (t * (L - 1)) + 2j, 1e9]), t, L)             # 700 itself is served
    LP.check_domain(np.array([-1e300]), 1.0, 1)                     # a single sample has no exponent at all
    with pytest.raises(ValueError):
        LP.check_domain(np.array([700.001 / (t * (L - 1))]), -t, L)                 # a negative t_step turns the sign


def test_plugin_registers_the_transform():
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin
    names = []

    class Reg:
        def add_transform(self, name, fn):
            names.append(name)
    SygnalsAmdPlugin().register_transforms(Reg())
    assert "laplace_transform_numerical" in names and "hilbert_transform" in names


def test_cli_s_values_and_usage_errors(tmp_path):
    import click
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli, parse_s_values
    assert np.array_equal(parse_s_values("1.0,0.5+0.2j, -3j ,2e-3-1J"), np.array([1.0, 0.5 + 0.2j, -3j, 2e-3 - 1j]))
    assert parse_s_values("7").dtype == np.complex128
    for bad in ("1.0,abc", "1,,2", "", "0.5 + 0.2j", "1;2"):
        with pytest.raises(click.UsageError):
            parse_s_values(bad)
    import pandas as pd
    pd.DataFrame({"value": np.arange(8.0)}).to_csv(tmp_path / "x.csv", index=False)
    run = lambda *a: CliRunner().invoke(cli, ["dsp", "laplace", str(tmp_path / "x.csv"), "-o", str(tmp_path / "y.csv"), *a])   # noqa: E731
    r = run("--s-values", "1.0,zz", "--t-step", "0.1")
    assert r.exit_code == 2 and "cannot read 'zz'" in r.output
    r = run("--s-values", "1.0")
    assert r.exit_code == 2 and "--t-step is required" in r.output
    r = run("--t-step", "0.1")
    assert r.exit_code == 2 and "--s-values" in r.output
    r = run("--s-values", "-1000", "--t-step", "1.0")
    assert r.exit_code == 2 and "outside the served domain" in r.output
    r = CliRunner().invoke(cli, ["dsp", "--help"])
    assert r.exit_code == 0 and "laplace" in r.output
