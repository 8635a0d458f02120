"""The CQT kernels across bins per octave, filter scale, tuning, sparsity, clipped octaves and hops (tests/cqt_cases.py): every
instantiation the entry points of cqt.hip can launch and the one-launch kernel at 8, 12 and 16 filters, against the float64
oracle at the project's gate (1e-5 of the peak), against each other (three modes = three independent device answers), and
for the structural properties the older tests pin at one shape only (one-launch = level-by-level to 2e-6, staged = per-frame
bit for bit, repeat / batch).  Which kernel a row runs on is tests/cqt_cases.ROUTES, pinned on the host by
tests/test_host_logic.py::test_cqt_route_is_pinned and checked here against the calls ops.cqt really makes."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import cpu_ref as O
from tests.cqt_cases import CASES, MODES, ROUTES, kwargs
from tests.gpu_util import peak_rel

TOL = 1e-5                     # README: "fp32 parity <= 1e-5 relative" (tests/test_gpu_api.py)
ONE_LAUNCH_TOL = 2e-6          # one-launch against level-by-level: the figure of test_gpu_api.py::test_cqt_one_launch_form
ROW_PEAK = 0.2                 # every CQT row of the noise clip peaks at >= 0.2 of the global peak (a condition on the INPUT)
ALL = sorted(CASES)
ONE_LAUNCH = [k for k in ALL if ROUTES[k][0]]
# rows that bring staged instantiations / hops the older tests do not reach: <128,2>, <128,1>, <256,1>, a five-filter tile,
# the 16-filter clipped octave at 128, and hops 80 / 40 / 20, 48 / 24 / 12 (slot skews and copy counts of their own)
STAGED = ["fs0.5", "bpo8-fs0.9", "bpo8", "bins80", "bins77", "bins7", "bins1", "bpo24-fs0.25", "16k-hop160", "hop192", "hop96"]


def _mode_pairs():
    out = []
    for k in ALL:
        one, early, b, g, f = ROUTES[k]
        out.append((k, "bf16x3"))
        if one or g != b:
            out.append((k, "gemm"))
        if f != g and f != b:
            out.append((k, "fft"))
    return out


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from sygnals_amd import ops
    ops.require_gpu()


@functools.lru_cache(maxsize=None)
def clips(case):
    """[2, 2 sr + 77] float32: noise at amplitude 0.3; weaker noise plus one tone in the lowest and one in the highest octave
    of the row's range."""
    c = CASES[case]
    L = 2 * c.sr + 77
    rng = np.random.default_rng(2000 + ALL.index(case))       # (a seed whose noise clip meets ROW_PEAK in every row)
    freqs = O.cqt_frequencies(c.n_bins, c.fmin or O.note_c1_hz(), c.bpo, c.tuning)
    f_lo = min(freqs[0] * 2.0 ** 0.4, freqs[-1])
    f_hi = max(freqs[-1] / 2.0 ** 0.4, freqs[0])
    t = np.arange(L) / c.sr
    noise = 0.3 * rng.standard_normal(L)
    tones = 0.05 * rng.standard_normal(L) + 0.3 * np.sin(2 * np.pi * f_lo * t) + 0.2 * np.sin(2 * np.pi * f_hi * t + 1.0)
    return np.stack([noise, tones]).astype(np.float32)


def oracle(case, x):
    return O.cqt(np.asarray(x, dtype=np.float64), CASES[case].sr, **kwargs(CASES[case]))


@functools.lru_cache(maxsize=None)
def oracle_clips(case):
    x = clips(case)
    return oracle(case, x[0]), oracle(case, x[1])


def device(case, x, **over):
    """ops.cqt of x [B, L] (host float32) under ops.override(**over) -> complex128 [B, n_bins, T]."""
    from sygnals_amd import ops
    with ops.override(**over):
        out = ops.cqt(ops.to_device_f32(x), CASES[case].sr, **kwargs(CASES[case]))
    return out


def cplx(t):
    a = t.cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def expected_calls(route):
    """(entry point, n_fft, n_filt) of every octave call ops.cqt makes for a cqt_route answer."""
    one, calls = route
    if one:
        return [(e, n_fft, n) for e, n_fft, n, _ in calls]
    out = []
    for e, n_fft, n, tiles in calls:
        if e == "syg_cqt_octave_f32":
            groups = [(e, n_fft, min(24, n - g)) for g in range(0, n, 24)]
            assert len(groups) == tiles
            out += groups
        elif e is not None:
            out.append((e, n_fft, n))
    return out


class Spy:
    """Records (entry point, n_fft, n_filt) of the CQT calls made through ops.lib()."""
    ARGS = {"syg_cqt_octave_f32": (4, 9), "syg_cqt_octave_gemm_f32": (4, 8), "syg_cqt_octave_bf16x3_f32": (4, 8),
            "syg_cqt_fused_f32": (None, 8)}

    def __init__(self, lib):
        self.lib, self.calls, self.decimations = lib, [], []

    def __getattr__(self, name):
        real = getattr(self.lib, name)
        if name.startswith("syg_decimate2"):
            self.decimations.append(name)
        if name not in self.ARGS:
            return real
        i_fft, i_filt = self.ARGS[name]

        def wrapped(*a):
            self.calls.append((name, 256 if i_fft is None else a[i_fft], a[i_filt]))
            return real(*a)
        return wrapped


@pytest.fixture()
def spy(monkeypatch):
    from sygnals_amd import ops
    s = Spy(ops.lib())
    monkeypatch.setattr(ops, "lib", lambda: s)
    return s


def route_of(case, mode, fused=True):
    from sygnals_amd._cqt import CqtPlan, cqt_route
    c = CASES[case]
    return cqt_route(CqtPlan(c.sr, c.hop, c.fmin, c.n_bins, c.bpo, c.tuning, c.filter_scale, c.sparsity), mode, fused)


@pytest.mark.parametrize("case,mode", _mode_pairs())
def test_parity_with_oracle(case, mode, spy):
    """The two 2 s clips as one batch against the float64 oracle at TOL, in every mode whose routing differs; the calls made
    are those of the routing function.  No row may hide behind the peak: on the ORACLE's output of the noise clip every
    row's own peak is >= ROW_PEAK of the global peak, so TOL of the global peak is <= 5 TOL of any row's.  In the default
    mode also the short clips: 3000 samples (parity) and one sample (shape, finiteness)."""
    x = clips(case)
    ref = oracle_clips(case)
    rows = np.abs(ref[0]).max(axis=1) / np.abs(ref[0]).max()
    print(f"cqt-params {case} {mode}: weakest row peak of the noise clip {rows.min():.3f} of the global peak")
    assert rows.min() >= ROW_PEAK
    got = cplx(device(case, x, cqt_mode=mode))
    want = route_of(case, mode)
    assert spy.calls == expected_calls(want), (spy.calls, want)
    assert want[1] == ([("syg_cqt_fused_f32", 256, CASES[case].bpo, 2)] if want[0] else ROUTES[case][2 + MODES.index(mode)])
    assert got.shape == (2,) + ref[0].shape and np.isfinite(got).all()
    errs = [peak_rel(got[i], ref[i]) for i in range(2)]
    row_err = float((np.abs(got[0] - ref[0]).max(axis=1) / np.abs(ref[0]).max(axis=1)).max())
    print(f"cqt-params {case} {mode} {'one-launch' if want[0] else sorted(set(want[1]))}: peak_rel noise {errs[0]:.3e} "
          f"tones {errs[1]:.3e}; worst row of the noise clip relative to its own peak {row_err:.3e}")
    assert max(errs) <= TOL                       # (with the row peaks above: row_err <= 5 TOL)
    if mode == "bf16x3":
        short = x[:1, 5000:8000]
        ref_s = oracle(case, short[0])
        got_s = cplx(device(case, short))
        assert got_s.shape == (1,) + ref_s.shape and np.isfinite(got_s).all()
        e = peak_rel(got_s[0], ref_s)
        print(f"cqt-params {case} {mode}: peak_rel 3000 samples {e:.3e}")
        assert e <= TOL
        one = np.full((1, 1), 0.25, dtype=np.float32)
        got_1 = cplx(device(case, one))
        assert got_1.shape == (1,) + oracle(case, one[0]).shape and np.isfinite(got_1).all()


@pytest.mark.parametrize("mode", MODES)
def test_refused_before_any_launch(mode, spy):
    """36 bins per octave at filter scale 2: octave frames of 2048 samples, which no kernel takes (the rfft form's eight
    transforms per workgroup stop fitting the LDS at 1024) -- ops.cqt says so, naming the parameters, and launches nothing."""
    from sygnals_amd import ops
    x = ops.to_device_f32(clips("bpo36")[:, :20000])
    with ops.override(cqt_mode=mode):
        with pytest.raises(ValueError, match=r"bins_per_octave=36 with filter_scale=2 needs an octave frame length of 2048"):
            ops.cqt(x, 48000, n_bins=252, bins_per_octave=36, filter_scale=2.0)
    assert spy.calls == [] and spy.decimations == []


@pytest.mark.parametrize("case", ONE_LAUNCH)
def test_one_launch_against_level_by_level(case, spy):
    """Wherever the one-launch form is taken (8, 12 and 16 filters, tuning, sparsity 0): the level-by-level kernels on the same
    operands to ONE_LAUNCH_TOL of the peak, both against the oracle at TOL; a batch, an odd row stride, short clips."""
    x = clips(case)
    ref = oracle_clips(case)
    a = cplx(device(case, x))
    assert spy.calls == [("syg_cqt_fused_f32", 256, CASES[case].bpo)]
    spy.calls.clear()
    b = cplx(device(case, x, cqt_fused=False))
    assert spy.calls == expected_calls(route_of(case, "bf16x3", fused=False)) and len(spy.calls) == 7
    assert a.shape == b.shape == (2,) + ref[0].shape
    d = float(np.abs(a - b).max() / np.abs(b).max())
    ea, eb = max(peak_rel(a[i], ref[i]) for i in range(2)), max(peak_rel(b[i], ref[i]) for i in range(2))
    print(f"cqt-params {case}: one-launch vs level-by-level {d:.3e}; peak_rel one-launch {ea:.3e} level-by-level {eb:.3e}")
    assert d <= ONE_LAUNCH_TOL
    assert ea <= TOL and eb <= TOL
    for L in (1, 511, 3000, 70001):
        xs = x[:, :L]
        a, b = cplx(device(case, xs)), cplx(device(case, xs, cqt_fused=False))
        assert a.shape == b.shape and np.isfinite(a).all()
        assert np.abs(a - b).max() <= ONE_LAUNCH_TOL * np.abs(b).max() + 1e-30, L


@pytest.mark.parametrize("B,L", [(1, 40000), (2, 40000), (2, 40001), (1, 3000)])
@pytest.mark.parametrize("case", STAGED)
def test_staged_frames_identical(case, B, L):
    """cqt_bf16x3_staged_kernel (a wave splits the sample run of its 16-frame tile once, in LDS) and the per-frame kernel: the
    same operands and the same order of matrix instructions per accumulator, so identical bits -- here for the
    instantiations <128,2>, <128,1>, <256,1> (eight, seven, five filters and one), and for hops that are not powers of two
    (80 / 40 / 20, 48 / 24 / 12: slot skews and two-copy planes of their own).  40000 samples: level lengths 20000 ... 625, row
    strides that are and are not multiples of four (a batch takes the staged form only where they are)."""
    x = np.tile(clips(case)[:1], (B, 1))[:, :L].copy()
    if B == 2:
        x[1] = clips(case)[1, :L]
    assert {e for e, *_ in route_of(case, "bf16x3", fused=False)[1]} >= {"syg_cqt_octave_bf16x3_f32"}
    a2 = device(case, x, cqt_fused=False, cqt_staged=2)
    a1 = device(case, x, cqt_fused=False, cqt_staged=1)
    a0 = device(case, x, cqt_fused=False, cqt_staged=0)
    assert a2.shape == a0.shape and torch.equal(a2, a0) and torch.equal(a1, a0)
    assert torch.isfinite(a0).all()


@pytest.mark.parametrize("case", ["tune+.37", "fs0.5", "dense", "bpo24"])
def test_through_the_mirror(case):
    """compute_cqt with tuning / filter_scale / sparsity / bins_per_octave: the ops.cqt result for the same arguments, as
    complex128 [n_bins, T]."""
    from sygnals_amd.core.dsp import compute_cqt
    c = CASES[case]
    y = clips(case)[1, :c.sr + 5]
    extra = {"tune+.37": dict(tuning=c.tuning), "fs0.5": dict(filter_scale=c.filter_scale), "dense": dict(sparsity=c.sparsity),
             "bpo24": {}}[case]
    assert extra or c.bpo != 12
    C = compute_cqt(y, c.sr, hop_length=c.hop, fmin=c.fmin, n_bins=c.n_bins, bins_per_octave=c.bpo,
                    res_type="kaiser_halfband", **extra)
    want = cplx(device(case, y[None]))[0]
    assert C.dtype == np.complex128 and C.shape == (c.n_bins, 1 + len(y) // c.hop)
    assert np.array_equal(C, want)
    ref = oracle(case, y)
    e = peak_rel(C, ref)
    print(f"cqt-params {case}: compute_cqt peak_rel {e:.3e}")
    assert e <= TOL
    # the keyword matters: the untuned / default transform is another one
    if extra:
        assert peak_rel(C, O.cqt(y.astype(np.float64), c.sr, hop_length=c.hop, fmin=c.fmin, n_bins=c.n_bins,
                                 bins_per_octave=c.bpo)) > 100 * TOL


@pytest.mark.parametrize("case", ALL)
def test_repeat_and_batch(case):
    """Two calls give identical bits; a row of a batch is the single-clip call, bit for bit -- for a batch whose row stride
    is a multiple of four and for one where it is not (the staged kernels and the decimator's 16-byte loads take another
    branch there)."""
    full = clips(case)
    for L in (30000, 30001, 30002):
        x = full[:, 1000:1000 + L].copy()
        a = device(case, x)
        assert torch.equal(a, device(case, x))
        for i in range(2):
            assert torch.equal(a[i], device(case, x[i:i + 1])[0]), (L, i)
        assert torch.isfinite(a).all()
