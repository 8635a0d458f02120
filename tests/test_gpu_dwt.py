"""Device wavelet transform (syg_dwt_f32 / syg_idwt_f32, ops.dwt / ops.idwt and the mirrors of core/transforms.py) against
the float64 restatement tests/dwt_ref.py.

Gate of the forward transform: for the arrays of level l, |device - reference| <= 1e-5 max|a_(l-1)|, a_(l-1) being the
restatement's input to that level (a_0 = x): a detail band of a smooth signal is a cancellation, so its float32 error
follows the level's input, not the near-zero result.  The inverse is held to 1e-5 of the peak of the signal."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import dwt_ref as R
from tests.gpu_util import assert_parity

pytestmark = pytest.mark.gpu

TOL = 1e-5
WAVELETS = ("haar", "db2", "db4", "db10")
LENGTHS = (1, 2, 3, 7, 8, 15, 16, 17, 255, 256, 257, 1000, 4097)
TILE = 1024                                     # outputs (pairs, for the inverse) a workgroup of the streaming kernels
WORST = {"dwt": 0.0, "idwt": 0.0}


def _flen(wavelet):
    return R.wavelet_filters(wavelet)[0].size


@functools.lru_cache(maxsize=None)
def _signals(L, rows=3):
    """float32 rows: seeded noise, a chirp, other noise, ..."""
    rng = np.random.default_rng(7000 + L)
    t = np.arange(L) / max(L, 1)
    chirp = np.sin(2 * np.pi * (2.0 * t + 0.5 * (0.2 * L) * t * t) + 0.3)
    X = np.stack([chirp if r == 1 else rng.standard_normal(L) for r in range(rows)]).astype(np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=256)
def _chain(L, wavelet, mode, nmax, rows=3):
    """The restatement on every row of _signals(L): per row (a[0 ... nmax], d[1 ... nmax])."""
    out = []
    for x in _signals(L, rows).astype(np.float64):
        a, d = [x], [None]
        for _ in range(nmax):
            ca, cd = R.dwt(a[-1], wavelet, mode)
            a.append(ca)
            d.append(cd)
        out.append((a, d))
    return out


def _levels(L, wavelet):
    mx = max(1, R.dwt_max_level(L, _flen(wavelet)))
    return sorted({1, mx, mx + 2})


def _quiet_dwt(y, wavelet, level, mode):
    from sygnals_amd import ops
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)           # a level above the maximum warns
        return ops.dwt(y, wavelet, level, mode)


def _check_forward(packed, lens, chain_rows, level, what):
    got = packed.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    for r, (a, d) in enumerate(chain_rows):
        want = [a[level]] + [d[l] for l in range(level, 0, -1)]
        scale = [np.max(np.abs(a[level - 1]))] + [np.max(np.abs(a[l - 1])) for l in range(level, 0, -1)]
        assert lens == [w.size for w in want], (what, lens)
        off = 0
        for w, s, n in zip(want, scale, lens):
            err = float(np.max(np.abs(got[r, off:off + n] - w)))
            ratio = err / s if s > 0 else err
            if ratio > WORST["dwt"]:
                WORST["dwt"] = ratio
                print(f"dwt worst so far {ratio:.3e} ({what}, row {r})")
            assert err <= TOL * s + 1e-30, f"{what}, row {r}: {err:.3e} > 1e-5 * {s:.3e}"
            off += n
        assert off == got.shape[1]


def _dev_rows(L, B, strided=False):
    """B rows of _signals(L) on the device (B = 1: the chirp); strided: a row stride larger than L."""
    X = _signals(L)
    rows = [1] if B == 1 else list(range(B))
    if strided:
        buf = torch.full((len(rows), L + 5), 7.0, dtype=torch.float32, device="cuda")
        buf[:, :L] = torch.from_numpy(X[rows].copy()).cuda()
        return buf[:, :L], rows
    return torch.from_numpy(X[rows].copy()).cuda(), rows


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_forward_parity(wavelet, mode, L):
    """B in {1, 3} (B = 3 with a row stride larger than L), levels 1, the maximum and the maximum + 2.  With db10 the
    lengths below 19 need the extension several times over."""
    levels = _levels(L, wavelet)
    chain = _chain(L, wavelet, mode, levels[-1])
    for B in (1, 3):
        y, rows = _dev_rows(L, B, strided=(B == 3))
        assert B == 1 or y.stride(0) == L + 5
        for level in levels:
            packed, lens = _quiet_dwt(y, wavelet, level, mode)
            assert packed.dtype == torch.float32 and packed.is_cuda and packed.shape == (B, sum(lens))
            _check_forward(packed, lens, [chain[r] for r in rows], level, f"{wavelet} {mode} L={L} B={B} level={level}")


def _tile_lengths(wavelet):
    """L one below, at and one above every multiple of the streaming tile that the outputs of a level reach."""
    F = _flen(wavelet)
    Ls = {2 * TILE - 1, 2 * TILE, 2 * TILE + 1}                 # the tile's input span
    for K in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):          # K outputs: L = 2 K - F + 1 and one more
        Ls.update({2 * K - F + 1, 2 * K - F + 2})
    for M in (TILE - 1, TILE, TILE + 1):                        # M output pairs of the inverse: K = M + F / 2 - 1
        Ls.add(2 * (M + F // 2 - 1) - F + 1)
    return sorted(Ls)


@pytest.mark.parametrize("wavelet", WAVELETS)
def test_streaming_form_around_its_tile(wavelet):
    """One launch per level (dwt_form = 0), forward and back, at lengths around the 1024-output tile."""
    from sygnals_amd import ops
    for L in _tile_lengths(wavelet):
        mx = max(1, R.dwt_max_level(L, _flen(wavelet)))
        for mode in ("symmetric", "periodic"):
            chain = _chain(L, wavelet, mode, mx, 2)
            y = torch.from_numpy(_signals(L, 2).copy()).cuda()
            for level in (1, mx):
                with ops.override(dwt_form=0):
                    assert not ops.dwt_fits(L, wavelet, level)
                    packed, lens = ops.dwt(y, wavelet, level, mode)
                    back = ops.idwt(packed, lens, wavelet, mode)
                _check_forward(packed, lens, chain, level, f"streaming {wavelet} {mode} L={L} level={level}")
                resident, lens2 = ops.dwt(y, wavelet, level, mode)
                assert lens2 == lens and torch.equal(resident, packed), "the two forms differ"
                assert torch.equal(ops.idwt(packed, lens, wavelet, mode), back), "the two inverse forms differ"
                _check_back(back, _signals(L, 2), f"streaming round trip {wavelet} {mode} L={L} level={level}")


def _check_back(y, want, what):
    got = y.cpu().numpy().astype(np.float64)
    L = want.shape[1]
    assert got.shape[1] in (L, L + 1), what
    for r in range(want.shape[0]):
        w = want[r].astype(np.float64)
        pk = np.max(np.abs(w))
        ratio = float(np.max(np.abs(got[r, :L] - w)) / (pk if pk > 0 else 1.0))
        if ratio > WORST["idwt"]:
            WORST["idwt"] = ratio
            print(f"idwt worst so far {ratio:.3e} ({what}, row {r})")
        assert_parity(got[r, :L], w, TOL, what)


def _fit_limit(wavelet):
    from sygnals_amd import ops
    lo, hi = 1, 1 << 20                          # fits(lo), not fits(hi); the rule is monotone in L
    assert ops.dwt_fits(lo, wavelet) and not ops.dwt_fits(hi, wavelet)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ops.dwt_fits(mid, wavelet) else (lo, mid)
    return lo


@pytest.mark.parametrize("over", (0, 1))
@pytest.mark.parametrize("wavelet", ("haar", "db4", "db10"))
def test_at_the_fit_limit_and_one_above(wavelet, over):
    """The longest row the clip-resident kernel takes (all 160 KiB of LDS) and the shortest one the streaming form takes
    (one pass, then the clip-resident kernel on what is left), forward and back."""
    from sygnals_amd import ops
    L = _fit_limit(wavelet) + over
    assert 50000 < L < 60000 and ops.dwt_fits(L, wavelet) == (over == 0)
    level = min(10, R.dwt_max_level(L, _flen(wavelet)))
    y = torch.from_numpy(_signals(L, 2).copy()).cuda()
    for mode in ("symmetric", "reflect"):
        chain = _chain(L, wavelet, mode, level, 2)
        packed, lens = ops.dwt(y, wavelet, level, mode)
        _check_forward(packed, lens, chain, level, f"fit limit + {over} {wavelet} {mode} L={L}")
        _check_back(ops.idwt(packed, lens, wavelet, mode), _signals(L, 2), f"fit limit + {over} round trip {wavelet} L={L}")


@pytest.mark.parametrize("mode", ("symmetric", "periodic"))
def test_long_row_through_the_streaming_form(mode):
    from sygnals_amd import ops
    L = 200001
    level = R.dwt_max_level(L, 8)
    assert level == 14 and not ops.dwt_fits(L, "db4")
    chain = _chain(L, "db4", mode, level, 1)
    y = torch.from_numpy(_signals(L, 1).copy()).cuda()
    packed, lens = ops.dwt(y, "db4", level, mode)
    _check_forward(packed, lens, chain, level, f"long row {mode}")
    assert ops.idwt(packed, lens, "db4", mode).shape == (1, L + 1)
    packed10, lens10 = ops.dwt(y, "db4", 10, mode)
    _check_back(ops.idwt(packed10, lens10, "db4", mode), _signals(L, 1), f"long row round trip {mode}, 10 levels")


def test_non_contiguous_input_is_made_contiguous():
    from sygnals_amd import ops
    L = 1000
    X = _signals(L)
    wide = torch.zeros((3, 2 * L), dtype=torch.float32, device="cuda")
    wide[:, ::2] = torch.from_numpy(X.copy()).cuda()
    view = wide[:, ::2]
    assert view.stride(1) == 2
    packed, lens = ops.dwt(view, "db4", 3, "symmetric")
    _check_forward(packed, lens, _chain(L, "db4", "symmetric", 3), 3, "non-contiguous")
    cols = packed.t().contiguous().t()            # coefficients with a stride along the row
    assert cols.stride(1) != 1
    _check_back(ops.idwt(cols, lens, "db4"), X, "non-contiguous coefficients")


@pytest.mark.parametrize("wavelet", WAVELETS)
def test_inverse_on_the_restatement_coefficients(wavelet):
    """ops.idwt on the restatement's coefficients (rounded to float32) against the restatement's waverec of those."""
    from sygnals_amd import ops
    for L in LENGTHS:
        for mode in ("symmetric", "periodic", "zero"):
            for level in _levels(L, wavelet):
                rows, lens = [], None
                want = []
                for x in _signals(L).astype(np.float64):
                    c32 = [c.astype(np.float32) for c in R.wavedec(x, wavelet, level=level, mode=mode)]
                    lens = [c.size for c in c32]
                    rows.append(np.concatenate(c32))
                    want.append(R.waverec([c.astype(np.float64) for c in c32], wavelet))
                y = ops.idwt(torch.from_numpy(np.stack(rows)).cuda(), lens, wavelet, mode)
                assert y.dtype == torch.float32 and y.shape == (3, want[0].size) and want[0].size in (L, L + 1)
                got = y.cpu().numpy()
                for r in range(3):
                    assert_parity(got[r], want[r], TOL, f"idwt {wavelet} {mode} L={L} level={level} row {r}")


@pytest.mark.parametrize("wavelet", WAVELETS)
def test_device_round_trip(wavelet):
    from sygnals_amd import ops
    for L in LENGTHS:
        for mode in R.MODES:
            for level in _levels(L, wavelet):
                if level > 10:
                    continue
                for B in (1, 3):
                    y, rows = _dev_rows(L, B)
                    packed, lens = _quiet_dwt(y, wavelet, level, mode)
                    _check_back(ops.idwt(packed, lens, wavelet, mode), _signals(L)[rows],
                                f"round trip {wavelet} {mode} L={L} B={B} level={level}")


def test_inverse_trims_a_longer_approximation_and_refuses_other_mismatches():
    from sygnals_amd import ops
    rng = np.random.default_rng(5)
    a = rng.standard_normal((2, 41)).astype(np.float32)
    d2 = rng.standard_normal((2, 40)).astype(np.float32)
    d1 = rng.standard_normal((2, 75)).astype(np.float32)          # level 2 gives 2 * 40 - 8 + 2 = 74: no trim there
    with pytest.raises(ValueError, match="mismatch"):
        ops.idwt(torch.from_numpy(np.concatenate([a, d2, d1], axis=1)).cuda(), [41, 40, 75], "db4")
    d1 = d1[:, :73]                                               # 74 = 73 + 1: trimmed again
    y = ops.idwt(torch.from_numpy(np.concatenate([a, d2, d1], axis=1)).cuda(), [41, 40, 73], "db4").cpu().numpy()
    assert y.shape == (2, 2 * 73 - 8 + 2)
    for r in range(2):
        want = R.waverec([a[r].astype(np.float64), d2[r].astype(np.float64), d1[r].astype(np.float64)], "db4")
        assert_parity(y[r], want, TOL, "trimmed approximation")
    for lens in ([43, 40, 73], [39, 40, 73], [41, 40, 71]):
        with pytest.raises(ValueError, match="mismatch"):
            ops.idwt(torch.zeros((2, sum(lens)), dtype=torch.float32, device="cuda"), lens, "db4")
    with pytest.raises(ValueError, match="adds up"):
        ops.idwt(torch.zeros((2, 100), dtype=torch.float32, device="cuda"), [41, 40, 73], "db4")


def test_refusals_and_level_rules():
    from sygnals_amd import ops
    y = torch.from_numpy(_signals(1000).copy()).cuda()
    with pytest.raises(ValueError, match="wavelets served are"):
        ops.dwt(y, "sym5")
    with pytest.raises(ValueError, match="modes served are"):
        ops.dwt(y, "db4", 2, "periodization")
    with pytest.raises(ValueError, match="modes served are"):
        ops.idwt(y, [500, 500], "haar", "smooth")
    for level in (0, -2, 1.5):
        with pytest.raises(ValueError, match="integer >= 1"):
            ops.dwt(y, "db4", level)
    with pytest.raises(ValueError):
        ops.dwt(y.double(), "db4")
    with pytest.warns(UserWarning, match="too high"):
        packed, lens = ops.dwt(y, "db4", 9)
    assert len(lens) == 10
    packed, lens = ops.dwt(y, "db4")                               # level=None: the maximum
    assert len(lens) == 1 + R.dwt_max_level(1000, 8) == 8
    packed, lens = ops.dwt(y[:, :5], "db4")                        # maximum 0 -> one level
    assert lens == [6, 6]


def test_mirrors_of_core_transforms():
    from sygnals_amd.core import transforms as TR
    x = _signals(1000)[0].astype(np.float64)
    c = TR.discrete_wavelet_transform(x)                           # db4, maximum level, symmetric
    want = R.wavedec(x, "db4")
    assert isinstance(c, list) and len(c) == len(want) == 8
    ins = R.level_inputs(x, "db4", 7)
    for i, (g, w) in enumerate(zip(c, want)):
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == w.shape
        lev = 7 if i == 0 else 8 - i
        assert np.max(np.abs(g - w)) <= TOL * np.max(np.abs(ins[lev - 1]))
    c = TR.discrete_wavelet_transform(x, wavelet="haar", level=2, mode="periodic")
    assert [a.size for a in c] == [250, 250, 500]
    back = TR.inverse_discrete_wavelet_transform(c, "haar", mode="periodic")
    assert back.dtype == np.float64 and back.shape == (1000,)
    assert_parity(back, x, TOL, "inverse mirror")
    with pytest.raises(ValueError, match="1D"):
        TR.discrete_wavelet_transform(np.zeros((2, 8)))
    for level in (0, -1, 2.0):
        with pytest.raises(ValueError, match="Decomposition level must be an integer >= 1"):
            TR.discrete_wavelet_transform(x, level=level)
    with pytest.raises(ValueError, match="Invalid wavelet name 'sym5'"):
        TR.discrete_wavelet_transform(x, wavelet="sym5")
    with pytest.raises(ValueError, match="wavelets served are"):
        TR.discrete_wavelet_transform(x, wavelet="sym5", level=2)
    for bad in ([c[0]], (c[0], c[1]), "abc"):
        with pytest.raises(ValueError, match="at least cA and cD"):
            TR.inverse_discrete_wavelet_transform(bad, "haar")
    with pytest.raises(ValueError, match="mismatch"):
        TR.inverse_discrete_wavelet_transform([np.zeros(5), np.zeros(9)], "haar")
    # the batched forms stay on the device
    y = torch.from_numpy(_signals(1000).copy()).cuda()
    packed, lens = TR.dwt_batch(y, "db2", 3, "reflect")
    assert packed.is_cuda and packed.shape == (3, sum(lens))
    _check_forward(packed, lens, _chain(1000, "db2", "reflect", 3), 3, "dwt_batch")
    yb = TR.idwt_batch(packed, lens, "db2", "reflect")
    assert yb.is_cuda
    _check_back(yb, _signals(1000), "idwt_batch")


def test_plugin_registers_both_transforms():
    from sygnals_amd.core import transforms as TR
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin

    class Registry:
        def __init__(self):
            self.transforms = {}

        def add_transform(self, name, fn):
            self.transforms[name] = fn
    reg = Registry()
    SygnalsAmdPlugin().register_transforms(reg)
    assert reg.transforms["discrete_wavelet_transform"] is TR.discrete_wavelet_transform
    assert reg.transforms["inverse_discrete_wavelet_transform"] is TR.inverse_discrete_wavelet_transform
    x = _signals(256)[1].astype(np.float64)
    c = reg.transforms["discrete_wavelet_transform"](x, "db2", 2)
    assert_parity(reg.transforms["inverse_discrete_wavelet_transform"](c, "db2"), x, TOL, "through the registry")
