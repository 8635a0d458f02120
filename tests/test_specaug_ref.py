"""The SpecAugment restatement (tests/specaug_ref.py) holds what the definition states, its segment resize equals torch's
linear interpolate on the CPU, and the host twin sygnals_amd/_specaug.py draws the same integers from different code.
No device."""
import numpy as np
import pytest
import torch

from sygnals_amd import _specaug as SA
from tests import rng_ref
from tests import specaug_ref as R

PAIRS = [(1, 1), (1, 5), (5, 1), (2, 3), (3, 2), (7, 7), (13, 29), (64, 65), (65, 64), (257, 100), (1000, 997)]
SEED = 0x5EC0A06D3A7F1234


def test_stream_and_item_layout():
    assert SA.STREAM_SPEC == R.STREAM == 2 and (SA.Q_WARP, SA.Q_FREQ, SA.Q_TIME) == (0, 1, 17) and SA.MAX_MASKS == 16
    # an item is ONE call of (seed, row) in stream 2: other streams and other items give other words
    w = rng_ref.words(SEED, 5, [0, 1, 17], stream=2)
    assert len({tuple(r) for r in w}) == 3 and not np.array_equal(w[0], rng_ref.words(SEED, 5, [0], stream=1)[0])


def test_draw_range_ends_and_zero():
    assert R.draw(0xFFFFFFFF, 0) == 0 and R.draw(0, 0) == 0 and int(SA.draw(np.uint32(0xFFFFFFFF), 0)) == 0
    words = rng_ref.words(SEED, 0, np.arange(2000), stream=2).reshape(-1)
    for n in (1, 2, 3, 5, 17):
        got = {R.draw(w, n) for w in words}
        assert got == set(range(n)), f"draw(w, {n}) reaches {sorted(got)}"
    for n in (1, 7, 1 << 20, (1 << 31) + 1):
        assert R.draw(0xFFFFFFFF, n) == n - 1 and R.draw(0, n) == 0
        assert int(SA.draw(np.uint32(0xFFFFFFFF), n)) == n - 1
    assert np.array_equal(SA.draw(words[:500], 12345), [R.draw(w, 12345) for w in words[:500]])


def test_every_draw_in_its_range_over_2000_rows():
    K, T, nf, F, nt, Wt, p, W = 5, 9, 2, 3, 2, 4, 0.5, 2
    ds = R.draws(SEED, 0, 2000, K, T, None, nf, F, nt, Wt, p, W)
    c, w = R.stack_params(ds, "c")[:, 0], R.stack_params(ds, "w")[:, 0]
    f, f0, t, t0 = (R.stack_params(ds, k) for k in ("f", "f0", "t", "t0"))
    assert c.min() == W and c.max() == T - W - 1                                # W <= c < T - W, both ends
    assert np.all((w >= c - W + 1) & (w <= c + W)) and w.min() >= 1 and w.max() <= T - 1
    assert (w - c).min() == -W + 1 and (w - c).max() == W
    assert f.min() == 0 and f.max() == F and np.all(f0 >= 0) and np.all(f0 + f <= K)
    assert f0[f == 0].max() == K and f0.min() == 0
    We = min(Wt, int(np.floor(p * T)))
    assert We == 4 and t.min() == 0 and t.max() == We and np.all(t0 >= 0) and np.all(t0 + t <= T)
    assert t0[t == 0].max() == T and t0.min() == 0


def test_time_ratio_caps_the_width():
    ds = R.draws(SEED, 0, 400, 4, 50, None, 0, 0, 3, 40, 0.1, 0)
    t = R.stack_params(ds, "t")
    assert t.max() == 5 and t.min() == 0                                        # floor(0.1 * 50) = 5 < 40


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_resize_equals_torch_linear(n_in, n_out):
    rng = np.random.default_rng(n_in * 1009 + n_out)
    x = rng.standard_normal((3, n_in))
    want = torch.nn.functional.interpolate(torch.from_numpy(x)[None], size=n_out, mode="linear", align_corners=False)[0].numpy()
    got = R.resize(x, n_out)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(x)))
    print(f"resize {n_in} -> {n_out}: {err:.2e} of the peak")
    assert err <= 1e-12
    assert got.shape == (3, n_out)


def test_resize_neighbours_stay_inside_the_segment():
    # a segment placed between NaNs: a neighbour outside would show
    for n_in, n_out in PAIRS:
        x = np.full((1, n_in + 2), np.nan)
        x[0, 1:-1] = np.arange(n_in)
        assert np.isfinite(R.resize(x[:, 1:-1], n_out)).all()


def test_warp_with_w_equal_c_is_the_identity():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 37))
    for c in (1, 5, 18, 36):
        assert np.array_equal(R.warp(x, c, c, 37), x)
    y = R.warp(x, 10, 14, 30)                                                   # frames past T_b are kept
    assert np.array_equal(y[:, 30:], x[:, 30:]) and not np.array_equal(y[:, :30], x[:, :30])
    assert np.array_equal(y[:, 0], x[:, 0])                                     # a stretched segment starts on its first frame


def test_short_clips_are_not_warped():
    W = 5
    x = np.random.default_rng(4).standard_normal((4, 3, 40))
    lengths = [1, W, 2 * W, 2 * W + 1]
    y, _, ds = R.apply(x, SEED, nf=0, nt=0, W=W, lengths=lengths)
    assert [d["c"] >= 0 for d in ds] == [False, False, False, True]
    assert np.array_equal(y[:3], x[:3]) and ds[3]["c"] == W                     # T_b = 2W + 1: the one centre
    p = SA.params(SEED, 0, 4, 3, 40, lengths, 0, 0, 0, 0, 1.0, W)
    assert list(p["c"]) == [-1, -1, -1, W] and list(p["w"][:3]) == [-1, -1, -1]


@pytest.mark.parametrize("B,K,T,nf,F,nt,Wt,p,W,first_row", [
    (33, 13, 65, 2, 13, 2, 100, 1.0, 5, 0),
    (7, 80, 3001, 16, 27, 16, 100, 0.2, 40, 123456),
    (64, 1, 2, 1, 1, 1, 2, 1.0, 1, (1 << 31) - 64),
    (9, 129, 257, 0, 0, 3, 300, 0.03, 0, 7),
])
def test_host_twin_equals_the_restatement(B, K, T, nf, F, nt, Wt, p, W, first_row):
    lengths = None if B == 33 else [1 + (b * 7919) % T for b in range(B)]
    ds = R.draws(SEED, first_row, B, K, T, lengths, nf, F, nt, Wt, p, W)
    got = SA.params(SEED, first_row, B, K, T, lengths, nf, F, nt, Wt, p, W)
    assert np.array_equal(got["c"], R.stack_params(ds, "c")[:, 0]) and np.array_equal(got["w"], R.stack_params(ds, "w")[:, 0])
    for k in ("f", "f0"):
        assert got[k].shape == (B, nf) and np.array_equal(got[k], R.stack_params(ds, k))
    for k in ("t", "t0"):
        assert got[k].shape == (B, nt) and np.array_equal(got[k], R.stack_params(ds, k))
    assert all(v.dtype == np.int64 for v in got.values())
    # a batch equals its clips through first_row
    one = SA.params(SEED, first_row + B - 1, 1, K, T, None if lengths is None else lengths[-1:], nf, F, nt, Wt, p, W)
    assert all(np.array_equal(one[k][0], got[k][-1]) for k in got)


def test_masks_are_a_union():
    x = np.random.default_rng(5).standard_normal((20, 13, 65)) + 10.0
    y, m, ds = R.apply(x, SEED, nf=3, F=6, nt=3, Wt=20, mask_value=-7.5)
    for b, d in enumerate(ds):
        want = np.zeros((13, 65), dtype=bool)
        for f, f0 in zip(d["f"], d["f0"]):
            want |= ((np.arange(13) >= f0) & (np.arange(13) < f0 + f))[:, None]
        for t, t0 in zip(d["t"], d["t0"]):
            want |= ((np.arange(65) >= t0) & (np.arange(65) < t0 + t))[None, :]
        assert np.array_equal(m[b], want)
    assert np.all(y[m] == -7.5) and np.array_equal(y[~m], x[~m]) and 0 < m.mean() < 1
    assert any(m[b].sum() < sum(f * 65 for f in d["f"]) + sum(t * 13 for t in d["t"]) for b, d in enumerate(ds))   # overlaps exist


def test_lengths_confine_every_draw_and_write():
    B, K, T = 200, 6, 50
    lengths = [1 + (b * 31) % T for b in range(B)]
    x = np.random.default_rng(6).standard_normal((B, K, T))
    y, m, ds = R.apply(x, SEED, nf=2, F=6, nt=4, Wt=60, W=3, mask_value="mean", lengths=lengths)
    for b, d in enumerate(ds):
        Tb = lengths[b]
        assert all(0 <= t0 and t0 + t <= Tb for t, t0 in zip(d["t"], d["t0"]))
        assert not m[b][:, Tb:].any() and np.array_equal(y[b][:, Tb:], x[b][:, Tb:])
        if d["c"] >= 0:
            assert 3 <= d["c"] < Tb - 3 and 1 <= d["w"] <= Tb - 1
        else:
            assert Tb <= 6
        if m[b].any():
            assert np.all(y[b][m[b]] == np.mean(x[b][:, :Tb]))


def test_all_off_is_a_copy():
    x = np.random.default_rng(7).standard_normal((3, 4, 9))
    y, m, _ = R.apply(x, SEED, nf=0, F=0, nt=0, Wt=0, W=0)
    assert np.array_equal(y, x) and not m.any()
    y, m, _ = R.apply(x, SEED, nf=4, F=0, nt=4, Wt=0, W=0)                      # widths zero: masks of no cells
    assert np.array_equal(y, x) and not m.any()
