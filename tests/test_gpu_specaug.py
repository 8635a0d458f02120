"""Device SpecAugment (syg_spec_augment_f32; ops.spec_augment, core.augment.spec_augment*) against the integer / float64
restatement of tests/specaug_ref.py.

Gates: masks bit for bit (the masked set, the mask value, every unmasked cell); "mean" within 2 float32 ulp of the
float64 mean rounded to float32; the warp |y - y_ref| <= 1e-5 max|x_b| per clip.  Every call writes into an `out` filled
with NaN, and the warp tests print their worst fraction of the gate."""
import numpy as np
import pytest
import torch

from sygnals_amd import _specaug as SA
from sygnals_amd import ops
from sygnals_amd.core import augment as A
from tests import specaug_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x5EC0A06D3A7F1234
VALUE = -3.25
# K in 1, 2, 13, 80, 129; T in 1, 2, 63, 64, 65, 257, 1025, 3001; B in 1, 3, 33: every value at least once, the tile of 4096
# cells missed, met and passed, clips whose cell count is no multiple of four
SHAPES = [(1, 1, 1), (3, 2, 2), (33, 13, 63), (3, 13, 64), (1, 80, 65), (3, 129, 257), (33, 1, 1025), (1, 13, 3001), (3, 80, 3001),
          (33, 129, 65), (1, 2, 1025), (3, 1, 64), (1, 64, 64), (3, 2, 63)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cpu(t):
    return t.cpu().numpy()


def nan_out(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits_of(v):
    """The bit pattern of one float32 as an int."""
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def bits_equal(a, b):
    return np.array_equal(bits(a), bits(b))


def clips(B, K, T, seed=0):
    """float32 [B, K, T], no cell equal to VALUE, a level per clip so that means differ."""
    rng = np.random.default_rng(seed + 131 * B + 17 * K + T)
    return (rng.standard_normal((B, K, T)) * 3.0 + rng.uniform(-20, 20, (B, 1, 1))).astype(np.float32)


def run(x, **kw):
    return cpu(ops.spec_augment(dev(x), SEED, out=nan_out(*x.shape), **kw))


def check_masks(x, got, kw, lengths=None):
    want, m, _ = R.apply(x, SEED, nf=kw.get("freq_masks", 2), F=kw.get("freq_width", 27), nt=kw.get("time_masks", 2),
                         Wt=kw.get("time_width", 100), p=kw.get("time_ratio", 1.0), mask_value=VALUE, lengths=lengths,
                         first_row=kw.get("first_row", 0))
    assert np.array_equal(bits(got) == bits_of(VALUE), m), "the masked set differs from the restatement's"
    assert bits_equal(got[~m], x[~m]), "an unmasked cell lost its bits"
    return m


# ---------------------------------------------------------------- masks only
@pytest.mark.parametrize("B,K,T", SHAPES)
def test_masks_only_bit_for_bit(B, K, T):
    x = clips(B, K, T)
    kw = dict(freq_masks=2, freq_width=min(27, K), time_masks=2, time_width=100, mask_value=VALUE)
    m = check_masks(x, run(x, **kw), kw)
    if K * T >= 64:
        assert m.any()


@pytest.mark.parametrize("kw", [
    dict(freq_masks=0, freq_width=0, time_masks=0, time_width=0),
    dict(freq_masks=1, freq_width=13, time_masks=0, time_width=0),                  # freq_width = K
    dict(freq_masks=0, freq_width=0, time_masks=1, time_width=5000),                # time_width >= T
    dict(freq_masks=16, freq_width=3, time_masks=16, time_width=9),
    dict(freq_masks=16, freq_width=0, time_masks=16, time_width=0),
    dict(freq_masks=2, freq_width=5, time_masks=3, time_width=200, time_ratio=0.05),    # the ratio caps the width at 12
    dict(freq_masks=2, freq_width=5, time_masks=2, time_width=30, first_row=(1 << 31) - 3),
], ids=lambda k: "-".join(str(v) for v in k.values()))
def test_counts_widths_and_ratio(kw):
    for B, K, T in ((3, 13, 257), (3, 13, 65)):
        x = clips(B, K, T, seed=1)
        got = run(x, mask_value=VALUE, **kw)
        m = check_masks(x, got, kw)
        if kw["freq_masks"] == 0 and kw["time_masks"] == 0 or (kw["freq_width"] == 0 and kw["time_width"] == 0):
            assert bits_equal(got, x) and not m.any()                               # all off: a copy
        if kw.get("time_ratio", 1.0) < 1.0 and T == 257:
            t = R.stack_params(R.draws(SEED, 0, B, K, T, None, 2, 5, 3, 200, 0.05, 0), "t")
            assert 0 < t.max() <= 12


def test_mask_value_bits_are_stored():
    x = clips(3, 13, 65, seed=2)
    for v in (0.0, -0.0, 1e-42, 3.4e38, np.float32(np.pi)):                         # signed zero, a subnormal, near the top
        got = run(x, freq_width=6, time_width=20, mask_value=float(v))
        _, m, _ = R.apply(x, SEED, F=6, Wt=20)
        assert m.any() and np.all(bits(got[m]) == bits_of(v)) and bits_equal(got[~m], x[~m])


def test_one_long_clip():
    T = 1 << 20
    x = clips(1, 1, T, seed=3)
    kw = dict(freq_masks=1, freq_width=0, time_masks=4, time_width=300000)
    check_masks(x, run(x, mask_value=VALUE, **kw), kw)
    got = run(x, time_masks=2, time_width=1000, freq_masks=0, freq_width=0, time_warp=40, mask_value="mean")
    want, m, ds = R.apply(x, SEED, nf=0, F=0, nt=2, Wt=1000, W=40, mask_value="mean")
    assert ds[0]["c"] >= 40 and ds[0]["w"] != ds[0]["c"]
    err = np.abs(got.astype(np.float64) - want)
    assert np.max(err[~m]) <= 1e-5 * np.max(np.abs(x))
    assert np.all(np.abs(bits(got[m]).astype(np.int64) - bits_of(R.clip_mean(x[0], T))) <= 2)


# ---------------------------------------------------------------- mean
@pytest.mark.parametrize("B,K,T", [(3, 13, 65), (1, 80, 65), (3, 129, 257), (3, 80, 3001), (33, 2, 63), (1, 1, 1)])
def test_mean_within_two_ulp_and_forms_agree(B, K, T):
    x = clips(B, K, T, seed=4)
    lengths = [max(1, T - 7 * b) for b in range(B)]
    kw = dict(freq_masks=2, freq_width=min(5, K), time_masks=2, time_width=40, mask_value="mean", lengths=lengths)
    outs = [run(x, form=form, **kw) for form in (None, "resident", "tiled")]
    assert all(bits_equal(outs[0], o) for o in outs[1:]), "the forms of the mean differ"
    _, m, _ = R.apply(x, SEED, F=min(5, K), Wt=40, lengths=lengths)
    worst = 0
    for b in range(B):
        want = np.float32(R.clip_mean(x[b], lengths[b]))
        d = np.abs(bits(outs[0][b][m[b]]).astype(np.int64) - bits_of(want))
        worst = max(worst, int(d.max()) if d.size else 0)
        assert bits_equal(outs[0][b][~m[b]], x[b][~m[b]])
    print(f"mean [{B}, {K}, {T}]: worst {worst} ulp")
    assert worst <= 2


def test_mean_is_exact_on_a_constant_clip():
    x = np.empty((3, 80, 257), dtype=np.float32)
    x[0], x[1], x[2] = 0.1, -7.3, 1e-3
    for form in (None, "resident", "tiled"):
        got = run(x, freq_width=20, time_width=60, mask_value="mean", form=form)
        assert bits_equal(got, x)
    y = dev(x)
    assert ops.spec_augment(y, SEED, freq_width=20, time_width=60, mask_value="mean", out=y) is y and bits_equal(cpu(y), x)


# ---------------------------------------------------------------- warp
def warp_fraction(x, got, kw, lengths=None):
    want, m, ds = R.apply(x, SEED, nf=kw.get("freq_masks", 0), F=kw.get("freq_width", 0), nt=kw.get("time_masks", 0),
                          Wt=kw.get("time_width", 0), W=kw["time_warp"], mask_value=VALUE, lengths=lengths)
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got) == bits_of(VALUE), m)
    peak = np.max(np.abs(x.astype(np.float64)), axis=(1, 2), keepdims=True)
    frac = np.abs(got.astype(np.float64) - want) / (1e-5 * peak)
    assert np.all(frac <= 1.0), f"worst {float(frac.max()):.3e} of the gate"
    return float(frac.max()), ds


@pytest.mark.parametrize("W", [1, 5, 40])
def test_warp_against_the_restatement(W):
    worst = 0.0
    for B, K, T in ((3, 13, 2 * W + 1), (33, 2, 65), (3, 80, 257), (1, 129, 1025), (3, 13, 3001)):
        x = clips(B, K, T, seed=5)
        f, ds = warp_fraction(x, run(x, freq_masks=0, freq_width=0, time_masks=0, time_width=0, time_warp=W), dict(time_warp=W))
        worst = max(worst, f)
        assert all((d["c"] >= 0) == (T > 2 * W) for d in ds)
        kw = dict(freq_masks=2, freq_width=min(4, K), time_masks=2, time_width=10, time_warp=W)
        f, _ = warp_fraction(x, run(x, mask_value=VALUE, **kw), kw)
        worst = max(worst, f)
    print(f"warp W={W}: worst fraction of the gate {worst:.3e}")


@pytest.mark.parametrize("W", [1, 5, 40])
def test_warp_gate_at_two_w_frames(W):
    K, T = 13, 2 * W + 8
    x = clips(4, K, T, seed=6)
    lengths = [2 * W, 2 * W + 1, 2 * W + 1, T]
    got = run(x, freq_masks=0, freq_width=0, time_masks=0, time_width=0, time_warp=W, lengths=lengths)
    f, ds = warp_fraction(x, got, dict(time_warp=W), lengths)
    assert [d["c"] for d in ds[:3]] == [-1, W, W] and bits_equal(got[0], x[0])     # T_b = 2W: untouched; 2W + 1: one centre
    print(f"warp W={W} at T_b = 2W, 2W + 1: worst fraction of the gate {f:.3e}")


def test_warp_to_the_same_place_is_the_identity():
    W, K, T = 5, 13, 257
    seed = next(s for s in range(1000) if (lambda p: p["c"][0] == p["w"][0])(SA.params(s, 0, 1, K, T, time_warp=W, freq_width=0)))
    x = np.random.default_rng(7).integers(-1000, 1000, (1, K, T)).astype(np.float32)
    got = cpu(ops.spec_augment(dev(x), seed, freq_masks=0, freq_width=0, time_masks=0, time_warp=W, out=nan_out(1, K, T)))
    assert bits_equal(got, x)
    other = cpu(ops.spec_augment(dev(x), seed + 1, freq_masks=0, freq_width=0, time_masks=0, time_warp=W))
    p = SA.params(seed + 1, 0, 1, K, T, time_warp=W, freq_width=0)
    assert (p["c"][0] == p["w"][0]) == bits_equal(other, x)


# ---------------------------------------------------------------- ragged batches
@pytest.mark.parametrize("W", [0, 5, 40])
def test_ragged_batches_keep_the_tail(W):
    K, T = 13, 257
    lengths = [1, max(W, 2), 2 * W + 1, T]
    x = clips(4, K, T, seed=8)
    kw = dict(freq_masks=2, freq_width=5, time_masks=2, time_width=100, time_warp=W)
    got = run(x, mask_value=VALUE, lengths=torch.tensor(lengths), **kw)
    warp_fraction(x, got, kw, lengths)
    for b, Tb in enumerate(lengths):
        assert bits_equal(got[b][:, Tb:], x[b][:, Tb:])
    got2 = run(x, mask_value=VALUE, lengths=np.array(lengths), **kw)
    assert bits_equal(got, got2)


# ---------------------------------------------------------------- strides, in place
@pytest.mark.parametrize("W,mask_value", [(0, VALUE), (5, VALUE), (0, "mean")])
def test_strided_rows_give_the_contiguous_bits(W, mask_value):
    B, K, T = 3, 13, 130
    x = clips(B, K + 1, T + 9, seed=9)
    buf = torch.full((B * (K + 1) * (T + 9) + 7,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[7:].view(B, K + 1, T + 9)                                          # rows 7 floats into a NaN buffer
    view.copy_(dev(x))
    xs = view[:, 1:, :T]                                                          # strided over B and K
    assert not xs.is_contiguous() and xs.data_ptr() % 16 != 0
    kw = dict(freq_width=5, time_width=40, time_warp=W, mask_value=mask_value)
    want = cpu(ops.spec_augment(dev(x[:, 1:, :T]), SEED, out=nan_out(B, K, T), **kw))
    got = cpu(ops.spec_augment(xs, SEED, out=nan_out(B, K, T), **kw))
    assert bits_equal(got, want)
    obuf = torch.full((B * (K + 2) * (T + 5) + 7,), float("nan"), dtype=torch.float32, device="cuda")
    oview = obuf[7:].view(B, K + 2, T + 5)
    ops.spec_augment(xs, SEED, out=oview[:, 2:, :T], **kw)
    assert bits_equal(cpu(oview[:, 2:, :T]), want)
    rest = cpu(oview).copy()
    rest[:, 2:, :T] = np.nan
    assert np.isnan(rest).all() and np.isnan(cpu(obuf[:7])).all()                 # nothing written outside the rows
    assert bits_equal(cpu(view), x)                                               # the input is untouched


@pytest.mark.parametrize("B,K,T,mask_value", [(3, 13, 65, VALUE), (3, 80, 3001, VALUE), (33, 2, 63, "mean"), (1, 129, 1025, "mean"),
                                              (3, 13, 257, 0.0)])
def test_in_place_equals_the_copy(B, K, T, mask_value):
    rng = np.random.default_rng(10)
    pattern = rng.integers(0x3F000000, 0x40FFFFFF, (B, K, T), dtype=np.uint32)    # finite floats, compared as integers
    x = pattern.view(np.float32)
    lengths = [max(1, T - 3 * b) for b in range(B)]
    kw = dict(freq_masks=3, freq_width=min(6, K), time_masks=3, time_width=50, mask_value=mask_value, lengths=lengths)
    want = cpu(ops.spec_augment(dev(x), SEED, out=nan_out(B, K, T), **kw))
    y = dev(x)
    assert ops.spec_augment(y, SEED, out=y, **kw) is y
    got = cpu(y)
    assert np.array_equal(bits(got), bits(want))
    _, m, _ = R.apply(x, SEED, nf=3, F=min(6, K), nt=3, Wt=50, lengths=lengths)
    assert np.array_equal(bits(got)[~m], pattern[~m]) and m.any()
    ys = dev(np.concatenate([x, x], axis=1))[:, :K]                               # in place on strided rows
    ops.spec_augment(ys, SEED, out=ys, **kw)
    assert np.array_equal(bits(cpu(ys)), bits(want))


# ---------------------------------------------------------------- determinism
def test_a_batch_equals_its_clips_and_calls_repeat():
    B, K, T = 5, 13, 257
    x = clips(B, K, T, seed=11)
    lengths = [T, 200, 11, T, 64]
    for kw in (dict(freq_width=6, time_width=60, time_warp=5, mask_value="mean"), dict(freq_width=6, time_width=60, mask_value=VALUE)):
        whole = run(x, first_row=100, lengths=lengths, **kw)
        assert bits_equal(whole, run(x, first_row=100, lengths=lengths, **kw))
        for b in range(B):
            one = cpu(ops.spec_augment(dev(x[b:b + 1]), SEED, first_row=100 + b, lengths=lengths[b:b + 1], out=nan_out(1, K, T), **kw))
            assert bits_equal(one[0], whole[b]), f"clip {b} differs from its batch"
    assert not bits_equal(run(x, freq_width=6), run(x, freq_width=6, first_row=1))


def test_single_purpose_forms_equal_their_part():
    B, K, T = 3, 13, 257
    x = clips(B, K, T, seed=12)
    xd = dev(x)
    full = dict(freq_masks=2, freq_width=6, time_masks=3, time_width=50, time_ratio=0.5, time_warp=5)
    assert bits_equal(cpu(A.freq_mask_batch(xd, 2, 6, VALUE, seed=SEED, out=nan_out(B, K, T))),
                      run(x, freq_masks=2, freq_width=6, time_masks=0, time_width=0, mask_value=VALUE))
    y, p = A.freq_mask_batch(xd, 2, 6, seed=SEED, return_params=True)
    pf = SA.params(SEED, 0, B, K, T, **full)
    assert np.array_equal(p["f"], pf["f"]) and np.array_equal(p["f0"], pf["f0"])
    y, p = A.time_mask_batch(xd, 3, 50, 0.5, VALUE, seed=SEED, return_params=True)
    assert np.array_equal(p["t"], pf["t"]) and np.array_equal(p["t0"], pf["t0"])
    assert bits_equal(cpu(y), run(x, freq_masks=0, freq_width=0, time_masks=3, time_width=50, time_ratio=0.5, mask_value=VALUE))
    y, p = A.time_warp_batch(xd, 5, seed=SEED, return_params=True)
    assert np.array_equal(p["c"], pf["c"]) and np.array_equal(p["w"], pf["w"])
    assert bits_equal(cpu(y), run(x, freq_masks=0, freq_width=0, time_masks=0, time_width=0, time_warp=5))
    # the parts compose: the full call is the warp, then the union of the masks
    got = cpu(A.spec_augment_batch(xd, mask_value=VALUE, seed=SEED, out=nan_out(B, K, T), **full))
    step = A.time_warp_batch(xd, 5, seed=SEED)
    step = A.freq_mask_batch(step, 2, 6, VALUE, seed=SEED, out=step)
    step = A.time_mask_batch(step, 3, 50, 0.5, VALUE, seed=SEED, out=step)
    assert bits_equal(got, cpu(step))


def test_return_params_and_seed():
    B, K, T = 4, 13, 257
    xd = dev(clips(B, K, T, seed=13))
    lengths = [T, 100, 7, 257]
    y, seed, p = A.spec_augment_batch(xd, 3, 6, 2, 50, 0.5, 5, "mean", first_row=9, lengths=lengths, return_seed=True, return_params=True)
    assert isinstance(seed, int) and 0 <= seed < 1 << 64
    ds = R.draws(seed, 9, B, K, T, lengths, 3, 6, 2, 50, 0.5, 5)
    assert np.array_equal(p["c"], R.stack_params(ds, "c")[:, 0]) and np.array_equal(p["w"], R.stack_params(ds, "w")[:, 0])
    assert all(np.array_equal(p[k], R.stack_params(ds, k)) for k in ("f", "f0", "t", "t0")) and list(p["lengths"]) == lengths
    again = A.spec_augment_batch(xd, 3, 6, 2, 50, 0.5, 5, "mean", seed=seed, first_row=9, lengths=lengths)
    assert bits_equal(cpu(y), cpu(again))                                         # a call is replayed from its seed
    y2, seed2 = A.spec_augment_batch(xd, freq_width=6, return_seed=True)
    assert seed2 != seed


# ---------------------------------------------------------------- end to end
def test_numpy_function_is_clip_zero():
    K, T = 13, 257
    x = clips(3, K, T, seed=14)
    whole = cpu(A.spec_augment_batch(dev(x), 2, 6, 2, 50, 1.0, 5, "mean", seed=SEED))
    got, p = A.spec_augment(x[0].astype(np.float64), 2, 6, 2, 50, 1.0, 5, "mean", seed=SEED, return_params=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (K, T)
    assert bits_equal(got, whole[0]) and p["f"].shape == (1, 2)
    assert bits_equal(A.spec_augment(x[1], 2, 6, 2, 50, 1.0, 5, "mean", seed=SEED, first_row=1), whole[1])


def test_cli_round_trips_the_layout(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli.main import cli
    rng = np.random.default_rng(15)
    wavfile.write(str(tmp_path / "a.wav"), 16000, np.round(rng.uniform(-0.5, 0.5, 16000) * 32767).astype(np.int16))
    run_cli = CliRunner().invoke
    for ext in ("npz", "csv"):
        src, dst = tmp_path / f"f.{ext}", tmp_path / f"o.{ext}"
        r = run_cli(cli, ["features", "extract", str(tmp_path / "a.wav"), "-o", str(src), "-f", "mfcc", "-f", "spectral_centroid"])
        assert r.exit_code == 0, r.output
        r = run_cli(cli, ["augment", "spec-augment", str(src), "-o", str(dst), "--freq-width", "5", "--time-width", "8", "--time-warp",
                          "3", "--mask-value", "mean", "--seed", "11"])
        assert r.exit_code == 0, r.output
        assert "seed=11" in r.output
        if ext == "npz":
            a, b = dict(np.load(src)), dict(np.load(dst))
        else:
            a, b = (dict(pd.read_csv(f).items()) for f in (src, dst))
        assert list(a) == list(b)
        names = [k for k in a if k != "time"]
        if "time" in a:
            assert np.array_equal(np.asarray(a["time"]), np.asarray(b["time"]))
        S = np.stack([np.asarray(a[k], dtype=np.float32) for k in names])
        want = A.spec_augment(S, 2, 5, 2, 8, 1.0, 3, "mean", seed=11)
        got = np.stack([np.asarray(b[k], dtype=np.float32) for k in names])
        assert got.shape == S.shape and not bits_equal(got, S)
        if ext == "npz":
            assert bits_equal(got, want)
        else:
            assert np.allclose(got, want, rtol=1e-6, atol=0)                      # a table holds decimal text
