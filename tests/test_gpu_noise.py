"""Device noise generation (syg_rng_*, syg_fx_add_noise_gen_f32, ops.randn / colored_noise / fx_add_noise_gen and the
device-generator functions of sygnals_amd.core.augment) against the float64 restatement of tests/rng_ref.py.

Gates: raw words bit for bit; normals |z - z_ref| <= 1e-5 max(1, max |z_ref|) per row; coloured rows and mixes 1e-5 of the
row's peak; the achieved SNR 1e-4 dB.  What depends on (seed, row, sample index) alone is compared bit for bit."""
import functools
import warnings

import numpy as np
import pytest
import torch

import sygnals_amd.core.augment as A
from sygnals_amd import ops
from tests import rng_ref as R
from tests import vocoder_ref as V
from tests.gpu_util import peak_rel

pytestmark = pytest.mark.gpu

SEED = (1 << 40) + 7
ROW_MAX = (1 << 31) - 1


def cpu(t):
    return t.cpu().numpy()


def resident(which):
    """The longest row of the one-launch mixes ("mix"), and twice that ("gen": 128 KiB of y, the most LDS could hold of a
    row; lengths either side of it lie in the three-launch form of the generating mix)."""
    return ops.fx_add_noise_resident_max() * (1 if which == "mix" else 2)


@functools.lru_cache(maxsize=None)
def ref_rows(seed, first_row, B, L):
    """The restatement's rows, computed once and shared (read-only)."""
    z = R.normal_rows(seed, first_row, B, L)
    z.setflags(write=False)
    return z


def normal_gate(got, want, what):
    for b in range(want.shape[0]):
        err = float(np.max(np.abs(got[b].astype(np.float64) - want[b])))
        bound = 1e-5 * max(1.0, float(np.max(np.abs(want[b]))))
        if b == 0:
            print(f"{what} row 0: {err:.2e} against {bound:.2e}")
        assert err <= bound, f"{what} row {b}: {err:.3e} > {bound:.3e}"


# ---------------------------------------------------------------- raw words
def test_philox_words_bit_for_bit():
    ctr = [c for c, _, _ in R.KNOWN_ANSWERS]
    key = [k for _, k, _ in R.KNOWN_ANSWERS]
    got = cpu(ops.philox_words(ctr, key)).view(np.uint32)
    assert got.tolist() == [list(w) for _, _, w in R.KNOWN_ANSWERS]
    from sygnals_amd import _rng
    q = np.array([0, 1, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 62) - 1], dtype=np.uint64)
    for row in (0, 1, ROW_MAX):
        for stream in (0, 1):
            c = _rng.counters(q, row, stream)
            got = cpu(ops.philox_words(c, _rng.key_of(SEED))).view(np.uint32)
            assert np.array_equal(got, R.words(SEED, row, q, stream)), (row, stream)
    rng = np.random.default_rng(3)
    c = rng.integers(0, 1 << 32, size=(1000, 4), dtype=np.uint64)
    k = rng.integers(0, 1 << 32, size=(1000, 2), dtype=np.uint64)
    assert np.array_equal(cpu(ops.philox_words(c, k)).view(np.uint32), R.philox(c, k))


# ---------------------------------------------------------------- normals
LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, ("mix", -1), ("mix", 0), ("mix", 1), ("gen", -1), ("gen", 1), 65537]


def _length(L):
    return resident(L[0]) + L[1] if isinstance(L, tuple) else L


@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("L", LENGTHS, ids=str)
def test_randn_against_the_restatement(L, B):
    L = _length(L)
    got = cpu(ops.randn(B, L, SEED))
    assert got.shape == (B, L) and got.dtype == np.float32 and np.isfinite(got).all()
    normal_gate(got, ref_rows(SEED, 0, 33, 65537)[:B, :L], f"randn B={B} L={L}")


@pytest.mark.parametrize("L,pad,offset", [(1, 3, 0), (5, 1, 0), (257, 4, 0), (1000, 24, 0), (1001, 7, 2), (4096, 4, 37)])
def test_randn_into_a_wider_buffer_leaves_the_padding(L, pad, offset):
    buf = torch.full((3, L + pad), float("nan"), dtype=torch.float32, device="cuda")
    out = ops.randn(3, L, 5, first_row=2, offset=offset, out=buf[:, :L])
    assert out.data_ptr() == buf.data_ptr()
    got = cpu(buf)
    assert np.isnan(got[:, L:]).all() and np.isfinite(got[:, :L]).all()
    assert np.array_equal(got[:, :L], cpu(ops.randn(3, L, 5, first_row=2, offset=offset)))
    normal_gate(got[:, :L], R.normal_rows(5, 2, 3, L, start=offset), f"randn strided L={L}")
    odd = torch.full((L + 3,), float("nan"), dtype=torch.float32, device="cuda")        # a row that starts 4 bytes off
    ops.randn(1, L, 5, first_row=2, offset=offset, out=odd[1:L + 1][None, :])
    assert np.array_equal(cpu(odd)[1:L + 1], got[0, :L]) and np.isnan(cpu(odd)[[0, L + 1, L + 2]]).all()


def test_randn_bit_for_bit():
    B, L = 5, 4099
    a = cpu(ops.randn(B, L, SEED, first_row=3))
    assert np.array_equal(a, cpu(ops.randn(B, L, SEED, first_row=3)))                     # the same call twice
    for b in range(B):
        assert np.array_equal(cpu(ops.randn(1, L, SEED, first_row=3 + b))[0], a[b])       # a batch equals its rows
    assert np.array_equal(cpu(ops.randn(2, 63, SEED, first_row=3, offset=37)), cpu(ops.randn(2, 100, SEED, first_row=3))[:, 37:])
    for k in (1, 2, 3, 4, 1021):
        assert np.array_equal(cpu(ops.randn(1, L - k, SEED, first_row=4, offset=k))[0], a[1, k:])
    assert not np.array_equal(a, cpu(ops.randn(B, L, SEED + 1, first_row=3)))             # two seeds differ
    assert not np.array_equal(a[0], a[1])
    last = cpu(ops.randn(1, 64, SEED, first_row=ROW_MAX))
    normal_gate(last, R.normal_rows(SEED, ROW_MAX, 1, 64), "the last row")


def test_randn_offset_past_two_to_the_34():
    off = (1 << 34) - 5                                             # q crosses 2^32 inside the call
    got = cpu(ops.randn(2, 23, 9, first_row=1, offset=off))
    normal_gate(got, R.normal_rows(9, 1, 2, 23, start=off), "offset 2^34 - 5")
    assert np.array_equal(got[:, 5:], cpu(ops.randn(2, 18, 9, first_row=1, offset=1 << 34)))


# ---------------------------------------------------------------- the generating mix
def snr_of(y, out):
    n = np.asarray(out, dtype=np.float64) - y
    return 10.0 * np.log10(np.mean(y ** 2) / np.mean(n ** 2))


def within_one_ulp(a, b):
    return np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))


GEN_LENGTHS = [1, 7, 1000, ("mix", 0), ("mix", 1), ("gen", 0), ("gen", 1), 65537]


@pytest.mark.parametrize("L", GEN_LENGTHS, ids=str)
def test_add_noise_gen(L):
    L = _length(L)
    rng = np.random.default_rng(L)
    B, first_row = 5, 11
    y = (0.4 * rng.standard_normal((B, L)) + 0.1).astype(np.float32)
    y[2] = 0.0                                                        # a silent row
    y[3] = np.float32(1e-9)                                           # power 1e-18: silent by the reference's rule
    snr = np.array([-5.0, 10.0, 40.0, 40.0, 23.5])
    yd = torch.from_numpy(y).cuda()
    got = cpu(ops.fx_add_noise_gen(yd, snr, SEED, first_row))
    noise = ops.randn(B, L, SEED, first_row)
    stored = cpu(ops.fx_add_noise(yd, noise, snr))
    z = R.normal_rows(SEED, first_row, B, L)
    for b in range(B):
        if b in (2, 3):
            assert np.array_equal(got[b], y[b])                      # bit for bit
            continue
        want = V.add_noise_with(y[b], z[b], snr[b])
        err = peak_rel(got[b], want)
        print(f"gen mix L={L} row {b}: {err:.2e}")
        assert err <= 1e-5
        assert within_one_ulp(got[b], stored[b]), f"row {b} is more than one ulp from the mix of the stored noise"
        d = abs(snr_of(y[b].astype(np.float64), got[b]) - snr[b])
        print(f"gen mix L={L} row {b}: SNR off by {d:.2e} dB")
        assert d <= 1e-4
    assert np.array_equal(cpu(ops.fx_add_noise_gen(yd, snr, SEED, first_row)), got)              # the same call twice
    alone = cpu(ops.fx_add_noise_gen(yd[1:2], 10.0, SEED, first_row + 1))[0]                     # a number; the row alone
    if L <= resident("mix"):
        assert np.array_equal(alone, got[1])
    else:
        assert within_one_ulp(alone, got[1])                         # (the slices of a long row depend on the batch)
    assert np.array_equal(cpu(ops.fx_add_noise_gen(yd, torch.from_numpy(snr).cuda(), SEED, first_row)), got)
    buf = yd.clone()
    assert ops.fx_add_noise_gen(buf, snr, SEED, first_row, out=buf) is buf and np.array_equal(cpu(buf), got)
    wide = torch.full((B, L + 3), float("nan"), dtype=torch.float32, device="cuda")              # rows 12 bytes off a multiple of 16
    src = torch.full((B, L + 1), float("nan"), dtype=torch.float32, device="cuda")
    src[:, :L] = yd
    ops.fx_add_noise_gen(src[:, :L], snr, SEED, first_row, out=wide[:, :L])
    assert np.array_equal(cpu(wide)[:, :L], got) and np.isnan(cpu(wide)[:, L:]).all()


def test_add_noise_device_batch_snr_forms():
    L, B, first_row = 3000, 6, 4
    rng = np.random.default_rng(2)
    y = (0.3 * rng.standard_normal((B, L))).astype(np.float32)
    yd = torch.from_numpy(y).cuda()
    z = R.normal_rows(77, first_row, B, L)
    draws = R.snr_draws(77, first_row, B, 5.0, 30.0)
    assert np.all(draws >= 5.0) and np.all(draws < 30.0) and len(np.unique(draws)) == B
    got, seed = A.add_noise_device_batch(yd, (5.0, 30.0), seed=77, first_row=first_row, return_seed=True)
    assert seed == 77 and got.is_cuda and tuple(got.shape) == (B, L)
    got = cpu(got)
    for b in range(B):
        assert peak_rel(got[b], V.add_noise_with(y[b], z[b], draws[b])) <= 1e-5
        assert abs(snr_of(y[b].astype(np.float64), got[b]) - draws[b]) <= 1e-4
        alone = cpu(A.add_noise_device_batch(yd[b:b + 1], (5.0, 30.0), seed=77, first_row=first_row + b))[0]
        assert np.array_equal(alone, got[b])                                                # a row's draw is its own
    per_row = np.linspace(0.0, 25.0, B)
    for snr in (12.0, per_row, list(per_row), torch.from_numpy(per_row).cuda()):
        out = cpu(A.add_noise_device_batch(yd, snr, "white", seed=77, first_row=first_row))
        want = np.broadcast_to(np.asarray(snr.cpu() if isinstance(snr, torch.Tensor) else snr, dtype=np.float64), (B,))
        for b in range(B):
            assert peak_rel(out[b], V.add_noise_with(y[b], z[b], want[b])) <= 1e-5
    _, s1 = A.add_noise_device_batch(yd, 10.0, return_seed=True)
    _, s2 = A.add_noise_device_batch(yd, 10.0, return_seed=True)
    assert s1 != s2 and 0 <= s1 < (1 << 64)                                                # fresh seeds
    with pytest.raises(ValueError, match="Invalid noise_type: 'violet'"):
        A.add_noise_device_batch(yd, 10.0, "violet")


# ---------------------------------------------------------------- coloured noise
@pytest.mark.parametrize("B", [1, 2, 3, 33])
@pytest.mark.parametrize("L", [2, 3, 1000, 1024, 1025, 4097])
def test_coloured_against_the_restatement(L, B):
    first_row = 7                                                    # odd: the first row's partner (6) is not asked for
    for name, alpha in (("pink", 1.0), ("brown", 2.0)):
        got = cpu(A.generate_noise_batch(B, L, name, seed=9, first_row=first_row))
        assert got.shape == (B, L) and got.dtype == np.float32
        want = R.colored_rows(9, first_row, B, L, alpha)
        worst = max(peak_rel(got[b], want[b]) for b in range(B))
        print(f"{name} B={B} L={L}: {worst:.2e}")
        assert worst <= 1e-5
        for b in sorted({0, B // 2, B - 1}):                          # a batch equals its rows, bit for bit
            assert np.array_equal(cpu(ops.colored_noise(1, L, 9, alpha, first_row + b))[0], got[b])
        if B == 3:
            assert np.array_equal(cpu(ops.colored_noise(2, L, 9, alpha, first_row + 1)), got[1:])      # rows 8, 9: one pair


def test_coloured_exponent_zero_custom_exponent_and_one_sample():
    L = 1000
    white = cpu(ops.randn(3, L, 9, first_row=2)).astype(np.float64)
    got = cpu(ops.colored_noise(3, L, 9, 0.0, first_row=2))
    for b in range(3):
        assert peak_rel(got[b], white[b]) <= 1e-5
    got = cpu(A.generate_noise_batch(2, L, "white", seed=9, exponent=1.5, first_row=2))
    want = R.colored_rows(9, 2, 2, L, 1.5)
    assert max(peak_rel(got[b], want[b]) for b in range(2)) <= 1e-5
    assert np.array_equal(cpu(ops.colored_noise(3, 1, 9, 1.0)), np.zeros((3, 1), dtype=np.float32))
    y = torch.full((2, 1), 0.5, dtype=torch.float32, device="cuda")
    assert np.array_equal(cpu(A.add_noise_device_batch(y, 10.0, "pink", seed=9)), cpu(y))               # a zero noise row: copied


@pytest.mark.parametrize("name,alpha", [("pink", 1.0), ("brown", 2.0)])
def test_coloured_slope_of_the_device_row(name, alpha):
    x = cpu(A.generate_noise_batch(1, 65536, name, seed=9))[0].astype(np.float64)
    slope = R.octave_slope(x)
    print(f"{name}: {slope:.3f} dB per octave; mean / peak {abs(np.mean(x)) / np.max(np.abs(x)):.1e}")
    assert abs(slope - (-3.01 * alpha)) <= 0.2
    assert peak_rel(x, R.colored(9, 0, 65536, alpha)) <= 1e-5
    assert abs(np.mean(x)) <= 1e-5 * np.max(np.abs(x))               # (float32 transforms: the restatement's own is 1e-12)


# ---------------------------------------------------------------- the mirror and the CLI
def test_add_noise_device_and_cli(tmp_path):
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    L, sr = 6000, 8000
    y = V.tones_noise(L).astype(np.float32).astype(np.float64)
    np.savez(tmp_path / "x.npz", data=y, sr=np.array(sr))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for name, alpha in (("gaussian", 0.0), ("pink", 1.0), ("brown", 2.0)):
            got = A.add_noise_device(y, 10.0, name, seed=21)
            assert got.dtype == np.float64 and got.shape == (L,)
            noise = R.normals(21, 0, L) if alpha == 0.0 else R.colored(21, 0, L, alpha)
            want = V.add_noise_with(y, noise, 10.0)
            print(f"add_noise_device {name}: {peak_rel(got, want):.2e}")
            assert peak_rel(got, want) <= 1e-5 and abs(snr_of(y, got) - 10.0) <= 1e-4
        r = CliRunner().invoke(cli, ["augment", "add-noise", str(tmp_path / "x.npz"), "-o", str(tmp_path / "p.npz"), "--snr", "10",
                                     "--seed", "21", "--generator", "device", "--noise-type", "pink"])
        assert r.exit_code == 0, r.output
        assert np.array_equal(np.load(tmp_path / "p.npz")["data"], A.add_noise_device(y, 10.0, "pink", seed=21))
        r = CliRunner().invoke(cli, ["augment", "add-noise", str(tmp_path / "x.npz"), "-o", str(tmp_path / "e.npz"), "--snr", "10",
                                     "--seed", "21", "--generator", "device", "--exponent", "2"])
        assert r.exit_code == 0, r.output
        assert np.array_equal(np.load(tmp_path / "e.npz")["data"], A.add_noise_device(y, 10.0, "brown", seed=21))
    mine = [w for w in seen if issubclass(w.category, UserWarning) and ("sygnals_amd" in w.filename or "noise" in str(w.message))]
    assert not mine, [str(w.message) for w in mine]                  # no UserWarning: pink and brown are real here
    # the host generator is what it was: the reference's draw, with and without the new option
    base = ["augment", "add-noise", str(tmp_path / "x.npz"), "--snr", "10", "--seed", "3"]
    for extra, name in ((["--generator", "host"], "h.npz"), ([], "d.npz")):
        r = CliRunner().invoke(cli, base + ["-o", str(tmp_path / name)] + extra)
        assert r.exit_code == 0, r.output
        assert np.array_equal(np.load(tmp_path / name)["data"], A.add_noise(y, 10.0, "gaussian", 3))
    assert peak_rel(A.add_noise(y, 10.0, "gaussian", 3), V.add_noise(y, 10.0, 3)) <= 1e-5
    with pytest.warns(UserWarning, match="Pink noise generation is currently a placeholder"):
        A.add_noise(y, 10.0, "pink", seed=3)
