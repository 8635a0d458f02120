"""syg_laplace_f32 / ops.laplace and the mirrors of sygnals_amd.core.transforms on the device against the float64
restatement tests/laplace_ref.py, under the project's gate |F_dev - F_ref| <= 1e-5 A with the natural scale
A = |t_step| sum_n |x[n]| exp(-Re(s) n t_step) (a gate relative to |F| would be wrong at a spectral null).  Every size
comes from the library's constants.  A tile never spans clips (a short clip pads its tile with zero chunks), so a batch
equals its rows bit for bit under the same launch form, and within the gate when the rule picks different forms.

Worst |err| / A measured on MI355X (gate 1e-5): 5.6e-7 in the whole-row and in the segmented form alike (33 clips, mixed
signs), forward columns alone 2.1e-7, reversed alone 6.6e-8, at the domain's edge 6.9e-8, steep columns 2.7e-8, unit
impulses 5.8e-8, the geometric row 1.7e-7, the unit circle against np.fft 4.1e-8, one row of 2^20 samples 3.3e-9, the
reference's recorded rows 1.6e-7."""
import os

import numpy as np
import pytest
import torch

import sygnals_amd.core.transforms as TR
from sygnals_amd import _laplace as LP
from sygnals_amd import ops
from tests import laplace_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_laplace.npz"))
GATE = 1e-5
T_STEP = 1.0 / 8000.0


@pytest.fixture(scope="module")
def K():
    return ops.laplace_constants()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def noise(B, L, seed=0):
    rng = np.random.default_rng(100003 * B + L + seed)
    n = np.arange(L)
    return (0.5 * np.sin(0.05 * n + 0.2)[None, :] + 0.5 * rng.standard_normal((B, L))).astype(np.float32)


def under_gate(got, ref, A, what):
    """|got - ref| <= GATE * A elementwise, the worst ratio printed first (pytest -s shows the measured errors)."""
    err = np.abs(np.asarray(got) - ref)
    ratio = np.max(err / np.where(A > 0, A, 1.0)) if err.size else 0.0
    print(f"laplace {what}: worst |err| / A = {ratio:.2e}")
    assert np.all(np.isfinite(np.asarray(got))), what
    assert np.all(err <= GATE * A), what


def check(x, s, t=T_STEP, form=None, what="", y=None):
    """ops.laplace of the rows x (numpy [B, L]; y: the device tensor to pass instead, e.g. a strided view) under the gate."""
    got = ops.laplace(dev(x) if y is None else y, s, t, form=form).cpu().numpy()
    assert got.dtype == np.complex128 and got.shape == (x.shape[0], len(s))
    under_gate(got, R.laplace(x, s, t), R.scale(x, s, t), what)
    return got


def s_mixed(L, t=T_STEP):
    """Both signs of sigma in one call, forward / reversed / steep columns, omega past pi / t_step, the domain's edge."""
    lim = 700.0 / max(L - 1, 1)                                      # the most -sigma t_step may be
    neg = lambda a: -min(a, lim)                                     # noqa: E731
    a = np.array([0.0, 0.0, 1e-3, neg(1e-3), 0.3, neg(0.3), 0.63, neg(0.63), 0.64, neg(0.64), 5.0, neg(11.0), 100.0, -0.0,
                  30.0 / max(L - 1, 1), neg(lim), 2e-5, neg(2e-5), neg(lim)])
    w = np.array([0.0, np.pi, 3.1, -2.0, 0.0, 1.0, 0.1, 0.0, 2.0, 1.0, 1.0, 0.0, 0.3, 1.0, 0.7, 0.0, -5.3, 1.7 * np.pi, 2.9])
    return (a + 1j * w) / t


# ---------------------------------------------------------------- sizes
def _sizes(K):
    C, RC = K["C"], K["tile_rows"] * K["C"]
    return [1, 2, C - 1, C, C + 1, RC - 1, RC, RC + 1]


@pytest.mark.parametrize("i", range(8))
@pytest.mark.parametrize("form", [None, "segmented"])
def test_sizes_around_chunk_and_tile(K, i, form):
    L = _sizes(K)[i]
    check(noise(2, L), s_mixed(L), form=form, what=f"L={L} form={form}")


def test_both_sides_of_the_segment_switch_and_a_long_row(K):
    seg = K["segment"]
    s = np.array([0.4j, 2e-5 + 1.3j, -2e-5 - 0.7j]) / T_STEP
    assert ops.lib().syg_laplace_work_bytes(1, seg, 16, -1) == 0 and ops.lib().syg_laplace_work_bytes(1, seg + 1, 32, -1) > 0
    for L in (seg, seg + 1, 3 * seg - 5):
        x = noise(1, L)
        a = check(x, s, what=f"L={L} rule")
        b = check(x, s, form="whole", what=f"L={L} whole")
        c = check(x, s, form="segmented", what=f"L={L} segmented")
        assert np.array_equal(a, b if L <= seg else c)               # the rule took that form
    L = 1 << 20                                                      # 64 segments
    sl = np.array([0.4j, 6e-4 + 1.3j, -6e-4 - 0.7j]) / T_STEP        # |sigma| t L = 629
    x = noise(1, L)
    check(x, sl, what="L=2^20 rule (segmented)")
    check(x, sl, form="whole", what="L=2^20 whole")


@pytest.mark.parametrize("S", [1, 15, 16, 17, 33])
def test_column_counts_around_the_tile(K, S):
    L = 3 * K["C"] + 5
    rng = np.random.default_rng(S)
    fwd = (rng.uniform(0, 0.5, S) + 1j * rng.uniform(-np.pi, np.pi, S)) / T_STEP
    check(noise(2, L), fwd, what=f"S={S} forward only")
    check(noise(2, L), -fwd, what=f"S={S} reversed only")
    mixed = np.where(np.arange(S) % 3 == 1, -fwd, fwd)
    mixed[::5] *= 6.0                                                # some steep ones
    check(noise(2, L), mixed, what=f"S={S} mixed")


@pytest.mark.parametrize("B", [1, 3, 33])
def test_batch_rows_strides_and_forms(K, B):
    C, Rr = K["C"], K["tile_rows"]
    L = (Rr + 1) * C + C // 2 + 3                                    # a full tile, a partial one, a partial chunk
    x, s = noise(B, L), s_mixed(L)
    whole = check(x, s, form="whole", what=f"B={B} whole")
    for pad in (4, 5):                                               # ldx > L: rows 16-byte aligned, and not
        buf = torch.zeros((B, L + pad), dtype=torch.float32, device="cuda")
        buf[:, :L] = dev(x)
        buf[:, L:] = float("nan")                                    # what lies past a row's end is never read
        got = ops.laplace(buf[:, :L], s, T_STEP, form="whole").cpu().numpy()
        assert np.array_equal(got, whole)
    rows = np.stack([ops.laplace(dev(x[b:b + 1]), s, T_STEP, form="whole").cpu().numpy()[0] for b in range(min(B, 4))])
    assert np.array_equal(rows, whole[:len(rows)])                   # same form: a batch is its rows, bit for bit
    other = check(x, s, form="segmented", what=f"B={B} segmented")
    assert np.all(np.abs(other - whole) <= 2 * GATE * R.scale(x, s, T_STEP))


# ---------------------------------------------------------------- s-values
@pytest.mark.parametrize("L", [1, 2, 65, 1000])
def test_s_value_families(K, L):
    t, x = T_STEP, noise(2, L)
    T = max(L - 1, 1) * t
    om = np.concatenate([np.linspace(0.0, np.pi, 17), [1.7 * np.pi]]) / t
    check(x, 1j * om, what=f"L={L} sigma=0")
    check(x, np.array([0.0, 1e-3, 0.2, -1e-3, -min(0.2, 700.0 / max(L - 1, 1))]) / t + 0j, what=f"L={L} real s")
    check(x, (np.array([1e-4, 1e-2, 5.0, 100.0]) + 1j * np.array([1.0, 2.0, 0.5, 3.0])) / t, what=f"L={L} sigma>0, underflow")
    bound = -700.0 / T if L > 1 else -1e6
    check(x, np.array([-1e-4 / t + 1j / t, -1.0 / T, bound, bound + 2j / t]), what=f"L={L} sigma<0 to the bound")
    check(x, s_mixed(L), what=f"L={L} mixed signs")


def test_bound_at_chunk_plus_one(K):
    L = K["C"] + 1                                                   # a chunk anchored past the row's end would overflow here
    s = np.array([-700.0 / ((L - 1) * T_STEP), -700.0 / ((L - 1) * T_STEP) + 3j / T_STEP, -600.0 / ((L - 1) * T_STEP)])
    x = noise(3, L)
    x[1, L - 3:] = 0.0                                               # the samples that carry the sum are not the last ones
    check(x, s, what="L=C+1 at the bound")


# ---------------------------------------------------------------- known answers, independent of the restatement
def _impulses(L, n0s, s, t, form=None):
    x = np.zeros((len(n0s), L), dtype=np.float32)
    x[np.arange(len(n0s)), n0s] = 1.0
    got = ops.laplace(dev(x), s, t, form=form).cpu().numpy()
    n0 = np.asarray(n0s, dtype=np.float64)[:, None]
    with np.errstate(under="ignore"):
        want = t * np.exp(-s[None, :] * (n0 * t))
        A = abs(t) * np.exp(-s.real[None, :] * (n0 * t))
    under_gate(got, want, A, f"impulses L={L} form={form}")


def test_unit_impulse_everywhere_in_the_first_chunks(K):
    C = K["C"]
    L = 2 * C + 2
    _impulses(L, list(range(L)), s_mixed(L), T_STEP)                 # n0 in [0, 2C + 1], L - 1 among them


@pytest.mark.parametrize("form", ["whole", "segmented"])
def test_unit_impulse_at_segment_boundaries(K, form):
    C, seg = K["C"], K["segment"]
    L = 2 * seg + C + 7
    n0s = [0, C, seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, L - seg - 1, L - seg, L - seg + 1, L - 2, L - 1]
    _impulses(L, n0s, s_mixed(L), T_STEP, form)


def test_geometric_row(K):
    L, t = 5 * K["C"] + 9, T_STEP
    a = 40.0
    n = np.arange(L)
    x = np.exp(-a * n * t)[None, :].astype(np.float32)               # rounded: 6e-8 of every term, far under the gate
    s = s_mixed(L)
    q = np.exp(-(s + a) * t)
    with np.errstate(over="ignore", invalid="ignore"):
        want = t * np.where(q == 1, L, (1 - np.exp(-(s + a) * t * L)) / (1 - q))
    keep = np.isfinite(want)                                         # the closed form itself overflows at the domain's edge
    got = ops.laplace(dev(x), s, t).cpu().numpy()
    under_gate(got[:, keep], want[None, keep], R.scale(x, s, t)[:, keep], "geometric row")
    assert keep.sum() >= len(s) - 3


def test_unit_circle_is_the_fft(K):
    L, t = 1000, T_STEP
    x = noise(2, L)
    s = 2j * np.pi * np.arange(L) / (L * t)
    got = ops.laplace(dev(x), s, t).cpu().numpy()
    A = np.broadcast_to(t * np.abs(x.astype(np.float64)).sum(axis=1)[:, None], got.shape)
    under_gate(got, t * np.fft.fft(x.astype(np.float64), axis=1), A, "unit circle vs np.fft")


# ---------------------------------------------------------------- properties
def test_conjugate_linearity_and_repeatability(K):
    L = K["tile_rows"] * K["C"] + 77
    x, y = noise(2, L), noise(2, L, seed=9)
    s = s_mixed(L)
    A = R.scale(x, s, T_STEP)
    F = ops.laplace(dev(x), s, T_STEP)
    again = ops.laplace(dev(x), s, T_STEP)
    assert torch.equal(torch.view_as_real(F), torch.view_as_real(again))             # the same call twice: equal bits
    F = F.cpu().numpy()
    Fc = ops.laplace(dev(x), np.conj(s), T_STEP).cpu().numpy()
    assert np.all(np.abs(Fc - np.conj(F)) <= GATE * A)
    z = (0.5 * x - 2.0 * y).astype(np.float32)                       # exact in float32? no: rounded once, 6e-8 of each term
    Fy, Fz = ops.laplace(dev(y), s, T_STEP).cpu().numpy(), ops.laplace(dev(z), s, T_STEP).cpu().numpy()
    Az = 0.5 * A + 2.0 * R.scale(y, s, T_STEP)
    assert np.all(np.abs(Fz - (0.5 * F - 2.0 * Fy)) <= GATE * Az)
    out = torch.empty((2, len(s)), dtype=torch.complex128, device="cuda")
    assert ops.laplace(dev(x), s, T_STEP, out=out) is out and np.array_equal(out.cpu().numpy(), F)


def test_wrapper_rejects(K):
    x = dev(noise(2, 100))
    for bad in (x.double(), x[0], x.cpu()):
        with pytest.raises(ValueError):
            ops.laplace(bad, [1.0])
    with pytest.raises(ValueError):
        ops.laplace(x, [[1.0]])
    with pytest.raises(ValueError):
        ops.laplace(x, [])
    with pytest.raises(ValueError):
        ops.laplace(x, [1.0], form="fast")
    with pytest.raises(ValueError) as e:
        ops.laplace(x, [0.0, -700.001 / 99.0], 1.0)
    assert "s_values[1]" in str(e.value) and "700" in str(e.value)
    ops.laplace(x, [0.0, -700.0 / 99.0], 1.0)                        # the bound itself is served
    with pytest.raises(ValueError):
        ops.laplace(x, [1.0], out=torch.empty((2, 2), dtype=torch.complex128, device="cuda"))


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("i", range(int(GOLDEN["n"])))
def test_mirror_against_the_reference_recorded(i):
    x, s, t, F = GOLDEN[f"x_{i}"], GOLDEN[f"s_{i}"], float(GOLDEN[f"t_step_{i}"]), GOLDEN[f"F_{i}"]
    got = TR.laplace_transform_numerical(x, s, t)
    assert got.dtype == np.complex128 and got.shape == F.shape
    under_gate(got, F, R.scale(x, s, t), f"golden row {i}")
    batch = TR.laplace_batch(dev(x[None, :]), s, t)
    assert batch.is_cuda and np.array_equal(batch.cpu().numpy()[0], got)


def test_cli_both_formats(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    x = noise(1, 300)[0].astype(np.float64)
    pd.DataFrame({"value": x}).to_csv(tmp_path / "x.csv", index=False)
    s = np.array([1.0, 0.5 + 0.2j, -2.0 - 40j])
    ref, A = R.laplace(x, s, 0.001), R.scale(x, s, 0.001)
    for name in ("y.npz", "y.csv"):
        r = CliRunner().invoke(cli, ["dsp", "laplace", str(tmp_path / "x.csv"), "-o", str(tmp_path / name), "--s-values",
                                     "1.0,0.5+0.2j,-2-40j", "--t-step", "0.001"])
        assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "y.npz")
    assert sorted(z.files) == ["laplace", "s_values", "t_step"] and np.array_equal(z["s_values"], s) and float(z["t_step"]) == 0.001
    under_gate(z["laplace"], ref, A, "cli npz")
    df = pd.read_csv(tmp_path / "y.csv")
    assert list(df.columns) == ["s_real", "s_imag", "Real", "Imag", "Magnitude"]
    under_gate(df["Real"].to_numpy() + 1j * df["Imag"].to_numpy(), ref, A, "cli csv")
    assert np.allclose(df["Magnitude"], np.abs(z["laplace"]), rtol=1e-12) and np.array_equal(df["s_imag"], s.imag)
    np.savez(tmp_path / "r.npz", data=x, sr=np.array(1000))         # the rate of the input gives t_step = 1 / sr
    r = CliRunner().invoke(cli, ["dsp", "laplace", str(tmp_path / "r.npz"), "-o", str(tmp_path / "r_out.npz"), "--s-values", "1.0,0.5+0.2j,-2-40j"])
    assert r.exit_code == 0, r.output
    zr = np.load(tmp_path / "r_out.npz")
    assert float(zr["t_step"]) == 0.001 and np.array_equal(zr["laplace"], z["laplace"])
