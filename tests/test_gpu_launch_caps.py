"""Every row loop and split launch past its grid cap (the table of tests/launch_cap_cases.py), on the device.

One pattern, that of test_istft_more_waves_than_the_grid_holds: eight distinct rows are run as a call of eight and held
to the feature's float64 reference with the feature's own gate (imported, not restated); the large batch is built on the
device as rows8[idx], idx = arange(B) % 8, run once (into a buffer of NaN wider than the row where the entry takes out=)
and must equal result8[idx] bit for bit, every row of it.  Where the rows of one pass of a capped grid are a multiple of
eight (cu x 8 workgroups), idx is (b + b div pass) % 8, so that a workgroup meets another row on every turn (index8).
Where the row index is part of the value (the generators), the large call is compared with smaller calls at shifted
first_row instead.  Each test asserts with the device's own CU count that its case crosses the cap it names, and prints
the cap, the shape and the worst figure of its reference check.

Already crossed before this module, and so not repeated here: resample_poly (test_more_rows_than_a_launch_takes, 65537
rows), the CWT (65537 rows), PCEN (grid_max + 1), istft2048 (test_istft_more_waves_than_the_grid_holds), the cepstrogram
(more frames than the grid holds) and Welch (70000 segments).

ops.colored_noise cuts a batch into pieces of 32767 pairs, so no call of it fills the grid of the pair kernels
(tests/test_launch_cap_cases.py holds that); their row loops are reached here through the library's entries, with one
launch over all pairs, and ops.colored_noise's own pieces are checked beside it.

Worst figures of the reference checks measured on MI355X (256 CUs); no test found a defect in a kernel.  Against 1e-5 of
the peak: fx_mix 3.8e-8, fx_compress 3.7e-8, fx_midside 9.0e-8, fx_tremolo 5.3e-8, fx_add_noise 5.0e-8 (SNR 2.7e-6 of 1e-4
dB), fx_add_noise_gen resident 6.5e-8 (1.7e-6 dB), three launches 1.1e-7 (7.0e-8 dB), more than 64 slices 9.8e-8 (8.4e-10
dB), coloured rows 1.5e-7, sosfilt y 6.3e-8 and zf 3.1e-9, CMNDF 1.9e-6 (no lag on the fp32 floor, no margin or half-bin
frame).  randn 2.2e-7 against 3.8e-5; true peak 5.3e-7 of 1e-4 dB; segment powers 1.5e-15 of 1e-5; LPC frames 0.006 and
the envelope 0.025 of their gates; gain_rows and stack_memory bit for bit.  Durations: every case under 0.2 s, the first of a
process 0.7 s with the device's start; the 38 cases about 4 s in one process."""
import functools

import numpy as np
import pytest
import torch

from sygnals_amd import _pitch as P
from sygnals_amd import ops
from tests import dynamics_ref, effects_ref, iir_cases, loudness_cases, loudness_ref, lpc_cases, lpc_ref, rng_ref, vocoder_ref
from tests import launch_cap_cases as LC
from tests.gpu_util import assert_parity, peak_rel
from tests.test_gpu_iir import fractions as iir_fractions
from tests.test_gpu_lpc import GATE as LPC_GATE
from tests.test_gpu_lpc import _fractions as lpc_fractions
from tests.test_gpu_lpc import _reference as lpc_reference
from tests.test_gpu_lpc import _window64 as lpc_window64
from tests.test_gpu_noise import SEED, normal_gate, snr_of, within_one_ulp
from tests.test_gpu_pitch import _mixed_clips, _vibrato_clips, host_frames
from tests.test_gpu_pitch_params import _check_cmndf, _check_emission, _check_yin, _report

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 3                                                              # floats of NaN behind every row of an out= buffer


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan(name):
    """The case's shape at this device's CU count, after asserting that it takes the path it names."""
    c, k, cu = LC.case(name), LC.constants(), cu_count()
    shape = c.shape(cu, k)
    assert c.crosses(cu, k), f"{name} at {cu} CUs ({shape}) no longer takes: {c.cap}"
    assert c.bytes(cu, k) <= LC.GIB
    print(f"\n{name} [{c.where}] {c.cap}; {cu} CUs; shape {shape}")
    return shape


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared clips are read-only)


def cpu(t):
    return t.cpu().numpy()


def index8(B, turn=0):
    """Which of the eight rows row b of the large batch is: b % 8.  turn: the rows a capped grid serves in one pass, or the
    rows of one launch of a split call.  Where that is a multiple of eight it is (b + b div turn) % 8 instead: b % 8 alone
    would hand a workgroup the same row on every turn (a piece the same rows as the piece before), and what is left behind
    in LDS or scratch from the turn before, or a pointer not moved on per piece, could not show."""
    b = torch.arange(B, device="cuda")
    idx = (b + b // turn if turn and turn % LC.ROWS8 == 0 else b) % LC.ROWS8
    if turn:
        assert B > turn and not bool((idx[:B - turn] == idx[turn:]).any())
    return idx


def cap8():
    return LC.FX_NOISE_WGS_PER_CU * cu_count()


def wide(B, L, lead=()):
    """A buffer of NaN [B, *lead, L + PAD] and its view of the rows."""
    buf = torch.full((B,) + tuple(lead) + (L + PAD,), NAN, dtype=torch.float32, device="cuda")
    return buf, buf[..., :L]


def untouched(buf, L):
    return bool(torch.isnan(buf[..., L:]).all())


def same_bits(a, b):
    """torch.equal on the bits: shapes, and every element's pattern (a NaN equals the same NaN)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    if a.dtype == torch.float64:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


def rows(B, L, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal((B, L))).astype(np.float32)


def parity(a, b, what):
    """assert_parity (1e-5 of the peak); returns the figure."""
    assert_parity(a, b, what=what)
    return peak_rel(a, b)


# ---------------------------------------------------------------------------- effects.hip: pointwise
@pytest.mark.parametrize("with_y", [True, False])
def test_fx_mix(with_y):
    s = plan("fx_mix")
    B, L, Lx, Ly = s["B"], s["L"], s["Lx"], s["Ly"]
    assert Lx < L < Ly
    x8, y8 = rows(8, Lx, 1), rows(8, Ly, 2)
    a, b = 0.7, -1.3
    dx8, dy8 = dev(x8), dev(y8) if with_y else None
    got8 = ops.fx_mix(dx8, dy8, a, b, length=L)
    ref = np.zeros((8, L))
    ref[:, :Lx] += float(np.float32(a)) * x8
    if with_y:
        ref += float(np.float32(b)) * y8[:, :L]
    print(f"eight rows: {parity(cpu(got8), ref, 'fx_mix'):.2e} of the peak (gate 1e-5)")
    idx = index8(B, LC.FX_MAX_ROWS_Y)
    buf, out = wide(B, L)
    assert ops.fx_mix(dx8[idx], dy8[idx] if with_y else None, a, b, length=L, out=out) is out
    assert same_bits(out, got8[idx]) and untouched(buf, L)


def test_fx_compress():
    s = plan("fx_compress")
    B, L = s["B"], s["L"]
    x8 = rows(8, L, 4, scale=0.6)
    assert (np.abs(x8) > 0.5).any() and (np.abs(x8) <= 0.5).any()
    got8 = ops.fx_compress(dev(x8), 0.5, 3.0)
    worst = max(parity(cpu(got8)[b], effects_ref.compress(x8[b], 0.5, 3.0), f"row {b}") for b in range(8))
    print(f"eight rows: {worst:.2e} of the peak (gate 1e-5)")
    idx = index8(B, LC.FX_MAX_ROWS_Y)
    buf, out = wide(B, L)
    assert ops.fx_compress(dev(x8)[idx], 0.5, 3.0, out=out) is out
    assert same_bits(out, got8[idx]) and untouched(buf, L)


def test_fx_midside():
    s = plan("fx_midside")
    B, L = s["B"], s["L"]                                              # B counts stereo pairs
    st8 = rows(16, L, 5).reshape(8, 2, L)
    got8 = ops.fx_midside(dev(st8), 1.8)
    worst = max(parity(cpu(got8)[b], effects_ref.midside(st8[b], float(np.float32(1.8))), f"clip {b}") for b in range(8))
    print(f"eight clips: {worst:.2e} of the peak (gate 1e-5)")
    idx = index8(B, LC.FX_MAX_ROWS_Y)
    assert same_bits(ops.fx_midside(dev(st8)[idx], 1.8), got8[idx])


@pytest.mark.parametrize("shape", ["sine", "triangle", "square"])
def test_fx_tremolo_largest_batch_and_refusal(shape):
    """The entry refuses more than 8 x 65535 rows; ops.fx_tremolo raised the library's RuntimeError for it where every other
    bad argument of the effects is a ValueError: it now checks the row count itself, and the library's own refusal is
    asserted through the entry."""
    s = plan("fx_tremolo")
    B, L = s["B"], s["L"]
    sr, rate, depth, n0 = 22050, 5.0, 0.8, 7
    x8 = rows(8, L, 6)
    got8 = ops.fx_tremolo(dev(x8), sr, rate, depth, shape, n0=n0)
    worst = max(parity(cpu(got8)[b], effects_ref.apply_tremolo(x8[b], sr, rate, depth, shape, n0=n0), f"row {b}") for b in range(8))
    print(f"eight rows, {shape}: {worst:.2e} of the peak (gate 1e-5)")
    idx = index8(B + 1)
    x = dev(x8)[idx]                                                   # B + 1 rows
    buf, out = wide(B, L)
    assert ops.fx_tremolo(x[:B], sr, rate, depth, shape, n0=n0, out=out) is out
    assert same_bits(out, got8[idx[:B]]) and untouched(buf, L)
    with pytest.raises(ValueError, match="too many rows"):
        ops.fx_tremolo(x, sr, rate, depth, shape, n0=n0)
    more = torch.full((B + 1, L), NAN, dtype=torch.float32, device="cuda")
    with pytest.raises(ops.SygnalsHipError, match="too many rows"):
        ops._call("syg_fx_tremolo_f32", ops._ptr(x), B + 1, L, L, float(sr), rate, depth, ops.LFO_SHAPES[shape], n0, ops._ptr(more), L)
    assert bool(torch.isnan(more).all())                               # refused before anything was launched


# ---------------------------------------------------------------------------- effects.hip: add_noise
SNR8 = np.array([-5.0, 10.0, 40.0, 40.0, 23.5, 0.0, 17.25, 31.0])
SILENT = (2, 3)


def noise_rows8(L):
    y = (0.4 * np.random.default_rng(L).standard_normal((8, L)) + 0.1).astype(np.float32)
    y[2] = 0.0                                                        # a silent row
    y[3] = np.float32(1e-9)                                           # power 1e-18: silent by the reference's rule
    return y


def gate_mix(got, y, noise, snr, what):
    """The existing gates of the mixes: 1e-5 of the row's peak, 1e-4 dB of SNR, silent rows copied.  Returns the worst two."""
    worst, worst_db = 0.0, 0.0
    for b in range(len(y)):
        if np.mean(y[b].astype(np.float64) ** 2) < np.finfo(np.float64).eps:
            assert np.array_equal(got[b], y[b]), f"{what} row {b}: a silent row is not copied"
            continue
        err = peak_rel(got[b], vocoder_ref.add_noise_with(y[b], noise[b], snr[b]))
        d = abs(snr_of(y[b].astype(np.float64), got[b]) - snr[b])
        assert err <= 1e-5 and d <= 1e-4, f"{what} row {b}: {err:.3e} of the peak, SNR off by {d:.3e} dB"
        worst, worst_db = max(worst, err), max(worst_db, d)
    return worst, worst_db


@functools.lru_cache(maxsize=None)
def ref_normals(first_row, B, L):
    z = rng_ref.normal_rows(SEED, first_row, B, L)
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("L", [7, 1000])
def test_fx_add_noise_more_rows_than_workgroups(L):
    s = plan(f"fx_add_noise-L{L}")
    B = s["B"]
    y8, n8 = noise_rows8(L), rows(8, L, L + 1)
    assert all(np.mean(y8[b].astype(np.float64) ** 2) < 2.3e-16 for b in SILENT)
    got8 = ops.fx_add_noise(dev(y8), dev(n8), SNR8)
    w = gate_mix(cpu(got8), y8, n8, SNR8, f"L={L}")
    print(f"eight rows: {w[0]:.2e} of the peak (gate 1e-5), SNR off by {w[1]:.2e} dB (gate 1e-4)")
    idx = index8(B, cap8())
    buf, out = wide(B, L)
    assert ops.fx_add_noise(dev(y8)[idx], dev(n8)[idx], dev(SNR8)[idx], out=out) is out
    assert same_bits(out, got8[idx]) and untouched(buf, L)


@pytest.mark.parametrize("L", [7, 1000])
def test_fx_add_noise_gen_more_rows_than_workgroups(L):
    s = plan(f"fx_add_noise_gen-L{L}")
    B, first = s["B"], LC.GEN_FIRST_ROW
    y8 = noise_rows8(L)
    got8 = ops.fx_add_noise_gen(dev(y8), SNR8, SEED, first)
    w = gate_mix(cpu(got8), y8, ref_normals(first, 8, L), SNR8, f"L={L}")
    print(f"eight rows: {w[0]:.2e} of the peak (gate 1e-5), SNR off by {w[1]:.2e} dB (gate 1e-4)")
    idx = index8(B, cap8())
    y, snr = dev(y8)[idx], dev(SNR8)[idx]
    buf, out = wide(B, L)
    assert ops.fx_add_noise_gen(y, snr, SEED, first, out=out) is out and untouched(buf, L)
    groups = -(-B // 8)
    for g in (0, groups // 2, groups - 1):                            # calls of eight (the last group: what is left of it)
        n = min(8, B - 8 * g)
        rows_g = slice(8 * g, 8 * g + n)
        part = ops.fx_add_noise_gen(y[rows_g], snr[rows_g], SEED, first + 8 * g)
        assert same_bits(out[rows_g], part), f"group {g}"
    stored = ops.fx_add_noise(y, ops.randn(B, L, SEED, first), snr)
    assert within_one_ulp(cpu(out), cpu(stored)), "more than one ulp from the mix of the stored noise"
    silent = torch.tensor([b in SILENT for b in range(8)], device="cuda")[idx]
    assert same_bits(out[silent], y[silent])


def test_fx_add_noise_gen_three_launches_more_rows_than_workgroups():
    s = plan("fx_add_noise_gen-long")
    B, L, head, first = s["B"], s["L"], s["head"], LC.GEN_FIRST_ROW
    y8 = noise_rows8(L)
    idx = index8(B, cap8())
    y, snr = dev(y8)[idx], dev(SNR8)[idx]
    buf, out = wide(B, L)
    assert ops.fx_add_noise_gen(y, snr, SEED, first, out=out) is out and untouched(buf, L)
    assert same_bits(out[:head], ops.fx_add_noise_gen(y[:head], snr[:head], SEED, first))
    assert same_bits(out[head:], ops.fx_add_noise_gen(y[head:], snr[head:], SEED, first + head))
    w = gate_mix(cpu(out[:8]), y8, ref_normals(first, 8, L), SNR8, "three launches")
    print(f"rows 0 to 7: {w[0]:.2e} of the peak (gate 1e-5), SNR off by {w[1]:.2e} dB (gate 1e-4)")


@pytest.mark.parametrize("B,L,per", LC.GEN_SLICE_CASES, ids=lambda v: str(v))
def test_fx_add_noise_gen_more_than_64_slices(B, L, per):
    s = plan(f"fx_add_noise_gen-B{B}-L{L}")
    assert (s["B"], s["L"], s["per"]) == (B, L, per)
    first = LC.GEN_FIRST_ROW
    y = (0.4 * np.random.default_rng(L).standard_normal((3, L)) + 0.1).astype(np.float32)[:B]
    snr = SNR8[[1, 0, 4]][:B]
    yd = dev(y)
    got = ops.fx_add_noise_gen(yd, snr, SEED, first)
    w = gate_mix(cpu(got), y, ref_normals(first, 3, L)[:B], snr, f"B={B} L={L}")
    print(f"{B} rows: {w[0]:.2e} of the peak (gate 1e-5), SNR off by {w[1]:.2e} dB (gate 1e-4)")
    stored = ops.fx_add_noise(yd, ops.randn(B, L, SEED, first), snr)
    assert within_one_ulp(cpu(got), cpu(stored)), "more than one ulp from the mix of the stored noise"
    assert same_bits(ops.fx_add_noise_gen(yd, snr, SEED, first), got)                              # the same call twice


# ---------------------------------------------------------------------------- rng.hip
@pytest.mark.parametrize("offset", [0, 37])
@pytest.mark.parametrize("L", [5, 1025])
def test_randn_more_rows_than_a_launch_takes(L, offset):
    s = plan(f"randn-L{L}")
    B, first, cap = s["B"], s["first_row"], LC.RNG_MAX_ROWS_Y
    buf, out = wide(B, L)
    assert ops.randn(B, L, SEED, first, offset, out=out) is out and untouched(buf, L)
    assert same_bits(out[:cap], ops.randn(cap, L, SEED, first, offset))
    assert same_bits(out[cap:], ops.randn(B - cap, L, SEED, first + cap, offset))
    seam = [0, cap - 1, cap, cap + 1, B - 1]
    got = cpu(out[seam])
    want = np.concatenate([rng_ref.normal_rows(SEED, first + r, 1, L, start=offset) for r in seam])
    normal_gate(got, want, f"randn L={L} offset={offset}, rows {seam}")


def test_colored_noise_pair_rows_and_unpack_more_rows_than_a_launch_takes():
    s = plan("colored_noise")
    B, L, first, alpha, seed = s["B"], s["L"], s["first_row"], 1.0, 9
    M = ops.colored_noise_fft_len(L)
    p0, Pn = LC.colored_pairs(first, B)
    assert first % 2 == 1 and 2 * Pn > LC.RNG_MAX_ROWS_Y

    def pairs(p, n):
        Z = torch.full((n, M, 2), NAN, dtype=torch.float32, device="cuda")
        ops._call("syg_rng_normal_pairs_c64", ops._ptr(Z), n, M, seed, 2 * p)
        return Z

    Z = pairs(p0, Pn)                                                  # one launch over 2 Pn > 65535 rows
    half = Pn // 2 + 1
    assert same_bits(Z[:half], pairs(p0, half)) and same_bits(Z[half:], pairs(p0 + half, Pn - half))
    X = ops.fft_pow2_any(Z)
    ops._call("syg_rng_power_gain_c64", ops._ptr(X), Pn, M, alpha)
    Z = ops.fft_pow2_any(X, inverse=True)
    buf, out = wide(B, L)
    ops._call("syg_rng_unpack_pairs_f32", ops._ptr(Z), M, first, ops._ptr(out), B, L, L + PAD)     # one launch over B > 65535 rows
    assert untouched(buf, L)
    whole = ops.colored_noise(B, L, seed, alpha, first)               # the library's own pieces of 32767 pairs
    assert same_bits(out, whole)
    cut = 32769 - first                                               # rows before the even absolute row 32769 + 1
    cut += (first + cut) % 2
    assert same_bits(whole[:cut], ops.colored_noise(cut, L, seed, alpha, first))
    assert same_bits(whole[cut:], ops.colored_noise(B - cut, L, seed, alpha, first + cut))
    cap = LC.RNG_MAX_ROWS_Y
    seam = [0, cap - 1, cap, cap + 1, B - 1]
    got = cpu(out[seam])
    worst = max(peak_rel(got[i], rng_ref.colored_rows(seed, first + r, 1, L, alpha)[0]) for i, r in enumerate(seam))
    print(f"rows {seam}: {worst:.2e} of the row's peak (gate 1e-5)")
    assert worst <= 1e-5


# ---------------------------------------------------------------------------- loudness.hip
def loud_rows8(C, L, fs, seed):
    rng = np.random.default_rng(seed)
    return np.stack([loudness_cases.draw_clip(rng, fs, C, L) for _ in range(8)])


@pytest.mark.parametrize("name,fs", [("true_peak", 48000), ("true_peak-sample", 192000)])
def test_true_peak_more_clips_than_a_launch_takes(name, fs):
    s = plan(name)
    B, C, L = s["B"], s["C"], s["L"]
    x8 = loud_rows8(C, L, fs, 3)
    got8 = ops.true_peak(dev(x8), fs)
    want = np.array([loudness_ref.true_peak(c, fs) for c in x8])
    e = loudness_cases.db_error(20 * np.log10(cpu(got8).astype(np.float64)), 20 * np.log10(want))
    print(f"eight clips: dBTP off by {e:.2e} dB (gate {loudness_cases.DB_TOL:g})")
    assert e <= loudness_cases.DB_TOL
    idx = index8(B, LC.LOUD_MAX_GRID_Y // C)
    assert same_bits(ops.true_peak(dev(x8)[idx], fs), got8[idx])


def test_gain_rows_more_clips_than_a_launch_takes():
    s = plan("gain_rows")
    B, C, L = s["B"], s["C"], s["L"]
    x8 = loud_rows8(C, L, s["fs"], 4)
    g8 = torch.tensor([0.5, 1.0, 3.0, 0.1, 1.7, 2.5e-3, 12.0, 0.999], dtype=torch.float64, device="cuda")
    want8 = (dev(x8).double() * g8[:, None, None]).float()
    assert same_bits(ops.gain_rows(dev(x8), g8), want8)               # the reference itself: one rounding, bit for bit
    print("eight clips: equal to (x.double() * g).float() bit for bit")
    idx = index8(B, LC.LOUD_MAX_GRID_Y // C)
    x, g = dev(x8)[idx], g8[idx]
    want = (x.double() * g[:, None, None]).float()
    buf, out = wide(B, L, lead=(C,))
    assert ops.gain_rows(x, g, out=out) is out
    assert same_bits(out, want) and same_bits(out, want8[idx]) and untouched(buf, L)
    assert ops.gain_rows(x, g, out=x) is x and same_bits(x, want)      # in place


@pytest.mark.parametrize("C", [3, 2])
def test_loudness_segments_more_clips_than_a_launch_takes(C):
    s = plan(f"loudness_segments-C{C}")
    B, L, fs = s["B"], s["L"], s["fs"]
    x8 = loud_rows8(C, L, fs, 5 + C)
    got8 = ops.loudness_segments(dev(x8), fs)
    ref = np.stack([loudness_ref.segment_powers(c, fs) for c in x8])
    assert tuple(got8.shape) == ref.shape == (8, C, 2)
    peak = np.max(ref, axis=-1, keepdims=True)
    frac = float(np.max(np.abs(cpu(got8) - ref) / peak))
    print(f"eight clips: segment powers {frac:.2e} of the row's largest (gate {loudness_cases.POWER_TOL:g})")
    assert frac <= loudness_cases.POWER_TOL
    idx = index8(B, LC.LOUD_MAX_GRID_Y // C)
    assert same_bits(ops.loudness_segments(dev(x8)[idx], fs), got8[idx])


# ---------------------------------------------------------------------------- sosfilt_causal.hip
@pytest.mark.parametrize("design", ["bessel4_lp", "ellip10_bs"])
def test_sosfilt_more_rows_than_a_launch_takes(design):
    sections = iir_cases.SECTIONS[design]
    s = plan(f"sosfilt-S{sections}")
    B, L = s["B"], s["L"]
    sos = iir_cases.DESIGNS[design]
    x8, zi8 = iir_cases.make_input(iir_cases.Case(design, 8, L, "random"))
    y8, zf8 = ops.sosfilt(dev(x8), sos, zi=dev(zi8), return_state=True)
    fy, fz = iir_fractions(cpu(y8), cpu(zf8), *iir_cases.scipy_ref(sos, x8, zi8))
    print(f"eight rows, {design}: y {fy:.2e} zf {fz:.2e} of the row's peak (gate {iir_cases.GATE:g})")
    assert fy <= iir_cases.GATE and fz <= iir_cases.GATE
    idx = index8(B, LC.SOS_MAX_GRID_Y)
    buf, out = wide(B, L)
    y, zf = ops.sosfilt(dev(x8)[idx], sos, zi=dev(zi8)[idx], return_state=True, out=out)
    assert y is out and untouched(buf, L)
    assert same_bits(y, y8[idx]) and same_bits(zf, zf8[idx])


# ---------------------------------------------------------------------------- dynamics.hip
def test_stack_memory_more_output_rows_than_the_grid_holds():
    s = plan("stack_memory")
    x = rows(s["B"] * s["K"], s["T"], 8).reshape(s["B"], s["K"], s["T"])
    got = ops.stack_memory(dev(x), s["n_steps"], s["delay"])
    want = dynamics_ref.stack_memory(x, s["n_steps"], s["delay"])
    assert got.shape == want.shape and np.array_equal(cpu(got), want)
    print("equal to the restatement bit for bit (a pure gather)")


# ---------------------------------------------------------------------------- lpc.hip
def lpc_gate(a, k, err, frames, order, method):
    """The three gates of tests/test_gpu_lpc.py on frames [n, N] (float64, windowed) against a [p + 1, n], k [p, n], err [n]."""
    ref = [lpc_reference(f, order, method) for f in frames]
    a_ref, k_ref, err_ref = (np.stack([r[i] for r in ref], axis=-1) for i in range(3))
    fr = lpc_fractions(a, k, err, a_ref, k_ref, err_ref, axis=0)
    assert max(fr) <= 1.0, fr
    return fr


@pytest.mark.parametrize("method", ["burg", "autocorr"])
@pytest.mark.parametrize("name", ["lpc_frames-staged", "lpc_frames-unstaged"])
def test_lpc_frames_more_tiles_than_workgroups(name, method):
    s = plan(name)
    B, N, order, hop, L, T = s["B"], s["N"], s["order"], s["hop"], s["L"], s["T"]
    y8 = lpc_cases.clips(8, L)
    a8, k8, e8 = ops.lpc_frames(dev(y8), order, N, hop, False, method, None, True, True)
    assert tuple(a8.shape) == (8, order + 1, T)
    w = lpc_window64(ops, "hann" if method == "autocorr" else None, N)
    worst = (0.0, 0.0, 0.0)
    for b in range(8):
        fr = lpc_gate(*(cpu(v[b]).astype(np.float64) for v in (a8, k8, e8)), lpc_ref.frames_of(y8[b], N, hop, False, w), order, method)
        worst = tuple(max(u, v) for u, v in zip(worst, fr))
    print(f"eight clips, {method}: a {worst[0]:.3g}, k {worst[1]:.3g}, err {worst[2]:.3g} of the gates ({LPC_GATE:g})")
    idx = index8(B, LC.LPC_WGS_PER_CU * cu_count())                   # one tile a clip: a workgroup's next clip is cu * 8 on
    nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device="cuda")
    a, k, e = nan(B, order + 1, T), nan(B, order, T), nan(B, T)
    ops.lpc_frames(dev(y8)[idx], order, N, hop, False, method, None, True, True, out=a, out_k=k, out_err=e)
    assert same_bits(a, a8[idx]) and same_bits(k, k8[idx]) and same_bits(e, e8[idx])


@pytest.mark.parametrize("method", ["burg", "autocorr"])
def test_lpc_frames_one_long_clip_more_tiles_than_workgroups(method):
    s = plan("lpc_frames-long")
    N, order, hop, L, T = s["N"], s["order"], s["hop"], s["L"], s["T"]
    y = lpc_cases.clip("noise", L)
    a, k, e = ops.lpc_frames(dev(y[None]), order, N, hop, True, method, None, True, True)
    assert tuple(a.shape) == (1, order + 1, T)
    padded = np.concatenate([np.zeros(N // 2, np.float32), y, np.zeros(N, np.float32)])      # frame t starts at padded[t hop]
    w = lpc_window64(ops, "hann" if method == "autocorr" else None, N)

    def alone(t0, cnt):
        """Frames [t0, t0 + cnt) from an uncentred call on the samples that hold them."""
        piece = padded[t0 * hop:(t0 + cnt - 1) * hop + N]
        return piece, ops.lpc_frames(dev(piece[None]), order, N, hop, False, method, None, True, True)

    worst = (0.0, 0.0, 0.0)
    for t0 in LC.lpc_long_tiles(cu_count(), LC.constants()):
        cnt = min(16, T - t0)
        piece, (ap, kp, ep) = alone(t0, cnt)
        assert same_bits(a[:, :, t0:t0 + cnt], ap) and same_bits(k[:, :, t0:t0 + cnt], kp) and same_bits(e[:, t0:t0 + cnt], ep), f"tile at {t0}"
        fr = lpc_gate(*(cpu(v[0]).astype(np.float64) for v in (ap, kp, ep)), lpc_ref.frames_of(piece, N, hop, False, w), order, method)
        worst = tuple(max(u, v) for u, v in zip(worst, fr))
    print(f"three tiles, {method}: a {worst[0]:.3g}, k {worst[1]:.3g}, err {worst[2]:.3g} of the gates ({LPC_GATE:g})")
    h = T // 2 + 5                                                     # and every frame: two calls under the cap, cut off a tile's edge
    assert -(-max(h, T - h) // 16) <= LC.LPC_WGS_PER_CU * cu_count()
    for t0, cnt in ((0, h), (h, T - h)):
        _, (ap, kp, ep) = alone(t0, cnt)
        assert same_bits(a[:, :, t0:t0 + cnt], ap) and same_bits(k[:, :, t0:t0 + cnt], kp) and same_bits(e[:, t0:t0 + cnt], ep), f"frames from {t0}"


@pytest.mark.parametrize("order", [1, 64])
def test_lpc_envelope_more_elements_than_a_pass_of_the_grid(order):
    s = plan(f"lpc_envelope-p{order}")
    T, n_fft = s["T"], s["n_fft"]
    N, hop = 128, 7
    y = lpc_cases.clip("ar4", N + hop * (T - 1))
    a, err = ops.lpc_frames(dev(y[None]), order, N, hop, False, "burg", None, False, True)
    assert tuple(a.shape) == (1, order + 1, T)
    K = n_fft // 2 + 1
    Pw, D = (torch.full((1, K, T), NAN, dtype=torch.float32, device="cuda") for _ in range(2))
    assert ops.lpc_envelope(a, err, n_fft, out=Pw) is Pw and ops.lpc_envelope(a, err, n_fft, db=True, out=D) is D
    h = T // 2 + 1
    for lo, hi in ((0, h), (h, T)):                                    # the call cut in two along T: each under the cap
        assert -(-K * (hi - lo) // LC.LPC_ENV_THREADS) <= LC.LPC_ENV_WGS_PER_CU * cu_count()
        ac, ec = a[:, :, lo:hi].contiguous(), err[:, lo:hi].contiguous()
        assert same_bits(Pw[:, :, lo:hi], ops.lpc_envelope(ac, ec, n_fft))
        assert same_bits(D[:, :, lo:hi], ops.lpc_envelope(ac, ec, n_fft, db=True))
    a64, e64 = cpu(a)[0].astype(np.float64), cpu(err)[0].astype(np.float64)
    P64, D64 = cpu(Pw)[0].astype(np.float64), cpu(D)[0].astype(np.float64)
    assert np.isfinite(P64).all() and np.isfinite(D64).all()
    worst = 0.0
    for t in np.linspace(0, T - 1, 32).astype(int):                    # test_envelope's gate on 32 frames spread over T
        A = np.abs(lpc_ref.transfer(a64[:, t], n_fft))
        worst = max(worst, np.max(np.abs(np.sqrt(e64[t] / P64[:, t]) - A)) / (LPC_GATE * np.sum(np.abs(a64[:, t]))))
    want = 10.0 * np.log10(np.maximum(P64, 1e-10))
    wdb = np.max(np.abs(D64 - want) / (LPC_GATE * np.maximum(1.0, np.abs(want))))
    print(f"envelope p={order}: |A| {worst:.3g}, dB {wdb:.3g} of the gates ({LPC_GATE:g})")
    assert worst <= 1.0 and wdb <= 1.0


# ---------------------------------------------------------------------------- pitch.hip
def test_pitch_frames_more_frames_than_the_grid_holds():
    s = plan("pitch_frames")
    B, L, T = s["B"], s["L"], s["T"]
    sr, win, hop = LC.PITCH_SR, LC.PITCH_WIN, LC.PITCH_HOP
    cfg = (sr, P.C2, P.C7, win, hop)
    Y8 = np.concatenate([_mixed_clips(sr, L), _vibrato_clips(4, sr, 0.25, seed=21)[:, :L]])
    assert Y8.shape == (8, L)
    run = lambda y, mode: ops.pitch_frames(y, sr, P.C2, P.C7, win_length=win, hop=hop, center=False, mode=mode, want_cmndf=True)
    yin8, py8 = run(dev(Y8), "yin"), run(dev(Y8), "pyin")
    assert yin8["T"] == T
    hy, hp = host_frames(yin8), host_frames(py8)
    n_fl, n_lags, worst = _check_cmndf(hy["cmndf"], Y8, cfg, False, "eight clips")
    print(f"eight clips: CMNDF worst error {worst * 1e-5:.2e} of the frame peak (gate 1e-5, else the fp32 floor)")
    _report("cmndf lags past 1e-5 (held to the fp32 floor)", n_fl, n_lags)
    _report("yin margin frames", *_check_yin(hy["f0"], Y8, cfg, False, 0.1, "eight clips")[:2])
    _report("pyin half-bin frames", *_check_emission(hp, cfg, "eight clips"))
    idx = index8(B, LC.PITCH_WGS_PER_CU * cu_count() * LC.PITCH_WAVES // T)      # clips of one pass of the grid
    y = dev(Y8)[idx]
    yin, py = run(y, "yin"), run(y, "pyin")
    assert same_bits(yin["f0"], yin8["f0"][idx]) and same_bits(yin["cmndf"], yin8["cmndf"][idx])
    assert same_bits(py["cmndf"], py8["cmndf"][idx])
    assert same_bits(py["cand_count"], py8["cand_count"][idx]) and same_bits(py["voiced_prob"], py8["voiced_prob"][idx])
    live8 = torch.arange(py8["K"], device="cuda")[None, None, :] < py8["cand_count"][:, :, None]      # entries past the count are unset
    for key in ("cand_bin", "cand_prob"):
        zero = torch.zeros((), dtype=py[key].dtype, device="cuda")
        assert same_bits(torch.where(live8[idx], py[key], zero), torch.where(live8, py8[key], zero)[idx]), key
