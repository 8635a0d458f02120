"""The loudness meter and normaliser on the device (csrc/loudness.hip through sygnals_amd.ops and
sygnals_amd.core.audio.loudness) against the float64 restatement tests/loudness_ref.py on the same float32 clips.

Gates: segment powers per row to 1e-5 of the row's largest (the project's gate); momentary, short-term and integrated
loudness, loudness range and dBTP to 1e-4 dB (the dB gate add_noise's SNR uses).  Every gated case is built with a margin of
0.01 LU between the reference's blocks and every threshold (tests/loudness_cases.py), so the device must select exactly the
reference's blocks.  Every test prints its worst figures; those measured on MI355X are in README.md, "Loudness"."""
import numpy as np
import pytest
import torch

from sygnals_amd import _loudness as LD
from sygnals_amd import ops
from sygnals_amd.core.audio import loudness as LN
from tests import loudness_cases as K
from tests import loudness_ref as R

pytestmark = pytest.mark.gpu

WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    print(f"{key}: {float(v):.3e}, worst so far {WORST[key]:.3e}")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # (a copy: the shared cases are read-only)


def _check_meter(x, ref, fs, weights=None, what=""):
    """Segment powers, M, S, I and LRA of the clips x [B, C, L] against ref."""
    xd = _dev(x)
    seg = ops.loudness_segments(xd, fs)
    M, S, I, thr = ops.loudness_blocks(seg, fs, weights)
    lra = ops.loudness_range(S, thr)
    seg = seg.cpu().numpy()
    assert seg.shape == ref["seg"].shape and np.isfinite(seg).all(), what
    if seg.shape[-1]:
        peak = np.max(ref["seg"], axis=-1, keepdims=True)
        frac = np.abs(seg - ref["seg"]) / np.where(peak > 0, peak, 1.0)
        assert np.all(seg[np.broadcast_to(peak == 0, seg.shape)] == 0), f"{what}: a silent row's powers are not exactly zero"
        _note("segment powers / row max", frac.max())
        assert frac.max() <= K.POWER_TOL, f"{what}: segment powers {frac.max():.3e}"
    for name, got, want in (("M", M, ref["M"]), ("S", S, ref["S"]), ("I", I, ref["I"]), ("LRA", lra, ref["LRA"])):
        e = K.db_error(got.cpu().numpy(), want)
        _note(f"{name} dB", e)
        assert e <= K.DB_TOL, f"{what}: {name} off by {e:.3e} dB"
    return I


@pytest.mark.parametrize("fs,C", [(8000, 1), (8000, 2), (11025, 5), (48000, 2)])
def test_meter_at_every_path_length(fs, C):
    for L in K.lengths(fs):
        x, ref = K.case(fs, C, L, 3, seed=L)
        _check_meter(x, ref, fs, what=f"fs={fs} C={C} L={L}")


def _chunks_read(L, fs):
    """Chunks of the segment-power passes: only the samples below s_n_seg are read."""
    chunk = ops.loudness_constants()["chunk"]
    return -(-LD.segment_start(LD.n_segments(L, fs), fs) // chunk)


def test_meter_batch_of_33_at_65537_samples():
    # 65 537 samples hold 59 whole segments at 11 025 Hz: 65 047 samples are read, 255 chunks, the one-launch scan at its top
    assert _chunks_read(65537, 11025) == 255 <= ops.sosfilt_constants()["two_level_chunks"]
    x, ref = K.case(11025, 2, 65537, 33, seed=7)
    _check_meter(x, ref, 11025, what="B=33 L=65537")


@pytest.mark.parametrize("fs,L", [(11025, 66151), (8000, 66401)])
def test_meter_batch_of_33_runs_the_segmented_scan(fs, L):
    two_level = ops.sosfilt_constants()["two_level_chunks"]
    assert two_level < _chunks_read(L, fs) <= two_level + 4          # just past the threshold: 259 and 260 chunks
    x, ref = K.case(fs, 2, L, 33, seed=9)
    _check_meter(x, ref, fs, what=f"segmented scan, B=33 fs={fs} L={L}")
    one = ops.loudness_segments(_dev(x[5:6]), fs)                     # a row of the batch alone: the same bits
    assert torch.equal(one, ops.loudness_segments(_dev(x), fs)[5:6])


def test_meter_44100_five_channels_default_and_explicit_weights():
    L = LD.segment_start(30, 44100) + 1
    x, ref = K.case(44100, 5, L, 3, seed=3)
    _check_meter(x, ref, 44100, what="5 channels")
    w = (0.5, 2.0, 0.0, 1.0, 1.41)
    x, ref = K.case(44100, 5, L, 1, seed=4, weights=w)
    _check_meter(x, ref, 44100, weights=list(w), what="explicit weights")


def test_meter_one_row_of_2_20_samples():
    x, ref = K.case(48000, 1, 1 << 20, 1, seed=11)
    _check_meter(x, ref, 48000, what="2^20")
    e = K.db_error(LN.integrated_loudness_batch(_dev(x[:, 0]), 48000).cpu().numpy(), ref["I"])       # [B, L] mono
    assert e <= K.DB_TOL


def test_strided_rows_and_channels_batch_equals_rows_and_call_equals_call():
    fs, C, L, B = 8000, 2, 24001, 3
    x, ref = K.case(fs, C, L, B, seed=24001)
    xd = _dev(x)
    wide = torch.full((C, B + 1, L + 37), float("nan"), dtype=torch.float32, device="cuda")
    xs = wide[:, 1:, 5:5 + L].permute(1, 0, 2)                    # channel-major storage, rows 4-byte aligned only
    xs.copy_(xd)
    assert xs.stride(2) == 1 and xs.stride(0) < xs.stride(1)

    def meter(t):
        seg = ops.loudness_segments(t, fs)
        M, S, I, thr = ops.loudness_blocks(seg, fs)
        return [seg, M, S, I, ops.loudness_range(S, thr), ops.true_peak(t, fs)]
    a, again, strided = meter(xd), meter(xd), meter(xs)
    for u, v, w in zip(a, again, strided):
        assert torch.equal(u, v), "the same call gave other bits"
        assert torch.equal(u, w), "strided rows gave other bits than contiguous ones"
    for b in range(B):
        for u, v in zip(a, meter(xd[b:b + 1])):
            assert torch.equal(u[b:b + 1], v), "a batch differs from its rows"
    _check_meter(xs.cpu().numpy(), ref, fs, what="strided")


def test_silence_and_rows_without_a_block():
    fs = 8000
    s4 = LD.segment_start(4, fs)
    x, ref = K.case(fs, 2, 40000, 2, seed=5)
    x = np.concatenate([x, np.zeros((1, 2, 40000), np.float32), 1e-5 * x[:1]])   # silence, and a clip under the absolute gate
    xd = _dev(x)
    M, S, I, thr = ops.loudness_blocks(ops.loudness_segments(xd, fs), fs)
    lra, tp = ops.loudness_range(S, thr), ops.true_peak(xd, fs)
    I = I.cpu().numpy()
    assert np.isneginf(I[2]) and np.isneginf(I[3]) and K.db_error(I[:2], ref["I"]) <= K.DB_TOL
    assert torch.isneginf(M[2]).all() and torch.isneginf(S[2]).all() and lra[2].item() == 0.0 and lra[3].item() == 0.0
    assert tp[2].item() == 0.0 and torch.isneginf(LN.true_peak_batch(xd, fs, db=True)[2])
    assert torch.isfinite(M[3]).any() and (M[3] < -70).all()
    out, g, I2 = ops.normalize_loudness(xd, fs, -16.0, return_gain=True)
    assert torch.equal(out[2:], xd[2:]) and g[2].item() == 1.0 and g[3].item() == 1.0      # copied bit for bit
    assert torch.equal(I2, torch.from_numpy(I).cuda())
    # one sample short of the first block: no block, -inf, no NaN, nothing launched for the segments' sake
    short = _dev(x[:, :, :s4 - 1])
    M, S, I, thr = ops.loudness_blocks(ops.loudness_segments(short, fs), fs)
    assert M.shape == (4, 0) and S.shape == (4, 0) and torch.isneginf(I).all() and (ops.loudness_range(S, thr) == 0).all()
    out = ops.normalize_loudness(short, fs)
    assert torch.equal(out, short)
    tiny = _dev(x[:1, :, :100])                                                    # shorter than one segment
    assert ops.loudness_segments(tiny, fs).shape == (1, 2, 0) and torch.isneginf(ops.integrated_loudness(tiny, fs)).all()
    assert LN.loudness_metrics(x[0, :, :100], fs)["I"] == -np.inf


@pytest.mark.parametrize("fs,up", [(48000, 4), (96000, 2), (192000, 1)])
def test_true_peak_tiers_against_the_reference_and_resample_poly(fs, up):
    assert LD.true_peak_up(fs) == up
    for L in (1, 255, 1025, 24001):
        x, _ = K.case(8000, 2, 24001, 3, seed=24001)               # any noise will do: the rate only picks the tier
        x = x[:, :, :L]
        xd = _dev(x)
        tp = ops.true_peak(xd, fs)
        want = np.array([R.true_peak(c, fs) for c in x])
        e = K.db_error(20 * np.log10(tp.cpu().numpy().astype(np.float64)), 20 * np.log10(want))
        _note(f"dBTP up={up}", e)
        assert e <= K.DB_TOL
        over = ops.resample_poly(xd.reshape(-1, L), up, 1).reshape(3, 2, -1) if up > 1 else xd
        assert torch.equal(tp, over.abs().amax(dim=(1, 2))), "not resample_poly's own values"


def test_true_peak_of_unit_impulses_is_the_filters_phase_maxima():
    fs, L = 48000, 4099
    plan, _ = ops.resample_plan(4, 1, L)
    x = np.zeros((4, 1, L), dtype=np.float32)
    for b, pos in enumerate((0, 1000, 2048, L - 1)):                # first sample, mid-tile, a tile's edge, last sample
        x[b, 0, pos] = 1.0
    tp = ops.true_peak(_dev(x), fs).cpu().numpy()
    assert np.all(tp == np.max(np.abs(plan.table)))                 # tap times one, plus zeros: the taps themselves
    assert abs(tp[0] - 1.0) < 1e-3                                  # the filter's centre tap
    x2 = np.stack([-0.5 * x[1, 0], x[1, 0]])[None]                  # [1, 2, L]: the louder channel decides
    assert ops.true_peak(_dev(x2), fs).item() == tp[1]


def test_true_peak_of_a_quarter_rate_sine():
    fs = 48000
    n = np.arange(fs // 2)
    x = np.sin(2 * np.pi * n / 4 + np.pi / 4).astype(np.float32)[None]
    d = LN.true_peak_batch(_dev(x), fs, db=True).item()
    assert abs(np.max(np.abs(x)) - 0.7071) < 1e-4 and -0.4 <= d <= 0.2
    assert abs(d - R.dbtp(R.true_peak(x, fs))) <= K.DB_TOL


def test_normalisation_hits_the_target_and_respects_the_peak_limit():
    fs = 8000
    x, ref = K.case(fs, 2, 40000, 3, seed=5)
    xd = _dev(x)
    out, g, I = ops.normalize_loudness(xd, fs, -23.0, return_gain=True)
    want_g = np.array([R.gain(ref["I"][b], 0.0, -23.0) for b in range(3)])
    assert np.max(np.abs(g.cpu().numpy() / want_g - 1)) <= 1e-4 * np.log(10) / 20      # 1e-4 dB of gain
    assert K.db_error(I.cpu().numpy(), ref["I"]) <= K.DB_TOL
    e = float((ops.integrated_loudness(out, fs) + 23.0).abs().max())
    _note("re-measured I - target (LU)", e)
    assert e <= 1e-3
    for b in range(3):
        y, _, _ = R.normalize(x[b], fs, -23.0)
        assert np.max(np.abs(out[b].cpu().numpy() - y)) <= 2 ** -22 * np.max(np.abs(y))      # one float32 rounding apart
    # a target the peak limit forbids: the limit decides the gain
    limit = -1.0
    out, g, I = ops.normalize_loudness(xd, fs, -6.0, peak_limit_dbtp=limit, return_gain=True)
    want_g = np.array([R.gain(ref["I"][b], ref["TP"][b], -6.0, limit) for b in range(3)])
    assert np.all(want_g < 10 ** ((-6.0 - ref["I"]) / 20)), "the case does not exercise the limit"
    assert np.max(np.abs(g.cpu().numpy() / want_g - 1)) <= 1e-5
    d = LN.true_peak_batch(out, fs, db=True).cpu().numpy()
    _note("dBTP over the limit", float(np.max(d - limit)))
    assert np.all(d <= limit + K.DB_TOL)
    # the mirrors: NumPy in, NumPy out
    y = LN.normalize_loudness(x[0], fs, -30.0)
    assert y.shape == x[0].shape and y.dtype == np.float64 and abs(LN.integrated_loudness(y, fs) + 30.0) <= 1e-3
    m = LN.loudness_metrics(x[1], fs)
    assert set(m) == {"I", "LRA", "TP_dbtp", "M_max", "S_max"} and abs(m["I"] - ref["I"][1]) <= K.DB_TOL
    assert abs(m["LRA"] - ref["LRA"][1]) <= K.DB_TOL and abs(m["M_max"] - ref["M"][1].max()) <= K.DB_TOL
    assert abs(m["TP_dbtp"] - R.dbtp(ref["TP"][1])) <= K.DB_TOL and abs(m["S_max"] - ref["S"][1].max()) <= K.DB_TOL
    mono = LN.normalize_loudness(x[0, 0], fs, -20.0)
    assert mono.shape == (40000,) and abs(LN.integrated_loudness(mono, fs) + 20.0) <= 1e-3


def test_gain_rows_in_place_and_strided_out():
    x, _ = K.case(8000, 2, 24001, 3, seed=24001)
    xd = _dev(x)
    g = torch.tensor([0.5, 1.0, 3.0], dtype=torch.float64, device="cuda")
    want = (xd.double() * g[:, None, None]).float()
    assert torch.equal(ops.gain_rows(xd, g), want)
    buf = xd.clone()
    assert ops.gain_rows(buf, g, out=buf) is buf and torch.equal(buf, want)
    assert torch.equal(ops.gain_rows(xd[:, 0], g), want[:, 0])        # [B, L] rows of a strided view


def test_get_basic_audio_metrics_keeps_its_keys():
    from sygnals_amd.core.audio import features as af
    y = np.sin(np.arange(800) * 0.1)
    m = af.get_basic_audio_metrics(y, 8000)
    assert set(m) == {"duration_seconds", "rms_global", "peak_amplitude"}
    assert abs(m["duration_seconds"] - 0.1) < 1e-12 and abs(m["peak_amplitude"] - np.max(np.abs(y))) < 1e-6
