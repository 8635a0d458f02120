"""yin / pyin on the device away from the C2-C7 / win 1024 / hop 512 setting of tests/test_gpu_pitch.py: the frame kernel
at other win_length, hop, fmin / fmax, sample rates, strided rows, short lengths and quiet or loud input; the Viterbi
kernel's table forms (R == n, width > n, width == 1, a single bin, LDS above 64 KiB) and launch shapes; and the public
fundamental_frequency / jitter / shimmer at the settings their callers use.  Everything is checked against the float64
restatement of tests/pitch_ref.py with the rules of tests/test_gpu_pitch.py."""
import multiprocessing as mp
import warnings

import numpy as np
import pytest

from sygnals_amd import _pitch as P
from tests import pitch_ref as R
from tests.gpu_util import EPS32, assert_parity
from tests.test_gpu_pitch import (_margin_frames, _mixed_clips, _pack, _vibrato_clips, check_emission_frame,
                                  host_frames)

pytestmark = pytest.mark.gpu

NF = 2048

# (id, sr, fmin, fmax, win_length, hop); the derived constants are in the comments (sygnals_amd/_pitch.py)
CASES = {
    "jitter": (22050, 75.0, 600.0, 1024, 512),      # the jitter / shimmer setting: n_bins 361, lags 36..294
    "sr96k": (96000, P.C2, P.C7, 1024, 512),        # max_p clipped to 1023
    "w1536": (48000, P.C2, P.C7, 1536, 512),        # W = 1536, max_p clipped to 511
    "w256": (48000, 30.0, 1000.0, 256, 441),        # W = 256, n_lag 1553, hop not a power of two
    "w64": (48000, 1.5, 24000.0, 64, 512),          # n_lag 1982, K 992, n_bins 1676 (Viterbi LDS > 64 KiB)
    "nlag13": (8000, 400.0, 1000.0, 1024, 160),     # n_lag 13: most lanes idle in the trough ballots
    "hop4096": (44100, P.C2, P.C7, 1024, 4096),     # hop > frame_length
}
FRAME_GRID = [(k, True) for k in CASES] + [(k, False) for k in ("jitter", "w256", "w64", "hop4096")]


def _ops():
    from sygnals_amd import ops
    return ops


def _clips(sr, secs=1.0, n_vib=4, seed=21):
    L = int(sr * secs)
    return np.concatenate([_mixed_clips(sr, L), _vibrato_clips(n_vib, sr, secs, seed=seed)])


def _ref_cmndf(y, case, center):
    sr, fmin, fmax, win, hop = CASES[case] if isinstance(case, str) else case
    min_p, max_p = P.periods(sr, fmin, fmax, NF, win)
    return R.cmndf(R.frames(y, NF, hop, center), win, min_p, max_p)


def _check_cmndf(cm, Y, case, center, what):
    """CMNDF parity: every lag is held to 1e-5 of its frame's peak first (assert_parity's gate).  A lag that misses it
    falls back to the float32 FFT floor propagated to the CMNDF: the float32 acf carries an error of a few
    eps32 * sum(x^2) of the whole 2048-sample frame (gpu_util.fft_floor), while d(tau) and its cumulative mean are sums
    over W samples, so at small W that floor can exceed 1e-5 of the CMNDF.  Fallback lags are counted; the caller caps
    them at 1 % of the case's lags.  Returns (fallback lags, lags, worst error / (1e-5 * peak))."""
    sr, fmin, fmax, win, hop = CASES[case] if isinstance(case, str) else case
    min_p, max_p = P.periods(sr, fmin, fmax, NF, win)
    n_fall = n_tot = 0
    worst = 0.0
    for b in range(len(Y)):
        fx = R.frames(Y[b], NF, hop, center)
        ref = R.cmndf(fx, win, min_p, max_p)
        assert cm.shape[1] == ref.shape[0], f"{what}: T = {cm.shape[1]}, reference {ref.shape[0]}"
        dev = cm[b].astype(np.float64)
        assert dev.shape == ref.shape and np.isfinite(dev).all(), f"{what} clip {b}: shape or non-finite"
        gate = 1e-5 * np.max(np.abs(ref), axis=1, keepdims=True) + 1e-30
        err = np.abs(dev - ref)
        worst = max(worst, float(np.max(err / gate)))
        miss = err > gate
        if miss.any():
            acf, en = R.acf_energy(fx, win)
            acf[np.abs(acf) < 1e-6] = 0
            en[np.abs(en) < 1e-6] = 0
            d = en[:, :1] + en - 2 * acf
            cmean = np.cumsum(d[:, 1:max_p + 1], axis=1)[:, min_p - 1:] / np.arange(min_p, max_p + 1)[None, :]
            floor = 8 * EPS32 * np.sum(fx ** 2, axis=1)
            bound = floor[:, None] * (1 + np.abs(ref)) / np.maximum(cmean, 1e-300)
            bad = miss & (err > bound)
            assert not bad.any(), f"{what} clip {b}: {int(bad.sum())} lags miss 1e-5 and the propagated fp32 floor " \
                                  f"(first at frame {np.argwhere(bad)[0][0]})"
            n_fall += int(miss.sum())
        n_tot += ref.size
    return n_fall, n_tot, worst


def _check_yin(f0, Y, case, center, thr, what):
    """test_yin_period_index's rule: same period index outside the float64 near-tie margin, f0 within 1e-5 there;
    returns (margin frames, frames, flat frames); the caller caps the margin at 1 %.

    A frame holding a single sample (L = 1) has d(tau) = 2 x^2 at every lag: its CMNDF is 1 up to float64 rounding, a
    tie over all lags.  Such flat frames are held to the float32 rule instead (no trough, first minimum: lag 0) and
    leave the margin count."""
    sr, fmin, fmax, win, hop = CASES[case] if isinstance(case, str) else case
    min_p, _ = P.periods(sr, fmin, fmax, NF, win)
    n_margin = n_tot = n_flat = 0
    for b in range(len(Y)):
        ref = _ref_cmndf(Y[b], case, center)
        idx, rf0 = R.yin_from_cmndf(ref, sr, min_p, trough_threshold=thr)
        flat = (np.ptp(ref, axis=1) < 1e-12) & (np.abs(ref).max(axis=1) > 0)
        assert np.all(f0[b][flat] == np.float32(sr / min_p)), f"{what} clip {b}: flat frame off lag 0"
        n_flat += int(flat.sum())
        margin = _margin_frames(ref, idx, thr=thr) & ~flat
        rf0 = np.where(flat, np.float32(sr / min_p), rf0)
        agree = np.abs(sr / f0[b] - sr / rf0) < 0.5
        assert np.all(agree | margin), f"{what} clip {b}: period index differs outside the margin at " \
                                       f"{np.nonzero(~(agree | margin))[0].tolist()}"
        ok = agree & ~margin
        assert np.all(np.abs(f0[b][ok] - rf0[ok]) <= 1e-5 * rf0[ok]), f"{what} clip {b}: f0 beyond 1e-5"
        n_margin += int(margin.sum())
        n_tot += len(idx)
    return n_margin, n_tot, n_flat


def _check_emission(h, case, what):
    """pYIN candidate lists on the device CMNDF (check_emission_frame); returns (half-bin frames skipped, frames)."""
    sr, fmin = CASES[case][:2] if isinstance(case, str) else case[:2]
    skipped = 0
    B = h["cand_count"].shape[0]
    for b in range(B):
        for t in range(h["T"]):
            skipped += not check_emission_frame(h, b, t, sr, fmin)
    return skipped, B * h["T"]


def _report(what, n, tot):
    print(f"{what}: {n} exempt of {tot} (cap {int(0.01 * tot)})")
    assert n <= 0.01 * tot, f"{what}: {n} exempt of {tot} (> 1 %)"


# ------------------------------------------------------------------------------------------------ 1. frame-stage matrix
@pytest.mark.parametrize("case,center", FRAME_GRID)
def test_frame_stage_matrix(case, center):
    ops = _ops()
    sr, fmin, fmax, win, hop = CASES[case]
    Y = _clips(sr, 2.0 if hop > NF else 1.0)
    y = ops.to_device_f32(Y)
    yin = host_frames(ops.pitch_frames(y, sr, fmin, fmax, win_length=win, hop=hop, center=center, mode="yin",
                                       want_cmndf=True))
    assert yin["T"] == P.num_frames(Y.shape[1], NF, hop, center)
    n_fl, n_lags, worst = _check_cmndf(yin["cmndf"], Y, case, center, f"{case} center={center}")
    print(f"cmndf {case} center={center}: worst error {worst * 1e-5:.2e} of the frame peak")
    _report(f"cmndf {case} center={center} lags past 1e-5 (held to the fp32 floor)", n_fl, n_lags)
    _report(f"yin {case} center={center} margin frames", *_check_yin(yin["f0"], Y, case, center, 0.1, case)[:2])
    py = host_frames(ops.pitch_frames(y, sr, fmin, fmax, win_length=win, hop=hop, center=center, mode="pyin",
                                      want_cmndf=True))
    assert py["n_bins"] == P.n_pitch_bins(fmin, fmax) and py["K"] == P.cand_stride(py["max_p"] - py["min_p"] + 1)
    assert np.array_equal(py["cmndf"], yin["cmndf"]), "the CMNDF depends on the mode"
    assert int(py["cand_count"].max()) <= py["K"]
    _report(f"pyin {case} center={center} half-bin frames", *_check_emission(py, case, case))


@pytest.mark.parametrize("thr", [0.05, 0.3])
def test_yin_trough_threshold(thr):
    ops = _ops()
    case = "jitter"
    sr, fmin, fmax, win, hop = CASES[case]
    Y = _clips(sr, n_vib=8, seed=int(thr * 100))
    fr = ops.pitch_frames(ops.to_device_f32(Y), sr, fmin, fmax, win_length=win, hop=hop, mode="yin",
                          trough_threshold=thr)
    _report(f"yin thr={thr} margin frames", *_check_yin(fr["f0"].cpu().numpy(), Y, case, True, thr, f"thr={thr}")[:2])


def test_pyin_trough_on_a_threshold():
    """A trough whose float32 CMNDF equals a pYIN threshold exactly (0.25, representable in float32) is NOT below it
    (librosa: h < threshold).  A sine plus noise whose noise scale is swept in relative steps of 5e-9 around the value
    that puts the float64 trough at 0.25 moves the trough by ~2e-9 a clip (a float32 ulp there is 1.5e-8 / 3e-8) over
    +-1.5e-5: some clips' device CMNDF hits 0.25 exactly, and their emission must still match the restatement (every
    such clip, and every 16th clip besides)."""
    ops = _ops()
    sr, f, B, thr = 22050, 220.0, 16384, 0.25
    min_p, max_p = P.periods(sr, P.C2, P.C7, NF, 1024)
    t = np.arange(NF) / sr
    noise = np.random.default_rng(5).standard_normal(NF)
    lag = int(round(sr / f)) - min_p
    clip = lambda a: (np.sin(2 * np.pi * f * t) + a * noise).astype(np.float32)

    def trough(a):
        c = R.cmndf(R.frames(clip(a), NF, 512, False), 1024, min_p, max_p)[0]
        return c[lag - 3 + int(np.argmin(c[lag - 3:lag + 4]))]

    lo, hi = 0.01, 2.0                                   # trough value grows with the noise scale
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if trough(mid) < thr else (lo, mid)
    Y = np.stack([clip(mid * (1 + 5e-9 * (b - B // 2))) for b in range(B)])
    h = host_frames(ops.pitch_frames(ops.to_device_f32(Y), sr, P.C2, P.C7, center=False, mode="pyin", want_cmndf=True))
    c = h["cmndf"][:, 0]
    on = np.array([bool(np.any(R.troughs(c[b].astype(np.float64)) & (c[b] == np.float32(thr)))) for b in range(B)])
    assert on.sum() >= 1, "no clip put a trough exactly on the threshold"
    sel = np.nonzero(on | (np.arange(B) % 16 == 0))[0]
    skipped = sum(not check_emission_frame(h, b, 0, sr, P.C2) for b in sel)
    print(f"{int(on.sum())} clips with a trough at exactly {thr}; {skipped} half-bin frames of {len(sel)}")
    assert skipped <= 0.01 * len(sel) and not any(not check_emission_frame(h, b, 0, sr, P.C2) for b in np.nonzero(on)[0])


# ------------------------------------------------------------------------------------------------ 2. layout and lengths
def test_strided_rows_bit_identical():
    import torch
    ops = _ops()
    case = "w256"
    sr, fmin, fmax, win, hop = CASES[case]
    Y = _clips(sr)
    B, L = Y.shape
    big = torch.full((B, L + 777), 1e3, dtype=torch.float32, device=ops.require_gpu())   # loud tail: an over-read shows
    big[:, :L] = ops.to_device_f32(Y)
    ys = big[:, :L]
    assert ys.stride(1) == 1 and ops._ld(ys) == L + 777
    yc = ys.contiguous()
    for mode in ("yin", "pyin"):
        a = host_frames(ops.pitch_frames(ys, sr, fmin, fmax, win_length=win, hop=hop, mode=mode, want_cmndf=True))
        c = host_frames(ops.pitch_frames(yc, sr, fmin, fmax, win_length=win, hop=hop, mode=mode, want_cmndf=True))
        keys = ("f0", "cmndf") if mode == "yin" else ("cmndf", "cand_count", "voiced_prob")
        for k in keys:
            assert np.array_equal(a[k], c[k], equal_nan=True), f"{mode}: {k} differs between strided and contiguous"
        if mode == "pyin":
            for b in range(B):
                for t in range(a["T"]):
                    n = a["cand_count"][b, t]
                    assert np.array_equal(a["cand_bin"][b, t, :n], c["cand_bin"][b, t, :n])
                    assert np.array_equal(a["cand_prob"][b, t, :n], c["cand_prob"][b, t, :n])
            _report("strided cmndf lags past 1e-5 (held to the fp32 floor)", *_check_cmndf(a["cmndf"], Y, case, True,
                                                                                        "strided")[:2])
            _report("strided half-bin frames", *_check_emission(a, case, "strided"))


LENGTHS = [(1, True), (700, True), (2047, True), (2048, True), (2049, True), (48001, True),
           (2048, False), (2049, False), (2048 + 511, False)]


@pytest.mark.parametrize("L,center", LENGTHS)
@pytest.mark.parametrize("case", ["sr48k", "w256"])
def test_short_and_awkward_lengths(L, center, case):
    ops = _ops()
    cfg = (48000, P.C2, P.C7, 1024, 512) if case == "sr48k" else CASES[case]
    sr, fmin, fmax, win, hop = cfg
    Y = _clips(sr, secs=max(L, 2) / sr + 1e-9, seed=L)[:, :L]
    assert Y.shape[1] == L
    y = ops.to_device_f32(Y)
    yin = host_frames(ops.pitch_frames(y, sr, fmin, fmax, win_length=win, hop=hop, center=center, mode="yin",
                                       want_cmndf=True))
    assert yin["T"] == P.num_frames(L, NF, hop, center) == yin["cmndf"].shape[1]
    n_fl, n_lags, _ = _check_cmndf(yin["cmndf"], Y, cfg, center, f"L={L}")
    _report(f"L={L} center={center} {case} cmndf lags past 1e-5 (held to the fp32 floor)", n_fl, n_lags)
    n_m, n_t, n_flat = _check_yin(yin["f0"], Y, cfg, center, 0.1, f"L={L}")
    py = host_frames(ops.pitch_frames(y, sr, fmin, fmax, win_length=win, hop=hop, center=center, mode="pyin",
                                      want_cmndf=True))
    n_h, _ = _check_emission(py, cfg, f"L={L}")
    print(f"L={L} center={center} {case}: {n_m} margin (besides {n_flat} flat), {n_h} half-bin of {n_t} frames")
    assert n_m + n_h <= 0.01 * n_t


def test_too_short_raises_and_launches_nothing(monkeypatch):
    ops = _ops()
    y = ops.to_device_f32(np.ones((2, NF - 1), np.float32))
    calls = []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            raise AssertionError(f"{name} called")

    monkeypatch.setattr(ops, "lib", lambda: Spy())
    for mode in ("yin", "pyin"):
        with pytest.raises(ValueError, match="too short"):
            ops.pitch_frames(y, 48000, P.C2, P.C7, center=False, mode=mode)
    with pytest.raises(ValueError, match="too short"):
        ops.pitch_pyin(y, 48000, P.C2, P.C7, center=False)
    assert calls == []


# ------------------------------------------------------------------------------------------------ 3. amplitude sweep
AMP_DELTA = 1e-2    # a lag is exempt when the float64 |acf| or |e| lies within 1 % of librosa's 1e-6 clamp


@pytest.mark.parametrize("scale", [1e-4, 1e-3, 1e-2, 1.0, 30.0])
def test_cmndf_amplitude_sweep(scale):
    """The kernel clamps |acf| < 1e-6 on its float32 FFT output, the restatement on float64 values.  The float32 FFT's
    error is a few eps32 * sum(x^2) of the frame (gpu_util.fft_floor): below 1 % of 1e-6 at every scale where a flipped
    clamp moves the CMNDF by more than the tolerance (scale <= 1e-2), so lags whose float64 |acf| or |e| lie within
    1 % of 1e-6 are the only ones exempt; every other lag is held to 1e-5.  A frame whose e(0) is that close is exempt
    as a whole (e(0) enters every lag)."""
    ops = _ops()
    sr = 22050
    Y = (np.concatenate([_mixed_clips(sr, sr), _vibrato_clips(4, sr, 1.0, seed=7)]) * np.float32(scale)).astype(np.float32)
    min_p, max_p = P.periods(sr, P.C2, P.C7, NF, 1024)
    fr = host_frames(ops.pitch_frames(ops.to_device_f32(Y), sr, P.C2, P.C7, mode="pyin", want_cmndf=True))
    cm = fr["cmndf"]
    near = lambda v: np.abs(np.abs(v) - 1e-6) <= AMP_DELTA * 1e-6
    n_ex = n_tot = 0
    for b in range(len(Y)):
        fx = R.frames(Y[b])
        acf, en = R.acf_energy(fx, 1024)
        ref = R.cmndf(fx, 1024, min_p, max_p)
        ex = near(acf[:, min_p:max_p + 1]) | near(en[:, min_p:max_p + 1]) | near(en[:, :1])
        for t in range(ref.shape[0]):
            keep = ~ex[t]
            if keep.any():
                assert_parity(cm[b, t][keep], ref[t][keep], 1e-5, f"scale {scale} clip {b} frame {t}")
        n_ex += int(ex.sum())
        n_tot += ex.size
    _report(f"scale {scale:g} clamp-exempt lags", n_ex, n_tot)
    n_h, n_f = _check_emission(fr, (sr, P.C2), f"scale {scale:g}")
    _report(f"scale {scale:g} half-bin frames", n_h, n_f)


# ------------------------------------------------------------------------------------------------ 4. Viterbi branches
def _synthetic(n, B, Tn, K, seed, mode="walk"):
    """Candidate lists like test_viterbi_exact's: a random walk with up to K bins a frame (mode 'walk'), every
    candidate on bin 0 / n - 1 ('edges'), no candidate ('silent') or exactly K candidates a frame ('full')."""
    rng = np.random.default_rng(seed)
    cands, vps = [], []
    for b in range(B):
        cl, vl = [], []
        f = rng.uniform(0, n)
        for t in range(Tn):
            if mode == "silent":
                cl.append((np.zeros(0, np.int64), np.zeros(0))); vl.append(0.0); continue
            if mode == "edges":
                bins = np.array([0]) if (t + b) % 3 == 0 else (np.array([n - 1]) if (t + b) % 3 == 1 else
                                                               np.unique(np.array([0, n - 1])))
            elif mode == "full":
                bins = np.sort(rng.choice(n, size=K, replace=False)) if n >= K else np.arange(n)
            else:
                f = np.clip(f + rng.normal(0, max(1.0, n / 75)), 0, n - 1)
                k = rng.integers(0, K + 1)
                bins = np.unique(np.clip(np.round(f + rng.normal(0, max(1.0, n / 10), k)), 0, n - 1).astype(np.int64))
            p = rng.uniform(0.01, 1.0 / max(1, len(bins)), len(bins)).astype(np.float32).astype(np.float64)
            cl.append((bins, p)); vl.append(float(np.float32(min(1.0, p.sum()))))
        cands.append(cl); vps.append(vl)
    return cands, vps


def _run_viterbi(n, width, cands, vps, K):
    import torch
    ops = _ops()
    cb, cp, cc, vp32 = _pack(cands, vps, K)
    dev = lambda a: torch.from_numpy(a).cuda()
    f0, voiced, st = ops.pyin_viterbi(dev(cb), dev(cp), dev(cc), dev(vp32), n, width, P.C2)
    return f0.cpu().numpy(), voiced.cpu().numpy(), st.cpu().numpy(), cp, vp32


def _check_viterbi(n, width, cands, vps, K, dense=True):
    f0, voiced, st, cp, vp32 = _run_viterbi(n, width, cands, vps, K)
    for b in range(len(cands)):
        obs = R.emission_matrix([(bb, cp[b, t, :len(bb)].astype(np.float64)) for t, (bb, _) in enumerate(cands[b])],
                                vp32[b].astype(np.float64), n)
        ref = R.viterbi_band(obs, n, width)
        assert np.array_equal(st[b], ref), f"n={n} width={width} clip {b}: {np.count_nonzero(st[b] != ref)} states differ"
        if dense and 2 * n <= 200:
            p_init = np.zeros(2 * n)
            p_init[n:] = 1 / n
            sd, _ = R.viterbi_dense(obs, R.full_transition(n, width), p_init)
            assert np.array_equal(sd, ref), f"n={n} width={width} clip {b}: band != dense"
        rf0, rv = R.states_to_f0(ref, n, P.C2)
        np.testing.assert_array_equal(voiced[b], rv)
        np.testing.assert_allclose(f0[b][rv], rf0[rv], rtol=1e-6)
        assert np.all(np.isnan(f0[b][~rv]))


# (n, width, B, T): R == n and width > n; width == n; jitter's range at hop 2048 / 16 kHz; h = 0 (hop 32 / 48 kHz);
# a single pitch bin; n_bins 1676 (5 n doubles of LDS > 64 KiB); an even n below the width.  The kernel and the
# restatement share _pitch's tables, so this checks the kernel on those tables; the even-n centring of
# transition_local itself is pinned on the host by test_pitch_ref.py::test_transition_wider_than_states
TABLE_FORMS = [(39, 141, 8, 60), (51, 51, 8, 60), (361, 551, 2, 16), (601, 1, 8, 60), (1, 1, 4, 40), (1, 51, 4, 40),
               (1676, 51, 2, 24), (40, 51, 8, 60)]


@pytest.mark.parametrize("n,width,B,Tn", TABLE_FORMS)
def test_viterbi_table_forms(n, width, B, Tn):
    tabs, Rr, h = P.transition_tables(n, width)
    assert (Rr == n) == (n <= 2 * h + 1)
    _check_viterbi(n, width, *_synthetic(n, B, Tn, 6, seed=n * 1000 + width), K=6)


@pytest.mark.parametrize("B,Tn", [(1, 1), (1, 40), (255, 6), (256, 6), (257, 6), (257, 1)])
def test_viterbi_launch_shapes(B, Tn):
    n, width = 61, 21                            # 1024 threads below 256 clips, 256 from 256 clips on
    _check_viterbi(n, width, *_synthetic(n, B, Tn, 5, seed=B * 7 + Tn), K=5)


@pytest.mark.parametrize("mode", ["edges", "silent", "full"])
@pytest.mark.parametrize("n,width", [(601, 51), (39, 141), (1, 1)])
def test_viterbi_candidate_edges(mode, n, width):
    K = min(n, 8)
    _check_viterbi(n, width, *_synthetic(n, 4, 40, K, seed=len(mode) + n, mode=mode), K=K)


# ------------------------------------------------------------------------------------------------ 5. public API
def _pool_pyin_args(args):
    y, sr, fmin, fmax, win, hop, center = args
    r = R.pyin(y.astype(np.float64), sr, fmin, fmax, NF, win, hop, center)
    return r["f0"], r["voiced"], r["vps"]


def _bins(f0, v):
    return np.where(v, np.round(120 * np.log2(np.where(v, f0, 75.0) / 75.0)), -1)


@pytest.mark.parametrize("hop", [256, 2048])
def test_fundamental_frequency_params(hop):
    from sygnals_amd.core.audio.features import fundamental_frequency, fundamental_frequency_batch
    sr, fmin, fmax, win = 16000, 75.0, 600.0, 1536
    B = 16
    Y = _vibrato_clips(B, sr, 2.0 if hop < 1024 else 6.0, seed=hop)
    times, f0, vf, vp = fundamental_frequency_batch(Y, sr, fmin, fmax, "pyin", hop, win_length=win, center=False)
    f0, vf, vp = f0.cpu().numpy(), vf.cpu().numpy() > 0.5, vp.cpu().numpy()
    Tn = P.num_frames(Y.shape[1], NF, hop, False)
    assert f0.shape == (B, Tn) and np.allclose(times, np.arange(Tn) * hop / sr)
    with mp.get_context("spawn").Pool(min(16, B)) as pool:
        refs = pool.map(_pool_pyin_args, [(Y[b], sr, fmin, fmax, win, hop, False) for b in range(B)])
    agree = tot = vp_bad = 0
    for b, (rf0, rv, rvp) in enumerate(refs):
        agree += int(np.sum((vf[b] == rv) & (_bins(f0[b], vf[b]) == _bins(rf0, rv))))
        tot += len(rv)
        vp_bad += int(np.sum(np.abs(vp[b] - rvp) > 1e-4))
    assert agree >= 0.99 * tot, f"voicing + bin agree on {agree / tot:.4f} of frames"
    assert vp_bad <= 0.01 * tot, f"voiced_prob off by > 1e-4 on {vp_bad} of {tot} frames"
    # the single-clip entry point is the batch's row
    _, g0, gv, gp = fundamental_frequency(Y[3].astype(np.float64), sr, fmin, fmax, "pyin", hop, win_length=win,
                                          center=False)
    assert np.array_equal(np.nan_to_num(g0, nan=-1), np.nan_to_num(f0[3].astype(np.float64), nan=-1))
    assert np.array_equal(gv > 0.5, vf[3]) and np.array_equal(gp, vp[3].astype(np.float64))


def test_jitter_shimmer_internal_pyin():
    from sygnals_amd.core.audio.features import jitter, shimmer
    sr = 22050
    Y = _vibrato_clips(6, sr, 1.5, seed=99).astype(np.float64)
    with mp.get_context("spawn").Pool(len(Y)) as pool:
        refs = pool.map(_pool_pyin_args, [(Y[b], sr, 75.0, 600.0, 1024, 512, True) for b in range(len(Y))])
    used = tot = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        for y, (rf0, rv, _) in zip(Y, refs):
            from sygnals_amd.core.audio.features import fundamental_frequency
            _, f0, vf, _ = fundamental_frequency(y, sr, fmin=75.0, fmax=600.0, method="pyin", hop_length=512)
            v = vf > 0.5
            same = (v == rv) & (_bins(f0, v) == _bins(rf0, rv))
            ok = same.copy()
            ok[1:] &= same[:-1]                      # jitter and shimmer of frame t read frames t and t - 1
            used += int(ok.sum())
            tot += len(ok)
            jd, jr = jitter(y, sr), jitter(y, sr, f0=rf0, voiced_flag=rv.astype(np.float64))
            sd, sh = shimmer(y, sr), shimmer(y, sr, voiced_flag=rv.astype(np.float64))
            assert jd.shape == jr.shape == sd.shape == sh.shape == rv.shape
            # device f0 is float32: a period 1 / f0 <= 1 / 75 carries 2^-24 relative, a difference of two of them
            # 2 / (75 * 2^24); 3 / (75 * 2^24) leaves room for the float64 arithmetic
            np.testing.assert_allclose(jd[ok], jr[ok], rtol=0, atol=3.0 / (75.0 * 2 ** 24), equal_nan=True)
            np.testing.assert_array_equal(np.isnan(jd[ok]), np.isnan(jr[ok]))
            np.testing.assert_array_equal(sd[ok], sh[ok])
    assert used >= 0.98 * tot, f"voicing + bins agree at frames t and t - 1 on {used} of {tot}"
