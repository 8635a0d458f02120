"""yin / pyin on the device (syg_pitch_frames_f32, syg_pyin_viterbi_f32) against the float64 restatement of
tests/pitch_ref.py (librosa 0.10, unpinned), and the reference's own pitch tests mirrored."""
import multiprocessing as mp
import warnings

import numpy as np
import pytest

from sygnals_amd import _pitch as P
from tests import pitch_ref as R
from tests.gpu_util import assert_parity

pytestmark = pytest.mark.gpu


def _ops():
    from sygnals_amd import ops
    return ops


def _vibrato_clips(B, sr, secs, snr_db=30.0, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(int(sr * secs)) / sr
    Y = np.empty((B, len(t)), np.float32)
    for b in range(B):
        f = rng.uniform(80, 900)
        ph = 2 * np.pi * np.cumsum(f * (1 + 0.01 * np.sin(2 * np.pi * rng.uniform(3, 7) * t))) / sr
        x = sum(0.4 / k * np.sin(k * ph) for k in (1, 2, 3))
        x = x + rng.standard_normal(len(t)) * np.std(x) * 10 ** (-snr_db / 20)
        Y[b] = x
    return Y


def _mixed_clips(sr, L, seed=1):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / sr
    return np.stack([0.5 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 660 * t),
                     rng.standard_normal(L) * 0.3, np.zeros(L),
                     np.where(t < t[-1] / 2, np.sin(2 * np.pi * 150 * t), 0.0)]).astype(np.float32)


@pytest.mark.parametrize("sr,center", [(48000, True), (22050, True), (16000, True), (48000, False), (16000, False)])
def test_cmndf_parity(sr, center):
    ops = _ops()
    Y = _mixed_clips(sr, sr)
    fr = ops.pitch_frames(ops.to_device_f32(Y), sr, P.C2, P.C7, center=center, mode="yin", want_cmndf=True)
    cm = fr["cmndf"].cpu().numpy()
    for b in range(len(Y)):
        ref = R.cmndf(R.frames(Y[b], 2048, 512, center), 1024, fr["min_p"], fr["max_p"])
        for t in range(ref.shape[0]):
            assert_parity(cm[b, t], ref[t], 1e-5, f"sr={sr} center={center} clip {b} frame {t}")


def _margin_frames(c, idx, thr=0.1, eps=1e-6):
    """Frames whose YIN decision rests on a float64 near-tie: a CMNDF value up to the chosen lag (plus its right
    neighbour) lies within eps of, but not equal to, a neighbour or the threshold; or, on the argmin fallback, the two
    smallest values are that close."""
    T, n = c.shape
    out = np.zeros(T, bool)
    tt = R.troughs(c) & (c < thr)
    for t in range(T):
        row = c[t]
        seg = row[:min(n, idx[t] + 2)]
        d = np.abs(np.diff(seg))
        near = np.any((d < eps) & (d > 0) & (np.minimum(seg[:-1], seg[1:]) < thr + eps)) if len(d) else False
        near |= np.any((np.abs(seg - thr) < eps) & (seg != thr))
        if not tt[t].any():
            s2 = np.sort(row)[:2]
            near |= bool(0 < s2[1] - s2[0] < eps)
        out[t] = near
    return out


@pytest.mark.parametrize("sr", [48000, 22050])
def test_yin_period_index(sr):
    ops = _ops()
    Y = np.concatenate([_mixed_clips(sr, sr), _vibrato_clips(12, sr, 1.0, seed=3)])
    fr = ops.pitch_frames(ops.to_device_f32(Y), sr, P.C2, P.C7, mode="yin", want_cmndf=True)
    f0 = fr["f0"].cpu().numpy()
    n_margin = n_tot = 0
    for b in range(len(Y)):
        ref = R.cmndf(R.frames(Y[b]), 1024, fr["min_p"], fr["max_p"])
        idx, rf0 = R.yin_from_cmndf(ref, sr, fr["min_p"])
        margin = _margin_frames(ref, idx)
        agree = np.abs(sr / f0[b] - sr / rf0) < 0.5              # same period index (|parabolic shift| < 1/2 apart)
        assert np.all(agree | margin), f"clip {b}: period index differs outside the margin"
        ok = agree & ~margin
        assert np.all(np.abs(f0[b][ok] - rf0[ok]) <= 1e-5 * rf0[ok]), f"clip {b}: f0 beyond 1e-5"
        n_margin += int(margin.sum())
        n_tot += len(idx)
    assert n_margin <= 0.01 * n_tot, f"{n_margin} margin frames of {n_tot}"


def _device_candidates(fr, b, t):
    n = int(fr["cand_count"][b, t])
    return fr["cand_bin"][b, t, :n], fr["cand_prob"][b, t, :n]


def check_emission_frame(h, b, t, sr, fmin):
    """pYIN emission of the device frame (b, t) against R.pyin_frame fed the device CMNDF: bins exact, probabilities and
    voiced_prob within 1e-6.  h: pitch_frames output on the host.  Returns False (nothing checked) when a trough's
    120 log2 argument sits within 1e-6 of a rounding point, where the bins may differ."""
    sr = float(sr)
    c = h["cmndf"][b, t].astype(np.float64)
    tr = np.nonzero(R.troughs(c))[0]
    sh = R.parabolic_shifts(c)
    x = 120 * np.log2(sr / (h["min_p"] + tr + sh[tr]) / fmin)
    if np.any(np.abs(np.abs(x - np.floor(x)) - 0.5) < 1e-6):
        return False
    rb, rp, rvp = R.pyin_frame(c, sr, h["min_p"], fmin, h["n_bins"])
    db, dp = _device_candidates(h, b, t)
    where = f"clip {b} frame {t}"
    assert sorted(db.tolist()) == sorted(rb.tolist()), where
    np.testing.assert_allclose(dp[np.argsort(db)], rp[np.argsort(rb)], rtol=0, atol=1e-6, err_msg=where)
    assert abs(h["voiced_prob"][b, t] - rvp) <= 1e-6, where
    return True


def host_frames(fr):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in fr.items()}


@pytest.mark.parametrize("sr", [48000, 22050])
def test_emission_exact_on_device_cmndf(sr):
    ops = _ops()
    Y = np.concatenate([_mixed_clips(sr, sr), _vibrato_clips(8, sr, 1.0, seed=5)])
    fr = ops.pitch_frames(ops.to_device_f32(Y), sr, P.C2, P.C7, mode="pyin", want_cmndf=True)
    h = host_frames(fr)
    for b in range(len(Y)):
        for t in range(h["T"]):
            check_emission_frame(h, b, t, sr, P.C2)


def _ref_lists(Y, sr):
    out = []
    for y in Y:
        r = R.pyin(y, sr)
        out.append(r)
    return out


def _pack(cands, vps, K):
    B, Tn = len(cands), len(cands[0])
    cb = np.zeros((B, Tn, K), np.int32)
    cp = np.zeros((B, Tn, K), np.float32)
    cc = np.zeros((B, Tn), np.int32)
    for b in range(B):
        for t, (bb, pp) in enumerate(cands[b]):
            cb[b, t, :len(bb)] = bb
            cp[b, t, :len(bb)] = pp
            cc[b, t] = len(bb)
    return cb, cp, cc, np.asarray(vps, np.float32)


@pytest.mark.parametrize("width,B,Tn", [(51, 64, 200), (101, 16, 200)])
def test_viterbi_exact(width, B, Tn):
    import torch
    ops = _ops()
    n, K = 601, 12
    rng = np.random.default_rng(width)
    cands, vps = [], []
    for b in range(B):
        cl, vl = [], []
        kind = b % 4
        f = rng.uniform(0, n)
        for t in range(Tn):
            if kind == 0 and b == 0:                  # silence
                cl.append((np.zeros(0, int), np.zeros(0))); vl.append(0.0); continue
            if kind == 1 and b == 1:                  # every candidate at one edge
                bins = np.array([n - 1]) if t % 2 else np.array([0])
            else:
                f = np.clip(f + rng.normal(0, 8), 0, n - 1)
                k = rng.integers(0, 5)
                bins = np.unique(np.clip(np.round(f + rng.normal(0, 60, k)), 0, n - 1).astype(int))
            p = rng.uniform(0.01, 0.5, len(bins)).astype(np.float32).astype(np.float64)
            vp = float(np.float32(min(1.0, p.sum())))
            cl.append((bins, p)); vl.append(vp)
        cands.append(cl); vps.append(vl)
    cb, cp, cc, vp32 = _pack(cands, vps, K)
    dev = lambda a: torch.from_numpy(a).cuda()
    f0, voiced, st = ops.pyin_viterbi(dev(cb), dev(cp), dev(cc), dev(vp32), n, width, P.C2)
    st = st.cpu().numpy()
    for b in range(B):
        obs = R.emission_matrix([(bb, cp[b, t, :len(bb)].astype(np.float64)) for t, (bb, _) in enumerate(cands[b])],
                                vp32[b].astype(np.float64), n)
        ref = R.viterbi_band(obs, n, width)
        assert np.array_equal(st[b], ref), f"clip {b}: {np.count_nonzero(st[b] != ref)} states differ"
        rf0, rv = R.states_to_f0(ref, n, P.C2)
        np.testing.assert_array_equal(voiced.cpu().numpy()[b], rv)
        np.testing.assert_allclose(f0.cpu().numpy()[b][rv], rf0[rv], rtol=1e-6)


def _pool_pyin(args):
    y, sr = args
    r = R.pyin(y.astype(np.float64), sr)
    return r["f0"], r["voiced"], r["vps"]


@pytest.mark.parametrize("sr", [48000, 22050])
def test_end_to_end_vibrato(sr):
    ops = _ops()
    B = 256
    Y = _vibrato_clips(B, sr, 1.0, seed=sr)
    f0, vf, vp = ops.pitch_pyin(ops.to_device_f32(Y), sr, P.C2, P.C7)
    f0, vf, vp = f0.cpu().numpy(), vf.cpu().numpy(), vp.cpu().numpy()
    with mp.get_context("spawn").Pool(16) as pool:
        refs = pool.map(_pool_pyin, [(Y[b], sr) for b in range(B)])
    agree = tot = vp_bad = 0
    for b, (rf0, rv, rvp) in enumerate(refs):
        same_v = vf[b] == rv
        bins_d = np.where(vf[b], np.round(120 * np.log2(np.where(vf[b], f0[b], P.C2) / P.C2)), -1)
        bins_r = np.where(rv, np.round(120 * np.log2(np.where(rv, rf0, P.C2) / P.C2)), -1)
        agree += int(np.sum(same_v & (bins_d == bins_r)))
        tot += len(rv)
        vp_bad += int(np.sum(np.abs(vp[b] - rvp) > 1e-4))
    assert agree >= 0.99 * tot, f"voicing + bin agree on {agree / tot:.4f} of frames"
    assert vp_bad <= 0.01 * tot, f"voiced_prob off by > 1e-4 on {vp_bad} of {tot} frames"


@pytest.fixture
def sine_wave_audio():
    sr, freq, amp = 22050, 440.0, 0.8
    t = np.linspace(0.0, 1.0, sr, endpoint=False)
    return (amp * np.sin(2 * np.pi * freq * t)).astype(np.float64), sr, freq, amp


def test_fundamental_frequency(sine_wave_audio):
    from sygnals_amd.core.audio.features import fundamental_frequency
    y, sr, freq, _ = sine_wave_audio
    times, f0, vf, vp = fundamental_frequency(y, sr=sr, method="pyin")
    assert times.ndim == f0.ndim == vf.ndim == vp.ndim == 1
    assert f0.dtype == np.float64 and vf.dtype == np.float64
    v = np.where(vf > 0.5)[0]
    assert len(v) > 0
    np.testing.assert_allclose(np.nanmean(f0[v]), freq, rtol=0.05)
    np.testing.assert_allclose(times, np.arange(len(f0)) * 512 / sr)
    _, f0s, vfs, _ = fundamental_frequency(np.zeros(sr), sr=sr, method="pyin")
    assert np.sum(vfs) < 0.1 * len(vfs) and np.all(np.isnan(f0s))
    _, f0y, vfy, _ = fundamental_frequency(y, sr=sr, method="yin")
    np.testing.assert_allclose(np.median(f0y), freq, rtol=0.01)
    with pytest.raises(ValueError, match="Unsupported pitch estimation method"):
        fundamental_frequency(y, sr=sr, method="crepe")


def test_jitter_approx(sine_wave_audio):
    from sygnals_amd.core.audio.features import fundamental_frequency, jitter
    y, sr, freq, _ = sine_wave_audio
    t = np.arange(len(y)) / sr
    yv = np.sin(2 * np.pi * np.cumsum(freq * (1 + 0.05 * np.sin(2 * np.pi * 5 * t))) / sr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        _, f0, vf, _ = fundamental_frequency(y, sr, fmin=75.0, fmax=600.0)
        js = jitter(y, sr, f0=f0, voiced_flag=vf)
        _, f0v, vfv, _ = fundamental_frequency(yv, sr, fmin=75.0, fmax=600.0)
        jv = jitter(yv, sr, f0=f0v, voiced_flag=vfv)
        ji = jitter(y, sr)                              # internal pYIN
    assert np.nanmean(js) < 1e-5 < np.nanmean(jv)
    assert np.all(np.isnan(js[vf <= 0.5])) and np.isnan(js[0])
    assert ji.shape == js.shape
    with pytest.warns(UserWarning, match="Jitter feature is an approximation"):
        jitter(y, sr, f0=f0, voiced_flag=vf)


def test_shimmer_approx(sine_wave_audio):
    from sygnals_amd.core.audio.features import shimmer
    y, sr, _, _ = sine_wave_audio
    t = np.arange(len(y)) / sr
    ya = y * (1 + 0.5 * np.sin(2 * np.pi * 3 * t))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        ss = shimmer(y, sr)
        sa = shimmer(ya, sr)
    assert np.nanmean(ss) < 0.05 < np.nanmean(sa)


def test_batch_consistency_and_long_stream():
    ops = _ops()
    sr = 16000
    Y = _vibrato_clips(1024, sr, 1.0, seed=11)
    yd = ops.to_device_f32(Y)
    f0, vf, vp = (x.cpu().numpy() for x in ops.pitch_pyin(yd, sr, P.C2, P.C7))
    for b in (0, 5, 511, 1023):
        g0, gv, gp = (x.cpu().numpy() for x in ops.pitch_pyin(yd[b:b + 1], sr, P.C2, P.C7))
        assert np.array_equal(np.nan_to_num(g0[0], nan=-1), np.nan_to_num(f0[b], nan=-1))
        assert np.array_equal(gv[0], vf[b]) and np.array_equal(gp[0], vp[b])
    long = _vibrato_clips(1, sr, 600.0, seed=12)
    lf0, lv, lp = (x.cpu().numpy()[0] for x in ops.pitch_pyin(ops.to_device_f32(long), sr, P.C2, P.C7))
    rf0, rv, rvp = _pool_pyin((long[0], sr))
    bd = np.where(lv, np.round(120 * np.log2(np.where(lv, lf0, P.C2) / P.C2)), -1)
    br = np.where(rv, np.round(120 * np.log2(np.where(rv, rf0, P.C2) / P.C2)), -1)
    assert np.mean((lv == rv) & (bd == br)) >= 0.99
    assert np.mean(np.abs(lp - rvp) > 1e-4) <= 0.01
