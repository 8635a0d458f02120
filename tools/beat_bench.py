"""Time the device rhythm family (ops.tempogram, ops.tempo_pick, ops.beat_local_score, ops.beat_dp, ops.beat_track and the
chain core.rhythm.beat_track_batch) with HIP events: every shape warmed, each sample a window of --inner calls, median of
--reps windows.

Shapes: 1024 envelopes x 65 frames and x 3001 frames at win_length 384, one row of 2^20 frames, and beat_track_batch from
audio at 1024 x 32768.  Per shape:
  the time of each kernel;
  the tempogram beside its arithmetic floor (win_length^2 / 2 multiply-adds a frame at the float32 vector peak, 157.3 TFLOP/s)
  and its byte floor (4 B win_length T bytes written once at 8 TB/s);
  the yardstick from the same run, a torch formulation a user would write: unfold, torch.fft autocorrelation, amax for the
  tempogram; the DP as a Python loop over frames on device tensors (on the first --dp-frames frames of a longer row, the
  time per frame carried to the whole row).
The worst errors of the tempogram and the local score against the float64 restatement (tests/beat_ref.py) on small inputs
are recorded too.  Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _rhythm as RH, ops  # noqa: E402
from sygnals_amd.core import rhythm as RY  # noqa: E402
from sygnals_amd.core.audio import features as F  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
F32_FMA_PER_S = 157.3e12 / 2.0


def timed(fn, reps, inner, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return dict(ms=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)))


def measure(fn, reps, inner, **info):
    one = timed(fn, 1, 1, warm=1)["ms"]
    n_in = int(min(inner, max(1, 50.0 // one)))                      # windows of about 50 ms
    return dict(timed(fn, reps, n_in, warm=1), inner=n_in, **info)


def click_env(B, T, device="cuda"):
    g = torch.Generator(device=device).manual_seed(11)
    env = 0.1 * torch.rand((B, T), dtype=torch.float32, device=device, generator=g)
    for b in range(min(B, 64)):
        env[b::64, (b % 17)::20 + b % 13] += 1.0
    return env


def torch_tempogram(env, win, w):
    p = win // 2
    T = env.shape[1]
    i = torch.arange(p, device=env.device, dtype=env.dtype)
    xp = torch.cat([env[:, :1] * i / p, env, env[:, -1:] * (p - 1 - i) / p], dim=1)
    fr = xp.unfold(1, win, 1)[:, :T] * w
    n = 1 << (2 * win - 1).bit_length()
    S = torch.fft.rfft(fr, n=n, dim=-1)
    r = torch.fft.irfft(S.real ** 2 + S.imag ** 2, n=n, dim=-1)[..., :win]
    m = r.abs().amax(-1, keepdim=True)
    return (r / torch.where(m < 1.1754944e-38, torch.ones_like(m), m)).transpose(1, 2)


def torch_dp(ls, period, tightness, frames):
    """beat_track's DP as a loop over frames, every row at once (one period for all rows)."""
    B, T = ls.shape
    o = torch.arange(-2 * period, -int(np.round(period / 2)) + 1, device=ls.device)
    tx = -tightness * torch.log(-o.double() / period) ** 2
    cum = torch.zeros((B, T), dtype=torch.float64, device=ls.device)
    back = torch.full((B, T), -1, dtype=torch.int64, device=ls.device)
    first = torch.ones(B, dtype=torch.bool, device=ls.device)
    thr = 0.01 * ls.amax(1).double()
    ls64 = ls.double()
    for i in range(min(T, frames)):
        src = i + o
        c = tx + torch.where(src >= 0, cum[:, src.clamp(min=0)], torch.zeros((), dtype=torch.float64, device=ls.device))
        best, bj = c.max(1)
        cum[:, i] = ls64[:, i] + best
        wait = first & (ls64[:, i] < thr)
        back[:, i] = torch.where(wait, torch.full_like(bj, -1), src[bj])
        first = wait
    return cum, back


def worst_errors():
    sys.path.insert(0, ROOT)
    from tests import beat_ref as R
    rng = np.random.default_rng(0)
    out = {"tempogram_normalised": 0.0, "tempogram_unnormalised_of_max_r": 0.0, "local_score_of_g1_max_e": 0.0}
    for win, T in ((8, 70), (64, 130), (384, 100), (2048, 6)):
        env = rng.random((2, T)).astype(np.float32)
        d = ops.to_device_f32(env)
        tg, raw = ops.tempogram(d, win).cpu().numpy(), ops.tempogram(d, win, norm=None).cpu().numpy()
        for b in range(2):
            r = R.autocorr(env[b], win)
            out["tempogram_normalised"] = max(out["tempogram_normalised"], float(np.abs(tg[b] - R.normalise(r)).max()))
            out["tempogram_unnormalised_of_max_r"] = max(out["tempogram_unnormalised_of_max_r"],
                                                         float(np.abs(raw[b] - r).max() / np.abs(r).max()))
    for P, T in ((3, 50), (21, 300), (383, 1030), (2047, 3000)):
        env = R.click_envelope(T, P, 1, 1.0, 0.3, P)
        ls = ops.beat_local_score(ops.to_device_f32(env[None]), [P])[0][0].cpu().numpy()
        e = np.abs(ls - R.local_score(env, P)).max() / (np.sum(R.taps(P)) * np.abs(R.scaled(env)).max())
        out["local_score_of_g1_max_e"] = max(out["local_score_of_g1_max_e"], float(e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--dp-frames", type=int, default=3001)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beat_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")

    res["worst_errors"] = worst_errors()
    write()
    win, sr, hop = 384, 22050, 512
    bpms, lp = RH.tempo_prior(win, sr, hop)
    wd = torch.from_numpy(RH.window_table("hann", win)).cuda()
    for B, T in ((1024, 65), (1024, 3001), (1, 1 << 20)):
        key = f"{B}x{T}"
        env = click_env(B, T)
        info = dict(B=B, T=T, win_length=win)
        t = measure(lambda: ops.tempogram(env, win), a.reps, a.inner, **info)
        fl_a = B * T * (win * win / 2.0) / F32_FMA_PER_S * 1e3
        fl_b = 4.0 * B * win * T / HBM_BPS * 1e3
        t.update(arith_floor_ms=fl_a, byte_floor_ms=fl_b, arith_floor_fraction=fl_a / t["ms"], byte_floor_fraction=fl_b / t["ms"])
        res[key + "_tempogram"] = t
        res[key + "_tempogram_aggregate_only"] = measure(lambda: ops.tempogram(env, win, aggregate="only"), a.reps, a.inner, **info)
        agg = ops.tempogram(env, win, aggregate="only")
        res[key + "_tempo_pick"] = measure(lambda: ops.tempo_pick(agg, env, lp, bpms), a.reps, a.inner, **info)
        period = ops.tempo_pick(agg, env, lp, bpms)[0]
        res[key + "_local_score"] = measure(lambda: ops.beat_local_score(env, period), a.reps, a.inner, **info)
        ls, lsmax = ops.beat_local_score(env, period)
        res[key + "_dp"] = measure(lambda: ops.beat_dp(ls, lsmax, period, 100.0, period_max=win - 1), a.reps, a.inner,
                                   us_per_frame=None, **info)
        res[key + "_dp"]["us_per_frame"] = res[key + "_dp"]["ms"] * 1e3 / T
        cum, back = ops.beat_dp(ls, lsmax, period, 100.0, period_max=win - 1)
        res[key + "_beats"] = measure(lambda: ops.beat_track(ls, cum, back, period), a.reps, a.inner, **info)
        res[key + "_chain_from_envelope"] = measure(lambda: RY.beat_track_batch(onset_envelope=env, sr=sr, hop_length=hop),
                                                    a.reps, a.inner, **info)
        write()
        print(f"{key}: device timings done", flush=True)
        # the yardstick
        base = torch_tempogram(env, win, wd)
        ours = ops.tempogram(env, win)
        tb = measure(lambda: torch_tempogram(env, win, wd), 3, 2, form="torch", **info)
        tb["diff_to_kernel"] = float((base - ours).abs().max())
        tb["baseline_over_kernel_time"] = tb["ms"] / t["ms"]
        res[key + "_torch_tempogram"] = tb
        del base, ours
        torch.cuda.empty_cache()
        P = int(period[0].item()) or 20
        nfr = min(T, a.dp_frames)
        td = measure(lambda: torch_dp(ls, P, 100.0, nfr), 3, 1, form="torch loop", frames_timed=nfr, period=P, **info)
        td["ms_whole_row"] = td["ms"] * T / nfr
        td["baseline_over_kernel_time"] = td["ms_whole_row"] / res[key + "_dp"]["ms"]
        res[key + "_torch_dp"] = td
        write()
        print(f"{key}: yardstick done", flush=True)
        del env, ls, lsmax, cum, back, agg
        torch.cuda.empty_cache()
    B, L = 1024, 32768
    g = torch.Generator(device="cuda").manual_seed(5)
    y = 1e-3 * torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    y[:, 2000::20 * hop] += 0.8
    y[:, 2001::20 * hop] -= 0.8
    res[f"{B}x{L}_onset_strength"] = measure(lambda: F.onset_strength_batch(y, sr, hop_length=hop), a.reps, a.inner, B=B, L=L)
    res[f"{B}x{L}_beat_track_batch"] = measure(lambda: RY.beat_track_batch(y, sr, hop_length=hop), a.reps, a.inner, B=B, L=L)
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
