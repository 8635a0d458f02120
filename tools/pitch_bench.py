"""Time the pitch kernels with HIP events: the frame stage (yin / pyin) and the Viterbi decode separately, on config
C2's shape (1024 x 48000 at 48 kHz, C2-C7, hop 512) and on one 1-hour 16 kHz stream; the float64 restatement's CPU
time on a slice of the same input as the baseline.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _pitch as P, ops  # noqa: E402
from tests import pitch_ref as R  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def case(Y, sr, reps):
    y = ops.to_device_f32(Y)
    fr = ops.pitch_frames(y, sr, P.C2, P.C7, mode="pyin")
    width = P.transition_width(sr, 512)
    return dict(
        B=int(Y.shape[0]), L=int(Y.shape[1]), sr=sr, T=fr["T"], n_lag=fr["max_p"] - fr["min_p"] + 1, states=2 * fr["n_bins"],
        yin_frames_us=timed(lambda: ops.pitch_yin(y, sr, P.C2, P.C7), reps),
        pyin_frames_us=timed(lambda: ops.pitch_frames(y, sr, P.C2, P.C7, mode="pyin"), reps),
        viterbi_us=timed(lambda: ops.pyin_viterbi(fr["cand_bin"], fr["cand_prob"], fr["cand_count"], fr["voiced_prob"],
                                                  fr["n_bins"], width, P.C2), reps),
        pyin_total_us=timed(lambda: ops.pitch_pyin(y, sr, P.C2, P.C7), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-clips", type=int, default=4)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    sr = 48000
    t = np.arange(sr) / sr
    f = rng.uniform(80, 900, (1024, 1))
    Y = (0.5 * np.sin(2 * np.pi * f * t[None, :]) + 0.01 * rng.standard_normal((1024, sr))).astype(np.float32)
    out = {"c2_shape": case(Y, sr, a.reps)}
    t0 = time.perf_counter()
    for b in range(a.cpu_clips):
        R.pyin(Y[b].astype(np.float64), sr)
    per_clip = (time.perf_counter() - t0) / a.cpu_clips
    out["restatement_cpu_s_per_clip"] = per_clip
    out["restatement_cpu_s_1024_clips_est"] = per_clip * 1024
    L = 3600 * 16000
    ts = np.arange(L) / 16000
    long = (0.5 * np.sin(2 * np.pi * 220 * ts * (1 + 0.001 * np.sin(ts))) + 0.01 * rng.standard_normal(L)).astype(np.float32)
    out["one_hour_16k"] = case(long[None, :], 16000, max(2, a.reps // 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
