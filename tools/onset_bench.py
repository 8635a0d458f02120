"""Time onset detection with HIP events (median of --reps, warmed): onset_strength after the mel front end, onset_peaks
and the whole detect_onsets_batch, on 1024 x 48000 at 48 kHz, 1024 x 22050 at 22.05 kHz and one 1-hour 48 kHz stream,
each against its HBM floor (bytes it must move / 8 TB/s; the strength kernel is not LDS-staged, so its two passes count
2 x B x M x T x 4 bytes); the float64 restatement's CPU time per clip as the baseline.  Prints one JSON object and
writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import ops  # noqa: E402
from sygnals_amd.core.audio import features as F  # noqa: E402
from sygnals_amd.core.features import manager as M  # noqa: E402
from tests import onset_ref as R  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
N_FFT, HOP, N_MELS = 2048, 512, 128


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
    B, L = y.shape
    mel = M.mel_power_batch(y, sr, N_FFT, HOP, True, "hann", N_MELS, 0.0, None)
    Tn = mel.shape[2]
    pk = F._peak_defaults(sr, HOP, {})
    pad = 1 + N_FFT // (2 * HOP)
    env = ops.onset_strength(mel, 1, 1, pad, Tn)
    frames, count = ops.onset_peaks(env, **pk)
    floors = dict(front_end=4 * B * L + 4 * B * N_MELS * Tn, strength=2 * 4 * B * N_MELS * Tn + 4 * B * Tn,
                  peaks=4 * B * Tn + 4 * B * Tn + 4 * B)
    floors["total"] = floors["front_end"] + floors["strength"] + floors["peaks"]
    us = dict(
        front_end=timed(lambda: M.mel_power_batch(y, sr, N_FFT, HOP, True, "hann", N_MELS, 0.0, None), reps),
        strength=timed(lambda: ops.onset_strength(mel, 1, 1, pad, Tn), reps),
        peaks=timed(lambda: ops.onset_peaks(env, **pk), reps),
        total=timed(lambda: F.detect_onsets_batch(y, sr, HOP), reps))
    out = dict(B=int(B), L=int(L), sr=sr, T=int(Tn), onsets=int(count.sum().item()), windows=pk)
    for k, v in us.items():
        fl_us = floors[k] / HBM_BPS * 1e6
        out[k] = dict(us=v, hbm_floor_us=fl_us, floor_fraction=fl_us / v)
    return out


def clips(sr, n, length):
    base = np.stack([R.burst_clip(sr, length, 500 + i) for i in range(64)]).astype(np.float32)
    return np.tile(base, (n // 64, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-clips", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onset_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {}
    for sr in (48000, 22050):
        Y = clips(sr, 1024, sr)
        res[f"batch_1024x{sr}"] = case(Y, sr, a.reps)
        t0 = time.perf_counter()
        for b in range(a.cpu_clips):
            R.onset_detect(Y[b].astype(np.float64), sr=sr, hop_length=HOP)
        res[f"batch_1024x{sr}"]["restatement_cpu_s_per_clip"] = (time.perf_counter() - t0) / a.cpu_clips
        del Y
    minute = R.burst_clip(48000, 60 * 48000, 7, n_bursts=120).astype(np.float32)
    res["one_hour_48k"] = case(np.tile(minute, 60)[None, :], 48000, max(3, a.reps // 2))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
