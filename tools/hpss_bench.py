"""Time the HPSS chain of harmonic_to_noise_ratio with HIP events (median of --reps): the STFT, the median-filter
masks, the two-component inverse STFT, the HNR rows and the whole chain, on 1024 x 48000 at 48 kHz, 1024 x 22050 at
22.05 kHz and one 1-hour 48 kHz stream, with each stage's HBM floor (bytes it must move / 8 TB/s); the float64
restatement's CPU time per clip as the baseline.  Prints one JSON object and writes it to --out."""
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
from tests import hpss_ref as R  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s


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
    D = ops.stft2048_c2c(y)
    Tn = D.shape[1]
    Mh, Mp = ops.hpss_masks(D)
    yh, yp = ops.istft2048(D, 512, L, mask=(Mh, Mp))
    cells = B * Tn * 1025
    fl, hop = 2048, 512
    Th = 1 + L // hop
    # compulsory HBM traffic of each stage (bytes): inputs read once, outputs written once
    floors = dict(stft=4 * B * L + 8 * cells, masks=8 * cells + 8 * cells, istft=8 * cells + 8 * cells + 8 * B * L,
                  hnr=8 * B * L + 4 * B * Th)
    floors["total"] = floors["stft"] + floors["masks"] + floors["istft"] + floors["hnr"]
    us = dict(
        stft=timed(lambda: ops.stft2048_c2c(y), reps),
        masks=timed(lambda: ops.hpss_masks(D), reps),
        istft=timed(lambda: ops.istft2048(D, 512, L, mask=(Mh, Mp)), reps),
        hnr=timed(lambda: ops.hnr_rows(yh, yp, fl, hop), reps),
        total=timed(lambda: ops.hnr_rows(*ops.hpss(y), fl, hop), reps))
    out = dict(B=int(B), L=int(L), sr=sr, T=int(Tn), medians=2 * cells)
    for k, v in us.items():
        fl_us = floors[k] / HBM_BPS * 1e6
        out[k] = dict(us=v, hbm_floor_us=fl_us, floor_fraction=fl_us / v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-clips", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpss_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    res = {}
    for sr in (48000, 22050):
        t = np.arange(sr) / sr
        f = rng.uniform(80, 900, (1024, 1))
        Y = (0.5 * np.sin(2 * np.pi * f * t[None, :]) + 0.05 * rng.standard_normal((1024, sr))).astype(np.float32)
        res[f"batch_1024x{sr}"] = case(Y, sr, a.reps)
        t0 = time.perf_counter()
        for b in range(a.cpu_clips):
            R.hnr_from_components(*R.hpss(Y[b].astype(np.float64)), 2048, 512)
        res[f"batch_1024x{sr}"]["restatement_cpu_s_per_clip"] = (time.perf_counter() - t0) / a.cpu_clips
        del Y
    L = 3600 * 48000
    ts = np.arange(L, dtype=np.float64) / 48000
    long = (0.5 * np.sin(2 * np.pi * 220 * ts) + 0.05 * rng.standard_normal(L)).astype(np.float32)
    res["one_hour_48k"] = case(long[None, :], 48000, max(3, a.reps // 2))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
