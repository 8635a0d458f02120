"""Time the device loudness meter and normaliser with HIP events: every case warmed, each sample a window of calls of
about 50 ms, median of --reps windows.

Shapes: 1024 clips of 32 768 samples and one clip of 2^24 samples, at 48 kHz, mono and stereo.  Per shape: the segment
powers (ops.loudness_segments), the integrated-loudness chain (segments, blocks and gates), the true peak, and the
normaliser end to end (measure, gain, apply).  Beside the two fused kernels, in the same run, the composed path the
operators already allowed: ops.sosfilt of the K-weighting cascade followed by torch squares and per-segment sums, and
ops.resample_poly followed by abs().amax().  Per case the time, Msamples/s and the fraction of the byte floor (the signal
read once, 4 bytes a sample, at 8 TB/s; the normaliser also writes it once and reads it for each of its two measurements;
none for the blocks-and-gates kernel, which reads segment powers, not the signal).
Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _loudness as LD  # noqa: E402
from sygnals_amd import ops  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
FS = 48000


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


def measure(fn, reps, n, name, passes=1):
    """passes: times the signal crosses the memory interface at least; 0 for a case that never touches the signal (no
    throughput and no floor are given for it)."""
    one = timed(fn, 1, 1, warm=1)["ms"]
    n_in = int(min(200, max(1, 50.0 // max(one, 1e-3))))
    r = dict(timed(fn, reps, n_in, warm=1), inner=n_in, case=name)
    if passes:
        r["msamples_per_s"] = n / r["ms"] / 1e3
        r["floor_ms"] = 4 * passes * n / HBM_BPS * 1e3
        r["of_floor"] = r["floor_ms"] / r["ms"]
    return r


def composed_segments(x, sos, n_seg, seg_len):
    """ops.sosfilt, then torch: square in float64 and sum per segment (fs a multiple of 10: segments of one length)."""
    B, C, L = x.shape
    y = ops.sosfilt(x.reshape(B * C, L), sos)
    return y[:, :n_seg * seg_len].double().square_().view(B, C, n_seg, seg_len).sum(dim=-1)


def bench_shape(B, C, L, reps):
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((B, C, L), device="cuda", generator=g) * 0.1
    n = B * C * L
    sos = LD.k_weighting_sos(FS)
    n_seg, seg_len, up = LD.n_segments(L, FS), FS // 10, LD.true_peak_up(FS)
    res = {"B": B, "C": C, "L": L, "fs": FS, "cases": []}
    add = res["cases"].append
    seg = ops.loudness_segments(x, FS)
    ref = composed_segments(x, sos, n_seg, seg_len)
    res["segments_fused_vs_composed_rel"] = float(((seg - ref).abs().amax() / ref.abs().amax()).item())
    add(measure(lambda: ops.loudness_segments(x, FS), reps, n, "segments fused"))
    add(measure(lambda: composed_segments(x, sos, n_seg, seg_len), reps, n, "segments composed (sosfilt + torch)"))
    add(measure(lambda: ops.loudness_blocks(seg, FS), reps, n, "blocks and gates", passes=0))
    add(measure(lambda: ops.integrated_loudness(x, FS), reps, n, "integrated loudness fused"))
    add(measure(lambda: ops.loudness_blocks(composed_segments(x, sos, n_seg, seg_len), FS)[2], reps, n,
                "integrated loudness composed (sosfilt + torch, then blocks)"))
    add(measure(lambda: ops.true_peak(x, FS), reps, n, "true peak fused"))
    x2 = x.reshape(B * C, L)
    add(measure(lambda: ops.resample_poly(x2, up, 1).abs().amax(dim=1), reps, n, "true peak composed (resample_poly + abs amax)"))
    add(measure(lambda: ops.normalize_loudness(x, FS, -23.0), reps, n, "normalise to -23 LUFS", passes=3))
    add(measure(lambda: ops.normalize_loudness(x, FS, -23.0, peak_limit_dbtp=-1.0), reps, n, "normalise with a -1 dBTP limit", passes=4))
    t = {c["case"]: c["ms"] for c in res["cases"]}
    res["speedup_segments"] = t["segments composed (sosfilt + torch)"] / t["segments fused"]
    res["speedup_integrated"] = t["integrated loudness composed (sosfilt + torch, then blocks)"] / t["integrated loudness fused"]
    res["speedup_true_peak"] = t["true peak composed (resample_poly + abs amax)"] / t["true peak fused"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.json"))
    ap.add_argument("--shapes", default="1024x1x32768,1024x2x32768,1x1x16777216,1x2x16777216")
    a = ap.parse_args()
    ops.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BPS, "constants": ops.loudness_constants(), "shapes": []}
    for s in a.shapes.split(","):
        B, C, L = (int(v) for v in s.split("x"))
        out["shapes"].append(bench_shape(B, C, L, a.reps))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
