"""Time the device cross-spectral analysis (ops.cross_spectrum: Pxy, Pxx, Pyy and the coherence from one pass) and the delay
chain (core.alignment.estimate_delay_batch) with HIP events: every shape warmed, each sample a window of --inner calls,
median of --reps windows.

Shapes: 1024 rows x 32768 samples at nperseg 256 / 1024 / 4096 with 50 % overlap, and one row of 2^24 samples at 4096
(detrend 'constant', hann, density).  Per shape:
  fused       the fused kernel producing all four outputs, beside its byte floor 4 B (2 L + 5 F) bytes at 8 TB/s;
  welch_x2    the yardstick: two welch_batch calls, on x and on y, timed in the same run (Pxx and Pyy only);
  torch       unfold, torch.fft.rfft, products, mean; its difference from the kernel's result as a fraction of
              max sqrt(Pxx Pyy) (Pxy) and absolute (coherence).
The delay chain: estimate_delay_batch at 1024 x 32768 (max_lag 1024) and 64 x 2^20, both weightings, with the weighting
and the picker kernels timed on their own.

Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import ops  # noqa: E402
from sygnals_amd.core import alignment as AL, dsp as D  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s


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


def pair(B, L):
    g = torch.Generator(device="cuda").manual_seed(7)
    s = torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    x = s + 0.5 * torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    y = 0.8 * torch.roll(s, 3, 1) + 0.5 * torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    return x, y


def torch_cross(x, y, nperseg, w, scale):
    step = nperseg // 2
    spec = []
    for v in (x, y):
        seg = v.unfold(1, nperseg, step)
        spec.append(torch.fft.rfft((seg - seg.mean(-1, keepdim=True)) * w, dim=-1))
    X, Y = spec
    one = torch.full((nperseg // 2 + 1,), 2.0 * scale, device=x.device)
    one[0] = scale
    one[-1] = scale
    sxy, sxx, syy = (X.conj() * Y).mean(1), (X.abs() ** 2).mean(1), (Y.abs() ** 2).mean(1)
    return sxy * one, sxx * one, syy * one, sxy.abs() ** 2 / (sxx * syy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csd_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")

    for B, L, segs in ((1024, 32768, (256, 1024, 4096)), (1, 1 << 24, (4096,))):
        x, y = pair(B, L)
        for n in segs:
            key = f"{B}x{L}_nperseg{n}"
            F = n // 2 + 1
            nseg = (L - n // 2) // (n // 2)
            wh = scipy.signal.get_window("hann", n)
            scale = 1.0 / (wh * wh).sum()
            floor = 4.0 * B * (2 * L + 5 * F) / HBM_BPS * 1e3
            info = dict(B=B, L=L, nperseg=n, nseg=nseg, work_bytes=int(ops.lib().syg_csd_work_bytes(B, nseg, n)))
            t = measure(lambda: ops.cross_spectrum(x, y, n, n // 2, n, wh, "constant", scale), a.reps, a.inner, **info)
            t["byte_floor_ms"] = floor
            t["floor_fraction"] = floor / t["ms"]
            res[key + "_fused"] = t
            res[key + "_csd_only"] = measure(lambda: ops.cross_spectrum(x, y, n, n // 2, n, wh, "constant", scale, want=("pxy",)),
                                             a.reps, a.inner, **info)
            w2 = measure(lambda: (D.welch_batch(x, nperseg=n), D.welch_batch(y, nperseg=n)), a.reps, a.inner, **info)
            w2["fused_over_welch_x2_time"] = t["ms"] / w2["ms"]
            res[key + "_welch_x2"] = w2
            wd = torch.from_numpy(wh.astype(np.float32)).cuda()
            base = torch_cross(x, y, n, wd, scale)
            tb = measure(lambda: torch_cross(x, y, n, wd, scale), 3, 2, form="torch", **info)
            ours = ops.cross_spectrum(x, y, n, n // 2, n, wh, "constant", scale)
            S = torch.sqrt(base[1].double() * base[2].double()).amax(1, keepdim=True)
            pxy = torch.view_as_complex(ours["pxy"].contiguous())
            tb["pxy_diff_to_kernel_of_max_S"] = float(((base[0] - pxy).abs().double() / S).max())
            tb["coherence_diff_to_kernel"] = float((base[3] - ours["coherence"]).abs().max())
            tb["baseline_over_kernel_time"] = tb["ms"] / t["ms"]
            res[key + "_torch"] = tb
            del base, ours, pxy, S
            torch.cuda.empty_cache()
            write()
        del x, y
        torch.cuda.empty_cache()

    for B, L, max_lag in ((1024, 32768, 1024), (64, 1 << 20, 4096)):
        x, y = pair(B, L)
        n = ops.gcc_fft_len(L, L)
        for w in ("none", "phat"):
            key = f"delay_{B}x{L}_{w}"
            t = measure(lambda: AL.estimate_delay_batch(x, y, 48000.0, max_lag, w), a.reps, a.inner, B=B, L=L, n_fft=n,
                        max_lag=max_lag, weighting=w)
            X = torch.randn((B, n, 2), dtype=torch.float32, device="cuda")
            Y = torch.randn((B, n, 2), dtype=torch.float32, device="cuda")
            tw = measure(lambda: ops._call("syg_gcc_weight_c64", ops._ptr(X), ops._ptr(Y), B, B, n, int(w == "phat"), ops._ptr(X)),
                         a.reps, a.inner)
            r = ops.gcc(x, y, max_lag, w)
            tp = measure(lambda: ops.peak_pick(r, -max_lag, 48000.0), a.reps, a.inner)
            t["weight_kernel_ms"], t["picker_kernel_ms"] = tw["ms"], tp["ms"]
            t["weight_share"], t["picker_share"] = tw["ms"] / t["ms"], tp["ms"] / t["ms"]
            res[key] = t
            del X, Y, r
            torch.cuda.empty_cache()
            write()
        del x, y
    print(json.dumps(res))


if __name__ == "__main__":
    main()
