"""Time the structure kernels with HIP events: path_enhance (n = 51, 7 filters), the diagonal median (w = 7) and the
agglomerative clustering (D = 12, k = 10), each on one three-minute clip (B = 1, T = 7750) and on 64 ten-second clips
(B = 64, T = 431).  Every case is warmed, each sample is a window of calls of about 50 ms, the figure is the median of
--reps windows, and where there is a baseline the two sides alternate window by window (a side whose single call takes
more than a second gets three windows).

Baselines, measured in the same run: for path_enhance the composition a user has today, torch's explicit padding, ONE
conv2d with seven output channels (the filters as dense arrays) and amax; for the clustering scikit-learn's
AgglomerativeClustering over the chain's connectivity on the host, where it is installed.  path_enhance also reports
the fraction of the fp32 vector peak that its tap lists' fma count reaches.
Reported, not gated: the capability is new, there is no parent-commit time, and nothing is routed to a composition.
Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _structure as ST  # noqa: E402
from sygnals_amd import ops  # noqa: E402

PEAK_FP32_TFLOPS = 157.3                     # MI355X vector fp32, the data sheet's figure


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, reps):
    """{name: fn} -> {name: stats}: every fn warmed, then rounds of one window each, in turn."""
    inner, rounds = {}, {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        one = window(fn, 1)
        inner[k] = int(min(200, max(1, 50.0 // max(one, 1e-3))))
        rounds[k] = reps if one < 1000.0 else min(reps, 3)
    ts = {k: [] for k in fns}
    for r in range(reps):
        for k, fn in fns.items():
            if r < rounds[k]:
                ts[k].append(window(fn, inner[k]))
    return {k: dict(ms=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)), inner=inner[k], windows=len(v))
            for k, v in ts.items()}


def dense_bank(F):
    """The tap lists as one dense correlation bank [n_filters, 1, rows, cols] and the padding (top, bottom, left, right)."""
    r0, r1, c0, c1 = F.span
    W = np.zeros((len(F.fstart) - 1, 1, r1 - r0 + 1, c1 - c0 + 1), dtype=np.float32)
    for f in range(W.shape[0]):
        lo, hi = F.fstart[f], F.fstart[f + 1]
        W[f, 0, F.taps[lo:hi, 0] - r0, F.taps[lo:hi, 1] - c0] = F.taps[lo:hi, 2].view(np.float32)
    return torch.from_numpy(W).cuda(), (-r0, r1, -c0, c1)


def torch_path_enhance(R, W, pad):
    x = torch.nn.functional.pad(R[:, None], (pad[2], pad[3], pad[0], pad[1]), mode="reflect")      # scipy's "mirror"
    return torch.nn.functional.conv2d(x, W).amax(dim=1).clamp_(min=0)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def bench_path(B, T, n, reps, composition=True):
    g = torch.Generator(device="cuda").manual_seed(5)
    R = torch.rand((B, T, T), device="cuda", generator=g)
    F = ST.path_filters(n)
    W, pad = dense_bank(F)
    taps = int(F.taps.shape[0])
    res = {"B": B, "T": T, "n": n, "n_filters": 7, "taps": taps, "dense_taps": int(W[0].numel() * W.shape[0]),
           "fma": B * T * T * taps}
    fns = {"device": lambda: ops.path_enhance(R, n, mode="mirror")}
    try:
        if not composition:
            raise RuntimeError("not run (--skip-composition-above)")
        res["difference_max"] = float((ops.path_enhance(R, n, mode="mirror") - torch_path_enhance(R, W, pad)).abs().max().item())
        fns["torch composition"] = lambda: torch_path_enhance(R, W, pad)
    except RuntimeError as e:                # (the composition's workspace may not fit)
        res["torch composition failed"] = str(e)[:200]
    t = alternate(fns, reps)
    if "torch composition" in t:
        t["composition_over_device"] = t["torch composition"]["ms"] / t["device"]["ms"]
    t["device_tflops"] = 2 * res["fma"] / (t["device"]["ms"] * 1e-3) / 1e12
    t["fraction_of_fp32_vector_peak"] = t["device_tflops"] / PEAK_FP32_TFLOPS
    res["path_enhance"] = t
    return res


def bench_median(B, T, w, reps):
    g = torch.Generator(device="cuda").manual_seed(6)
    R = torch.rand((B, T, T), device="cuda", generator=g)
    t = alternate({"device": lambda: ops.diag_median(R, w)}, reps)
    t["bytes_moved"] = 2 * B * T * T * 4
    t["device_gb_per_s"] = t["bytes_moved"] / (t["device"]["ms"] * 1e-3) / 1e9
    return {"B": B, "T": T, "w": w, "diag_median": t}


def bench_ward(B, T, D, k, reps):
    g = torch.Generator(device="cuda").manual_seed(7)
    X = torch.randn((B, T, D), device="cuda", generator=g)
    res = {"B": B, "T": T, "D": D, "k": k}
    t = alternate({"device": lambda: ops.agglomerative(X, k)}, reps)
    try:
        from sklearn.cluster import AgglomerativeClustering
        from sklearn.feature_extraction.image import grid_to_graph
        Xh = X.cpu().numpy().astype(np.float64)
        conn = grid_to_graph(n_x=T, n_y=1, n_z=1)
        got = ops.agglomerative(X, k)[0].cpu().numpy()
        equal, t0 = 0, time.perf_counter()
        for b in range(B):
            labels = AgglomerativeClustering(n_clusters=k, connectivity=conn).fit(Xh[b]).labels_
            equal += int(np.array_equal(np.concatenate(([0], 1 + np.nonzero(np.diff(labels))[0])), got[b]))
        t["scikit-learn on the host"] = dict(ms=(time.perf_counter() - t0) * 1e3, windows=1)
        t["clips_with_equal_boundaries"] = equal
        t["host_over_device"] = t["scikit-learn on the host"]["ms"] / t["device"]["ms"]
    except ImportError:
        t["scikit-learn on the host"] = None
    res["agglomerative"] = t
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_bench.json"))
    ap.add_argument("--shapes", default="1x7750,64x431", help="B x T, comma separated")
    ap.add_argument("--only", default="path,median,ward", help="which of path, median, ward to run")
    ap.add_argument("--skip-composition-above", type=int, default=0,
                    help="leave the torch composition of path_enhance out above this T (0: always run it; its first call can "
                         "spend minutes choosing and building a convolution)")
    a = ap.parse_args()
    ops.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "cases": []}
    for s in a.shapes.split(","):
        B, T = (int(v) for v in s.split("x"))
        for name, fn in (("path", lambda: bench_path(B, T, 51, a.reps, not a.skip_composition_above or T <= a.skip_composition_above)),
                         ("median", lambda: bench_median(B, T, 7, a.reps)), ("ward", lambda: bench_ward(B, T, 12, 10, a.reps))):
            if name not in a.only.split(","):
                continue
            say(f"{name} B={B} T={T} ...")
            out["cases"].append(fn())
            say(json.dumps(out["cases"][-1]))
            torch.cuda.empty_cache()
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:                   # (after every case: a run that is cut short leaves what it has)
                f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
