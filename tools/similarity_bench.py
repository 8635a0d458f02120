"""Time the k-NN search (syg_sim_knn_f32, cosine) and the median nn_filter (syg_nn_filter_f32) with HIP events: every
case warmed, each sample a window of calls of about 50 ms, median of --reps windows; the device kernels and a composition
alternate window by window.

Shapes (B, T, D, k): one three-minute clip of 7750 frames x 1025 bins at k = 178, 64 ten-second clips of 431 frames at
k = 40, and 1024 short sequences of 128 frames x 12 features at k = 23.
Beside each timing stands the same result composed from torch on the same device -- the baseline a user has today:
normalised frames, torch.bmm to the dense [B, T, T] similarity, the diagonal masked, torch.topk; and for the filter a
gather of the neighbours' rows ([rows, k, F], at most 1 GiB at a time) and torch.median along k (which takes the lower
middle value at an even count, where the kernel takes numpy's mean of the two).
Reported, not gated: the capability is new, there is no parent-commit time, and nothing is routed to the composition.
Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import ops  # noqa: E402

GATHER_BYTES = 1 << 30


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, reps):
    """{name: fn} -> {name: stats}: every fn warmed, then reps rounds of one window each, in turn."""
    inner = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        one = window(fn, 1)
        inner[k] = int(min(200, max(1, 50.0 // max(one, 1e-3))))
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(window(fn, inner[k]))
    return {k: dict(ms=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)), inner=inner[k]) for k, v in ts.items()}


def torch_knn(X, k):
    """Cosine k-NN as a user composes it today: the dense similarity, the frame itself masked, topk."""
    Xn = X / X.norm(dim=2, keepdim=True).clamp_(min=1e-30)
    sim = torch.bmm(Xn, Xn.transpose(1, 2))
    sim.diagonal(dim1=1, dim2=2).fill_(-float("inf"))
    val, idx = torch.topk(sim, k, dim=2)
    return idx, 1.0 - val


def torch_median_filter(S, idx):
    B, T, F = S.shape
    k = idx.shape[2]
    out = torch.empty_like(S)
    rows = max(1, GATHER_BYTES // (k * F * 4))
    for b in range(B):
        for lo in range(0, T, rows):
            out[b, lo:lo + rows] = S[b][idx[b, lo:lo + rows].long()].median(dim=1).values
    return out


def bench_shape(B, T, D, k, reps):
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.rand((B, T, D), device="cuda", generator=g)
    res = {"B": B, "T": T, "D": D, "k": k, "metric": "cosine", "contraction_flop": 2 * B * T * T * D}
    idx, dist, count = ops.sim_knn(X, None, k, 1, "cosine")
    tidx, tdist = torch_knn(X, k)
    torch.cuda.synchronize()
    # the two agree before they are timed: the same neighbour sets on nearly every row (ties and fp32 order aside)
    same = (torch.sort(idx.long(), dim=2).values == torch.sort(tidx, dim=2).values).all(dim=2).float().mean()
    res["rows_with_equal_sets"] = float(same.item())
    res["distance_difference_max"] = float((dist - tdist).abs().max().item())
    t = alternate({"device": lambda: ops.sim_knn(X, None, k, 1, "cosine"), "torch composition": lambda: torch_knn(X, k)}, reps)
    t["composition_over_device"] = t["torch composition"]["ms"] / t["device"]["ms"]
    t["device_tflops"] = res["contraction_flop"] / (t["device"]["ms"] * 1e-3) / 1e12
    res["sim_knn"] = t
    f = alternate({"device": lambda: ops.nn_filter(X, idx, count, None, "median"),
                   "torch composition": lambda: torch_median_filter(X, idx)}, reps)
    f["composition_over_device"] = f["torch composition"]["ms"] / f["device"]["ms"]
    res["nn_filter_median"] = f
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_bench.json"))
    ap.add_argument("--shapes", default="1x7750x1025x178,64x431x1025x40,1024x128x12x23")
    a = ap.parse_args()
    ops.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for s in a.shapes.split(","):
        B, T, D, k = (int(v) for v in s.split("x"))
        out["shapes"].append(bench_shape(B, T, D, k, a.reps))
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
