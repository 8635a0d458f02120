"""Time the device PCEN (ops.pcen) with HIP events: every shape warmed, each sample a window of calls of about 50 ms,
median of --reps windows.

Shapes [B, M, T]: 1024 x [128, 65] and 1024 x [40, 65] (training batches), 256 x [128, 3001] (30 s clips) and 1 x [128, 2^20]
(one long recording); max_size 1 and 3; the form the library's rule takes and, where it runs, the other one.  Per case:
the time, Msamples/s and the fraction of the byte floor (the input read once and the output written once, 8 B M T bytes
at 8 TB/s).  Beside it, in the same run, the torch formulation a user would write: the running maximum by slices, a T-step
loop of in-place lerp launches for the smoother, then the pointwise law.  Where that loop would take more than --torch-steps
launches it is timed over its first --torch-steps frames and scaled to T (marked "extrapolated").
Prints one JSON object and writes it to --out."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import ops  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
GAIN, BIAS, POWER, EPS, SCALE = 0.98, 2.0, 0.5, 1e-6, float(2 ** 31)
B_COEF = 0.05638943879134889


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


def measure(fn, reps, n, **info):
    one = timed(fn, 1, 1, warm=1)["ms"]
    n_in = int(min(200, max(1, 50.0 // max(one, 1e-3))))
    r = dict(timed(fn, reps, n_in, warm=1), inner=n_in, **info)
    r["msamples_per_s"] = n / r["ms"] / 1e3
    r["floor_ms"] = 8 * n / HBM_BPS * 1e3
    r["of_floor"] = r["floor_ms"] / r["ms"]
    return r


def torch_pcen(S, ms, steps):
    """The torch formulation over the first `steps` frames of the smoother (all of them when steps >= T)."""
    S = S * SCALE
    if ms == 3:
        P = torch.cat([S[:, :1], S, S[:, -1:]], dim=1)
        ref = torch.maximum(torch.maximum(P[:, :-2], P[:, 1:-1]), P[:, 2:])
    else:
        ref = S
    M = torch.empty_like(S)
    M[..., 0] = ref[..., 0] * B_COEF + (1.0 - B_COEF)
    for t in range(1, min(steps, S.shape[-1])):
        torch.lerp(M[..., t - 1], ref[..., t], B_COEF, out=M[..., t])
    if steps < S.shape[-1]:
        M[..., steps:] = ref[..., steps:]
    smooth = torch.exp(-GAIN * (math.log(EPS) + torch.log1p(M / EPS)))
    return BIAS ** POWER * torch.expm1(POWER * torch.log1p(S * smooth / BIAS))


def bench_shape(B, M, T, reps, torch_steps):
    g = torch.Generator(device="cuda").manual_seed(5)
    S = torch.randn((B, M, T), device="cuda", generator=g).square_() * 1e-3
    out = torch.empty_like(S)
    n = B * M * T
    res = {"B": B, "M": M, "T": T, "cases": []}
    for ms in (1, 3):
        rule = ops.pcen_form(T, M, ms)
        k = ops.pcen_constants()
        fits = ((2 + ms - 1) * (T | 1) + 8) * 4 <= k["lds_max"]
        for form in ("resident", "tiled"):
            if form == "resident" and not fits:
                continue
            r = measure(lambda: ops.pcen(S, b=B_COEF, max_size=ms, scale=SCALE, out=out, form=form), reps, n,
                        max_size=ms, form=form, is_rule=form == rule)
            res["cases"].append(r)
        steps = min(T, torch_steps)
        whole = timed(lambda: torch_pcen(S, ms, steps), 3, 1, warm=1)
        tr = dict(max_size=ms, form="torch loop", launches_timed=steps, **whole)
        if steps < T:
            head = timed(lambda: torch_pcen(S, ms, 1), 3, 1, warm=1)["ms"]         # everything but the loop
            tr["extrapolated"] = True
            tr["ms"] = head + (whole["ms"] - head) * (T - 1) / (steps - 1)
        tr["msamples_per_s"] = n / tr["ms"] / 1e3
        res["cases"].append(tr)
        for r in res["cases"]:
            if r["max_size"] == ms and r["form"] != "torch loop":
                r["of_torch_loop"] = r["ms"] / tr["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-steps", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcen_bench.json"))
    ap.add_argument("--shapes", default="1024x128x65,1024x40x65,256x128x3001,1x128x1048576")
    a = ap.parse_args()
    ops.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "gain": GAIN, "bias": BIAS, "power": POWER, "eps": EPS, "b": B_COEF, "scale": SCALE,
           "hbm_bytes_per_s": HBM_BPS, "constants": ops.pcen_constants(), "shapes": []}
    for s in a.shapes.split(","):
        B, M, T = (int(v) for v in s.split("x"))
        out["shapes"].append(bench_shape(B, M, T, a.reps, a.torch_steps))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
