"""Time one NMF iteration (syg_nmf_f32, both losses) with HIP events: every case warmed, each sample a window of calls of
about 50 ms, median of --reps windows; the device kernels and the composition alternate window by window.

Shapes: 1024 clips x 65 frames x 1025 bins at K = 8, 16, 32, 64, and one clip of 10 000 frames x 1025 bins at K = 16.
The device kernels are timed in both forms of their contractions, plain FMA and the f32-input MFMA; `form_auto` names the
one the library takes by itself at that K, and the ratios are that form's.
Beside each timing stands the same iteration written here as torch.bmm plus pointwise ops on the same device -- the
baseline a user has today; under Kullback-Leibler it writes AC and V / AC as [B, T, F] tensors twice an iteration.
The byte floor of an iteration is two reads of V plus the factor traffic (A and C each read and written once, 4 B an
entry) at 8 TB/s.  There is no parent-commit time: the capability is new.
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

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
EPS = float(np.finfo(np.float32).eps)
N_ITER = 4                # iterations per timed call (one call is one host entry into syg_nmf_f32)


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


def torch_iteration(V, A, C, kl):
    """One iteration as a user composes it today (in place on A and C)."""
    if kl:
        R = V / torch.bmm(A, C).clamp_(min=EPS)
        den = C.sum(dim=2)[:, None, :]
        A.mul_(torch.bmm(R, C.transpose(1, 2)) / torch.where(den == 0, EPS, den))
        R = V / torch.bmm(A, C).clamp_(min=EPS)
        den = A.sum(dim=1)[:, :, None]
        C.mul_(torch.bmm(A.transpose(1, 2), R) / torch.where(den == 0, EPS, den))
    else:
        den = torch.bmm(A, torch.bmm(C, C.transpose(1, 2)))
        A.mul_(torch.bmm(V, C.transpose(1, 2)) / torch.where(den == 0, EPS, den))
        At = A.transpose(1, 2)
        den = torch.bmm(torch.bmm(At, A), C)
        C.mul_(torch.bmm(At, V) / torch.where(den == 0, EPS, den))


def bench_shape(B, T, F, K, reps):
    g = torch.Generator(device="cuda").manual_seed(5)
    V = torch.rand((B, T, F), device="cuda", generator=g)
    A0, C0 = ops.nmf(V, K, n_iter=0, seed=1)
    work = ops._workspace("syg_nmf_work_bytes", B, T, F, K, dtype=torch.float64, device=V.device)
    p = ops._ptr
    res = {"B": B, "T": T, "F": F, "K": K, "iterations_per_call": N_ITER}
    floor = 4 * (2 * B * T * F + 2 * (B * T * K + B * K * F))
    res["floor_bytes"] = floor
    res["floor_ms"] = floor / HBM_BPS * 1e3
    cases = {}
    for loss, name in ((0, "frobenius"), (1, "kullback-leibler")):
        A, C = A0.clone(), C0.clone()
        At, Ct = A0.clone(), C0.clone()
        Am, Cm = A0.clone(), C0.clone()

        def device():
            ops._call("syg_nmf_f32", p(V), B, T, F, K, p(A), p(C), 0, N_ITER, loss, 1, 1, 0, p(work))

        def device_mfma():
            ops._call("syg_nmf_f32", p(V), B, T, F, K, p(Am), p(Cm), 0, N_ITER, loss, 1, 1, 1, p(work))

        def composed():
            for _ in range(N_ITER):
                torch_iteration(V, At, Ct, loss == 1)

        # the two agree before they are timed (fp32, different summation orders)
        device()
        device_mfma()
        composed()
        torch.cuda.synchronize()
        agree = float(((A - At).abs().max() / At.abs().max()).item())
        agree_m = float(((Am - At).abs().max() / At.abs().max()).item())
        t = alternate({"device, fma": device, "device, mfma": device_mfma, "torch.bmm composition": composed}, reps)
        for v in t.values():
            v["ms_per_iteration"] = v["ms"] / N_ITER
        auto = "mfma" if K >= ops.nmf_constants()["mfma_min_components"] else "fma"
        d, c = t[f"device, {auto}"]["ms_per_iteration"], t["torch.bmm composition"]["ms_per_iteration"]
        cases[name] = dict(t, form_auto=auto, agree_after_first_call=dict(fma=agree, mfma=agree_m), of_floor=res["floor_ms"] / d,
                           composition_over_device=c / d)
    res["cases"] = cases
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmf_bench.json"))
    ap.add_argument("--shapes", default="1024x65x1025x8,1024x65x1025x16,1024x65x1025x32,1024x65x1025x64,1x10000x1025x16")
    a = ap.parse_args()
    ops.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BPS, "shapes": []}
    for s in a.shapes.split(","):
        B, T, F, K = (int(v) for v in s.split("x"))
        out["shapes"].append(bench_shape(B, T, F, K, a.reps))
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
