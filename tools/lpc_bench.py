"""Time the device linear prediction (ops.lpc_frames, ops.lpc_rows, ops.lpc_envelope) with HIP events: every shape warmed,
each sample a window of --inner calls, median of --reps windows.

Shapes: 1024 clips x 32768 samples at frames of 2048 / hop 512 and at frames of 400 / hop 160 (the speech shape), order
16, both methods; one row of 2^24 samples at order 16 in the stage form, both methods.  Each time stands beside its byte
floor, 4 B (L + (p + 1) T) bytes at 8 TB/s, its float64 arithmetic by the count 8 p N flop a frame for Burg and
2 (p + 1) N for the autocorrelation method, and a torch baseline of the same run (unfold, then the stage loop in float64).

Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _lpc, ops  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
TINY = float(np.finfo(np.float64).tiny)


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


def rows(B, L):
    g = torch.Generator(device="cuda").manual_seed(7)
    return torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)


def measure(fn, reps, inner, floor_bytes, flop, **info):
    one = timed(fn, 1, 1, warm=1)["ms"]
    n_in = int(min(inner, max(1, 50.0 // one)))                      # windows of about 50 ms
    t = timed(fn, reps, n_in, warm=1)
    floor = floor_bytes / HBM_BPS * 1e3
    return dict(t, inner=n_in, byte_floor_ms=floor, floor_fraction=floor / t["ms"], f64_flop=flop, f64_tflops=flop / t["ms"] * 1e-9, **info)


def torch_frames(y, N, hop):
    return torch.nn.functional.pad(y, (N // 2, N // 2)).unfold(1, N, hop).to(torch.float64)      # [B, T, N]


def torch_burg(x, p):
    """Burg's stage loop on rows x [..., N] float64 -> a [..., p + 1]."""
    f, b = x[..., 1:], x[..., :-1]
    a = torch.zeros(x.shape[:-1] + (p + 1,), dtype=torch.float64, device=x.device)
    a[..., 0] = 1.0
    for i in range(p):
        k = -2.0 * (f * b).sum(-1) / ((f * f + b * b).sum(-1) + TINY)
        prev = a[..., :i + 2].clone()
        a[..., :i + 2] = prev + k[..., None] * prev.flip(-1)
        f, b = (f + k[..., None] * b)[..., 1:], (b + k[..., None] * f)[..., :-1]
    return a


def torch_autocorr(xw, p):
    r = torch.stack([(xw[..., :xw.shape[-1] - l] * xw[..., l:]).sum(-1) for l in range(p + 1)], -1)
    a = torch.zeros_like(r)
    a[..., 0] = 1.0
    E = r[..., 0].clone()
    for i in range(p):
        acc = r[..., i + 1] + (a[..., 1:i + 1] * r[..., 1:i + 1].flip(-1)).sum(-1)
        k = -acc / E
        prev = a[..., :i + 2].clone()
        a[..., :i + 2] = prev + k[..., None] * prev.flip(-1)
        E = E * (1.0 - k * k)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpc_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"constants": ops.lpc_constants()}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")

    B, L, p = 1024, 32768, 16
    y = rows(B, L)
    for N, hop in ((2048, 512), (400, 160)):
        T = ops.cepstrogram_frames(L, N, hop, True)
        floor = 4.0 * B * (L + (p + 1) * T)
        out = torch.empty((B, p + 1, T), dtype=torch.float32, device="cuda")
        for method, flop in (("burg", 8.0 * p * N), ("autocorr", 2.0 * (p + 1) * N)):
            key = f"frames_1024x32768_n{N}_hop{hop}_p{p}_{method}"
            info = dict(B=B, L=L, N=N, hop=hop, order=p, T=T, method=method)
            res[key] = measure(lambda: ops.lpc_frames(y, p, N, hop, True, method, out=out), a.reps, a.inner, floor, flop * B * T, **info)
            win = None if method == "burg" else ops.window_dev("hann", N, N).double()
            fn = (lambda: torch_burg(torch_frames(y, N, hop), p)) if method == "burg" else \
                (lambda: torch_autocorr(torch_frames(y, N, hop) * win, p))
            base = fn()[:, :T].transpose(1, 2)
            t = measure(fn, 3, 2, floor, flop * B * T, form="torch", **info)
            ours = ops.lpc_frames(y, p, N, hop, True, method).double()
            t["max_diff_to_kernel"] = float((base - ours).abs().max())
            t["baseline_over_kernel_time"] = t["ms"] / res[key]["ms"]
            res[key + "_torch"] = t
            del base, ours
            torch.cuda.empty_cache()
            write()
    # with k, err and the envelope in dB on top (2048 / 512)
    T = ops.cepstrogram_frames(L, 2048, 512, True)
    aa, _, ee = ops.lpc_frames(y, p, 2048, 512, True, "burg", None, True, True)
    res["envelope_1024x1025x65_p16_db"] = measure(lambda: ops.lpc_envelope(aa, ee, 2048, db=True), a.reps, a.inner,
                                                  4.0 * B * T * (p + 2 + 1025), 8.0 * p * 1025 * B * T, B=B, T=T, n_fft=2048, order=p)
    write()
    del y, aa, ee
    n = 1 << 24
    x = rows(1, n)
    for method, flop in (("burg", 8.0 * p * n), ("autocorr", 2.0 * (p + 1) * n)):
        key = f"rows_1x2p24_p{p}_{method}_stage"
        res[key] = measure(lambda: ops.lpc_rows(x, p, method, form="stage"), max(3, a.reps // 2), a.inner, 4.0 * (n + p + 1), flop,
                           B=1, L=n, order=p, method=method, work_bytes=int(ops.lib().syg_lpc_rows_work_bytes(1, n, p, _lpc.METHODS[method])))
        win = None if method == "burg" else ops.window_dev("hann", n, n).double()
        fn = (lambda: torch_burg(x.double(), p)) if method == "burg" else (lambda: torch_autocorr(x.double() * win, p))
        base = fn()
        t = measure(fn, 3, 2, 4.0 * (n + p + 1), flop, form="torch", B=1, L=n, order=p, method=method)
        t["max_diff_to_kernel"] = float((base - ops.lpc_rows(x, p, method, form="stage").double()).abs().max())
        t["baseline_over_kernel_time"] = t["ms"] / res[key]["ms"]
        res[key + "_torch"] = t
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
