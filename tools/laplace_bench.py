"""Time the device numerical Laplace transform (syg_laplace_f32 through the C ABI, tables and buffers made once) with HIP
events: every shape warmed, each sample a window of --inner calls, median of --reps windows.

Shapes: 1024 clips x 32768 samples with S = 16, 64 and 256 s-values, once with sigma >= 0 (forward columns) and once with
sigma < 0 (reversed columns); one row of 2^24 samples with S = 64 (the segmented form, and the whole-row form beside it);
one row of 32768 samples with S = 4096, the sigma x omega surface of `dsp laplace`.  Each time is reported against the
larger of two floors, both from the hardware's own figures: reading the rows once (4 B L bytes at 8 TB/s) and the
contraction's 4 B S L flop at the float32 matrix peak (157.3 TF); `form` names the launch form the library's rule picked.
Each case also reports its worst error against the float64 formula on a few rows, on the natural scale A.

In the same run an independent baseline on the same device at 1024 x 32768, S = 64: torch.exp materialising E [L, S] in
complex64, then x.to(complex64) @ E, with its error against float64 beside its time (its float32 phase is expected to
miss the 1e-5 gate).

Prints one JSON object and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _laplace as LP  # noqa: E402
from sygnals_amd import ops  # noqa: E402
from sygnals_amd._lib import check, lib  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
F32_MATRIX_FLOPS = 157.3e12
T_STEP = 1.0 / 22050.0


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


def floors(t, B, L, S):
    byte_ms, flop_ms = 4.0 * B * L / HBM_BPS * 1e3, 4.0 * B * S * L / F32_MATRIX_FLOPS * 1e3
    floor = max(byte_ms, flop_ms)
    return dict(t, byte_floor_ms=byte_ms, flop_floor_ms=flop_ms, floor="bytes" if byte_ms >= flop_ms else "flop",
                floor_fraction=floor / t["ms"], tflops=4.0 * B * S * L / t["ms"] * 1e-9)


def s_grid(S, L, sign):
    """S points, sigma (L - 1) t_step in (0, 20] (decay or growth over the clip by up to e^20), omega over [0, pi / t_step]."""
    i = np.arange(S)
    return sign * (20.0 * ((i * 7) % S + 1) / S) / ((L - 1) * T_STEP) + 1j * np.pi * (i + 0.5) / S / T_STEP


def err_on_rows(x, got, s, rows=2):
    """worst |got - float64 formula| / A on the first rows (NumPy on the host, blocks of 4096 samples)."""
    xs = x[:rows].cpu().numpy().astype(np.float64)
    L = xs.shape[1]
    ref = np.zeros((rows, len(s)), dtype=np.complex128)
    A = np.zeros((rows, len(s)))
    for n0 in range(0, L, 4096):
        t = np.arange(n0, min(L, n0 + 4096)) * T_STEP
        E = np.exp(-s[:, None] * t[None, :])
        ref += xs[:, n0:n0 + 4096] @ E.T
        A += np.abs(xs[:, n0:n0 + 4096]) @ np.abs(E).T
    return float(np.max(np.abs(got[:rows].cpu().numpy() - ref * T_STEP) / (A * T_STEP)))


def case(B, L, s, reps, inner, form=None, err_cols=64):
    h = lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    S = len(s)
    p, table, fac, col = ops.laplace_plan(s, T_STEP)
    anchor = ops._dev(LP.anchors(p, L))
    f = ops.LAPLACE_FORMS[form]
    wb = h.syg_laplace_work_bytes(B, L, p.S16, f)
    work = torch.empty((max(wb, 16) // 8,), dtype=torch.float64, device="cuda")
    out = torch.empty((B, S), dtype=torch.complex128, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = ops._ptr

    def run():
        check(h.syg_laplace_f32(q(x), B, L, L, q(table), q(fac), q(anchor), q(col), p.S_fwd, p.S_rev, p.S_steep_fwd,
                                p.S_steep_rev, S, T_STEP, q(out), q(work), f, st), "syg_laplace_f32")

    run()
    keep = np.unique(np.linspace(0, S - 1, min(S, err_cols if L <= (1 << 16) else 8)).astype(int))      # a spread of the columns
    res = dict(B=B, L=L, S=S, form="segmented" if wb > 0 else "whole", work_bytes=int(wb),
               worst_err_over_A=err_on_rows(x, out[:, torch.from_numpy(keep).cuda()], s[keep], 2 if L <= (1 << 16) else 1))
    one = timed(run, 1, 1, warm=1)["ms"]
    n_in = int(min(inner, max(1, 50.0 // one)))                      # windows of about 50 ms
    res.update(floors(dict(timed(run, reps, n_in, warm=1), inner=n_in), B, L, S))
    return res


def baseline(B, L, S, reps):
    """torch alone: E = exp(-s t) [L, S] complex64 made on the device at every call, then a complex64 matmul."""
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    s = s_grid(S, L, 1.0)
    sd = torch.from_numpy(s.astype(np.complex64)).cuda()
    t = torch.arange(L, device="cuda", dtype=torch.float32) * T_STEP

    def run():
        E = torch.exp(-t[:, None] * sd[None, :])
        return (x.to(torch.complex64) @ E) * T_STEP

    got = run().to(torch.complex128)
    res = dict(B=B, L=L, S=S, what="torch.exp to E [L, S] complex64, then x.to(complex64) @ E",
               worst_err_over_A=err_on_rows(x, got, s))
    res.update(floors(timed(run, reps, 1, warm=1), B, L, S))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laplace_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"constants": ops.laplace_constants()}
    B, L = 1024, 32768
    for S in (16, 64, 256):
        for sign, name in ((1.0, "forward"), (-1.0, "reversed")):
            res[f"batch_1024x32768_S{S}_{name}"] = case(B, L, s_grid(S, L, sign), a.reps, a.inner)
    for form in (None, "whole"):
        res[f"one_row_2p24_S64_{form or 'rule'}"] = case(1, 1 << 24, s_grid(64, 1 << 24, 1.0), a.reps if form is None else 3,
                                                        a.inner, form)
    half = np.concatenate([s_grid(2048, 32768, 1.0), s_grid(2048, 32768, -1.0)])
    res["surface_1x32768_S4096"] = case(1, 32768, half, a.reps, a.inner)
    res["baseline_torch_1024x32768_S64"] = baseline(B, L, 64, a.reps)
    ours = res["batch_1024x32768_S64_forward"]["ms"]
    res["baseline_over_kernel_time"] = res["baseline_torch_1024x32768_S64"]["ms"] / ours
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
