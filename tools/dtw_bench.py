"""Time the device DTW chain (syg_dtw_cost_f32, syg_dtw_f32 through the C ABI, buffers made once) with HIP events: every
shape warmed, each sample a window of calls of about 50 ms, median of --reps windows.

Rows: 1024 pairs of 94 x 94 at K = 13; 256 pairs of 1000 x 1000 at K = 13 and K = 128; one pair of 16384 x 16384 at
K = 13 in the tiled form at several tile edges (the pair-resident form serves M <= syg_dtw_resident_max_cols() and so
not this row); a crossover table, both forms on 1 ... 256 pairs of 256 ... 1024 square.  Per row: the cost kernel, the
recurrence alone (distance only), the recurrence writing step codes, the backtrack (the chain with the path minus the
chain without), cells / s of the whole chain, and the chain's byte floor at 8 TB/s over its time: 4 bytes a cell of C
read, the step bytes written, and C written once where the cost kernel produced it.

In the same run a torch baseline on the same C: the recurrence one anti-diagonal at a time, torch.minimum on strided
diagonal views of a float64 matrix, values only (no step codes, no path).  Its end values are compared with the
kernel's in the run.

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
from sygnals_amd import ops  # noqa: E402
from sygnals_amd._lib import check, lib  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s


def timed(fn, reps, window_ms=50.0, inner_max=200):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    inner = int(min(inner_max, max(1, window_ms // max(a.elapsed_time(b), 1e-3))))
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return dict(ms=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)), inner=inner)


class Chain:
    """buffers of one shape, made once; the three entry calls"""

    def __init__(self, B, N, M, K=None, form=None, tile=0):
        g = torch.Generator(device="cuda").manual_seed(7)
        self.B, self.N, self.M, self.K, self.form, self.tile = B, N, M, K, form, tile
        self.h = lib()
        self.f = ops.DTW_FORMS[form]
        if K is not None:
            self.X = torch.randn((B, K, N), dtype=torch.float32, device="cuda", generator=g)
            self.Y = torch.randn((B, K, M), dtype=torch.float32, device="cuda", generator=g)
            self.Cm = torch.empty((B, N, M), dtype=torch.float32, device="cuda")
        else:
            self.Cm = torch.rand((B, N, M), dtype=torch.float32, device="cuda", generator=g)
        self.steps = torch.empty((B, N, M), dtype=torch.uint8, device="cuda")
        self.cost = torch.empty((B,), dtype=torch.float64, device="cuda")
        self.end = torch.empty((B,), dtype=torch.int32, device="cuda")
        self.path = torch.empty((B, N + M - 1, 2), dtype=torch.int32, device="cuda")
        self.plen = torch.empty((B,), dtype=torch.int32, device="cuda")
        self.wb = self.h.syg_dtw_work_bytes(B, N, M, self.f, tile)
        if self.wb < 0:
            check(-1, "syg_dtw_work_bytes")
        self.work = torch.empty((max(self.wb, 8) // 8,), dtype=torch.float64, device="cuda")
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run_cost(self):
        q = ops._ptr
        check(self.h.syg_dtw_cost_f32(q(self.X), q(self.Y), self.B, self.K, self.N, self.M, self.N, self.M, self.K * self.N,
                                      self.K * self.M, None, None, None, None, 0, q(self.Cm), self.st), "syg_dtw_cost_f32")

    def run_dtw(self, steps, path):
        q = ops._ptr
        check(self.h.syg_dtw_f32(q(self.Cm), self.B, self.N, self.M, self.M, self.N * self.M, None, None, None, None, None, None,
                                 0, self.f, self.tile, None, q(self.steps) if steps else None, q(self.cost), q(self.end),
                                 q(self.path) if path else None, q(self.plen) if path else None, q(self.work), self.wb, self.st),
              "syg_dtw_f32")


def row(B, N, M, K, form, tile, reps):
    c = Chain(B, N, M, K, form, tile)
    cells = float(B) * N * M
    out = dict(B=B, N=N, M=M, K=K, form=ops.dtw_plan(B, N, M, form=form, tile=tile)["form"], tile=tile or ops.dtw_constants()["tile"],
               work_bytes=c.wb)
    if K is not None:
        out["cost_kernel"] = timed(c.run_cost, reps)
    out["distance_only"] = timed(lambda: c.run_dtw(False, False), reps)
    out["with_steps"] = timed(lambda: c.run_dtw(True, False), reps)
    out["with_path"] = timed(lambda: c.run_dtw(True, True), reps)
    out["backtrack_ms"] = out["with_path"]["ms"] - out["with_steps"]["ms"]
    cost_ms = out["cost_kernel"]["ms"] if K is not None else 0.0
    for name, key, step_bytes in (("chain_distance", "distance_only", 0.0), ("chain_path", "with_path", 1.0)):
        ms = cost_ms + out[key]["ms"]
        floor = cells * (4.0 + step_bytes + (4.0 if K is not None else 0.0)) / HBM_BPS * 1e3
        out[name] = dict(ms=ms, gcells_per_s=cells / ms * 1e-6, byte_floor_ms=floor, floor_fraction=floor / ms)
    out["backtrack_share_of_chain_path"] = out["backtrack_ms"] / out["chain_path"]["ms"]
    return out, c


def torch_dtw(Cm):
    """values only, one anti-diagonal at a time: strided diagonal views of the padded float64 matrix"""
    B, N, M = Cm.shape
    W = M + 1
    D = torch.full((B, N + 1, W), float("inf"), dtype=torch.float64, device=Cm.device)
    C64 = Cm.double()
    bs, bc = (N + 1) * W, N * M
    for d in range(N + M - 1):
        n_lo, n_hi = max(0, d - (M - 1)), min(N - 1, d)
        L = n_hi - n_lo + 1
        o = n_lo * M + d
        c = torch.as_strided(C64, (B, L), (bc, M - 1), n_lo * (M - 1) + d)
        if d == 0:
            best = c
        else:
            diag = torch.as_strided(D, (B, L), (bs, M), o)
            up = torch.as_strided(D, (B, L), (bs, M), o + 1)
            left = torch.as_strided(D, (B, L), (bs, M), o + W)
            best = torch.minimum(torch.minimum(diag, left), up) + c
        torch.as_strided(D, (B, L), (bs, M), o + W + 1).copy_(best)
    return D[:, N, M]


def baseline(c, reps, ours_ms):
    c.run_dtw(False, False)
    got = torch_dtw(c.Cm)
    diff = float(((got - c.cost).abs() / c.cost.abs()).max())
    t = timed(lambda: torch_dtw(c.Cm), reps, window_ms=0.0)
    return dict(t, what="torch: float64 recurrence over anti-diagonals, torch.minimum on diagonal views, values only",
                max_rel_diff_of_cost_to_kernel=diff, baseline_over_kernel_distance_only=t["ms"] / ours_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-crossover", action="store_true")
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (the figures mean nothing)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"constants": ops.dtw_constants()}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")

    big = 16384 if not a.small else 1500
    shapes = [("batch_1024x94x94_K13", 1024, 94, 94, 13, None, 0), ("batch_256x1000x1000_K13", 256, 1000, 1000, 13, None, 0),
              ("batch_256x1000x1000_K128", 256, 1000, 1000, 128, None, 0)]
    if a.small:
        shapes = [("batch_8x94x94_K13", 8, 94, 94, 13, None, 0)]
    shapes += [(f"one_{big}x{big}_K13_tile{t}", 1, big, big, 13, "tiled", t) for t in (128, 256, 512, 1024)]
    for name, B, N, M, K, form, tile in shapes:
        res[name], c = row(B, N, M, K, form, tile, a.reps)
        write()
        if not a.no_baseline and tile in (0, 256):
            res[name]["baseline_torch"] = baseline(c, a.reps if B * N * M < (1 << 27) else 2, res[name]["distance_only"]["ms"])
            write()
        del c
    if not a.no_crossover:
        table = []
        for n in ((256, 512, 1000, 1024) if not a.small else (256,)):
            for B in ((1, 4, 16, 64, 256) if not a.small else (1, 4)):
                e = dict(B=B, N=n, M=n)
                for label, form, tile in (("resident", "resident", 0), ("tiled_128", "tiled", 128), ("tiled_256", "tiled", 256)):
                    c = Chain(B, n, n, None, form, tile)
                    e[label + "_ms"] = timed(lambda: c.run_dtw(True, False), a.reps)["ms"]
                    del c
                table.append(e)
        res["crossover_with_steps"] = table
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
