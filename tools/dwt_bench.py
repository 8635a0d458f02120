"""Time the device wavelet transform through the C ABI with HIP events (buffers allocated once, every shape warmed, each
sample a window of --inner calls, median of --reps): 1024 clips x 32768 samples and one row of 2^24 samples, db4 at the
maximum level, forward (syg_dwt_f32) and back (syg_idwt_f32), in the default form (the clip-resident kernels wherever a
row fits) and level by level (dwt_form = 0: one launch per level, the approximations through HBM), the two alternating
in one process.  Each figure is reported as ms, Msamples / s and a fraction of the HBM roofline, the algorithmic bytes
being one read of x plus one write of the packed row (and the reverse for the inverse) over 8 TB/s.  The two forms'
outputs are compared bit for bit at the timed sizes.  Prints one JSON object and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _wavelets as W  # noqa: E402
from sygnals_amd import ops  # noqa: E402
from sygnals_amd._lib import check, lib  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
WAVELET, MODE = "db4", "symmetric"


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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


class Case:
    """One shape: buffers and the two C calls."""

    def __init__(self, B, L):
        h = self.h = lib()
        self.B, self.L = B, L
        (self.dec_lo, self.dec_hi, self.rec_lo, self.rec_hi), self.F = ops._wavelet_dev(WAVELET)
        self.level = W.dwt_max_level(L, self.F)
        self.lens = (C.c_int64 * (self.level + 1))()
        self.lp = C.cast(self.lens, C.c_void_p)
        self.total = h.syg_dwt_lengths(L, self.F, self.level, self.lp)
        self.Lout = h.syg_idwt_length(self.lp, self.level, self.F)
        g = torch.Generator(device="cuda").manual_seed(11)
        self.x = torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
        self.out = torch.empty((B, self.total), dtype=torch.float32, device="cuda")
        self.y = torch.empty((B, self.Lout), dtype=torch.float32, device="cuda")
        with ops.override(dwt_form=0):         # the larger of the two forms' workspaces
            wb = max(h.syg_dwt_work_bytes(B, L, self.F, self.level), h.syg_idwt_work_bytes(B, self.lp, self.level, self.F))
        self.work = torch.empty((max(wb, 4) // 4,), dtype=torch.float32, device="cuda")
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward(self):
        p = ops._ptr
        check(self.h.syg_dwt_f32(p(self.x), self.B, self.L, self.L, p(self.dec_lo), p(self.dec_hi), self.F,
                                 W.mode_code(MODE), self.level, p(self.out), self.total, p(self.work), self.st), "syg_dwt_f32")

    def inverse(self):
        p = ops._ptr
        check(self.h.syg_idwt_f32(p(self.out), self.B, self.total, self.lp, self.level, p(self.rec_lo), p(self.rec_hi), self.F,
                                  p(self.y), self.Lout, p(self.work), self.st), "syg_idwt_f32")

    def figures(self, ms, nbytes):
        med, lo, hi = ms
        floor_ms = nbytes / HBM_BPS * 1e3
        return dict(ms=med, ms_min=lo, ms_max=hi, msamples_per_s=self.B * self.L / med * 1e-3, hbm_floor_ms=floor_ms,
                    hbm_fraction=floor_ms / med)


def run_case(B, L, reps, inner):
    c = Case(B, L)
    res = dict(B=B, L=L, wavelet=WAVELET, mode=MODE, level=c.level, packed_row=int(c.total),
               resident=bool(c.h.syg_dwt_fits(L, c.F, c.level)))
    nbytes = 4 * B * (L + c.total)
    # the two forms give the same bits
    c.forward()
    c.inverse()
    a_out, a_y = c.out.clone(), c.y.clone()
    with ops.override(dwt_form=0):
        c.forward()
        c.inverse()
    res["forms_identical"] = bool(torch.equal(a_out, c.out) and torch.equal(a_y, c.y))
    res["round_trip_peak_rel"] = float((c.y[:, :L] - c.x).abs().max() / c.x.abs().max())
    del a_out, a_y
    t = {k: [] for k in ("forward", "inverse", "forward_level_by_level", "inverse_level_by_level")}
    for _ in range(2):                          # default, level by level, default, level by level
        t["forward"].append(timed(c.forward, reps, inner))
        t["inverse"].append(timed(c.inverse, reps, inner))
        with ops.override(dwt_form=0):
            t["forward_level_by_level"].append(timed(c.forward, reps, inner))
            t["inverse_level_by_level"].append(timed(c.inverse, reps, inner))
    for k, v in t.items():
        best = min(v, key=lambda m: m[0])
        res[k] = c.figures(best, nbytes)
        res[k]["ms_runs"] = [m[0] for m in v]
    res["forward_speedup_over_level_by_level"] = res["forward_level_by_level"]["ms"] / res["forward"]["ms"]
    res["inverse_speedup_over_level_by_level"] = res["inverse_level_by_level"]["ms"] / res["inverse"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwt_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"batch_1024x32768": run_case(1024, 32768, a.reps, a.inner),
           "one_row_2p24": run_case(1, 1 << 24, a.reps, a.inner)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
