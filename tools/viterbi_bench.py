"""Time the Viterbi decoder (syg_viterbi_f32) with HIP events: every case warmed, each sample a window of calls of about
50 ms, median of --reps windows; the forms and the yardstick alternate window by window.

Shapes (B, S, T): chord-sized tables over short and long clips (1024 x 25 x 65, 64 x 25 x 3001), two-state masks
(12 288 x 2 x 65, 1024 x 2 x 3001), and one long sequence over many states (1 x 600 x 3001, 1 x 1024 x 300).  The input
is float32 probabilities [B, S, T], time fastest, so the device's float64 log is part of every timing.
Each form is timed wherever it is legal.  The yardstick is what a user writes today: the same recurrence as a Python loop
over the frames on device tensors in float64 (a broadcast add and a max with indices a step), the pointers copied to the
host and walked there.  Its paths are compared with the kernel's before anything is timed.
A second sweep times both forms at every S the narrow form serves (12 288 sequences of 65 frames): the library's default
rule (syg_viterbi_form) is set from it.
Reported, not gated: the capability is new and there is no parent-commit time.  Prints one JSON object and writes it to
--out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _sequence as SQ  # noqa: E402
from sygnals_amd import ops  # noqa: E402


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


def torch_viterbi(prob, lt, li, eps):
    """The recurrence as a loop over frames on device tensors, the walk on the host."""
    lp = torch.log(prob.to(torch.float64) + eps)
    B, S, T = lp.shape
    value = lp[:, :, 0] + li
    ptrs = []
    for t in range(1, T):
        best, p = (value[:, :, None] + lt[None]).max(dim=1)
        ptrs.append(p)
        value = lp[:, :, t] + best
    last = value.argmax(dim=1).cpu().numpy()
    states = np.zeros((B, T), dtype=np.int64)
    states[:, -1] = last
    if ptrs:
        ptr = torch.stack(ptrs).cpu().numpy()                       # [T - 1, B, S]
        rows = np.arange(B)
        for t in range(T - 2, -1, -1):
            states[:, t] = ptr[t, rows, states[:, t + 1]]
    return states


def inputs(B, S, T):
    g = torch.Generator(device="cuda").manual_seed(5)
    prob = torch.rand((B, S, T), device="cuda", generator=g) + 1e-3
    prob = prob / prob.sum(dim=1, keepdim=True)
    rng = np.random.default_rng(S)
    tr = rng.random((S, S)) ** 4
    tr /= tr.sum(axis=1, keepdims=True)
    return prob, tr


def bench_shape(B, S, T, reps, yardstick=True):
    K = ops.viterbi_constants()
    prob, tr = inputs(B, S, T)
    eps = SQ.tiny(np.float32)
    res = {"B": B, "S": S, "T": T, "default_form": ops.viterbi_form(B, S)}
    forms = ["wide"] + (["narrow"] if S <= K["s_narrow"] else [])
    fns = {f: (lambda f=f: ops.viterbi(prob, tr, form=f)) for f in forms}
    if yardstick:
        lt = torch.from_numpy(np.log(tr + eps)).cuda()
        li = torch.full((S,), float(np.log(1.0 / S + eps)), dtype=torch.float64, device="cuda")
        want = torch_viterbi(prob, lt, li, eps)
        for f in forms:                                             # the paths agree before anything is timed
            got = ops.viterbi(prob, tr, form=f).cpu().numpy()
            res[f"rows_equal_to_yardstick_{f}"] = float(np.mean(np.all(got == want, axis=1)))
        fns["torch loop over frames"] = lambda: torch_viterbi(prob, lt, li, eps)
    t = alternate(fns, reps)
    for f in forms:
        t[f]["us_per_frame"] = t[f]["ms"] * 1e3 / T
        t[f]["ns_per_sequence_frame"] = t[f]["ms"] * 1e6 / (B * T)
        if yardstick:
            t[f]["yardstick_over_form"] = t["torch loop over frames"]["ms"] / t[f]["ms"]
    if len(forms) == 2:
        t["wide_over_narrow"] = t["wide"]["ms"] / t["narrow"]["ms"]
    res["timings"] = t
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viterbi_bench.json"))
    ap.add_argument("--shapes", default="1024x25x65,64x25x3001,12288x2x65,1024x2x3001,1x600x3001,1x1024x300")
    ap.add_argument("--crossing", default="12288x65,64x65,64x3001", help="B x T of the sweep over the narrow form's S")
    a = ap.parse_args()
    ops.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "constants": ops.viterbi_constants(), "shapes": [], "crossing": []}
    for s in a.shapes.split(","):
        B, S, T = (int(v) for v in s.split("x"))
        out["shapes"].append(bench_shape(B, S, T, a.reps))
        torch.cuda.empty_cache()
    for s in a.crossing.split(","):
        B, T = (int(v) for v in s.split("x"))
        for S in range(1, out["constants"]["s_narrow"] + 2):
            out["crossing"].append(bench_shape(B, S, T, a.reps, yardstick=False))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
