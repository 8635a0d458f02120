"""Time device SpecAugment with HIP events (buffers allocated once, every shape warmed, each sample a window of --inner
calls, median of --reps), as the other bench tools do.  Shapes: 1024 x [13, 65], 1024 x [80, 65], 1024 x [80, 3001] and
1 x [80, 2^20].  At each shape:

  masks_copy     two frequency and two time masks into another tensor
  masks_inplace  the same onto the input (only masked cells are written)
  warp_masks     time_warp = 5 ahead of the masks
  mean           the masks written with the clip's mean (the library's rule; both forms beside it where a clip allows)

each beside the torch formulation a user would write, timed in the same run: arange comparisons broadcast over per-clip
parameters plus torch.where (masked_fill_ in place, a mean over the clip for "mean"), F.interpolate per clip and segment for
the warp (the draws themselves are taken beforehand and not timed); and beside the byte floor of 8 bytes an element at
8 TB/s.  `forms`: both forms of "mean" over clip sizes around the rule's switch.

Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _specaug as SA  # noqa: E402
from sygnals_amd import ops  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
SEED = 20190418
WARP = 5


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


class TorchFormulation:
    """What a user would write with torch on the device, given the per-clip parameters as tensors."""

    def __init__(self, B, K, T, p):
        dev = "cuda"
        self.k = torch.arange(K, device=dev).view(1, K, 1, 1)
        self.t = torch.arange(T, device=dev).view(1, 1, T, 1)
        self.f0, self.f1 = (torch.from_numpy(a).to(dev).view(B, 1, 1, -1) for a in (p["f0"], p["f0"] + p["f"]))
        self.t0, self.t1 = (torch.from_numpy(a).to(dev).view(B, 1, 1, -1) for a in (p["t0"], p["t0"] + p["t"]))
        self.c, self.w = p["c"].tolist(), p["w"].tolist()
        self.T = T

    def mask(self):
        fm = ((self.k >= self.f0) & (self.k < self.f1)).any(dim=-1)          # [B, K, 1]
        tm = ((self.t >= self.t0) & (self.t < self.t1)).any(dim=-1)          # [B, 1, T]
        return fm | tm

    def masks_copy(self, x, value, out):
        return torch.where(self.mask(), value, x, out=out)

    def masks_inplace(self, x, value):
        return x.masked_fill_(self.mask(), value)

    def mean(self, x, out):
        return torch.where(self.mask(), x.mean(dim=(1, 2), keepdim=True), x, out=out)

    def warp(self, x, out):
        T = self.T
        for b, (c, w) in enumerate(zip(self.c, self.w)):
            if c < 0:
                out[b] = x[b]
                continue
            out[b, :, :w] = F.interpolate(x[b:b + 1, :, :c], size=w, mode="linear", align_corners=False)[0]
            out[b, :, w:] = F.interpolate(x[b:b + 1, :, c:], size=T - w, mode="linear", align_corners=False)[0]
        return out

    def warp_masks(self, x, value, tmp, out):
        return torch.where(self.mask(), value, self.warp(x, tmp), out=out)


def shape_case(B, K, T, reps, inner):
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((B, K, T), dtype=torch.float32, device="cuda", generator=g)
    out, tmp, tout = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    y = x.clone()                                                            # the tensor the in-place forms write onto
    kw = dict(freq_masks=2, freq_width=min(27, K), time_masks=2, time_width=100)
    tf = TorchFormulation(B, K, T, SA.params(SEED, 0, B, K, T, time_warp=WARP, **kw))
    value = torch.zeros((), dtype=torch.float32, device="cuda")
    floor = 8.0 * B * K * T / HBM_BPS * 1e3
    k = ops.spec_augment_constants()
    res = dict(B=B, K=K, T=T, hbm_floor_ms=floor, mean_rule="resident" if K * T <= k["resident_max"] else "tiled")
    slow = max(1, reps // 3), max(1, inner // 5)                             # the per-clip interpolate loop takes B launches a call
    calls = {
        "masks_copy": (lambda: ops.spec_augment(x, SEED, out=out, **kw), lambda: tf.masks_copy(x, value, tout), (reps, inner)),
        "masks_inplace": (lambda: ops.spec_augment(y, SEED, out=y, **kw), lambda: tf.masks_inplace(y, 0.0), (reps, inner)),
        "warp_masks": (lambda: ops.spec_augment(x, SEED, time_warp=WARP, out=out, **kw), lambda: tf.warp_masks(x, value, tmp, tout),
                       slow if B > 1 else (reps, inner)),
        "mean": (lambda: ops.spec_augment(x, SEED, mask_value="mean", out=out, **kw), lambda: tf.mean(x, tout), (reps, inner)),
    }
    for name, (ours, theirs, (r_t, i_t)) in calls.items():
        a, b = [], []
        for _ in range(2):                                                   # alternating in one process
            a.append(timed(ours, reps, inner))
            b.append(timed(theirs, r_t, i_t, warm=1))
        best, tbest = min(a, key=lambda m: m["ms"]), min(b, key=lambda m: m["ms"])
        res[name] = dict(best, hbm_fraction=floor / best["ms"], torch_ms=tbest["ms"], over_torch_time=best["ms"] / tbest["ms"],
                         ms_runs=[m["ms"] for m in a], torch_ms_runs=[m["ms"] for m in b])
    for form in ("resident", "tiled"):
        if form == "resident" and K * T > (1 << 22):
            continue                                                         # one workgroup would walk the whole clip
        res["mean"][f"{form}_ms"] = timed(lambda: ops.spec_augment(x, SEED, mask_value="mean", out=out, form=form, **kw), reps, inner)["ms"]
    res["inplace_over_copy"] = res["masks_inplace"]["ms"] / res["masks_copy"]["ms"]
    # the two formulations agree on the masks, and on the warp within float32 rounding
    ours = ops.spec_augment(x, SEED, time_warp=WARP, **kw)
    theirs = tf.warp_masks(x, value, tmp, tout)
    res["max_abs_difference_from_torch"] = float((ours - theirs).abs().max())
    return res


def forms_case(reps, inner):
    """Both forms of "mean" for 1024 clips of 13 rows around the rule's switch."""
    res = dict(constants=ops.spec_augment_constants())
    B, K = 1024, 13
    for T in (65, 158, 315, 630, 1260, 2520, 5040):
        x = torch.randn((B, K, T), dtype=torch.float32, device="cuda")
        out = torch.empty_like(x)
        row = dict(cells=K * T)
        for form in ("resident", "tiled"):
            row[f"{form}_ms"] = timed(lambda: ops.spec_augment(x, SEED, freq_width=13, mask_value="mean", out=out, form=form), reps, inner)["ms"]
        res[f"T{T}"] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--shapes", default="1024x13x65,1024x80x65,1024x80x3001,1x80x1048576", help="BxKxT,...")
    ap.add_argument("--no-forms", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specaug_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {}
    for B, K, T in (tuple(int(v) for v in tok.split("x")) for tok in a.shapes.split(",")):
        res[f"{B}x{K}x{T}"] = shape_case(B, K, T, a.reps, a.inner)
    if not a.no_forms:
        res["forms"] = forms_case(a.reps, a.inner)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
