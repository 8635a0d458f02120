"""Time the feature dynamics with HIP events (buffers allocated once, every shape warmed, each sample a window of --inner
calls, median of --reps), as the other bench tools do.  Shapes: 1024 x [13, 65], 1024 x [40, 65], 1024 x [13, 3001] and
1 x [13, 2^20].

  feature_post   global CMVN + delta + delta-delta in one call, against its byte floor 4 B K T (1 + blocks) at 8 TB/s
  delta          ops.delta alone (order 1)
  cmvn_sliding   ops.cmvn at a window of 600 frames
each beside the torch formulation a user of the parent commit would write, timed in the same run: conv1d over the rows
plus two edge matmuls, mean / var, a float64 cumsum for the sliding form; and that formulation's distance from float64
beside the library's (both on the first clip, as fractions of the tests' gates).

  forms          both forms of feature_post, delta and the sliding cmvn on either side of the rule's switch: what the rule
                 rests on.

Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from scipy.signal import savgol_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import ops  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
WIDTH = 9
WINDOW = 600


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


def floor_ms(B, K, T, blocks):
    return 4.0 * B * K * T * (1 + blocks) / HBM_BPS * 1e3


class TorchFormulation:
    """What a user of the parent commit would write with torch on the device."""

    def __init__(self, T):
        self.tabs = {}
        for order in (1, 2):
            c, E = ops.delta_tables(WIDTH, order)
            self.tabs[order] = (torch.from_numpy(c[::-1].copy()).cuda().view(1, 1, -1), torch.from_numpy(E.copy()).cuda())
        W = WINDOW
        t = np.arange(T)
        s = t - W // 2
        e = s + W
        e = np.where(s < 0, e - s, e)
        s = np.maximum(s, 0)
        s = np.where(e > T, s - (e - T), s)
        e = np.minimum(e, T)
        s = np.maximum(s, 0)
        self.s, self.e = torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda()
        self.n = (self.e - self.s).double()

    def delta(self, x, order, out):
        B, K, T = x.shape
        h = WIDTH // 2
        w, E = self.tabs[order]
        out[:, :, h:T - h] = F.conv1d(x.reshape(B * K, 1, T), w).view(B, K, T - 2 * h)
        out[:, :, :h] = x[:, :, :WIDTH] @ E[:, :h]
        out[:, :, T - h:] = x[:, :, T - WIDTH:] @ E[:, WIDTH - h:]
        return out

    def cmvn_global(self, x):
        m = x.mean(dim=-1, keepdim=True)
        v = x.var(dim=-1, unbiased=False, keepdim=True)
        return (x - m) / torch.sqrt(torch.clamp(v, min=1e-20))

    def feature_post(self, x, out):
        K = x.shape[1]
        s = self.cmvn_global(x)
        out[:, :K] = s
        self.delta(s, 1, out[:, K:2 * K])
        self.delta(s, 2, out[:, 2 * K:])
        return out

    def cmvn_sliding(self, x):
        xd = x.double()
        S = F.pad(torch.cumsum(xd, dim=-1), (1, 0))
        Q = F.pad(torch.cumsum(xd * xd, dim=-1), (1, 0))
        m = (S[..., self.e] - S[..., self.s]) / self.n
        v = (Q[..., self.e] - Q[..., self.s]) / self.n - m * m
        return ((xd - m) / torch.sqrt(torch.clamp(v, min=1e-20))).float()


def gate_fraction_delta(got, x64, order):
    want = savgol_filter(x64, WIDTH, deriv=order, polyorder=order, axis=-1)
    c, _ = ops.delta_tables(WIDTH, order)
    bound = 1e-5 * float(np.sum(np.abs(c.astype(np.float64)))) * np.max(np.abs(x64), axis=-1, keepdims=True)
    return float(np.max(np.abs(got.astype(np.float64) - want) / bound))


def gate_fraction_cmvn(got, want):
    bound = 1e-5 * np.maximum(1.0, np.max(np.abs(want), axis=-1, keepdims=True))
    return float(np.max(np.abs(got.astype(np.float64) - want) / bound))


def cmvn_global64(x64):
    m = x64.mean(axis=-1, keepdims=True)
    v = ((x64 - m) ** 2).mean(axis=-1, keepdims=True)
    return (x64 - m) / np.sqrt(np.maximum(v, 1e-20))


def cmvn_sliding64(x64, tf):
    s, e = tf.s.cpu().numpy(), tf.e.cpu().numpy()
    n = (e - s).astype(np.float64)
    S = np.concatenate([np.zeros(x64.shape[:-1] + (1,)), np.cumsum(x64, axis=-1)], axis=-1)
    Q = np.concatenate([np.zeros(x64.shape[:-1] + (1,)), np.cumsum(x64 * x64, axis=-1)], axis=-1)
    m = (S[..., e] - S[..., s]) / n
    return (x64 - m) / np.sqrt(np.maximum((Q[..., e] - Q[..., s]) / n - m * m, 1e-20))


def make_input(B, K, T):
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((B, K, T), dtype=torch.float32, device="cuda", generator=g)
    x[:, 0] = -400.0 + 50.0 * x[:, 0]                       # c0-like
    return x


def shape_case(B, K, T, reps, inner):
    x = make_input(B, K, T)
    tf = TorchFormulation(T)
    out3, out1 = torch.empty((B, 3 * K, T), dtype=torch.float32, device="cuda"), torch.empty_like(x)
    t3, t1 = torch.empty_like(out3), torch.empty_like(x)
    res = dict(B=B, K=K, T=T, form=ops.dynamics_form(T), form_sliding=ops.dynamics_form(T, WINDOW))
    calls = {
        "feature_post": (lambda: ops.feature_post(x, cmvn="global", deltas=2, width=WIDTH, out=out3), lambda: tf.feature_post(x, t3), 3),
        "delta": (lambda: ops.delta(x, WIDTH, 1, out=out1), lambda: tf.delta(x, 1, t1), 1),
    }
    if T > 1:
        calls["cmvn_sliding"] = (lambda: ops.cmvn(x, WINDOW, out=out1), lambda: tf.cmvn_sliding(x), 1)
    for name, (ours, theirs, blocks) in calls.items():
        a, b = [], []
        for _ in range(2):                                  # alternating in one process
            a.append(timed(ours, reps, inner))
            b.append(timed(theirs, reps, inner))
        best, tbest = min(a, key=lambda m: m["ms"]), min(b, key=lambda m: m["ms"])
        fl = floor_ms(B, K, T, blocks)
        res[name] = dict(best, hbm_floor_ms=fl, hbm_fraction=fl / best["ms"], torch_ms=tbest["ms"], over_torch_time=best["ms"] / tbest["ms"],
                         ms_runs=[m["ms"] for m in a], torch_ms_runs=[m["ms"] for m in b])
    # distances from float64 on the first clip, as fractions of the gates
    x64 = x[0].cpu().numpy().astype(np.float64)
    s64 = cmvn_global64(x64)
    ours = ops.feature_post(x[:1], cmvn="global", deltas=2, width=WIDTH)[0].cpu().numpy()
    theirs = tf.feature_post(x[:1], torch.empty((1, 3 * K, T), dtype=torch.float32, device="cuda"))[0].cpu().numpy()
    acc = {}
    for who, y in (("library", ours), ("torch", theirs)):
        acc[who] = dict(cmvn_global=gate_fraction_cmvn(y[:K], s64),
                        delta_of_own_statics=max(gate_fraction_delta(y[d * K:(d + 1) * K], y[:K].astype(np.float64), d) for d in (1, 2)))
    if T > 1:
        w64 = cmvn_sliding64(x64, tf)
        acc["library"]["cmvn_sliding"] = gate_fraction_cmvn(ops.cmvn(x[:1], WINDOW)[0].cpu().numpy(), w64)
        acc["torch"]["cmvn_sliding"] = gate_fraction_cmvn(tf.cmvn_sliding(x[:1])[0].cpu().numpy(), w64)
    res["fraction_of_gate_vs_float64"] = acc
    return res


def forms_case(reps, inner):
    """Both forms around the rule's switches (and further out): 64 x 13 rows so that either form fills the chip."""
    k = ops.dynamics_constants()
    res = dict(constants=k)
    B, K = 64, 13
    for T in (65, 1024, 2048, k["resident_max_t"], k["resident_max_t"] + 1, 4096, 8192, 16384):
        x = make_input(B, K, T)
        out3, out1 = torch.empty((B, 3 * K, T), dtype=torch.float32, device="cuda"), torch.empty_like(x)
        row = dict(rule=ops.dynamics_form(T))
        for form in ("resident", "tiled"):
            row[f"feature_post_{form}_ms"] = timed(lambda: ops.feature_post(x, cmvn="global", deltas=2, out=out3, form=form), reps, inner)["ms"]
            row[f"delta_{form}_ms"] = timed(lambda: ops.delta(x, WIDTH, 1, out=out1, form=form), reps, inner)["ms"]
        res[f"T{T}"] = row
    B = 1024                                                # the headline batch: 13 312 rows
    for T in (65, 512, 1024, 1025, 2048, 3001):
        x = make_input(B, K, T)
        out3, out1 = torch.empty((B, 3 * K, T), dtype=torch.float32, device="cuda"), torch.empty_like(x)
        row = dict(rule=ops.dynamics_form(T))
        for form in ("resident", "tiled"):
            row[f"feature_post_{form}_ms"] = timed(lambda: ops.feature_post(x, cmvn="global", deltas=2, out=out3, form=form), reps, inner)["ms"]
            row[f"delta_{form}_ms"] = timed(lambda: ops.delta(x, WIDTH, 1, out=out1, form=form), reps, inner)["ms"]
        res[f"B1024_T{T}"] = row
        del x, out3, out1
    for T in (768, 1536, 2048, 3001):
        x = make_input(B, K, T)
        out1 = torch.empty_like(x)
        row = dict(rule=ops.dynamics_form(T, WINDOW))
        for form in ("resident", "tiled"):
            row[f"cmvn_sliding_{form}_ms"] = timed(lambda: ops.cmvn(x, WINDOW, out=out1, form=form), reps, inner)["ms"]
        res[f"B1024_sliding_T{T}"] = row
        del x, out1
    B = 64
    for T in (k["resident_max_t_sliding"], k["resident_max_t_sliding"] + 1, 1536, 3001):
        x = make_input(B, K, T)
        out1 = torch.empty_like(x)
        row = dict(rule=ops.dynamics_form(T, WINDOW))
        for form in ("resident", "tiled"):
            row[f"cmvn_sliding_{form}_ms"] = timed(lambda: ops.cmvn(x, WINDOW, out=out1, form=form), reps, inner)["ms"]
        res[f"sliding_T{T}"] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--shapes", default="1024x13x65,1024x40x65,1024x13x3001,1x13x1048576", help="BxKxT,...")
    ap.add_argument("--no-forms", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamics_bench.json"))
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
