"""Time the device polyphase resampler (syg_resample_poly_f32 through the C ABI, plan and buffers made once) with HIP
events: every shape warmed, each sample a window of --inner calls, median of --reps windows.

Shapes: 1024 clips x 32768 samples at 44100 -> 16000, 48000 -> 16000, 16000 -> 48000 and 44100 -> 48000, and one row of
2^24 samples at 44100 -> 16000, each with the table in LDS and in global memory where the library allows both.  Each time
stands beside its byte floor, 4 (L + n_out) bytes a row at 8 TB/s.

In the same run a torch baseline at the four batch shapes: the same table applied by ONE torch.nn.functional.conv1d with
`up` output channels and stride `down` (channel r holds the taps of the outputs n = r mod up, shifted to where their
window starts inside a common window of Kp + q(up - 1) - q(0) samples), then the channels interleaved.  Its result is
checked against the kernel's in the run.

A library built with the other ownership of outputs (EXTRA_HIPCC_FLAGS=-DSYG_RESAMPLE_SHARE=0, SYG_LIB_OUT elsewhere) is
timed by pointing SYGNALS_AMD_LIB at it and naming it with --tag; --no-baseline leaves torch out.

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
from sygnals_amd import _resample as RS  # noqa: E402
from sygnals_amd import ops  # noqa: E402
from sygnals_amd._lib import check, lib  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s


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


def case(B, L, orig_sr, target_sr, form, reps, inner):
    h = lib()
    up, down = RS.ratio_of_rates(orig_sr, target_sr)
    p, table = ops.resample_plan(up, down, L)
    x = rows(B, L)
    out = torch.empty((B, p.n_out), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q, f = ops._ptr, ops.RESAMPLE_FORMS[form]

    def run():
        check(h.syg_resample_poly_f32(q(x), B, L, L, p.up, p.down, p.n_pre_remove, p.Kp, q(table), 0, 0.0, f, p.n_out, q(out),
                                      p.n_out, st), "syg_resample_poly_f32")

    run()
    from scipy.signal import resample_poly
    n = min(L, 1 << 16)                                              # the head of the first row against scipy in float64
    ref = resample_poly(x[0, :n].cpu().numpy().astype(np.float64), up, down)
    m = ref.size - 2 * p.Kp                                          # clear of the cut's own edge
    err = float(np.max(np.abs(out[0, :m].cpu().numpy() - ref[:m])) / np.max(np.abs(ref)))
    one = timed(run, 1, 1, warm=1)["ms"]
    n_in = int(min(inner, max(1, 50.0 // one)))                      # windows of about 50 ms
    t = timed(run, reps, n_in, warm=1)
    floor = 4.0 * B * (L + p.n_out) / HBM_BPS * 1e3
    return dict(t, B=B, L=L, up=p.up, down=p.down, Kp=p.Kp, n_out=p.n_out, table_bytes=int(p.table.nbytes),
                table=form, rule_picks="lds" if ops.resample_table_in_lds(p.up, p.Kp) else "global",
                inner=n_in, byte_floor_ms=floor, floor_fraction=floor / t["ms"], worst_err_head=err,
                gsamples_in_per_s=B * L / t["ms"] * 1e-6)


def baseline(B, L, orig_sr, target_sr, reps):
    """One conv1d, `up` output channels, stride `down`; see the module docstring."""
    import torch.nn.functional as F
    up, down = RS.ratio_of_rates(orig_sr, target_sr)
    p, _ = ops.resample_plan(up, down, L)
    r = np.arange(up, dtype=np.int64)
    t = (r + p.n_pre_remove) * down
    ph, qq = t % up, t // up
    base, W = int(qq[0]) - (p.Kp - 1), int(qq[-1] - qq[0]) + p.Kp
    w = np.zeros((up, 1, W), dtype=np.float32)
    j = np.arange(p.Kp)
    for c in range(up):
        w[c, 0, qq[c] - j - base] = p.table[ph[c], j]
    wd = torch.from_numpy(w).cuda()
    K = -(-p.n_out // up)
    need = (K - 1) * down + W                                        # samples from `base` on
    x = rows(B, L)

    def run():
        xp = F.pad(x, (-base, need - (L - base)))[:, None, :]
        y = F.conv1d(xp, wd, stride=down)                            # [B, up, K]
        return y.transpose(1, 2).reshape(B, K * up)[:, :p.n_out]

    ours = ops.resample_poly(x, up, down)
    got = run()
    diff = float((got - ours).abs().max() / ours.abs().max())
    res = dict(timed(run, reps, 1, warm=1), B=B, L=L, up=up, down=down, window_taps=W,
               what="one torch conv1d, `up` output channels, stride `down`, then the channels interleaved",
               max_diff_to_kernel_over_peak=diff)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--tag", default="product")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"tag": a.tag, "constants": ops.resample_constants()}
    B, L = 1024, 32768
    pairs = ((44100, 16000), (48000, 16000), (16000, 48000), (44100, 48000))
    for o, t in pairs:
        for form in ("lds", "global"):
            res[f"batch_1024x32768_{o}_{t}_{form}"] = case(B, L, o, t, form, a.reps, a.inner)
    for form in ("lds", "global"):
        res[f"one_row_2p24_44100_16000_{form}"] = case(1, 1 << 24, 44100, 16000, form, a.reps, a.inner)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")

    write()                                                          # the kernel's own figures are kept whatever torch does
    if not a.no_baseline:
        for o, t in pairs:
            b = baseline(B, L, o, t, a.reps)
            ours = res[f"batch_1024x32768_{o}_{t}_lds"]
            ours = res[f"batch_1024x32768_{o}_{t}_{ours['rule_picks']}"]                 # what a caller gets
            b["baseline_over_kernel_time"] = b["ms"] / ours["ms"]
            res[f"baseline_torch_1024x32768_{o}_{t}"] = b
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
