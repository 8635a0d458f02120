"""Time the device noise generation with HIP events (buffers allocated once, every shape warmed, each sample a window of
--inner calls, median of --reps), as tools/augment_bench.py does.  Shapes: 1024 x 32768, 2048 x 16384, 1024 x 65536 and
one row of 2^24.

  randn          ops.randn into a buffer, against its floor of 4 bytes a sample; its time per Philox call (four samples:
                 ten rounds, two logarithms, two square roots, two sincospi) is the price of regenerating, beside the
                 price of materialising a call (32 bytes more traffic at the bandwidth the stored mix reaches).
  mix            ops.fx_add_noise_gen (noise in registers; floor 8 bytes a sample resident, 12 bytes past the resident length)
                 beside ops.randn + ops.fx_add_noise in the same run, alternating.  `rule` is what
                 core.augment.add_noise_device_batch calls at that shape.
  parent         what the parent commit does for the same result: np.random.default_rng(seed).standard_normal on the
                 host, upload, ops.fx_add_noise -- by wall clock, most of it is host time.
  pink           ops.colored_noise at 1024 x 32768, and its two transforms alone on a buffer of the same shape.

Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import ops  # noqa: E402
from sygnals_amd.core.augment import noise as N  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
SEED = 1234


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


def against_floor(t, nbytes, samples):
    floor_ms = nbytes / HBM_BPS * 1e3
    return dict(t, hbm_floor_ms=floor_ms, hbm_fraction=floor_ms / t["ms"], msamples_per_s=samples / t["ms"] * 1e-3)


def shape_case(B, L, reps, inner, parent_reps):
    g = torch.Generator(device="cuda").manual_seed(7)
    y = 0.1 * torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    noise, out = torch.empty_like(y), torch.empty_like(y)
    snr = torch.full((B,), 10.0, dtype=torch.float64, device="cuda")
    resident = L <= ops.fx_add_noise_resident_max()
    res = dict(B=B, L=L, gen_form="resident" if resident else "power, scale, mix", gen_bytes_per_sample=8 if resident else 12,
               stored_mix_launches=1 if L <= ops.fx_add_noise_resident_max() else 2)
    gen = lambda: ops.fx_add_noise_gen(y, snr, SEED, out=out)
    draw = lambda: ops.randn(B, L, SEED, out=noise)
    mix = lambda: ops.fx_add_noise(y, noise, snr, out=out)

    def stored():
        draw()
        mix()

    t = {"randn": [], "gen": [], "stored": [], "mix": []}
    for _ in range(2):                                  # alternating in one process
        for name, fn in (("randn", draw), ("gen", gen), ("stored", stored), ("mix", mix)):
            t[name].append(timed(fn, reps, inner))
    best = {k: min(v, key=lambda m: m["ms"]) for k, v in t.items()}
    calls = B * ((L + 3) // 4)
    res["randn"] = against_floor(best["randn"], 4 * B * L, B * L)
    res["randn"]["ns_per_philox_call_device_wide"] = best["randn"]["ms"] * 1e6 / calls
    res["mix_generated"] = against_floor(best["gen"], res["gen_bytes_per_sample"] * B * L, B * L)
    stored_bytes = (4 + (12 if res["stored_mix_launches"] == 1 else 20)) * B * L
    res["mix_stored_randn_plus_fx_add_noise"] = against_floor(best["stored"], stored_bytes, B * L)
    res["fx_add_noise_alone"] = against_floor(best["mix"], stored_bytes - 4 * B * L, B * L)
    for k in t:
        res.setdefault("ms_runs", {})[k] = [m["ms"] for m in t[k]]
    res["generated_over_stored_time"] = best["gen"]["ms"] / best["stored"]["ms"]
    # what regenerating a call costs beside what keeping it costs (written once, read back once or twice)
    bw = (stored_bytes - 4 * B * L) * 1e-6 / best["mix"]["ms"]                       # GB/s the stored mix reaches
    res["materialise_ns_per_call_at_stored_mix_bandwidth"] = 32.0 / bw
    res["rule"] = "generated" if N.GEN_MIX_MAX_L is None or L <= N.GEN_MIX_MAX_L else "stored"
    # the parent's path, by wall clock
    ws = []
    for _ in range(parent_reps if parent_reps > 0 else 0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = np.random.default_rng(SEED).standard_normal((B, L))
        t1 = time.perf_counter()
        dev = ops.to_device_f32(host, y.device)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ops.fx_add_noise(y, dev, snr, out=out)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        ws.append(dict(total_ms=(t3 - t0) * 1e3, host_draw_ms=(t1 - t0) * 1e3, convert_upload_ms=(t2 - t1) * 1e3, mix_ms=(t3 - t2) * 1e3))
        del host, dev
    if not ws:
        return res
    res["parent_host_draw_upload_mix_wall"] = min(ws, key=lambda m: m["total_ms"])
    res["parent_over_rule_time"] = res["parent_host_draw_upload_mix_wall"]["total_ms"] / min(best["gen"]["ms"], best["stored"]["ms"])
    return res


def pink_case(B, L, reps, inner):
    M = ops.colored_noise_fft_len(L)
    pairs = (B + 1) // 2
    Z = torch.zeros((pairs, M, 2), dtype=torch.float32, device="cuda")
    res = dict(B=B, L=L, M=M, pairs=pairs)
    res["colored_noise"] = timed(lambda: ops.colored_noise(B, L, SEED, 1.0), reps, inner)
    res["two_transforms_alone"] = timed(lambda: ops.fft_pow2_any(ops.fft_pow2_any(Z), inverse=True), reps, inner)
    res["transforms_share_of_time"] = res["two_transforms_alone"]["ms"] / res["colored_noise"]["ms"]
    y = 0.1 * torch.randn((B, L), dtype=torch.float32, device="cuda")
    res["add_noise_device_batch_pink"] = timed(lambda: N.add_noise_device_batch(y, 10.0, "pink", seed=SEED), reps, inner)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--parent-reps", type=int, default=2)
    ap.add_argument("--shapes", default="1024x32768,2048x16384,1024x65536,1x16777216", help="BxL,... of the mix cases")
    ap.add_argument("--no-pink", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"gen_mix_max_l_rule": N.GEN_MIX_MAX_L, "constants": ops.rng_constants()}
    for B, L in (tuple(int(v) for v in tok.split("x")) for tok in a.shapes.split(",")):
        res[f"{B}x{L}"] = shape_case(B, L, a.reps, a.inner, a.parent_reps)
    if not a.no_pink:
        res["pink_1024x32768"] = pink_case(1024, 32768, a.reps, max(1, a.inner // 2))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
