"""Time Griffin-Lim's iteration and the dense inversions with HIP events: every case warmed, each sample a window of calls
of about 50 ms, median of --reps windows; the cases of a group alternate window by window.

Shapes: 1024 clips of 32 768 samples (65 frames) and one clip of 2^24 samples (32 769 frames), 32 iterations.  Per shape:
  * the yardsticks: syg_stft2048_c2c_f32 and syg_istft2048_f32 alone, and the projection alone (with and without sums);
  * one iteration on preallocated buffers (syg_gl_project_f32, syg_istft2048_f32, syg_stft2048_c2c_f32);
  * ops.griffinlim at 32 iterations: the whole batch at once against chunks sized by the Infinity Cache's residency rule
    (chunk_rule() below) and, for a second point, chunks of 256;
  * mel_to_stft (128 bands) and mfcc_to_mel (13 coefficients) beside the loop.
The byte floor of an iteration is spelled out in `floor_bytes`: per bin the projection reads R, P and S (8 + 8 + 4 B) and
writes D (8 B), the inverse reads D (8 B) and the forward STFT writes R (8 B); per sample the clip is written and read once
(4 + 4 B); at 8 TB/s.  There is no parent-commit time: the capability is new.
(profiles/griffinlim_fused_ab.json is an earlier form of this tool run on the library while it still had the inverse STFT's
projecting load, which was never committed: "iteration, projecting load" against "iteration, two launches".)
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
N_ITER = 32


def chunk_rule(B, Tn, L):
    """Clips per chunk under the Infinity Cache's residency rule: a line stays on die while the table plus every byte moved
    between two uses of it fits in about 256 MiB.  Per clip the table is three spectra, S and y; an iteration moves about
    as many bytes again between two uses of a line.  So: the clips whose table fits in half of 256 MiB."""
    table = Tn * 1025 * (8 + 8 + 8 + 4) + 4 * L
    return int(max(1, min(B, (128 << 20) // table)))


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


def bench_shape(B, L, reps):
    Tn = 1 + L // 512
    bins = B * Tn * 1025
    g = torch.Generator(device="cuda").manual_seed(5)
    y = torch.randn((B, L), device="cuda", generator=g) * 0.1
    D0 = ops.stft2048_c2c(y)
    S = ops.cabs_pow(D0, 1)
    del D0
    Ra, Rb, D = (torch.empty((B, Tn, 1025, 2), device="cuda") for _ in range(3))
    ops.randn(B, Tn * 1025 * 2, 1, out=Ra.view(B, -1))
    ops.randn(B, Tn * 1025 * 2, 2, out=Rb.view(B, -1))
    alpha = ops.gl_alpha(0.99)
    win64, win32, tw = ops.window64_dev(), ops.window_dev("hann", 2048, 2048), ops.twiddle_dev(2048)
    sums = torch.empty((B, 2), dtype=torch.float64, device="cuda")
    work = ops._workspace("syg_gl_project_work_bytes", B, Tn, dtype=torch.float64, device=y.device)
    p = ops._ptr

    def forward(dst):
        ops._call("syg_stft2048_c2c_f32", p(y), B, L, L, 512, 1, Tn, p(win32), p(tw), p(dst))

    def inverse(src):
        ops._call("syg_istft2048_f32", p(src), B, Tn, 512, 1, L, p(win64), p(tw), None, p(y), None, None, L)

    def project():
        ops._call("syg_gl_project_f32", p(Ra), p(Rb), p(S), B, Tn, alpha, p(D), None, None)

    def project_sums():
        ops._call("syg_gl_project_f32", p(Ra), p(Rb), p(S), B, Tn, alpha, p(D), p(sums), p(work))

    def iteration():
        project()
        inverse(D)
        forward(Rb)

    res = {"B": B, "L": L, "T": Tn, "n_iter": N_ITER}
    floor = bins * (8 + 8 + 4 + 8 + 8 + 8) + B * L * (4 + 4)
    res["floor_bytes"] = {"per_bin": 44, "per_bin_projection": 28, "per_sample": 8, "iteration": floor, "projection": bins * 28}
    t = alternate({"stft2048_c2c": lambda: forward(Rb), "istft2048": lambda: inverse(Ra), "gl_project": project,
                   "gl_project with sums": project_sums, "iteration": iteration}, reps)
    for k, by in (("iteration", floor), ("gl_project", bins * 28), ("gl_project with sums", bins * 28)):
        t[k]["floor_ms"] = by / HBM_BPS * 1e3
        t[k]["of_floor"] = t[k]["floor_ms"] / t[k]["ms"]
    res["yardstick_ms"] = t["stft2048_c2c"]["ms"] + t["istft2048"]["ms"]
    res["yardstick_plus_projection_floor_ms"] = res["yardstick_ms"] + t["gl_project"]["floor_ms"]
    res["iteration_over_yardstick_plus_floor"] = t["iteration"]["ms"] / res["yardstick_plus_projection_floor_ms"]
    del Ra, Rb, D
    chunk = chunk_rule(B, Tn, L)
    runs = {"griffinlim, whole batch": lambda: ops.griffinlim(S, N_ITER),
            "griffinlim with trace, whole batch": lambda: ops.griffinlim(S, N_ITER, return_trace=True)}
    if chunk < B:
        runs[f"griffinlim, chunks of {chunk} (residency rule)"] = lambda: ops.griffinlim(S, N_ITER, chunk=chunk)
    if 256 < B and chunk != 256:
        runs["griffinlim, chunks of 256"] = lambda: ops.griffinlim(S, N_ITER, chunk=256)
    g = alternate(runs, max(3, reps // 2))
    for v in g.values():
        v["ms_per_iteration"] = v["ms"] / N_ITER
    t.update(g)
    res["chunk_rule"] = chunk
    mel = torch.rand((B, 128, Tn), device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    mfcc = torch.randn((B, 13, Tn), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    t.update(alternate({"mel_to_stft (128 bands)": lambda: ops.mel_to_stft(mel), "mfcc_to_mel (13 -> 128)": lambda: ops.mfcc_to_mel(mfcc)},
                       reps))
    res["mel_to_stft_over_loop"] = t["mel_to_stft (128 bands)"]["ms"] / t["griffinlim, whole batch"]["ms"]
    res["cases"] = t
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "griffinlim_bench.json"))
    ap.add_argument("--shapes", default="1024x32768,1x16777216")
    a = ap.parse_args()
    ops.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BPS, "shapes": []}
    for s in a.shapes.split(","):
        B, L = (int(v) for v in s.split("x"))
        out["shapes"].append(bench_shape(B, L, a.reps))
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
