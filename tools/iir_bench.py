"""Time the causal SOS filter (ops.sosfilt) with HIP events: every shape warmed, each sample a window of --inner calls,
median of --reps windows.

Shapes and designs: 1024 rows x 32768 samples at 4 sections (Butterworth band-pass 300 - 3400 Hz, order 4, 48 kHz), at 8
sections (elliptic band-pass, order 8) and at 10 sections (the graphic EQ: 10 peaking bands 31.25 * 2^i Hz, -+6 dB, Q
1.414: two groups); one row of 2^24 samples at 4 sections.  Each time stands beside its byte floor, 8 bytes a sample at
8 TB/s, and beside the zero-phase filter's chunked form (ops.sosfiltfilt under ops.override(sos_clip=0)) on the same
shape and sections in the same run: one sweep is a subset of that form's two, so the causal call is expected to take no
longer.  (The zero-phase form takes at most 8 sections: the 10-section row has no such partner.)  No torch baseline:
torch has no IIR filter.

Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _tables as T, ops  # noqa: E402
from sygnals_amd.core import filters as F  # noqa: E402
from sygnals_amd.core.audio.effects.equalizer import graphic_eq_sos  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
FS = 48000.0


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


def measure(fn, reps, inner, samples, **info):
    one = timed(fn, 1, 1, warm=1)["ms"]
    n_in = int(min(inner, max(1, 50.0 // one)))                      # windows of about 50 ms
    t = timed(fn, reps, n_in, warm=1)
    floor = 8.0 * samples / HBM_BPS * 1e3
    return dict(t, inner=n_in, byte_floor_ms=floor, floor_fraction=floor / t["ms"], msamples_per_s=samples / t["ms"] * 1e-3, **info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iir_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"constants": ops.sosfilt_constants()}
    designs = {
        "butter4_bp": F.design_iir_sos((300.0, 3400.0), FS, 4, "bandpass"),
        "ellip8_bp": F.design_iir_sos((300.0, 3400.0), FS, 8, "bandpass", family="ellip", rp=0.5, rs=60.0),
        "graphic_eq10": graphic_eq_sos(FS, [(31.25 * 2 ** i, -6.0 if i % 2 == 0 else 6.0) for i in range(10)], 1.414),
    }
    g = torch.Generator(device="cuda").manual_seed(7)
    for key, name, B, L in (("rows_1024x32768_s4", "butter4_bp", 1024, 32768), ("rows_1024x32768_s8", "ellip8_bp", 1024, 32768),
                            ("rows_1024x32768_s10", "graphic_eq10", 1024, 32768), ("row_1x2p24_s4", "butter4_bp", 1, 1 << 24)):
        sos = designs[name]
        S = sos.shape[0]
        x = torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
        y = torch.empty_like(x)
        zf_ref = signal.sosfilt(sos, x[0, :4096].cpu().numpy().astype(np.float64))
        got = ops.sosfilt(x[:1, :4096], sos)[0].cpu().numpy()
        err = float(np.max(np.abs(got - zf_ref)) / np.max(np.abs(zf_ref)))
        info = dict(B=B, L=L, sections=S, design=name, work_bytes=int(ops.lib().syg_sosfilt_work_bytes(B, L, S)), check_vs_scipy=err)
        res[key] = measure(lambda: ops.sosfilt(x, sos, out=y), a.reps, a.inner, B * L, **info)
        res[key + "_with_state"] = measure(lambda: ops.sosfilt(x, sos, return_state=True, out=y), a.reps, a.inner, B * L, **info)
        if S <= 8:
            zi, pad = F.sosfilt_zi(sos), T.butter_padlen(sos)
            with ops.override(sos_clip=0):
                zp = measure(lambda: ops.sosfiltfilt(x, sos, zi, pad), a.reps, a.inner, B * L, B=B, L=L, sections=S, design=name,
                             form="sosfiltfilt, chunked (sos_clip=0)", padlen=int(pad))
            zp["causal_over_zero_phase_time"] = res[key]["ms"] / zp["ms"]
            res[key + "_sosfiltfilt_chunked"] = zp
        del x, y
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
