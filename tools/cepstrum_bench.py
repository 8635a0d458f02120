"""Time the device cepstral analysis (ops.cepstrogram, real_cepstrum, complex_cepstrum, cepstrum_peaks) with HIP events:
every shape warmed, each sample a window of --inner calls, median of --reps windows.

Shapes: 1024 clips x 32768 samples, n_fft 2048, hop 512, at Q = 1025 and Q = 64, as the fused form, the chain form
(stft_any -> log|X| -> inverse transform -> gather) and a torch baseline (frames -> torch.fft.rfft -> log(clamp(abs)) ->
torch.fft.irfft), all three in the same run; one row of 2^24 samples (real_cepstrum, which has only the chain form, and
the torch baseline).  Each time stands beside its byte floor, 4 B (L + Q T) bytes at 8 TB/s.  Also: the whole-row
complex cepstrum at 1024 x 32768 and the peak picker alone on the Q = 1025 cepstrogram.

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
AMIN = 1e-5


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


def measure(fn, reps, inner, floor_bytes, **info):
    one = timed(fn, 1, 1, warm=1)["ms"]
    n_in = int(min(inner, max(1, 50.0 // one)))                      # windows of about 50 ms
    t = timed(fn, reps, n_in, warm=1)
    floor = floor_bytes / HBM_BPS * 1e3
    return dict(t, inner=n_in, byte_floor_ms=floor, floor_fraction=floor / t["ms"], **info)


def torch_cepstrogram(y, Q, win, n_fft=2048, hop=512):
    yp = torch.nn.functional.pad(y, (n_fft // 2, n_fft // 2))
    fr = yp.unfold(1, n_fft, hop) * win                              # [B, T, n_fft]
    c = torch.fft.irfft(torch.log(torch.clamp(torch.abs(torch.fft.rfft(fr)), min=AMIN)), n=n_fft)
    return c[:, :, :Q].transpose(1, 2).contiguous()


def torch_real_cepstrum(x):
    n = x.shape[1]
    return torch.fft.irfft(torch.log(torch.clamp(torch.abs(torch.fft.rfft(x)), min=AMIN)), n=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cepstrum_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"constants": ops.cepstrum_constants()}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")

    B, L, hop = 1024, 32768, 512
    T = 1 + L // hop
    y = rows(B, L)
    win = ops.window_dev("hann", 2048, 2048)
    for Q in (1025, 64):
        floor = 4.0 * B * (L + Q * T)
        out = torch.empty((B, Q, T), dtype=torch.float32, device="cuda")
        info = dict(B=B, L=L, n_fft=2048, hop=hop, Q=Q, T=T)
        for form in ("fused", "chain"):
            res[f"cepstrogram_1024x32768_q{Q}_{form}"] = measure(lambda: ops.cepstrogram(y, n_ceps=Q, form=form, out=out), a.reps,
                                                                 a.inner, floor, form=form, **info)
        ours = ops.cepstrogram(y, n_ceps=Q)
        base = torch_cepstrogram(y, Q, win)
        t = measure(lambda: torch_cepstrogram(y, Q, win), max(3, a.reps // 2), a.inner, floor, form="torch", **info)
        t["max_diff_to_kernel"] = float((base - ours).abs().max())
        t["baseline_over_fused_time"] = t["ms"] / res[f"cepstrogram_1024x32768_q{Q}_fused"]["ms"]
        res[f"cepstrogram_1024x32768_q{Q}_torch"] = t
        res[f"cepstrogram_1024x32768_q{Q}_chain_over_fused_time"] = (res[f"cepstrogram_1024x32768_q{Q}_chain"]["ms"]
                                                                     / res[f"cepstrogram_1024x32768_q{Q}_fused"]["ms"])
        del base, ours
        write()
    # the picker alone, on the stored cepstrogram
    ceps = ops.cepstrogram(y, n_ceps=1025)
    res["peaks_1024x1025x65_q23_339"] = measure(lambda: ops.cepstrum_peaks(ceps, 23, 339, 22050.0), a.reps, a.inner,
                                                4.0 * B * T * (339 - 23 + 1), B=B, Q=1025, T=T, qmin=23, qmax=339)
    del ceps
    write()
    # whole rows
    res["complex_cepstrum_1024x32768"] = measure(lambda: ops.complex_cepstrum(y), max(3, a.reps // 2), a.inner, 4.0 * B * 2 * L,
                                                 B=B, n=L)
    res["real_cepstrum_1024x32768"] = measure(lambda: ops.real_cepstrum(y), max(3, a.reps // 2), a.inner, 4.0 * B * 2 * L, B=B, n=L)
    write()
    n = 1 << 24
    x = rows(1, n)
    ours = ops.real_cepstrum(x)
    base = torch_real_cepstrum(x)
    res["real_cepstrum_1x2p24_chain"] = measure(lambda: ops.real_cepstrum(x), max(3, a.reps // 2), a.inner, 4.0 * 2 * n, B=1, n=n)
    t = measure(lambda: torch_real_cepstrum(x), max(3, a.reps // 2), a.inner, 4.0 * 2 * n, B=1, n=n, form="torch")
    t["max_diff_to_kernel"] = float((base - ours).abs().max())
    t["baseline_over_chain_time"] = t["ms"] / res["real_cepstrum_1x2p24_chain"]["ms"]
    res["real_cepstrum_1x2p24_torch"] = t
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
