"""Time the device tonal family (ops.chroma_fold in both layouts, ops.chroma_cens, ops.tuning_hist and the chains
core.features.tonal.chroma_stft_batch / chroma_cqt_batch / chroma_cens_batch / tonnetz_batch) with HIP events: every shape
warmed, each sample a window of calls of about 50 ms, median of --reps windows.

Shapes: 1024 clips x 32768 samples and one row of 2^24 samples, at 22 050 Hz, n_fft 2048, hop 512, 12 chroma rows, 252 CQT bins.
Per shape:
  each new kernel beside its byte floor (the input read once and the output written once at 8 TB/s);
  the chroma_stft and chroma_cqt chains (tuning given), each transform's share of its chain, and the chains with tuning=None;
  the existing ops' path to the same numbers, timed in the same run: stft2048_c2c -> cabs_pow -> mel_dense with the chroma
  table, then a host normalisation (timed on the host, copy included); ops.cqt, then a host fold and normalisation.
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
from sygnals_amd import _chroma as CH, ops  # noqa: E402
from sygnals_amd.core.features import tonal as TN  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s
SR, N_FFT, HOP, NC, BPO, NOCT = 22050, 2048, 512, 12, 36, 7


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


def measure(fn, reps, floor_bytes=None, **info):
    one = timed(fn, 1, 1, warm=1)["ms"]
    n_in = int(min(50, max(1, 50.0 // max(one, 1e-3))))
    r = dict(timed(fn, reps, n_in, warm=1), inner=n_in, **info)
    if floor_bytes is not None:
        r["floor_ms"] = floor_bytes / HBM_BPS * 1e3
        r["of_floor"] = r["floor_ms"] / r["ms"]
    return r


def host_timed(fn, reps):
    fn()
    ts = []
    for _ in range(max(3, reps // 2)):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return dict(ms=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)))


def signal(B, L):
    g = torch.Generator(device="cuda").manual_seed(5)
    t = torch.arange(L, device="cuda", dtype=torch.float32) / SR
    y = 0.01 * torch.randn((B, L), device="cuda", generator=g)
    for m in (57, 60, 64, 69, 72):
        y += 0.2 * torch.sin(2 * np.pi * 440.0 * 2.0 ** ((m - 69) / 12.0) * t)[None, :]
    return y


def bench_shape(B, L, reps):
    y = signal(B, L)
    res = {"B": B, "L": L}
    fb = ops._dev(CH.chroma_filterbank(SR, N_FFT, NC))
    X = ops.stft2048_c2c(y, HOP)
    T, F = int(X.shape[1]), int(X.shape[2])
    res["frames"] = T
    out12 = torch.empty((B, NC, T), device="cuda")
    res["fold_rows"] = measure(lambda: ops.chroma_fold(X, fb, "rows", 2, None, np.inf, out=out12), reps,
                               floor_bytes=B * T * (F * 8 + NC * 4))
    res["stft2048_c2c"] = measure(lambda: ops.stft2048_c2c(y, HOP), reps)
    res["chroma_stft"] = measure(lambda: TN.chroma_stft_batch(y, SR, tuning=0.0), reps)
    res["chroma_stft"]["stft_share"] = res["stft2048_c2c"]["ms"] / res["chroma_stft"]["ms"]
    res["chroma_stft"]["fold_share"] = res["fold_rows"]["ms"] / res["chroma_stft"]["ms"]
    # what the complex spectrogram's write and read is of the chain, at the byte floor: 2 x 8 F bytes a frame
    res["chroma_stft"]["spectrogram_round_trip_floor_ms"] = 2 * B * T * F * 8 / HBM_BPS * 1e3
    res["tuning_hist_power"] = measure(lambda: ops.tuning_hist(X, SR, N_FFT, 2), reps, floor_bytes=B * T * F * 8)
    res["chroma_stft_tuning_none"] = measure(lambda: TN.chroma_stft_batch(y, SR), max(3, reps // 2))

    def existing_stft():
        P = ops.cabs_pow(X, 2)
        return ops.mel_dense(P, fb)
    res["existing_cabs_pow_mel_dense"] = measure(existing_stft, reps)
    raw = existing_stft()

    def host_norm():
        a = raw.cpu().numpy()
        return a / np.maximum(np.abs(a).max(axis=1, keepdims=True), np.finfo(np.float32).tiny)
    res["existing_host_normalisation"] = host_timed(host_norm, reps)
    res["existing_stft_path_ms"] = (res["stft2048_c2c"]["ms"] + res["existing_cabs_pow_mel_dense"]["ms"]
                                    + res["existing_host_normalisation"]["ms"])
    res["chroma_stft"]["of_existing_path"] = res["chroma_stft"]["ms"] / res["existing_stft_path_ms"]
    del X, raw

    K = NOCT * BPO
    C = ops.cqt(y, SR, HOP, None, K, BPO, 0.0)
    Tc = int(C.shape[2])
    wt = CH.cq_to_chroma(K, BPO, NC)
    phi = CH.tonnetz_phi(NC)
    outc = torch.empty((B, NC, Tc), device="cuda")
    out6 = torch.empty((B, 6, Tc), device="cuda")
    res["fold_bins"] = measure(lambda: ops.chroma_fold(C, wt, "bins", 1, 0.0, np.inf, out=outc), reps,
                               floor_bytes=B * Tc * (K * 8 + NC * 4))
    res["fold_bins_tonnetz"] = measure(lambda: ops.chroma_fold(C, wt, "bins", 1, 0.0, np.inf, phi, out=out6), reps,
                                       floor_bytes=B * Tc * (K * 8 + 6 * 4))
    res["cqt"] = measure(lambda: ops.cqt(y, SR, HOP, None, K, BPO, 0.0), reps)
    res["chroma_cqt"] = measure(lambda: TN.chroma_cqt_batch(y, SR, tuning=0.0), reps)
    res["chroma_cqt"]["cqt_share"] = res["cqt"]["ms"] / res["chroma_cqt"]["ms"]
    res["chroma_cqt"]["fold_share"] = res["fold_bins"]["ms"] / res["chroma_cqt"]["ms"]
    raw_ch = ops.chroma_fold(C, wt, "bins", 1, 0.0, None)
    res["cens"] = measure(lambda: ops.chroma_cens(raw_ch, 41, out=outc), reps, floor_bytes=2 * B * NC * Tc * 4)
    res["cens_no_smoothing"] = measure(lambda: ops.chroma_cens(raw_ch, None, out=outc), reps, floor_bytes=2 * B * NC * Tc * 4)
    res["chroma_cens"] = measure(lambda: TN.chroma_cens_batch(y, SR, tuning=0.0), reps)
    res["tonnetz"] = measure(lambda: TN.tonnetz_batch(y, SR, tuning=0.0), reps)
    res["chroma_cqt_tuning_none"] = measure(lambda: TN.chroma_cqt_batch(y, SR), max(3, reps // 2))
    w64 = wt.astype(np.float64)

    def host_fold():
        a = C.cpu().numpy().astype(np.float64)
        ch = np.einsum("ck,bkt->bct", w64, np.sqrt((a ** 2).sum(axis=-1)))
        return ch / np.maximum(np.abs(ch).max(axis=1, keepdims=True), np.finfo(np.float32).tiny)
    res["existing_host_fold"] = host_timed(host_fold, 4)
    res["existing_cqt_path_ms"] = res["cqt"]["ms"] + res["existing_host_fold"]["ms"]
    res["chroma_cqt"]["of_existing_path"] = res["chroma_cqt"]["ms"] / res["existing_cqt_path_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chroma_bench.json"))
    ap.add_argument("--shapes", default="1024x32768,1x16777216")
    a = ap.parse_args()
    ops.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "sr": SR, "n_fft": N_FFT, "hop": HOP, "n_chroma": NC, "cqt_bins": NOCT * BPO,
           "hbm_bytes_per_s": HBM_BPS, "shapes": []}
    for s in a.shapes.split(","):
        B, L = (int(v) for v in s.split("x"))
        out["shapes"].append(bench_shape(B, L, a.reps))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
