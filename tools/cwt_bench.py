"""Time the device continuous wavelet transform (ops.cwt: plan, tables and filter transforms cached by the first call)
with HIP events: every shape warmed, each sample a window of --inner calls, median of --reps windows.

Shapes: 64 clips x 32768 samples x 64 geometric scales (1 ... 4096), morl and cmor1.5-1.0, as `coef` and as `magnitude`
with stride 64, under the rule and with every scale forced through the transforms; one clip of 2^20 samples x 32 scales
(1 ... 131072).  Each time stands beside its byte floor, 4 B (L + S ceil(L / stride)) bytes at 8 TB/s (the output term
doubled for complex `coef`).

The threshold's evidence: banks of 8 scales within +-10 % of one tap count, both forced forms, per tap count.

In the same run a torch baseline at the batch shapes: per scale, torch.fft.rfft convolution (fft for the complex wavelet)
with the same float32 table, transform of the filter made beforehand, cropped at the scale's offset.  Its result is
checked against the kernel's in the run.

Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _cwt as CW  # noqa: E402
from sygnals_amd import ops  # noqa: E402

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


def case(B, L, scales, wavelet, output, stride, form, reps, inner):
    p = CW.cwt_plan(scales, wavelet)
    x = rows(B, L)
    shape = ops.cwt_out_shape(B, p.S, L, stride, p.wavelet.complex, output)
    out = torch.empty(shape, dtype=torch.float32, device="cuda")

    def run():
        ops.cwt(x, scales, wavelet, output, stride, form=form, out=out)

    run()
    one = timed(run, 1, 1, warm=1)["ms"]
    n_in = int(min(inner, max(1, 50.0 // one)))                      # windows of about 50 ms
    t = timed(run, reps, n_in, warm=1)
    floor = 4.0 * B * (L + p.S * shape[2] * (2 if len(shape) == 4 else 1)) / HBM_BPS * 1e3
    direct, spec = CW.split_forms(p, ops.cwt_constants()["direct_taps_max"], form)
    return dict(t, B=B, L=L, S=p.S, wavelet=wavelet, output=output, stride=stride, form=form or "rule", inner=n_in,
                taps_min=int(p.taps.min()), taps_max=int(p.taps.max()), taps_sum=int(p.taps.sum()), direct_scales=int(direct.size),
                spectral_scales=int(spec.size), spectral_rows=len(CW.spectral_rows(p, spec)) if spec.size else 0,
                fft_len=ops.cwt_fft_len(L, int(p.taps[spec].max())) if spec.size else 0,
                byte_floor_ms=floor, floor_fraction=floor / t["ms"], ms_per_scale=t["ms"] / p.S)


def baseline(B, L, scales, wavelet, reps):
    """Per scale: (r)fft convolution with the same table, cropped.  The filters' transforms are made beforehand."""
    from scipy.fft import next_fast_len
    p = CW.cwt_plan(scales, wavelet)
    cplx = p.wavelet.complex
    x = rows(B, L)
    fwd = torch.fft.fft if cplx else torch.fft.rfft
    Hs, Ms = [], []
    for i in range(p.S):
        M = next_fast_len(L + int(p.taps[i]) - 1, real=not cplx)
        Hs.append(fwd(torch.from_numpy(p.filter32(i)).cuda(), n=M))
        Ms.append(M)
    out = torch.empty((B, p.S, L), dtype=torch.complex64 if cplx else torch.float32, device="cuda")

    def run():
        for i in range(p.S):
            sh = int(p.offset[i]) + 1
            X = fwd(x, n=Ms[i])
            y = torch.fft.ifft(X * Hs[i], n=Ms[i]) if cplx else torch.fft.irfft(X * Hs[i], n=Ms[i])
            out[:, i] = y[:, sh:sh + L]
        return out

    ours = ops.cwt(x, scales, wavelet)
    got = run()
    got = torch.view_as_real(got) if cplx else got
    A = torch.from_numpy(p.l1.astype(np.float32)).cuda().view(1, -1, *([1] * (ours.dim() - 2))) * x.abs().amax(dim=1).view(-1, 1, *([1] * (ours.dim() - 2)))
    diff = float(((got - ours).abs() / A).max())
    return dict(timed(run, reps, 1, warm=1), B=B, L=L, S=p.S, wavelet=wavelet,
                what="per scale: torch (r)fft of the rows, product with the filter's transform, inverse, crop",
                max_diff_to_kernel_over_A=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-big", action="store_true", help="leave the batch shapes out (the threshold table only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cwt_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"constants": ops.cwt_constants()}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")

    # both forced forms by tap count: 8 scales within +-10 % of s, taps = 16 s + 2
    B, L = 64, 32768
    for taps in (34, 66, 130, 258, 514, 770, 1026, 1538, 2050, 4098):
        s = (taps - 2) / 16.0
        bank = tuple(float(v) for v in s * np.linspace(0.9, 1.1, 8))
        for wavelet in ("morl", "cmor1.5-1.0"):
            for form in ("direct", "spectral"):
                res[f"by_taps_{taps}_{wavelet}_{form}"] = case(B, L, bank, wavelet, "coef", 1, form, a.reps, a.inner)
        write()
    if not a.no_big:
        scales = tuple(float(v) for v in CW.scalogram_scales(64, L))
        for wavelet in ("morl", "cmor1.5-1.0"):
            for output, stride in (("coef", 1), ("magnitude", 64)):
                for form in (None, "spectral"):
                    res[f"batch_64x32768x64_{wavelet}_{output}_stride{stride}_{form or 'rule'}"] = \
                        case(B, L, scales, wavelet, output, stride, form, a.reps, a.inner)
                write()
        big = tuple(float(v) for v in CW.scalogram_scales(32, 1 << 20))
        res["one_clip_2p20_x32_morl_coef_rule"] = case(1, 1 << 20, big, "morl", "coef", 1, None, max(3, a.reps // 3), 1)
        write()
        if not a.no_baseline:
            for wavelet in ("morl", "cmor1.5-1.0"):
                b = baseline(B, L, scales, wavelet, max(3, a.reps // 3))
                b["baseline_over_kernel_time"] = b["ms"] / res[f"batch_64x32768x64_{wavelet}_coef_stride1_rule"]["ms"]
                res[f"baseline_torch_64x32768x64_{wavelet}"] = b
            write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
