"""Time the device augmentation with HIP events (buffers allocated once, every shape warmed, each sample a window of
--inner calls, median of --reps) and measure the conditioning of time stretch.

Vocoder (syg_phase_vocoder_f32 through the C ABI, step table and buffers made once): 1024 clips x 32768 samples at
rates 0.8 and 1.25, and one row of 2^24 samples at 0.8, as ms and a fraction of the HBM floor (D read once, D' written once: 8 * 1025 * (T + T') bytes a
clip over 8 TB/s); for the single row both forms, chain and chunked, alternating in one process -- the figure the
library's switch rests on -- and for the batch too; `rule` names the form the library picks by itself.  The whole chain
ops.time_stretch (STFT, vocoder, inverse STFT) at the same shapes.  --vocoder-only stops there.  --switch adds a sweep
of the clip count B at 32768 samples and rate 0.8, both forms, around the rule's threshold.

add_noise (ops.fx_add_noise) against its floor of 12 bytes a sample (y and noise read, out written): 1024 x 32768 (two
launches), 2048 x 16384 (the resident form) and one row of 2^24.

Conditioning (not timed): ops.time_stretch against the full float64 restatement tests/vocoder_ref.time_stretch at rates
0.5, 0.8, 1.0, 1.25 and 2.0 on the tones-plus-noise and the white-noise signal, as a fraction of the output peak; beside
it the restatement's own shift when its STFT is replaced by the device's D (the floor the device cannot beat), and the
device against the restatement fed that D (the kernels' own error).

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
from sygnals_amd import ops  # noqa: E402
from sygnals_amd._lib import check, lib  # noqa: E402
from tests import hpss_ref as H  # noqa: E402
from tests import vocoder_ref as V  # noqa: E402

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


def against_floor(t, nbytes, samples):
    floor_ms = nbytes / HBM_BPS * 1e3
    return dict(t, hbm_floor_ms=floor_ms, hbm_fraction=floor_ms / t["ms"], msamples_per_s=samples / t["ms"] * 1e-3)


def vocoder_case(B, L, rate, reps, inner):
    g = torch.Generator(device="cuda").manual_seed(5)
    y = 0.1 * torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    D = ops.stft2048_c2c(y)
    Tn = D.shape[1]
    To = int(np.ceil(Tn / rate))
    nbytes = 8 * 1025 * (Tn + To) * B
    res = dict(B=B, L=L, rate=rate, frames=Tn, frames_out=To, chunk=ops.phase_vocoder_chunk(), floor_bytes=nbytes,
               rule="chunked" if lib().syg_phase_vocoder_work_bytes(B, To, -1) > 0 else "chain")
    # the kernel alone: the C ABI on buffers and a step table made once
    h, p = lib(), ops._ptr
    col, alpha = (torch.from_numpy(a).cuda() for a in ops.T.vocoder_steps(Tn, rate))
    out = torch.empty((B, To, 1025, 2), dtype=torch.float32, device="cuda")
    work = torch.empty((max(h.syg_phase_vocoder_work_bytes(B, To, 1), 16) // 8,), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(form):
        check(h.syg_phase_vocoder_f32(p(D), B, Tn, p(col), p(alpha), To, p(out), p(work), ops.VOCODER_FORMS[form], st),
              "syg_phase_vocoder_f32")

    outs = {}
    for f in ("chain", "chunked"):
        launch(f)
        outs[f] = out.clone()
    res["forms_peak_rel"] = float((outs["chain"] - outs["chunked"]).abs().max() / outs["chain"].abs().max())
    del outs
    t = {"chain": [], "chunked": []}
    for _ in range(2):                              # chain, chunked, chain, chunked
        for form in ("chain", "chunked"):
            run = lambda: launch(form)
            one = timed(run, 1, 1, warm=1)["ms"]
            n_in = int(min(inner, max(1, 50.0 // one)))             # windows of about 50 ms, fewer calls when slow
            t[form].append(dict(timed(run, reps if one < 100.0 else 3, n_in, warm=1), inner=n_in))
    for form, v in t.items():
        best = min(v, key=lambda m: m["ms"])
        res[form] = against_floor(best, nbytes, B * L)
        res[form]["ms_runs"] = [m["ms"] for m in v]
    res["chunked_over_chain_time"] = res["chunked"]["ms"] / res["chain"]["ms"]
    if not ARGS.vocoder_only:
        n_in = max(1, inner // 5)
        res["stft"] = timed(lambda: ops.stft2048_c2c(y), reps, n_in)
        Lo = int(round(L / rate))
        res["istft"] = timed(lambda: ops.istft2048(out, length=Lo), reps, n_in)
        # algorithmic traffic of the chain: y in, D out | the vocoder | D' in, y' out
        chain_bytes = (4 * B * L + 8 * 1025 * Tn * B) + nbytes + (8 * 1025 * To * B + 4 * B * Lo)
        res["chain_total"] = against_floor(timed(lambda: ops.time_stretch(y, rate), reps, n_in), chain_bytes, B * L)
        res["vocoder_share_of_chain_time"] = res[res["rule"]]["ms"] / res["chain_total"]["ms"]
    return res


def noise_case(B, L, reps, inner):
    g = torch.Generator(device="cuda").manual_seed(7)
    y = 0.1 * torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    noise = torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    out = torch.empty_like(y)
    snr = torch.full((B,), 10.0, dtype=torch.float64, device="cuda")
    res = dict(B=B, L=L, launches=1 if L <= ops.fx_add_noise_resident_max() else 2)
    res.update(against_floor(timed(lambda: ops.fx_add_noise(y, noise, snr, out=out), reps, inner), 12 * B * L, B * L))
    return res


def peak_rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def conditioning():
    rows = []
    for name in ("tones_noise", "white"):
        for L in (8192, 65536):
            y32 = getattr(V, name)(L).astype(np.float32)
            yd = torch.from_numpy(y32[None, :]).cuda()
            Dd = ops.stft2048_c2c(yd)[0].cpu().numpy()
            Dd = (Dd[..., 0].astype(np.float64) + 1j * Dd[..., 1].astype(np.float64)).T
            D64 = H.stft(y32.astype(np.float64))
            for rate in (0.5, 0.8, 1.0, 1.25, 2.0):
                Lo = V.stretch_length(L, rate)
                full = H.istft(V.phase_vocoder(D64, rate), Lo)
                shared = H.istft(V.phase_vocoder(Dd, rate), Lo)
                dev = ops.time_stretch(yd, rate)[0].cpu().numpy().astype(np.float64)
                rows.append(dict(signal=name, L=L, rate=rate, gated=rate in (0.5, 1.0),
                                 device_vs_float64=peak_rel(dev, full),
                                 float64_shift_through_device_stft=peak_rel(shared, full),
                                 device_vs_float64_from_device_stft=peak_rel(dev, shared)))
    return rows


def main():
    global ARGS
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--vocoder-only", action="store_true")
    ap.add_argument("--switch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    ARGS = a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"vocoder_batch_1024x32768_rate0.8": vocoder_case(1024, 32768, 0.8, a.reps, a.inner),
           "vocoder_batch_1024x32768_rate1.25": vocoder_case(1024, 32768, 1.25, a.reps, a.inner),
           "vocoder_one_row_2p24_rate0.8": vocoder_case(1, 1 << 24, 0.8, a.reps, a.inner)}
    if a.switch:
        keep, a.vocoder_only = a.vocoder_only, True
        res["switch_sweep_L32768_rate0.8"] = [
            {k: (v if k in ("B", "frames_out", "rule", "chunked_over_chain_time") else v["ms"])
             for k, v in vocoder_case(B, 32768, 0.8, a.reps, a.inner).items()
             if k in ("B", "frames_out", "rule", "chain", "chunked", "chunked_over_chain_time")}
            for B in (1, 4, 16, 32, 64, 120, 121, 256)]
        res["switch_sweep_L262144_rate0.8"] = [
            {k: (v if k in ("B", "frames_out", "rule", "chunked_over_chain_time") else v["ms"])
             for k, v in vocoder_case(B, 262144, 0.8, a.reps, a.inner).items()
             if k in ("B", "frames_out", "rule", "chain", "chunked", "chunked_over_chain_time")}
            for B in (1, 4, 16, 64, 120)]
        a.vocoder_only = keep
    if not a.vocoder_only:
        res["add_noise_1024x32768"] = noise_case(1024, 32768, a.reps, a.inner)
        res["add_noise_2048x16384"] = noise_case(2048, 16384, a.reps, a.inner)
        res["add_noise_one_row_2p24"] = noise_case(1, 1 << 24, a.reps, a.inner)
        res["conditioning"] = conditioning()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
