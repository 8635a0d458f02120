"""Time the device audio effects with HIP events (buffers allocated once, every shape warmed, each sample a window of
--inner calls, median of --reps).

Delay (syg_fx_delay_f32 through the C ABI): 1024 clips x 32768 samples at D = 11025, one row of 2^24 samples at D = 441
and at D = 7, each in both forms -- one lane per residue (fx_delay_form = 0) and chunked chains (1) -- alternating in one
process, as ms, Msamples / s and a fraction of the HBM floor (one read and one write: 8 bytes per sample over 8 TB/s);
`rule` names the form the library picks by itself.  The outputs of the two forms are compared at the timed sizes.
--delay-only stops there: run it against a library built with another chunk length
(EXTRA_HIPCC_FLAGS=-DSYG_FX_CHUNK=n SYG_LIB_OUT=<path> ./build_lib.sh, then SYGNALS_AMD_LIB=<path>) to time that length.

Denoise (noise_reduction_spectral_batch on 1024 x 32768 at 22050 Hz, 0.5 s of profile): the whole chain and its four
launches' stages one by one; the gate alone against its byte floor (8 bytes of D and 4 of gain per bin, plus the profile's
STFT and the profile); the share of the chain's algorithmic traffic that writing the gain and reading it back account for.

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
from sygnals_amd.core.audio.effects import noise_reduction_spectral_batch  # noqa: E402

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


def delay_case(B, L, D, reps, inner, fb=0.4):
    h = lib()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    out = torch.empty_like(x)
    with ops.override(fx_delay_form=1):
        wb = h.syg_fx_delay_work_bytes(B, L, D)
    work = torch.empty((max(wb, 4) // 4,), dtype=torch.float32, device="cuda")
    rule = "chunked" if h.syg_fx_delay_work_bytes(B, L, D) > 0 else "plain"
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = ops._ptr

    def run():
        check(h.syg_fx_delay_f32(p(x), B, L, L, D, fb, 1.0, 0.5, p(out), L, p(work), st), "syg_fx_delay_f32")

    res = dict(B=B, L=L, D=D, feedback=fb, chunk=int(h.syg_fx_delay_chunk()), steps_per_chain=-(-L // D), rule=rule,
               work_bytes_chunked=int(wb))
    outs = {}
    for form, name in ((0, "plain"), (1, "chunked")):
        with ops.override(fx_delay_form=form):
            run()
            outs[name] = out.clone()
    res["forms_peak_rel"] = float((outs["plain"] - outs["chunked"]).abs().max() / outs["plain"].abs().max())
    del outs
    t = {"plain": [], "chunked": []}
    for _ in range(2):                              # plain, chunked, plain, chunked
        for form, name in ((0, "plain"), (1, "chunked")):
            with ops.override(fx_delay_form=form):
                one = timed(run, 1, 1, warm=1)["ms"]            # a form that serialises a long chain takes a while:
                n_in = int(min(inner, max(1, 50.0 // one)))     # windows of about 50 ms, fewer of them when slow
                t[name].append(dict(timed(run, reps if one < 100.0 else 3, n_in, warm=1), inner=n_in))
    for name, v in t.items():
        best = min(v, key=lambda m: m["ms"])
        res[name] = against_floor(best, 8 * B * L, B * L)
        res[name]["ms_runs"] = [m["ms"] for m in v]
    res["chunked_over_plain_time"] = res["chunked"]["ms"] / res["plain"]["ms"]
    return res


def denoise_case(B, L, sr, dur, reps, inner):
    g = torch.Generator(device="cuda").manual_seed(6)
    y = 0.1 * torch.randn((B, L), dtype=torch.float32, device="cuda", generator=g)
    ns = int(dur * sr)
    D = ops.stft2048_c2c(y)
    Dn = ops.stft2048_c2c(y[:, :ns])
    G = ops.spectral_gate(D, Dn, 1.0)
    Tn, Tp = D.shape[1], Dn.shape[1]
    bins, pbins = B * Tn * 1025, B * Tp * 1025
    res = dict(B=B, L=L, sr=sr, noise_samples=ns, frames=Tn, profile_frames=Tp)
    res["chain"] = timed(lambda: noise_reduction_spectral_batch(y, sr, dur, 1.0), reps, inner)
    res["stft_clip"] = timed(lambda: ops.stft2048_c2c(y), reps, inner)
    res["stft_profile"] = timed(lambda: ops.stft2048_c2c(y[:, :ns]), reps, inner)
    gate_bytes = 12 * bins + 8 * pbins + 2 * 4 * B * 1025      # D in, gain out; Dn in; the profile out and in again
    res["gate"] = against_floor(timed(lambda: ops.spectral_gate(D, Dn, 1.0), reps, inner), gate_bytes, B * L)
    res["istft_masked"] = timed(lambda: ops.istft2048(D, 512, L, mask=G), reps, inner)
    # algorithmic traffic of the chain: y in, D out | profile in, Dn out | the gate | D and gain in, y out
    chain_bytes = (4 * B * L + 8 * bins) + (4 * B * ns + 8 * pbins) + gate_bytes + (12 * bins + 4 * B * L)
    res["chain_bytes"] = chain_bytes
    res["chain"] = against_floor(res["chain"], chain_bytes, B * L)
    res["gain_write_and_read_share_of_traffic"] = 8 * bins / chain_bytes
    res["gain_write_and_read_floor_ms"] = 8 * bins / HBM_BPS * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--delay-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "effects_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"delay_batch_1024x32768_D11025": delay_case(1024, 32768, 11025, a.reps, a.inner),
           "delay_one_row_2p24_D441": delay_case(1, 1 << 24, 441, a.reps, a.inner),
           "delay_one_row_2p24_D7": delay_case(1, 1 << 24, 7, a.reps, a.inner)}
    if not a.delay_only:
        res["denoise_1024x32768"] = denoise_case(1024, 32768, 22050, 0.5, a.reps, max(1, a.inner // 5))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
