"""Time the Kaldi front end (ops.kaldi_fbank / ops.kaldi_mfcc) with HIP events: every form warmed, each sample a window of
calls of about 50 ms, median of --reps windows, the forms of a workload alternating window by window.

Workloads: 1024 clips x 160 000 samples at 16 kHz with 80 and with 128 bins, and 1024 x 480 000 at 48 kHz with 80 bins; fbank
and the 13-coefficient MFCC.  Three yardsticks beside each, in the same run:
  floor   the bytes a clip needs, 4 (L + T C), at 8 TB/s;
  stft    the existing front end with the same transform and projection and none of the new stages
          (ops.stft_front(n_fft = N, hop, center=False) with the same band count: frames of N samples, hann, Slaney);
  torch   the composition a user would write on the device: unfold, the frame arithmetic, torch.fft.rfft, matmul, log
          (chunked over the clips so that the frames fit the memory).
Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import _kaldi as KD  # noqa: E402
from sygnals_amd import ops  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth, bytes / s


def window_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(forms, reps):
    """forms: name -> callable.  Each form warmed, its window sized to about 50 ms, then reps rounds over all forms."""
    inner = {}
    for name, fn in forms.items():
        fn()
        torch.cuda.synchronize()
        one = window_ms(fn, 1)
        inner[name] = int(min(200, max(1, 50.0 // max(one, 1e-3))))
    ts = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            ts[name].append(window_ms(fn, inner[name]))
    return {name: dict(ms=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)), inner=inner[name])
            for name, v in ts.items()}


def torch_fbank(y, s, win, basis, chunk):
    """The torch composition of the default fbank (snip_edges, DC removal, pre-emphasis, window, |rfft|^2, mel, log)."""
    outs = []
    for b0 in range(0, y.shape[0], chunk):
        fr = y[b0:b0 + chunk].unfold(1, s.wl, s.hop)
        fr = fr - fr.mean(dim=2, keepdim=True)
        prev = torch.cat([fr[..., :1], fr[..., :-1]], dim=2)
        fr = (fr - s.preemph * prev) * win
        spec = torch.fft.rfft(fr, n=s.N, dim=2)[..., :s.N // 2]
        E = torch.matmul(spec.real.square() + spec.imag.square(), basis)
        outs.append(torch.log(torch.clamp_min(E, KD.EPS)))
    return torch.cat(outs)


def bench(B, L, sr, M, reps, chunk):
    g = torch.Generator(device="cuda").manual_seed(3)
    y = torch.randn((B, L), device="cuda", generator=g) * 0.1
    s = KD.check("kaldi_bench", False, sr, dict(num_mel_bins=M))
    Tn = KD.frames_of(s, L)
    win = torch.from_numpy(KD.window(s.window_type, s.wl, s.blackman_coeff).astype(np.float32)).cuda()
    basis = torch.from_numpy(KD.mel_banks(M, s.N, s.sr, s.low, s.high).astype(np.float32).T.copy()).cuda()
    fb_out = torch.empty((B, M, Tn), device="cuda")
    mf_out = torch.empty((B, 13, Tn), device="cuda")
    forms = {"fbank": lambda: ops.kaldi_fbank(y, sr, num_mel_bins=M, out=fb_out),
             "fbank_tc": lambda: ops.kaldi_fbank(y, sr, num_mel_bins=M, layout="tc"),
             "mfcc13": lambda: ops.kaldi_mfcc(y, sr, num_mel_bins=M, out=mf_out),
             "stft_front": lambda: ops.stft_front(y, sr, s.N, s.hop, center=False, n_mels=M),
             "torch": lambda: torch_fbank(y, s, win, basis, chunk)}
    notes = {}
    for name in list(forms):
        try:
            forms[name]()
            torch.cuda.synchronize()
        except Exception as e:                                        # a yardstick that does not serve the shape: not measured
            notes[name] = f"not measured: {type(e).__name__}: {e}"
            del forms[name]
    r = alternate(forms, reps)
    err = float((torch_fbank(y[:8], s, win, basis, 8).transpose(1, 2) - ops.kaldi_fbank(y[:8], sr, num_mel_bins=M)).abs().max().item())
    for name, v in r.items():
        C = 13 if name == "mfcc13" else M
        v["floor_ms"] = 4.0 * B * (L + Tn * C) / HBM_BPS * 1e3
        v["of_floor"] = v["floor_ms"] / v["ms"]
        v["clips_per_s"] = B / v["ms"] * 1e3
        v["of_fbank"] = v["ms"] / r["fbank"]["ms"]
    return dict(B=B, L=L, sr=sr, num_mel_bins=M, wl=s.wl, hop=s.hop, N=s.N, T=Tn, forms=r, notes=notes,
                torch_vs_device_max_abs_log_difference=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=64, help="clips of one piece of the torch composition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kaldi_bench.json"))
    ap.add_argument("--workloads", default="1024x160000x16000x80,1024x160000x16000x128,1024x480000x48000x80")
    a = ap.parse_args()
    ops.require_gpu()
    out = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BPS, "constants": ops.kaldi_constants(), "workloads": []}
    for w in a.workloads.split(","):
        B, L, sr, M = (int(v) for v in w.split("x"))
        out["workloads"].append(bench(B, L, float(sr), M, a.reps, a.chunk))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
