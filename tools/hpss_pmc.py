"""The HPSS stages of harmonic_to_noise_ratio on 1024 x 48000 at 48 kHz, each launched back to back (the target of a
rocprofv3 --pmc pass; summarise with tools/pmc_kernels.py <dir> hpss_masks istft2048 hnr_rows).
    python tools/hpss_pmc.py [launches]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sygnals_amd import ops  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    sr = 48000
    t = np.arange(sr) / sr
    f = rng.uniform(80, 900, (1024, 1))
    y = ops.to_device_f32((0.5 * np.sin(2 * np.pi * f * t[None, :]) + 0.05 * rng.standard_normal((1024, sr)))
                          .astype(np.float32))
    D = ops.stft2048_c2c(y)
    Mh, Mp = ops.hpss_masks(D)
    yh, yp = ops.istft2048(D, 512, sr, mask=(Mh, Mp))
    for _ in range(n):
        ops.hpss_masks(D)
    for _ in range(n):
        ops.istft2048(D, 512, sr, mask=(Mh, Mp))
    for _ in range(n):
        ops.hnr_rows(yh, yp, 2048, 512)
    torch.cuda.synchronize()
    print("ok")


if __name__ == "__main__":
    main()
