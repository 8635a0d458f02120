#!/usr/bin/env python3
"""Record tests/golden/ref_augment.npz by EXECUTING the reference's own add_noise, once, where the reference checkout is
readable (the path is the first argument; default ../reference beside this repository):

    python tests/golden/make_golden_augment.py [path/to/reference]

sygnals/core/augment/__init__.py imports librosa (through effects_based.py), which is not installed, so noise.py is
loaded BY FILE PATH; it needs numpy alone.  Only inputs and outputs (data) are stored; no reference source is copied.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def clip(rng, n):
    t = np.arange(n) / 8000.0
    y = 0.5 * np.sin(2 * np.pi * 220.0 * t + 0.2) + 0.1 * rng.standard_normal(n)
    return y.astype(np.float32).astype(np.float64)                  # float32-representable inputs


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "..", "..", "reference")
    spec = importlib.util.spec_from_file_location("_ref_noise", os.path.join(ref, "sygnals", "core", "augment", "noise.py"))
    noise = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(noise)
    rng = np.random.default_rng(20)
    cases = []                                                        # (y, snr_db, seed, silent)
    for L in (1, 7, 4096):
        for snr, seed in ((-5.0, 0), (10.0, 1), (40.0, 12345)):
            cases.append((clip(rng, L) + (0.25 if L == 1 else 0.0), snr, seed, False))
    cases.append((np.zeros(4096), 10.0, 3, True))                     # a silent clip comes back as it is
    cases.append((np.full(7, np.float64(np.float32(1e-9))), -5.0, 4, True))                   # power 1e-18 < eps: silent by the reference's rule
    cases.append((clip(rng, 4096), 10.0, 1, False))                   # the seed of an earlier case on another clip
    out = {"n_cases": np.array(len(cases)), "snr_db": np.array([c[1] for c in cases]),
           "seed": np.array([c[2] for c in cases]), "silent": np.array([c[3] for c in cases])}
    for i, (y, snr, seed, _) in enumerate(cases):
        out[f"y_{i}"] = y
        out[f"out_{i}"] = noise.add_noise(y.copy(), snr, "gaussian", seed)
    np.savez_compressed(os.path.join(HERE, "ref_augment.npz"), **out)
    print(f"wrote ref_augment.npz: {len(cases)} cases")


if __name__ == "__main__":
    main()
