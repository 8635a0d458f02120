#!/usr/bin/env python3
"""Record tests/golden/ref_laplace.npz by EXECUTING the reference's own laplace_transform_numerical, once, where the
reference checkout is readable (the path is the first argument; default ../reference beside this repository):

    python tests/golden/make_golden_laplace.py [path/to/reference]

sygnals/core/transforms.py is loaded BY FILE PATH; its top-level `import pywt` gets an EMPTY placeholder module if
PyWavelets is not importable (the Laplace function does not touch it).  Only inputs and outputs (data) are stored; no
reference source is copied.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "..", "..", "reference")
    try:
        import pywt  # noqa: F401
    except ImportError:
        sys.modules["pywt"] = types.ModuleType("pywt")
    spec = importlib.util.spec_from_file_location("_ref_transforms", os.path.join(ref, "sygnals", "core", "transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fn = mod.laplace_transform_numerical
    rng = np.random.default_rng(20251)
    g = {}
    # (L, t_step): float32-representable rows; the s-values span both signs of sigma, omega past pi / t_step, the
    # domain's edge -sigma t_step (L - 1) = 700 and decays where exp underflows
    for i, (L, t_step) in enumerate(((1, 1.0), (65, 0.5), (700, 1.0 / 8000.0), (3001, 1.0 / 44100.0))):
        n = np.arange(L)
        x = (0.6 * np.sin(0.07 * n + 0.3) + 0.4 * rng.standard_normal(L)).astype(np.float32).astype(np.float64)
        T = max(L - 1, 1) * t_step
        sig = np.concatenate([[0.0, 0.0, 0.0, 0.0], [1.0 / T, 30.0 / T, -1.0 / T, -30.0 / T, -700.0 / T],
                              [5.0 / t_step, 100.0 / t_step, -0.3 / t_step if L <= 700 else -0.2 / t_step, 0.01 / t_step],
                              rng.uniform(-40.0, 40.0, 12) / T])
        om = np.concatenate([[0.0, 0.5 * np.pi / t_step, np.pi / t_step, 1.7 * np.pi / t_step],
                             [0.0, 2.0 / t_step, 0.0, -1.3 / t_step, 0.9 / t_step], [0.3 / t_step, 0.0, 2.5 / t_step, 0.0],
                             rng.uniform(-np.pi, np.pi, 12) / t_step])
        s = sig + 1j * om
        g[f"x_{i}"], g[f"s_{i}"], g[f"t_step_{i}"] = x, s, np.float64(t_step)
        g[f"F_{i}"] = fn(x, s, t_step)
    g["n"] = np.int64(4)
    g["F_empty_s"] = fn(g["x_1"], np.zeros(0, dtype=np.complex128), 0.5)
    g["F_empty_x"] = fn(np.zeros(0), g["s_1"][:3], 0.5)
    np.savez_compressed(os.path.join(HERE, "ref_laplace.npz"), **g)
    print("wrote ref_laplace.npz:", len(g), "arrays")


if __name__ == "__main__":
    main()
