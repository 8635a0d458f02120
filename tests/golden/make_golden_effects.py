#!/usr/bin/env python3
"""Record tests/golden/ref_effects.npz by EXECUTING the reference's own effect functions, once, where the reference
checkout is readable (the path is the first argument; default ../reference beside this repository):

    python tests/golden/make_golden_effects.py [path/to/reference]

sygnals/core/audio/effects/__init__.py imports librosa, which is not installed, so the modules are loaded BY FILE PATH
under a placeholder package (chorus.py imports `.tremolo`).  utility.py has a top-level `import librosa`: an EMPTY
placeholder module lets that statement pass; only adjust_gain and stereo_widening_midside are called from it, neither
touches librosa.  Only inputs and outputs (data) are stored; no reference source is copied.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = "_ref_effects"


def load(fx_dir, name):
    spec = importlib.util.spec_from_file_location(f"{PKG}.{name}", os.path.join(fx_dir, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def clip(rng, n, sr):
    t = np.arange(n) / sr
    y = 0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.3 * np.sin(2 * np.pi * 1730.0 * t + 0.4) + 0.1 * rng.standard_normal(n)
    return (y * np.linspace(0.2, 1.6, n)).astype(np.float32).astype(np.float64)      # float32-representable inputs


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "..", "..", "reference")
    fx_dir = os.path.join(ref, "sygnals", "core", "audio", "effects")
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))
    pkg = types.ModuleType(PKG)
    pkg.__path__ = [fx_dir]
    sys.modules[PKG] = pkg
    delay, tremolo, compression, reverb = (load(fx_dir, m) for m in ("delay", "tremolo", "compression", "reverb"))
    chorus, utility = load(fx_dir, "chorus"), load(fx_dir, "utility")
    rng = np.random.default_rng(20250)
    sr = 8000
    y = clip(rng, 4096, sr)
    g = {"sr": np.int64(sr), "y": y}
    # delay: (delay_time, feedback, wet, dry); delay_samples = int(delay_time * sr)
    g["delay_params"] = np.array([[0.05, 0.4, 0.5, 1.0], [0.0125, 0.95, 1.0, 0.3], [0.000125, 0.6, 0.7, 0.9],
                                  [0.3, 0.0, 0.25, 0.75], [0.0, 0.4, 0.5, 1.0], [0.6, 0.4, 0.5, 1.0]])
    for i, (dt, fb, wet, dry) in enumerate(g["delay_params"]):
        g[f"delay_{i}"] = delay.apply_delay(y, sr, dt, fb, wet, dry)
    # chorus on a shorter clip (it argsorts its buffer per sample): (rate, depth, delay, feedback, wet, dry)
    yc = y[:3000]
    g["chorus_params"] = np.array([[1.5, 0.002, 0.025, 0.2, 0.5, 1.0], [0.7, 0.001, 0.004, 0.5, 0.8, 0.6]])
    g["chorus_shapes"] = np.array(["sine", "triangle"])
    for i, (p, shp) in enumerate(zip(g["chorus_params"], g["chorus_shapes"])):
        g[f"chorus_{i}"] = chorus.apply_chorus(yc, sr, *p, lfo_shape=str(shp))
    # the pointwise effects on the first 2048 samples
    ys = y[:2048]
    # tremolo: (rate, depth) per shape, at sr and at 22050 Hz
    g["tremolo_params"] = np.array([[5.0, 0.5], [3.3, 1.0], [11.0, 0.25]])
    for shp in ("sine", "triangle", "square"):
        for i, (rate, depth) in enumerate(g["tremolo_params"]):
            g[f"tremolo_{shp}_{i}"] = tremolo.apply_tremolo(ys, 22050 if i == 0 else sr, rate, depth, shp)
    # compression: (threshold, ratio)
    g["compress_params"] = np.array([[0.8, 4.0], [0.3, 2.0], [0.0, 10.0], [0.5, 1.0]])
    for i, (thr, ratio) in enumerate(g["compress_params"]):
        g[f"compress_{i}"] = compression.simple_dynamic_range_compression(ys, thr, ratio)
    # reverb, seed 7: (decay_time, wet, dry)
    g["reverb_params"] = np.array([[0.0, 0.3, 0.7], [0.01, 0.5, 0.5], [0.3, 0.3, 0.7]])
    for i, (dec, wet, dry) in enumerate(g["reverb_params"]):
        g[f"reverb_{i}"] = reverb.apply_reverb(y, sr, dec, wet, dry, ir_seed=7)
        g[f"reverb_ir_{i}"] = reverb._generate_basic_ir(sr, dec, seed=7)
    g["gain_db"] = np.array([-6.0, 0.0, 3.5])
    for i, db in enumerate(g["gain_db"]):
        g[f"gain_{i}"] = utility.adjust_gain(ys, db)
    st = np.stack([ys, np.roll(ys, 37) * 0.8 + 0.05 * clip(rng, 2048, sr)]).astype(np.float32).astype(np.float64)
    g["stereo"] = st
    g["width"] = np.array([0.0, 1.0, 1.5, 2.5])
    for i, wd in enumerate(g["width"]):
        g[f"midside_{i}"] = utility.stereo_widening_midside(st, wd)
    np.savez_compressed(os.path.join(HERE, "ref_effects.npz"), **g)
    print("wrote ref_effects.npz:", len(g), "arrays")


if __name__ == "__main__":
    main()
