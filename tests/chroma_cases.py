"""The cases of tests/test_gpu_chroma.py: shapes, crafted inputs and end-to-end signals, all generated from seeds."""
import numpy as np

from tests import chroma_ref as R

NORMS = (np.inf, 1, 2, None)

# G1, frame-major fold: (T, F) sweeps against the table of n_fft = 2 (F - 1); (n_chroma, F) for the three table homes
ROWS_T = (1, 2, 63, 64, 65, 257)
ROWS_F = (2, 65, 129, 1025, 2049)
ROWS_TABLES = ((12, 1025), (12, 2049), (36, 1025), (36, 2049), (1, 129), (24, 65))      # LDS / LDS beyond 64 KiB / global memory

# G1, bin-major fold: (K, bins_per_octave, n_chroma, smoothing window of the merge table or None)
BINS_TABLES = ((1, 12, 12, None), (12, 12, 12, None), (36, 36, 36, None), (252, 36, 12, None), (253, 36, 12, None),
               (252, 36, 12, (0.25, 0.5, 0.25)), (36, 12, 1, None), (253, 72, 24, None))
BINS_T = (1, 63, 64, 65, 1000)

# G2
CENS_WIN = (None, 1, 2, 41, 42, 255)
CENS_WINDOWS = ("hann", "boxcar", "triang")


def cens_T(tile):
    return (1, 20, 21, 22, tile - 1, tile, tile + 1, 3 * tile + 5)


def positive(shape, seed, lo=0.05):
    """float32 values in [lo, 1): no cancellation and no silent frame."""
    return np.random.default_rng(seed).uniform(lo, 1.0, shape).astype(np.float32)


def complex_pairs(shape, seed):
    """Interleaved complex float32 [..., 2] with moduli in [0.05, 1)."""
    rng = np.random.default_rng(seed)
    m, ph = rng.uniform(0.05, 1.0, shape), rng.uniform(0, 2 * np.pi, shape)
    return np.stack([m * np.cos(ph), m * np.sin(ph)], axis=-1).astype(np.float32)


def cens_chroma(n_chroma, T, seed):
    """An unnormalised float32 chroma [n_chroma, T] whose L1-normalised entries all stay 1e-4 away from a quantiser step
    (frames that do not are drawn again), with a silent frame where T allows."""
    rng = np.random.default_rng(seed)
    ch = (rng.uniform(0.0, 1.0, (n_chroma, T)) ** 3).astype(np.float32)
    for _ in range(100):
        n = R.normalize(ch.astype(np.float64), 1, axis=0)
        bad = np.nonzero(np.min([np.min(np.abs(n - s), axis=0) for s in R.QUANT_STEPS], axis=0) < 2e-4)[0]
        if len(bad) == 0:
            break
        ch[:, bad] = (rng.uniform(0.0, 1.0, (n_chroma, len(bad))) ** 3).astype(np.float32)
    if T > 4:
        ch[:, 3] = 0.0
    return ch


def bumps(F, T, peaks, seed, floor=1e-4):
    """A crafted magnitude spectrogram float32 [F, T]: Gaussian bumps (centre, height) per frame over a small positive floor,
    heights jittered per frame so that no two magnitudes tie."""
    rng = np.random.default_rng(seed)
    k = np.arange(F, dtype=np.float64)[:, None]
    S = floor * rng.uniform(0.5, 1.0, (F, T))
    for v, h in peaks:
        vv = v + rng.uniform(-0.2, 0.2, (1, T))
        S = S + h * rng.uniform(0.9, 1.1, (1, T)) * np.exp(-0.5 * ((k - vv) / 1.3) ** 2)
    return S.astype(np.float32)


def chord(sr, L, cents=0.0, harmonics=1, seed=0, noise=0.002):
    """Five tones (A3 C4 E4 A4 C5) detuned by `cents`, with `harmonics` partials each, plus white noise: no silent frame."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / sr
    y = np.zeros(L)
    for m in (57, 60, 64, 69, 72):
        f = 440.0 * 2.0 ** ((m - 69) / 12.0) * 2.0 ** (cents / 1200.0)
        for h in range(1, harmonics + 1):
            y += np.sin(2 * np.pi * f * h * t + rng.uniform(0, 6)) / h
    return (0.2 * y + noise * rng.normal(size=L)).astype(np.float32)


def melody(sr, L, seed=0):
    """A note every quarter second over a noise floor: what an alignment can hold on to."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / sr
    notes = rng.permutation(np.arange(57, 81))
    f = 440.0 * 2.0 ** ((notes[(t * 4).astype(int) % len(notes)] - 69) / 12.0)
    return (0.3 * np.sin(2 * np.pi * np.cumsum(f) / sr) + 0.003 * rng.normal(size=L)).astype(np.float32)


# G4: (sr, L, n_fft, hop, tuning)
E2E_STFT = ((22050, 8192, 2048, 512, 0.0), (16000, 8192, 1024, 256, 0.13), (22050, 8192, 1000, 250, -0.3), (22050, 20000, 2048, 512, 0.25))
E2E_CQT = ((22050, 8192, 0.0), (16000, 8192, 0.13), (22050, 20000, -0.3))
# tuning=None: (cents, harmonics, seconds) that pass both checks of the issue at 22 050 Hz on the magnitude spectrogram at 12
# and 36 bins per octave and on the power spectrogram (asserted in the test); the chord at 0 and +20 cents does not
E2E_AUTO = ((-35, 1, 1), (-20, 3, 1), (-20, 1, 1))
