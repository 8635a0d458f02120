"""Inputs shared by tests/test_lpc_ref.py and tests/test_gpu_lpc.py, float32, built once per kind and length, and the list
of frame cases of the GPU tests.  Pure tones are not among them: two noiseless sines make the two float64 forms of Burg's
denominator differ by 1e-4 at order 8, so no float64 result is a reference for them."""
import functools

import numpy as np

# noise; a noise-driven AR(4); an impulse-train vowel with four resonances over noise 40 / 60 / 80 dB down; a 440 Hz sine
# (at 22 050 Hz) with 1 % noise, the input on which a float32 recurrence misses the gate at order 32
SIGNALS = ("noise", "ar4", "vowel40", "vowel60", "vowel80", "sine1")


@functools.lru_cache(maxsize=None)
def clip(kind: str, L: int, seed: int = 0) -> np.ndarray:
    """One clip [L] float32 (read-only)."""
    rng = np.random.default_rng(977 * len(kind) + 13 * L + seed + sum(map(ord, kind)))
    n = np.arange(L)
    if kind == "noise":
        x = rng.standard_normal(L)
    elif kind == "ar4":
        e = rng.standard_normal(L + 64)
        x = np.zeros(L + 64)
        for i in range(4, L + 64):
            x[i] = e[i] + 1.2 * x[i - 1] - 0.9 * x[i - 2] + 0.3 * x[i - 3] - 0.2 * x[i - 4]
        x = x[64:] / np.max(np.abs(x[64:]))
    elif kind.startswith("vowel"):
        from scipy.signal import lfilter
        level = 10.0 ** (-float(kind[5:]) / 20.0)
        src = np.zeros(L + 256)
        src[::147] = 1.0                                    # 150 Hz at 22 050 Hz
        den = np.array([1.0])
        for fc, bw in ((700.0, 110.0), (1220.0, 120.0), (2600.0, 160.0), (3300.0, 200.0)):
            r = np.exp(-np.pi * bw / 22050.0)
            den = np.convolve(den, [1.0, -2.0 * r * np.cos(2 * np.pi * fc / 22050.0), r * r])
        x = lfilter([1.0], den, src)[256:]
        x = x / np.max(np.abs(x)) + level * rng.standard_normal(L)
    elif kind == "sine1":
        x = np.sin(2 * np.pi * 440.0 / 22050.0 * n + 0.4) + 0.01 * rng.standard_normal(L)
    elif kind == "zero":
        x = np.zeros(L)
    elif kind == "constant":
        x = np.full(L, 0.25)
    else:
        raise ValueError(kind)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def clips(B: int, L: int) -> np.ndarray:
    """[B, L]: the signals in turn, a fresh seed each round."""
    return np.stack([clip(SIGNALS[b % len(SIGNALS)], L, b // len(SIGNALS)) for b in range(B)])


# (N, order, hop, center, B, L): every N of 3, 64, 65, 400, 1023, 1024, 2047, 2048; orders 1, 2, 16, 63, 64 and N - 2 for
# the small N; hops 1, 160, 512 and N; both centre rules; clips shorter than a frame; B of 1, 3 and 33
FRAME_CASES = (
    (3, 1, 1, True, 3, 40),
    (3, 1, 3, False, 1, 41),
    (64, 1, 64, True, 3, 300),
    (64, 2, 160, False, 3, 700),
    (64, 16, 1, True, 1, 90),
    (64, 62, 64, False, 3, 200),
    (65, 63, 65, True, 3, 400),
    (65, 16, 160, False, 1, 500),
    (400, 16, 160, True, 33, 1500),
    (400, 64, 400, False, 3, 1300),
    (400, 2, 512, True, 3, 300),            # clips shorter than a frame
    (1023, 16, 512, True, 3, 3000),
    (1023, 64, 1023, False, 1, 2100),
    (1024, 63, 512, True, 3, 2500),
    (1024, 32, 160, False, 3, 2000),
    (2047, 16, 2047, True, 3, 5000),
    (2047, 64, 512, False, 1, 4500),
    (2048, 32, 512, True, 6, 6000),         # the sine with 1 % noise at order 32 is row 5
    (2048, 64, 2048, False, 3, 4100),
    (2048, 1, 160, True, 3, 1000),          # clips shorter than a frame
    (2048, 16, 1, True, 1, 40),
)


def frame_case_clips(case) -> np.ndarray:
    N, order, hop, center, B, L = case
    return clips(B, L)


# (B, L, order) of the whole-row cases of the GPU tests (both methods; autocorr with the hann window of L points)
ROW_CASES = ((3, 2049, 1), (1, 2049, 16), (3, 2049, 64), (3, 4097, 1), (3, 4097, 16), (1, 4097, 64),
             (1, 100000, 1), (3, 100000, 16), (3, 100000, 64), (1, 1 << 20, 16))

# the end-to-end test: a clip of sygnals_amd.synth written as 16-bit PCM at 8 kHz and read back
E2E_SR, E2E_L = 8000, 6000
E2E_ROW_BURG_ORDER = 12                     # lpc(y, 12) and `dsp lpc --order 12` on the whole clip
E2E_ROW_AUTOCORR = (1500, 8)                # lpc(y[:1500], 8, method="autocorr"), hann
E2E_FRAMES = (400, 160, True, 12)           # lpc_batch(y, 12, 400, 160): frame_length, hop, center, order


@functools.lru_cache(maxsize=None)
def e2e_pcm() -> np.ndarray:
    from sygnals_amd import synth
    pcm = np.round(30000 * synth.synth_clips(1, E2E_L, E2E_SR, seed=3)[0]).astype(np.int16)
    pcm.setflags(write=False)
    return pcm


def e2e_clip() -> np.ndarray:
    """The float32 samples the WAV reader returns for e2e_pcm()."""
    return (e2e_pcm() / 32768.0).astype(np.float32)
