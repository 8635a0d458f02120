"""Float64 restatement of the cross-spectral functions and of generalised cross-correlation, the inputs and the parameter
sets of the GPU tests (tests/test_gpu_xspec.py).  tests/test_xspec_ref.py pins the restatement to scipy.signal.csd /
coherence / welch / correlate and asserts the conditions on the inputs."""
import numpy as np
import scipy.signal

from sygnals_amd._fftplan import conv_fft_len


# ------------------------------------------------------------------ restatement
def cross_spectra(x, y, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, detrend="constant", scaling="density"):
    """(freqs, Pxy, Pxx, Pyy, Cxy, S) of two 1-D rows by the explicit segment loop; S = the raw float64 sums
    (sum conj(X) Y, sum |X|^2, sum |Y|^2)."""
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    L = x.shape[0]
    nperseg = min(256 if nperseg is None else int(nperseg), L)
    nfft = nperseg if nfft is None else int(nfft)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    step = nperseg - noverlap
    nseg = (L - noverlap) // step
    w = scipy.signal.get_window(window, nperseg)
    scale = 1.0 / (fs * (w * w).sum()) if scaling == "density" else 1.0 / w.sum() ** 2
    F = nfft // 2 + 1
    idx = (np.arange(nseg) * step)[:, None] + np.arange(nperseg)[None, :]        # segment s starts at s * step
    spec = []
    for v in (x, y):
        seg = v[idx]
        if detrend not in (False, None):
            seg = scipy.signal.detrend(seg, type=detrend, axis=-1)               # per segment, per signal
        spec.append(np.fft.rfft(seg * w, nfft, axis=-1))                          # zero padding to nfft
    X, Y = spec
    sxy = (np.conj(X) * Y).sum(axis=0)
    sxx = (np.abs(X) ** 2).sum(axis=0)
    syy = (np.abs(Y) ** 2).sum(axis=0)
    one = np.full(F, 2.0)
    one[0] = 1.0
    if nfft % 2 == 0:
        one[-1] = 1.0
    m = scale * one / nseg
    with np.errstate(invalid="ignore", divide="ignore"):
        coh = np.abs(sxy) ** 2 / (sxx * syy)
    return np.fft.rfftfreq(nfft, 1 / fs), sxy * m, sxx * m, syy * m, coh, (sxy, sxx, syy)


def gcc(x, y, max_lag=None, weighting="none", n=None, dtype=np.float64):
    """(lags, r): r[t] = irfft(W X conj(Y), n)[t mod n]; n defaults to the device's transform length."""
    import scipy.fft
    x = np.asarray(x, dtype=dtype); y = np.asarray(y, dtype=dtype)
    if max_lag is None:
        max_lag = min(x.shape[0], y.shape[0]) - 1
    n = conv_fft_len(x.shape[0] + y.shape[0] - 1) if n is None else n
    G = scipy.fft.rfft(x, n) * np.conj(scipy.fft.rfft(y, n))
    if weighting == "phat":
        a = np.abs(G)
        G = np.where(a > 0, G / np.where(a > 0, a, 1), 0)
    r = scipy.fft.irfft(G, n)
    lags = np.arange(-max_lag, max_lag + 1, dtype=np.int64)
    return lags, r[lags % n]


def pick(r, lag0, fs=1.0):
    """(delay, lag, peak): the first maximum of r, refined by the parabola through its neighbours where it is interior and
    the parabola opens downwards (float64 arithmetic on the values as given)."""
    r = np.asarray(r)
    i = int(np.argmax(r))
    m = float(r[i])
    delta, pk = 0.0, m
    if 0 < i < r.shape[0] - 1:
        a, c = float(r[i - 1]), float(r[i + 1])
        den = a - 2.0 * m + c
        if den < 0.0:
            delta = 0.5 * (a - c) / den
            pk = m - 0.25 * (a - c) * delta
    return (lag0 + i + delta) / fs, lag0 + i, pk


# ------------------------------------------------------------------ inputs
def noise_pair(B, L, seed, offset=0.0, ramp=0.0, one_y=False):
    """Broadband pairs (float32): x = s + 0.5 n1, y = 0.8 s delayed by 3 samples + 0.5 n2, both with a DC offset and a ramp."""
    g = np.random.default_rng(seed)
    s = g.standard_normal((B, L + 3))
    t = np.arange(L) * ramp
    x = s[:, 3:] + 0.5 * g.standard_normal((B, L)) + offset + t
    y = 0.8 * s[:, :L] + 0.5 * g.standard_normal((B, L)) - offset + 0.5 * t
    if one_y:
        y = y[:1]
    return x.astype(np.float32), y.astype(np.float32)


def tone_pair(B, L, seed):
    """A tone with 1 % noise in both channels: the coherence is ill-conditioned in float32 (gated on the spectra only)."""
    g = np.random.default_rng(seed)
    n = np.arange(L)
    x = np.sin(0.05 * n)[None] + 0.01 * g.standard_normal((B, L))
    y = 0.7 * np.sin(0.05 * n + 0.4)[None] + 0.01 * g.standard_normal((B, L))
    return x.astype(np.float32), y.astype(np.float32)


def case_inputs(c):
    kind = c.get("input", "noise")
    if kind == "tone":
        return tone_pair(c["B"], c["L"], c["seed"])
    return noise_pair(c["B"], c["L"], c["seed"], c.get("offset", 0.0), c.get("ramp", 0.0), c.get("one_y", False))


def case_kw(c):
    return {k: c[k] for k in ("nperseg", "noverlap", "nfft", "detrend", "scaling") if k in c}


def _c(name, B, L, nperseg, coh, **kw):
    d = {"name": name, "B": B, "L": L, "nperseg": nperseg, "coh": coh, "seed": 1000 + len(name) * 7 + L % 97}
    d.update(kw)
    return d


# The fused form runs max(16, ceil(nseg / 2048)) consecutive segments per workgroup; the combine is cut into slices from
# 64 workgroups; the kernel has 64 threads up to nfft 512, 256 up to 2048 and 512 up to 8192.
# nperseg 16 at hop 8: L = 8 (nseg + 1).  coh: the coherence is gated (condition (a) is asserted for these).
FUSED_CASES = [
    _c("n8", 3, 100, 8, True),
    _c("n16_1seg", 1, 16, 16, False),
    _c("n16_2seg", 1, 24, 16, False),
    _c("n16_15seg", 1, 8 * 16, 16, True),
    _c("n16_16seg", 1, 8 * 17, 16, True),
    _c("n16_17seg", 1, 8 * 18, 16, True),
    _c("n16_40seg", 3, 8 * 41, 16, True),
    _c("n16_1100seg_slices", 1, 8 * 1101, 16, True),
    _c("n16_40000seg_long_runs", 1, 8 * 40001, 16, True),
    _c("n256_nov0", 1, 2000, 256, True, noverlap=0),
    _c("n256_default", 3, 2000, 256, True),
    _c("n256_nov255", 1, 2000, 256, True, noverlap=255),
    _c("n256_none_offset", 3, 2000, 256, False, detrend=False, offset=3.0, ramp=1e-4),
    _c("n256_constant_offset", 3, 2000, 256, True, detrend="constant", offset=3.0, ramp=1e-4),
    _c("n256_linear_offset", 3, 2000, 256, True, detrend="linear", offset=3.0, ramp=1e-4),
    _c("n256_spectrum", 1, 2000, 256, True, scaling="spectrum", offset=3.0, ramp=1e-4),
    _c("n100_in_128", 3, 1000, 100, True, nfft=128, detrend="linear", offset=3.0, ramp=1e-4),
    _c("n512", 1, 3000, 512, True),
    _c("n1024", 3, 6000, 1024, True, offset=3.0, ramp=1e-4),
    _c("n600_in_1024", 1, 6000, 600, True, nfft=1024, detrend="linear", scaling="spectrum"),
    _c("n2048", 1, 12000, 2048, True),
    _c("n4096", 1, 30000, 4096, True),
    _c("n8192", 2, 8192 * 6, 8192, True, offset=3.0, ramp=1e-5),
    _c("n5000_in_8192", 1, 30000, 5000, True, nfft=8192, detrend="linear"),
    _c("n8192_tone", 1, 8192 * 3, 8192, False, input="tone"),
    _c("n256_B33", 33, 2000, 256, True),
    _c("n256_B33_one_y", 33, 2000, 256, True, one_y=True),
]

ROWS_CASES = [
    _c("r12", 2, 400, 12, True),
    _c("r12_in_20", 1, 400, 12, True, nfft=20, detrend="linear", offset=3.0, ramp=1e-4),
    _c("r12_in_15_odd", 1, 400, 12, True, nfft=15),
    _c("r100", 2, 1500, 100, True, noverlap=30),
    _c("r100_in_150", 1, 1500, 100, True, nfft=150, scaling="spectrum"),
    _c("r101_odd", 1, 1500, 101, True, detrend=False),
    _c("r1000", 1, 8000, 1000, True),
    _c("r1000_in_1500", 2, 8000, 1000, True, nfft=1500, one_y=True),
    _c("r16384", 1, 16384 * 6, 16384, True),
]

ALL_CASES = FUSED_CASES + ROWS_CASES


# ------------------------------------------------------------------ GCC inputs
def delayed_pair(B, Lx, Ly, delays, seed, one_y=True):
    """y: noise rows [1 or B, Ly]; x[b][n] = y[n - d_b] (zero outside) + 0.1 noise, float32: the peak of r is at lag +d_b"""
    g = np.random.default_rng(seed)
    y = g.standard_normal((1 if one_y else B, Ly))
    x = np.zeros((B, Lx))
    for b in range(B):
        d = delays[b % len(delays)]
        src = y[0 if one_y else b]
        n = np.arange(Lx)
        k = n - d
        ok = (k >= 0) & (k < Ly)
        x[b, ok] = src[k[ok]]
    x += 0.1 * g.standard_normal((B, Lx))
    return x.astype(np.float32), y.astype(np.float32)


def _g(name, B, Lx, Ly, delays, max_lag, one_y=True):
    return {"name": name, "B": B, "Lx": Lx, "Ly": Ly, "delays": delays, "max_lag": max_lag, "one_y": one_y,
            "seed": 77 + Lx % 1013 + B}


GCC_CASES = [
    _g("L300", 1, 300, 300, [7], None),
    _g("L300_lag1", 1, 300, 300, [0], 1),
    _g("L1000_B3", 3, 1000, 1000, [0, 7, -33], 64),
    _g("L1000_d250", 1, 1000, 1000, [250], 999),
    _g("L4097", 1, 4097, 4097, [-33], 64),
    _g("L65536", 1, 65536, 65536, [250], 65535),
    _g("Lx700_Ly1000", 3, 700, 1000, [7, -33, 250], None, one_y=False),
    _g("L1000_B33", 33, 1000, 1000, [0, 7, -33, 250], 300),
]


def gcc_inputs(c):
    return delayed_pair(c["B"], c["Lx"], c["Ly"], c["delays"], c["seed"], c["one_y"])
