"""Float64 restatement of the cepstral analysis the device computes (sygnals_amd/csrc/cepstrum.hip): NumPy only.

No library fixes these definitions (SciPy has no cepstrum); tests/test_cepstrum_ref.py pins them by construction.  Inputs
are float32 values promoted to float64.

    real      c = ifft(log(max(|X|, amin))).real,                      X = fft(x, n)
    complex   c = ifft(log(max(|X|, amin)) + i phi_u).real             phi_u: the unwrapped phase without its linear term
    inverse   x = ifft(exp(Re Xh + i (Im Xh + pi ndelay k / center))).real,   Xh = fft(c)
"""
import numpy as np

AMIN = 1e-5
THRESHOLD = 0.13


def _row(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def spectrum(x, n=None):
    x = _row(x)
    n = x.shape[-1] if n is None else int(n)
    return np.fft.fft(x, n, axis=-1)


def log_magnitude(X, amin=AMIN):
    with np.errstate(divide="ignore"):
        return np.log(np.maximum(np.abs(X), amin))


def real_cepstrum(x, n=None, amin=AMIN):
    """c [n] of one row (or of every row of [B, L])."""
    return np.fft.ifft(log_magnitude(spectrum(x, n), amin), axis=-1).real


def phase(X):
    """angle(X), except bin 0: 0 for Re X[0] >= 0, else +pi (the sign of a zero imaginary part decides nothing)."""
    phi = np.angle(X)
    phi[0] = 0.0 if X[0].real >= 0 else np.pi
    return phi


def wrap_counts(phi):
    """np.unwrap's correction of every step as an integer count of 2 pi: M[0] = 0, M[k] = -1 for a step above pi, +1 for
    one below -pi, 0 otherwise -- np.unwrap leaves a step of exactly +-pi alone (its -pi / d > 0 tie rule)."""
    d = np.diff(phi)
    M = np.zeros(phi.shape[0], dtype=np.int64)
    M[1:] = np.where(d > np.pi, -1, np.where(d < -np.pi, 1, 0))
    return M


def unwrap_margin(phi):
    """min_k (pi - |phi[k] - phi[k-1] wrapped into (-pi, pi]|): how far the closest step is from changing its count."""
    d = np.diff(phi)
    d = d - 2 * np.pi * np.round(d / (2 * np.pi))
    return float(np.min(np.pi - np.abs(d))) if d.size else np.pi


def unwrapped_phase(X):
    """(phi_u before the linear term is taken out, ndelay, center)."""
    phi = phase(X)
    phi_u = phi + 2 * np.pi * np.cumsum(wrap_counts(phi))
    center = (X.shape[0] + 1) // 2
    ndelay = int(np.rint(phi_u[center] / np.pi))
    return phi_u, ndelay, center


def complex_cepstrum(x, n=None, amin=AMIN):
    """(c [n], ndelay) of one row, n >= 2."""
    X = spectrum(x, n)
    phi_u, ndelay, center = unwrapped_phase(X)
    phi_u = phi_u - np.pi * ndelay * np.arange(X.shape[0]) / center
    return np.fft.ifft(log_magnitude(X, amin) + 1j * phi_u).real, ndelay


def inverse_complex_cepstrum(c, ndelay):
    """Exact for even n at any ndelay; for odd n only at ndelay = 0 (the ramp is then no circular shift)."""
    c = np.asarray(c, dtype=np.float64)
    n = c.shape[0]
    Xh = np.fft.fft(c)
    center = (n + 1) // 2
    return np.fft.ifft(np.exp(Xh.real + 1j * (Xh.imag + np.pi * ndelay * np.arange(n) / center))).real


# ------------------------------------------------------------------ frames
def analysis_window(window, win_length, n_fft):
    """The window of compute_stft: a name (periodic hann, ones for 'boxcar' / 'ones') or an array of win_length values,
    centre-padded with zeros to n_fft."""
    win_length = n_fft if win_length is None else int(win_length)
    if isinstance(window, str):
        if window == "hann":
            w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)
        elif window in ("boxcar", "ones", "rectangular"):
            w = np.ones(win_length)
        else:
            raise ValueError(f"cepstrum_ref: window {window!r} is not restated here")
    else:
        w = np.asarray(window, dtype=np.float64)
        if w.shape != (win_length,):
            raise ValueError("window array must have win_length values")
    w = w.astype(np.float32).astype(np.float64)                      # the device holds the window in float32
    lp = (n_fft - win_length) // 2
    out = np.zeros(n_fft)
    out[lp:lp + win_length] = w
    return out


def num_frames(L, n_fft, hop, center):
    """The count of compute_stft on the zero-padded clip (librosa's)."""
    if center:
        return 1 + (L + 2 * (n_fft // 2) - n_fft) // hop
    return 1 + (L - n_fft) // hop if L >= n_fft else 0


def frames(y, n_fft=2048, hop=512, center=True, window="hann", win_length=None):
    """Windowed frames [T, n_fft] of one clip, float64."""
    y = _row(y)
    L = y.shape[0]
    T = num_frames(L, n_fft, hop, center)
    if T < 1:
        raise ValueError("signal too short for one frame")
    pad = n_fft // 2 if center else 0
    yp = np.zeros(L + 2 * pad + n_fft)
    yp[pad:pad + L] = y
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return yp[idx] * analysis_window(window, win_length, n_fft)[None, :]


def cepstrogram(y, n_fft=2048, hop=512, center=True, window="hann", win_length=None, n_ceps=None, amin=AMIN):
    """[Q, T] of one clip; also returns K [T], the gate's scale per frame."""
    xw = frames(y, n_fft, hop, center, window, win_length)
    Q = n_fft // 2 + 1 if n_ceps is None else int(n_ceps)
    if not 1 <= Q <= n_fft:
        raise ValueError("n_ceps outside 1 ... n_fft")
    X = np.fft.fft(xw, axis=-1)
    c = np.fft.ifft(log_magnitude(X, amin), axis=-1).real
    return c[:, :Q].T.copy(), gate_scale(xw, X, amin)


def gate_scale(xw, X, amin=AMIN):
    """K = mean over all n bins of ||xw||_1 / max(|X_k|, amin) (>= 1), per row."""
    l1 = np.abs(xw).sum(axis=-1, keepdims=True)
    K = np.mean(l1 / np.maximum(np.abs(X), amin), axis=-1)
    return np.maximum(K, 1.0)


def row_gate_scale(x, n=None, amin=AMIN):
    x = _row(x)
    n = x.shape[-1] if n is None else int(n)
    xs = x[..., :n]
    return gate_scale(xs, np.fft.fft(xs, n, axis=-1), amin)


# ------------------------------------------------------------------ pitch
def quefrency_range(sr, fmin, fmax, n_fft):
    qmin = int(np.ceil(sr / fmax))
    qmax = min(int(np.floor(sr / fmin)), n_fft // 2 - 1)
    if qmin < 1 or qmin > qmax:
        raise ValueError(f"cepstral pitch: fmin={fmin}, fmax={fmax} at sr={sr} leave no quefrency range (qmin={qmin}, qmax={qmax})")
    return qmin, qmax


def peaks(c, qmin, qmax, sr, threshold=THRESHOLD):
    """c [Q, T] float32 values -> (f0 [T] float64 with NaN unvoiced, strength [T], qstar [T], voiced [T] bool)."""
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    T = c.shape[1]
    f0 = np.full(T, np.nan)
    strength = np.zeros(T)
    qstar = np.zeros(T, dtype=np.int64)
    voiced = np.zeros(T, dtype=bool)
    for t in range(T):
        q = qmin + int(np.argmax(c[qmin:qmax + 1, t]))
        delta = 0.0
        if qmin < q < qmax:
            den = c[q - 1, t] - 2.0 * c[q, t] + c[q + 1, t]
            if den < 0:
                delta = 0.5 * (c[q - 1, t] - c[q + 1, t]) / den
        strength[t], qstar[t] = c[q, t], q
        voiced[t] = c[q, t] >= threshold
        if voiced[t]:
            f0[t] = sr / (q + delta)
    return f0, strength, qstar, voiced
