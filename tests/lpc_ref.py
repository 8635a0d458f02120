"""The float64 restatement of linear prediction that sygnals_amd's LPC kernels are held to (csrc/lpc.hip): Burg's method
as librosa.lpc computes it, in both forms of its denominator, the autocorrelation method with a Levinson-Durbin recursion,
the step-up from reflection coefficients to predictor coefficients, and the all-pole envelope.  NumPy only."""
import numpy as np

TINY = np.finfo(np.float64).tiny


def framing(L: int, N: int, hop: int, center: bool):
    """(T, pad): the frame count and left padding of ops.cepstrogram_frames; frame t starts at t hop - pad."""
    pow2 = N >= 8 and (N & (N - 1)) == 0
    if center:
        T = 1 + L // hop if pow2 else 1 + (L + 2 * (N // 2) - N) // hop
    else:
        T = 1 + (L - N) // hop if L >= N else 0
    return T, (N // 2 if center else 0)


def frames_of(y, N: int, hop: int, center: bool, window=None) -> np.ndarray:
    """[T, N] float64: the frames of the clip y (float32), zero outside it, times the float32 window table."""
    y = np.asarray(y)
    L = y.shape[0]
    T, pad = framing(L, N, hop, center)
    out = np.zeros((max(T, 0), N), dtype=np.float64)
    for t in range(T):
        s0 = t * hop - pad
        lo, hi = max(s0, 0), min(s0 + N, L)
        if hi > lo:
            out[t, lo - s0:hi - s0] = y[lo:hi].astype(np.float64)
    if window is not None:
        out *= np.asarray(window, dtype=np.float32).astype(np.float64)[None, :]
    return out


def step_up(k) -> np.ndarray:
    """Reflection coefficients k[0 .. p-1] -> a[0 .. p], a[0] = 1: a_new[j] = a[j] + k_i a[i + 1 - j]."""
    k = np.asarray(k, dtype=np.float64)
    a = np.zeros(k.shape[0] + 1, dtype=np.float64)
    a[0] = 1.0
    for i, ki in enumerate(k):
        prev = a[:i + 2].copy()
        a[:i + 2] = prev + ki * prev[::-1]
    return a


def burg(x, order: int, carry_den: bool = False):
    """(a [p + 1], k [p], err): Burg's recurrence on the float64 frame x.  carry_den=False sums the denominator again at
    every stage; True carries it forward as librosa.lpc does, den <- (1 - k^2) den - f_new[0]^2 - b_new[-1]^2."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    if not 1 <= order <= N - 2:
        raise ValueError("order outside 1 ... N - 2")
    f, b = x[1:].copy(), x[:-1].copy()
    a = np.zeros(order + 1, dtype=np.float64)
    a[0] = 1.0
    k = np.zeros(order, dtype=np.float64)
    den = np.sum(f * f + b * b)
    for i in range(order):
        if not carry_den:
            den = np.sum(f * f + b * b)
        k[i] = -2.0 * np.sum(f * b) / (den + TINY)
        prev = a[:i + 2].copy()
        a[:i + 2] = prev + k[i] * prev[::-1]
        fn, bn = f + k[i] * b, b + k[i] * f
        if carry_den:
            den = (1.0 - k[i] * k[i]) * den - fn[0] ** 2 - bn[-1] ** 2
        f, b = fn[1:], bn[:-1]
    err = np.sum(f * f + b * b) / (2.0 * (N - 1 - order))
    return a, k, err


def autocorrelation(xw, order: int) -> np.ndarray:
    """r[l] = sum_n xw[n] xw[n + l], l = 0 .. p (biased, not normalised)."""
    xw = np.asarray(xw, dtype=np.float64)
    N = xw.shape[0]
    return np.array([np.dot(xw[:N - l], xw[l:]) for l in range(order + 1)], dtype=np.float64)


def levinson(r):
    """(a [p + 1], k [p]) of the Toeplitz system R a[1:] = -r[1:]; r[0] = 0 gives a = [1, 0, ...]."""
    r = np.asarray(r, dtype=np.float64)
    p = r.shape[0] - 1
    a = np.zeros(p + 1, dtype=np.float64)
    a[0] = 1.0
    k = np.zeros(p, dtype=np.float64)
    if r[0] == 0.0:
        return a, k
    E = r[0]
    for i in range(p):
        acc = r[i + 1] + np.dot(a[1:i + 1], r[i:0:-1])
        k[i] = -acc / E if E > 0.0 else 0.0
        prev = a[:i + 2].copy()
        a[:i + 2] = prev + k[i] * prev[::-1]
        E *= 1.0 - k[i] * k[i]
    return a, k


def autocorr(xw, order: int):
    """(a, k, err, r) of the autocorrelation method on the windowed float64 frame xw; err = (r[0] + sum_j a[j] r[j]) / N."""
    r = autocorrelation(xw, order)
    a, k = levinson(r)
    err = (r[0] + np.dot(a[1:], r[1:])) / np.asarray(xw).shape[0]
    return a, k, err, r


def transfer(a, n_fft: int) -> np.ndarray:
    """A(e^{-2 pi i k / n_fft}) = sum_j a[j] e^{-2 pi i j k / n_fft}, k = 0 .. n_fft / 2, complex128."""
    a = np.asarray(a, dtype=np.float64)
    kk = np.arange(n_fft // 2 + 1, dtype=np.float64)
    ang = -2.0 * np.pi * np.outer(kk, np.arange(a.shape[0], dtype=np.float64)) / n_fft
    return np.exp(1j * ang) @ a


def envelope(a, err, n_fft: int, db: bool = False, amin: float = 1e-10) -> np.ndarray:
    """P[k] = err / |A|^2, or 10 log10(max(P, amin))."""
    P = err / np.abs(transfer(a, n_fft)) ** 2
    return 10.0 * np.log10(np.maximum(P, amin)) if db else P
