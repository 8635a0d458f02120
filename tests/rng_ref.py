"""Float64 NumPy restatement of the device noise generator: the contract of sygnals_amd/csrc/rng_dev.h, rng.hip and
sygnals_amd/_rng.py, with which it shares no code.

Philox4x32-10 (Random123): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds, the key
bumped between rounds; per round (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).
key = (seed low, seed high); counter = (q low, q high, row, stream), q = n // 4; stream 0 noise samples, 1 per-row draws.
u(w) = (2 (w >> 9) + 1) 2^-24; z[4q] = r cos t, z[4q + 1] = r sin t, r = sqrt(-2 ln u(w0)), t = 2 pi u(w1); z[4q + 2],
z[4q + 3] the same from (w2, w3).
Coloured noise: irfft(rfft(w) g, M)[:L], M the smallest power of two >= max(L, 2), g[0] = 0, g[k] = k^(-alpha / 2); at
alpha = 0 the gain is 1 everywhere (0^0 = 1); a row of one sample is zero."""
import numpy as np

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _mulhilo(m, x):
    """64-bit product of the constant m and the uint32 values x (held in uint64) as (high word, low word)."""
    p = np.uint64(m) * x
    return p >> np.uint64(32), p & np.uint64(0xFFFFFFFF)


def philox(counter, key):
    """counter [n, 4], key [n, 2] or [2] (anything that converts to unsigned integers) -> uint32 [n, 4]."""
    ctr = np.asarray(counter, dtype=np.uint64).reshape(-1, 4).T.copy()
    ky = np.asarray(key, dtype=np.uint64).reshape(-1, 2).T
    ky = np.repeat(ky, ctr.shape[1], axis=1) if ky.shape[1] == 1 and ctr.shape[1] > 1 else ky.copy()
    for rnd in range(10):
        k0 = (ky[0] + np.uint64(rnd) * np.uint64(0x9E3779B9)) % np.uint64(1 << 32)
        k1 = (ky[1] + np.uint64(rnd) * np.uint64(0xBB67AE85)) % np.uint64(1 << 32)
        hi0, lo0 = _mulhilo(0xD2511F53, ctr[0])
        hi1, lo1 = _mulhilo(0xCD9E8D57, ctr[2])
        ctr = np.stack([hi1 ^ ctr[1] ^ k0, lo1, hi0 ^ ctr[3] ^ k1, lo0])
    return ctr.T.astype(np.uint32)


def words(seed, row, q, stream=0):
    """uint32 [len(q), 4]: the calls q (Python ints or an integer array) of (seed, row) in `stream`."""
    q = np.atleast_1d(np.asarray(q, dtype=np.uint64))
    ctr = np.zeros((len(q), 4), dtype=np.uint64)
    ctr[:, 0] = q % np.uint64(1 << 32)
    ctr[:, 1] = q // np.uint64(1 << 32)
    ctr[:, 2] = row
    ctr[:, 3] = stream
    return philox(ctr, (seed % (1 << 32), seed // (1 << 32)))


def unit(w):
    return (2.0 * (np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def normals(seed, row, count, start=0):
    """float64 [count]: samples start .. start + count - 1 of (seed, row)."""
    q_first, q_last = start // 4, (start + count - 1) // 4
    w = words(seed, row, np.arange(q_first, q_last + 1, dtype=np.uint64))
    z = np.empty((len(w), 4))
    for j in (0, 2):
        r = np.sqrt(-2.0 * np.log(unit(w[:, j])))
        t = 2.0 * np.pi * unit(w[:, j + 1])
        z[:, j], z[:, j + 1] = r * np.cos(t), r * np.sin(t)
    return z.reshape(-1)[start - 4 * q_first:start - 4 * q_first + count]


def normal_rows(seed, first_row, B, L, start=0):
    return np.stack([normals(seed, first_row + b, L, start) for b in range(B)])


def fft_len(L):
    M = 2
    while M < L:
        M *= 2
    return M


def colored(seed, row, L, alpha):
    if L == 1:
        return np.zeros(1)
    M = fft_len(L)
    g = np.zeros(M // 2 + 1)
    g[1:] = np.arange(1, M // 2 + 1, dtype=np.float64) ** (-alpha / 2.0)
    if alpha == 0:
        g[0] = 1.0
    return np.fft.irfft(np.fft.rfft(normals(seed, row, M)) * g, M)[:L]


def colored_rows(seed, first_row, B, L, alpha):
    return np.stack([colored(seed, first_row + b, L, alpha) for b in range(B)])


def snr_draws(seed, first_row, B, lo, hi):
    """Row r: lo + (hi - lo) (w0 + 0.5) 2^-32, w0 the first word of counter (0, 0, first_row + r, stream 1)."""
    w0 = np.array([int(words(seed, first_row + b, [0], stream=1)[0, 0]) for b in range(B)], dtype=np.float64)
    return lo + (hi - lo) * (w0 + 0.5) / 2.0 ** 32


def octave_slope(x, k_lo=8, k_hi=16384):
    """Slope in dB per octave of a line through the mean power of the octave bands [k, 2k), k = k_lo .. k_hi / 2, of the
    one-sided spectrum of x, against the bands' log2 geometric centre."""
    P = np.abs(np.fft.rfft(np.asarray(x, dtype=np.float64))) ** 2
    xs, ys = [], []
    k = k_lo
    while 2 * k <= k_hi:
        xs.append(np.log2(k * np.sqrt(2.0)))
        ys.append(10.0 * np.log10(np.mean(P[k:2 * k])))
        k *= 2
    return float(np.polyfit(xs, ys, 1)[0])


def moments(z):
    """Deviations in standard errors of (mean, variance, third moment, fourth moment - 3) of a standard normal sample."""
    L = len(z)
    return np.array([np.mean(z) * np.sqrt(L), (np.mean(z ** 2) - 1.0) / np.sqrt(2.0 / L), np.mean(z ** 3) / np.sqrt(15.0 / L),
                     (np.mean(z ** 4) - 3.0) / np.sqrt(96.0 / L)])


def autocorr(z, lag):
    """Lag autocorrelation of z in standard errors 1 / sqrt(L)."""
    return float(np.mean(z[:-lag] * z[lag:]) * np.sqrt(len(z)))
