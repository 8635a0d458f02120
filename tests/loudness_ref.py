"""Float64 restatement of the loudness meter (ITU-R BS.1770-4, EBU R128 / Tech 3341 / Tech 3342): the contract of
csrc/loudness.hip.  No loudness library is a dependency; tests/test_loudness_ref.py pins this file to the standards' known
answers.  NumPy / SciPy only, one clip [C, L] (or [L]) at a time.

What is fixed here beyond the standards' text:
  * the K-weighting filters are redesigned per rate (sygnals_amd/_loudness.py); at 48 kHz they are BS.1770's table;
  * segments are s_j = j fs div 10, blocks are 4 and 30 segments, and a row of L samples has 10 L div fs whole segments
    (where fs is no multiple of 10 that may be one fewer than the blocks that would fit);
  * the loudness range's percentiles are nearest ranks, floor((n - 1) p + 1/2), taken in integers;
  * true peak is max |scipy.signal.resample_poly(x, up, 1)| with SciPy's default filter, not Annex 2's 48-tap table."""
import numpy as np
from scipy.signal import resample_poly, sosfilt

from sygnals_amd import _loudness as LD


def clip2(x):
    x = np.asarray(x, dtype=np.float64)
    return x[None, :] if x.ndim == 1 else x


def segment_powers(x, fs):
    """[C, n_seg] float64: sum of the squared K-weighted signal over every whole 100 ms segment."""
    x = clip2(x)
    n_seg = LD.n_segments(x.shape[1], fs)
    y = sosfilt(LD.k_weighting_sos(fs), x, axis=1)
    s = [LD.segment_start(j, fs) for j in range(n_seg + 1)]
    return np.array([[np.sum(y[c, s[j]:s[j + 1]] ** 2) for j in range(n_seg)] for c in range(x.shape[0])]).reshape(x.shape[0], n_seg)


def block_powers(seg, fs, K, weights=None):
    """z [n_blocks]: weighted mean square of the blocks of K segments."""
    C, n_seg = seg.shape
    w = LD.channel_weights(C, weights)
    nb = max(0, n_seg - (K - 1))
    z = np.zeros(nb)
    for j in range(nb):
        z[j] = np.dot(w, seg[:, j:j + K].sum(axis=1)) / (LD.segment_start(j + K, fs) - LD.segment_start(j, fs))
    return z


def lufs(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(z > 0, LD.OFFSET + 10.0 * np.log10(np.where(z > 0, z, 1.0)), -np.inf)


def momentary(x, fs, weights=None):
    return lufs(block_powers(segment_powers(x, fs), fs, LD.MOMENTARY, weights))


def short_term(x, fs, weights=None):
    return lufs(block_powers(segment_powers(x, fs), fs, LD.SHORT_TERM, weights))


def gates(z, below):
    """(l, absolute mask, relative threshold): the threshold is +inf where no block passes the absolute gate."""
    l = lufs(z)
    m = l > LD.ABSOLUTE_GATE
    thr = float(lufs(z[m].mean())) - below if m.any() else np.inf
    return l, m, thr


def integrated(x, fs, weights=None):
    z = block_powers(segment_powers(x, fs), fs, LD.MOMENTARY, weights)
    l, m, gamma = gates(z, 10.0)
    keep = m & (l > gamma)
    return float(lufs(z[keep].mean())) if keep.any() else -np.inf


def loudness_range(x, fs, weights=None):
    z = block_powers(segment_powers(x, fs), fs, LD.SHORT_TERM, weights)
    l, m, thr = gates(z, 20.0)
    v = np.sort(l[m & (l > thr)])
    if v.size < 2:
        return 0.0
    lo, hi = LD.lra_ranks(v.size)
    return float(v[hi] - v[lo])


def gate_margin(x, fs, weights=None):
    """Least distance (LU) of a momentary block from -70 and from the relative gate, and of a short-term value from
    the loudness range's two thresholds: the device must pick the reference's sets where this is comfortably positive."""
    seg = segment_powers(x, fs)
    d = [np.inf]
    for K, below in ((LD.MOMENTARY, 10.0), (LD.SHORT_TERM, 20.0)):
        l, m, thr = gates(block_powers(seg, fs, K, weights), below)
        fin = l[np.isfinite(l)]
        d.append(np.min(np.abs(fin - LD.ABSOLUTE_GATE), initial=np.inf))
        if np.isfinite(thr):
            d.append(np.min(np.abs(fin - thr), initial=np.inf))
    return float(min(d))


def true_peak(x, fs):
    """Linear true peak: the largest |value| of every channel oversampled by LD.true_peak_up(fs)."""
    x = clip2(x)
    up = LD.true_peak_up(fs)
    if up == 1:
        return float(np.max(np.abs(x)))
    return float(np.max(np.abs(resample_poly(x, up, 1, axis=1, padtype="constant"))))


def dbtp(tp):
    with np.errstate(divide="ignore"):
        return float(20.0 * np.log10(tp)) if tp > 0 else -np.inf


def gain(I, tp, target, limit_dbtp=None):
    if not np.isfinite(I):
        return 1.0
    g = 10.0 ** ((target - I) / 20.0)
    if limit_dbtp is not None and g * tp > 10.0 ** (limit_dbtp / 20.0):
        g = 10.0 ** (limit_dbtp / 20.0) / tp
    return g


def normalize(x, fs, target=-23.0, limit_dbtp=None, weights=None):
    """(float32 clip scaled, gain, I)."""
    x32 = np.asarray(x, dtype=np.float32)
    I = integrated(x32, fs, weights)
    g = gain(I, true_peak(x32, fs) if limit_dbtp is not None else 0.0, target, limit_dbtp)
    return (x32.astype(np.float64) * g).astype(np.float32), g, I
