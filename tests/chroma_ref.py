"""Float64 restatement of librosa 0.10.1's tonal features: filters.chroma, filters.cq_to_chroma, util.normalize,
feature.chroma_stft / chroma_cqt / chroma_cens / tonnetz, piptrack, pitch_tuning and estimate_tuning.

librosa is not a dependency; this file is the contract the device kernels are held to ("parity unpinned").  Everything is
NumPy float64 whatever the input's type; scipy.ndimage.convolve and scipy.signal.convolve are called directly where
librosa calls them.  Spectrograms are in librosa's layout, [F, T] / [K, T] / [n_chroma, T].  The transforms themselves
(STFT, CQT) are not restated here: callers pass S or C (oracle.cpu_ref.stft / .cqt, or what the device computed)."""
import warnings

import numpy as np
import scipy.ndimage
import scipy.signal

TINY = float(np.finfo(np.float32).tiny)
C1_HZ = 440.0 * 2.0 ** ((24 - 69) / 12.0)                 # note_to_hz("C1")
QUANT_STEPS = (0.4, 0.2, 0.1, 0.05)


def hz_to_octs(f, tuning=0.0, bins_per_octave=12):
    a440 = 440.0 * 2.0 ** (tuning / bins_per_octave)
    return np.log2(np.asarray(f, dtype=np.float64) / (a440 / 16.0))


def hz_to_midi(f):
    return 12.0 * (np.log2(np.asarray(f, dtype=np.float64)) - np.log2(440.0)) + 69.0


def normalize(x, norm=np.inf, axis=-2):
    x = np.asarray(x, dtype=np.float64)
    if norm is None:
        return x
    mag = np.abs(x)
    if norm == np.inf:
        length = np.max(mag, axis=axis, keepdims=True)
    elif norm == 1:
        length = np.sum(mag, axis=axis, keepdims=True)
    elif norm == 2:
        length = np.sqrt(np.sum(mag ** 2, axis=axis, keepdims=True))
    else:
        raise ValueError(f"unsupported norm {norm!r}")
    length = np.where(length < TINY, 1.0, length)
    return x / length


def filters_chroma(sr, n_fft, n_chroma=12, tuning=0.0, ctroct=5.0, octwidth=2, norm=2, base_c=True, dtype=np.float32):
    fr = np.linspace(0, sr, n_fft, endpoint=False)[1:]
    fb = n_chroma * hz_to_octs(fr, tuning, n_chroma)
    fb = np.concatenate(([fb[0] - 1.5 * n_chroma], fb))
    bw = np.concatenate((np.maximum(fb[1:] - fb[:-1], 1.0), [1]))
    D = np.subtract.outer(fb, np.arange(0, n_chroma, dtype="d")).T
    n2 = np.round(float(n_chroma) / 2)
    D = np.remainder(D + n2 + 10 * n_chroma, n_chroma) - n2
    w = np.exp(-0.5 * (2 * D / np.tile(bw, (n_chroma, 1))) ** 2)
    w = normalize(w, norm=norm, axis=0)
    if octwidth is not None:
        w = w * np.tile(np.exp(-0.5 * (((fb / n_chroma - ctroct) / octwidth) ** 2)), (n_chroma, 1))
    if base_c:
        w = np.roll(w, -3 * (n_chroma // 12), axis=0)
    return np.ascontiguousarray(w[:, :int(1 + n_fft / 2)], dtype=dtype)


def cq_to_chroma(n_input, bins_per_octave=12, n_chroma=12, fmin=None, window=None, base_c=True, dtype=np.float32):
    n_merge = float(bins_per_octave) / n_chroma
    if fmin is None:
        fmin = C1_HZ
    if np.mod(n_merge, 1) != 0:
        raise ValueError("Incompatible CQ merge: input bins must be an integer multiple of output bins.")
    w = np.repeat(np.eye(n_chroma), int(n_merge), axis=1)
    w = np.roll(w, -int(n_merge // 2), axis=1)
    w = np.tile(w, int(np.ceil(float(n_input) / bins_per_octave)))[:, :n_input]
    midi_0 = np.mod(hz_to_midi(fmin), 12)
    roll = midi_0 if base_c else midi_0 - 9
    w = np.roll(w, int(np.round(roll * (n_chroma / 12.0))), axis=0).astype(dtype)
    if window is not None:
        w = scipy.signal.convolve(w, np.atleast_2d(window), mode="same")
    return w


def chroma_stft(S, sr=22050, norm=np.inf, n_fft=None, tuning=None, n_chroma=12, **kwargs):
    """S: the power spectrogram [F, T].  The table enters as librosa applies it: rounded to float32."""
    S = np.asarray(S, dtype=np.float64)
    if n_fft is None or n_fft // 2 + 1 != S.shape[0]:
        n_fft = 2 * (S.shape[0] - 1)
    if tuning is None:
        tuning = estimate_tuning(S=S, sr=sr, n_fft=n_fft, bins_per_octave=n_chroma)
    fb = filters_chroma(sr, n_fft, n_chroma=n_chroma, tuning=tuning, **kwargs).astype(np.float64)
    return normalize(fb @ S, norm=norm, axis=-2)


def chroma_cqt(C, norm=np.inf, threshold=0.0, n_chroma=12, bins_per_octave=36, fmin=None, window=None):
    """C: the CQT magnitude [K, T] (computed with the tuning the caller chose)."""
    C = np.asarray(C, dtype=np.float64)
    if bins_per_octave is None:
        bins_per_octave = n_chroma
    w = cq_to_chroma(C.shape[0], bins_per_octave, n_chroma, fmin, window).astype(np.float64)
    chroma = w @ C
    if threshold is not None:
        chroma[chroma < threshold] = 0.0
    if norm is not None:
        chroma = normalize(chroma, norm=norm, axis=-2)
    return chroma


def cens_from_chroma(chroma, norm=2, win_len_smooth=41, smoothing_window="hann"):
    """chroma_cens after its chroma_cqt(norm=None)."""
    chroma = normalize(np.asarray(chroma, dtype=np.float64), norm=1, axis=-2)
    q = np.zeros_like(chroma)
    for step in QUANT_STEPS:
        q += (chroma > step) * 0.25
    if win_len_smooth:
        win = scipy.signal.get_window(smoothing_window, win_len_smooth + 2, fftbins=False)
        win = win / np.sum(win)
        cens = scipy.ndimage.convolve(q, win[None, :], mode="constant")
    else:
        cens = q
    return normalize(cens, norm=norm, axis=-2)


def cens_margin(chroma):
    """The least distance of an L1-normalised entry from a quantiser step."""
    n = normalize(np.asarray(chroma, dtype=np.float64), norm=1, axis=-2)
    return float(min(np.min(np.abs(n - s)) for s in QUANT_STEPS))


def chroma_cens(C, norm=2, win_len_smooth=41, smoothing_window="hann", **kwargs):
    return cens_from_chroma(chroma_cqt(C, norm=None, **kwargs), norm, win_len_smooth, smoothing_window)


def tonnetz_phi(n_chroma=12):
    dim = np.linspace(0, 12, num=n_chroma, endpoint=False)
    V = np.multiply.outer([7.0 / 6, 7.0 / 6, 3.0 / 2, 3.0 / 2, 2.0 / 3, 2.0 / 3], dim)
    V[::2] -= 0.5
    return np.array([1, 1, 1, 1, 0.5, 0.5])[:, None] * np.cos(np.pi * V)


def tonnetz(chroma):
    chroma = np.asarray(chroma, dtype=np.float64)
    return tonnetz_phi(chroma.shape[-2]) @ normalize(chroma, norm=1, axis=-2)


def _rel(a, b):
    """Relative margin of a comparison between a and b."""
    d = max(abs(a), abs(b))
    return abs(a - b) / d if d > 0 else np.inf


def piptrack(S, sr=22050, n_fft=None, fmin=150.0, fmax=4000.0, threshold=0.1, margins=None):
    """(pitches, mags) float64 [F, T] of the magnitude spectrogram S [F, T].  margins (a dict): for every admissible bin
    (k, t) the relative margin by which it is, or is not, a peak: for a peak the least margin of its conditions (S > ref for
    itself and both neighbours, the two comparisons of the local maximum, |b| < |a|); for another bin the largest margin
    among the conditions that would all have to turn for it to become one."""
    S = np.asarray(S, dtype=np.float64)
    F, T = S.shape
    if n_fft is None or n_fft // 2 + 1 != F:
        n_fft = 2 * (F - 1)
    fmin = max(fmin, 0.0)
    fmax = min(fmax, float(sr) / 2)
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
    a = S[2:] + S[:-2] - 2 * S[1:-1]
    b = (S[2:] - S[:-2]) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        sh = np.where(np.abs(b) >= np.abs(a), 0.0, -b / a)
    shift = np.pad(sh, ((1, 1), (0, 0)), mode="constant")
    avg = np.gradient(S, axis=0)
    dskew = 0.5 * avg * shift
    ref = threshold * np.max(S, axis=0, keepdims=True)
    x = S * (S > ref)
    xp = np.pad(x, ((1, 1), (0, 0)), mode="edge")
    lm = (x > xp[:-2]) & (x >= xp[2:])
    mask = ((fmin <= freqs) & (freqs < fmax))[:, None]
    idx = np.nonzero(mask & lm)
    pitches, mags = np.zeros_like(S), np.zeros_like(S)
    pitches[idx] = (idx[0] + shift[idx]) * float(sr) / n_fft
    mags[idx] = S[idx] + dskew[idx]
    if margins is not None:
        for k in np.nonzero(mask[:, 0])[0]:
            for t in range(T):
                r = ref[0, t]
                if lm[k, t]:
                    m = [_rel(S[j, t], r) for j in (k - 1, k, k + 1) if 0 <= j < F]
                    if k > 0:
                        m.append(_rel(x[k, t], x[k - 1, t]))
                    if k + 1 < F:
                        m.append(_rel(x[k, t], x[k + 1, t]) if x[k, t] != x[k + 1, t] else 0.0)
                    if 0 < k < F - 1:
                        m.append(_rel(abs(b[k - 1, t]), abs(a[k - 1, t])))
                    margins[(int(k), int(t))] = min(m)
                else:                                            # what would have to turn, with x[k] = S[k] once S[k] > ref
                    fail = [] if S[k, t] > r else [_rel(S[k, t], r)]
                    if k == 0 or not S[k, t] > x[k - 1, t]:
                        fail.append(_rel(S[k, t], x[k - 1, t]) if k > 0 else np.inf)
                    if k + 1 < F and not S[k, t] >= x[k + 1, t]:
                        fail.append(_rel(S[k, t], x[k + 1, t]))
                    margins[(int(k), int(t))] = max(fail) if fail else np.inf
    return pitches, mags


def tuning_edges(resolution=0.01):
    return np.linspace(-0.5, 0.5, int(np.ceil(1.0 / resolution)) + 1)


def residuals(frequencies, bins_per_octave=12):
    r = np.mod(bins_per_octave * hz_to_octs(frequencies), 1.0)
    r[r >= 0.5] -= 1.0
    return r


def pitch_tuning(frequencies, resolution=0.01, bins_per_octave=12, counts_out=None):
    frequencies = np.atleast_1d(np.asarray(frequencies, dtype=np.float64))
    frequencies = frequencies[frequencies > 0]
    edges = tuning_edges(resolution)
    if not np.any(frequencies):
        warnings.warn("Trying to estimate tuning from empty frequency set.", stacklevel=2)
        if counts_out is not None:
            counts_out.append(np.zeros(len(edges) - 1, dtype=np.int64))
        return 0.0
    counts, tuning = np.histogram(residuals(frequencies, bins_per_octave), edges)
    if counts_out is not None:
        counts_out.append(counts)
    return float(tuning[np.argmax(counts)])


def estimate_tuning(S, sr=22050, n_fft=None, resolution=0.01, bins_per_octave=12, detail=None, **kwargs):
    """S [F, T]: the spectrogram piptrack runs on.  detail (a dict) receives counts, n_peaks, threshold, worst_margin (the least
    relative margin of any decision: piptrack's, mag >= median, the bin edge) and fragile (the bins with a margin below 1e-4)."""
    margins = {} if detail is not None else None
    pitch, mag = piptrack(S, sr, n_fft, margins=margins, **kwargs)
    pm = pitch > 0
    th = np.median(mag[pm]) if pm.any() else 0.0
    keep = (mag >= th) & pm
    counts = []
    t = pitch_tuning(pitch[keep], resolution, bins_per_octave, counts_out=counts)
    if detail is not None:
        edges = tuning_edges(resolution)
        for k, t_ in zip(*np.nonzero(pm)):
            m = margins[(int(k), int(t_))]
            if mag[k, t_] != th:                                 # (the middle element of an odd count equals it exactly)
                m = min(m, _rel(mag[k, t_], th))
            r = residuals(np.array([pitch[k, t_]]), bins_per_octave)[0]
            margins[(int(k), int(t_))] = min(m, float(np.min(np.abs(edges - r))))     # the edges span 1: absolute
        v = np.array(list(margins.values())) if margins else np.array([np.inf])
        detail.update(counts=counts[0], n_peaks=int(pm.sum()), threshold=float(th), worst_margin=float(v.min()),
                      fragile=int((v < 1e-4).sum()))
    return t
