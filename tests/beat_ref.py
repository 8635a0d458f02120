"""Float64 restatement of the rhythm family: the contract of beat.hip (tempogram, tempo, beat tracking).

Written from the definitions alone (librosa 0.10's feature.tempogram, feature.tempo and beat.beat_track as the issue states
them); librosa is not a dependency and parity with it is unpinned.  Every function takes one clip's envelope.
"""
import numpy as np
import scipy.signal

LOG_N = 4096
L = np.log(np.arange(1, LOG_N + 1, dtype=np.float64))          # L[m - 1] = log(m)
TINY = float(np.finfo(np.float32).tiny)


def window32(window, win_length):
    """The analysis window as the device holds it: float64 on the host, rounded once to float32."""
    return scipy.signal.get_window(window, win_length, fftbins=True).astype(np.float64).astype(np.float32).astype(np.float64)


def pad_ramp(env, p):
    env = np.asarray(env, dtype=np.float64)
    T = len(env)
    i = np.arange(p, dtype=np.float64)
    return np.concatenate([env[0] * i / p, env, env[T - 1] * (p - 1 - i) / p])


def autocorr(env, win_length=384, center=True, window="hann"):
    """r [win_length, n]: the unnormalised windowed autocorrelation of every frame."""
    env = np.asarray(env, dtype=np.float64)
    T = len(env)
    xp = pad_ramp(env, win_length // 2) if center else env
    n = T if center else T - win_length + 1
    if n <= 0:
        raise ValueError(f"{T} frames are fewer than win_length={win_length}")
    w = window32(window, win_length)
    r = np.zeros((win_length, n))
    for t in range(n):
        f = w * xp[t:t + win_length]
        for k in range(win_length):
            r[k, t] = np.dot(f[:win_length - k], f[k:])
    return r


def normalise(r, norm=np.inf):
    if norm is None:
        return r
    m = np.max(np.abs(r), axis=0)
    return r / np.where(m < TINY, 1.0, m)[None, :]


def tempogram(env, win_length=384, center=True, window="hann", norm=np.inf):
    return normalise(autocorr(env, win_length, center, window), norm)


def aggregate(tg):
    """The mean over frames as a float64 sum in index order."""
    return np.cumsum(tg, axis=1)[:, -1] / tg.shape[1]


def prior(win_length, sr, hop_length=512, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0):
    bpms = np.full(win_length, np.inf)
    bpms[1:] = 60.0 * sr / (hop_length * np.arange(1.0, win_length))
    with np.errstate(divide="ignore", invalid="ignore"):
        logprior = -0.5 * ((np.log2(bpms) - np.log2(start_bpm)) / std_bpm) ** 2
    if max_tempo is not None:
        logprior[:int(np.argmax(bpms < max_tempo))] = -np.inf
    return bpms, logprior


def scores(a, logprior):
    with np.errstate(invalid="ignore"):
        return np.log1p(1e6 * np.asarray(a, dtype=np.float64)) + logprior


def tempo_pick(a, logprior):
    return int(np.argmax(scores(a, logprior)))


def tempo(env, sr, hop_length=512, start_bpm=120.0, std_bpm=1.0, ac_size=8.0, max_tempo=320.0, aggregated=True):
    """(tempo, k*) of a clip, or one pair per frame."""
    env = np.asarray(env, dtype=np.float64)
    win = int(np.floor(ac_size * sr / hop_length))
    bpms, lp = prior(win, sr, hop_length, start_bpm, std_bpm, max_tempo)
    if not env.any():
        return (0.0, 0) if aggregated else (np.zeros(len(env)), np.zeros(len(env), dtype=np.int64))
    tg = tempogram(env, win)
    if aggregated:
        k = tempo_pick(aggregate(tg), lp)
        return float(bpms[k]), k
    ks = np.array([tempo_pick(tg[:, t], lp) for t in range(tg.shape[1])], dtype=np.int64)
    return bpms[ks], ks


def half_even(x):
    return int(np.round(x))


def period_of(bpm, sr, hop_length):
    return half_even(60.0 * (sr / hop_length) / bpm)


def taps(period):
    q = np.arange(-period, period + 1, dtype=np.float64)
    return np.exp(-0.5 * (32.0 * q / period) ** 2)


def scaled(env):
    env = np.asarray(env, dtype=np.float64)
    if len(env) >= 2:
        s = np.std(env, ddof=1)
        if np.isfinite(s) and s > 0:
            return env / s
    return env


def local_score(env, period):
    """ls in float64: sum_q g[q] e[i - q] with zeros outside the clip."""
    e, g = scaled(env), taps(period)
    T = len(e)
    pad = np.concatenate([np.zeros(period), e, np.zeros(period)])
    return np.array([np.dot(g, pad[i:i + 2 * period + 1][::-1]) for i in range(T)])


def offsets(period):
    return np.arange(-2 * period, -half_even(period / 2) + 1)


def transition(period, tightness):
    o = offsets(period)
    d = L[-o - 1] - L[period - 1]
    return -tightness * (d * d)


def dp(ls32, period, tightness=100.0):
    """cum (float64), back (int64) from the float32 local score, every step spelt out."""
    ls = np.asarray(ls32).astype(np.float64)            # the contract feeds float32; float64 is taken as it is
    T = len(ls)
    o, tx = offsets(period), transition(period, float(tightness))
    cum, back = np.zeros(T), np.zeros(T, dtype=np.int64)
    thresh = 0.01 * ls.max()
    first = True
    for i in range(T):
        best, bj = -np.inf, 0
        for j in range(len(o)):
            c = tx[j] + (cum[i + o[j]] if i + o[j] >= 0 else 0.0)
            if c > best:
                best, bj = c, j
        cum[i] = ls[i] + best
        if first and ls[i] < thresh:
            back[i] = -1
        else:
            back[i] = i + o[bj]
            first = False
    return cum, back


def dp_vector(ls32, period, tightness=100.0):
    """The same recurrence with the candidates of a step as one array (what the tests of long rows use)."""
    ls = np.asarray(ls32).astype(np.float64)            # the contract feeds float32; float64 is taken as it is
    T = len(ls)
    o, tx = offsets(period), transition(period, float(tightness))
    cum, back = np.zeros(T), np.zeros(T, dtype=np.int64)
    thresh = 0.01 * ls.max()
    first = True
    for i in range(T):
        src = i + o
        c = tx + np.where(src >= 0, cum[np.maximum(src, 0)], 0.0)
        bj = int(np.argmax(c))
        cum[i] = ls[i] + c[bj]
        if first and ls[i] < thresh:
            back[i] = -1
        else:
            back[i] = src[bj]
            first = False
    return cum, back


def dp_negative_index(ls32, period, tightness=100.0):
    """librosa's form: the window of negative indices wraps into the zeros at the end of cum."""
    ls = np.asarray(ls32).astype(np.float64)            # the contract feeds float32; float64 is taken as it is
    T = len(ls)
    window = offsets(period).copy()
    tx = transition(period, float(tightness))
    cum, back = np.zeros(T), np.zeros(T, dtype=np.int64)
    thresh = 0.01 * ls.max()
    first = True
    for i in range(T):
        z = max(0, min(-window[0], len(window)))
        cand = tx.copy()
        cand[z:] = cand[z:] + cum[window[z:]]
        bj = int(np.argmax(cand))
        cum[i] = ls[i] + cand[bj]
        if first and ls[i] < thresh:
            back[i] = -1
        else:
            back[i] = window[bj]
            first = False
        window = window + 1
    return cum, back


def local_maxima(cum):
    T = len(cum)
    lm = np.zeros(T, dtype=bool)
    if T >= 2:
        lm[1:-1] = (cum[1:-1] > cum[:-2]) & (cum[1:-1] >= cum[2:])
        lm[T - 1] = cum[T - 1] > cum[T - 2]
    return lm


def last_beat(cum):
    lm = local_maxima(cum)
    if not lm.any():
        return -1
    med = np.median(cum[lm])
    hit = np.flatnonzero(2 * cum * lm > med)
    return int(hit.max()) if len(hit) else -1


def backtrack(back, last):
    b = []
    i = last
    while i >= 0:
        b.append(i)
        i = int(back[i])
    return np.array(b[::-1], dtype=np.int64)


def smooth(ls32, b):
    v = np.asarray(ls32).astype(np.float64)[b]
    z = np.concatenate([[0.0], v, [0.0]])
    return (0.5 * z[:-2] + z[1:-1]) + 0.5 * z[2:]


def trim_beats(ls32, b, trim=True):
    if len(b) == 0:
        return b
    sm = smooth(ls32, b)
    th = 0.5 * np.sqrt(np.cumsum(sm * sm)[-1] / len(sm)) if trim else 0.0
    v = np.flatnonzero(sm > th)
    if len(v) == 0:
        return b[:0]
    return b[v.min():v.max()]                      # the upper end is exclusive, as librosa 0.10.0 has it


def beats_from(ls32, period, tightness=100.0, trim=True, dp_fn=dp_vector):
    """(beats, last, cum, back) of a clip from its float32 local score."""
    T = len(ls32)
    if period < 2:
        return np.zeros(0, dtype=np.int64), -1, np.zeros(T), np.full(T, -1, dtype=np.int64)
    cum, back = dp_fn(ls32, period, tightness)
    last = last_beat(cum)
    b = backtrack(back, last)
    return trim_beats(ls32, b, trim), last, cum, back


def beat_track(env, period, tightness=100.0, trim=True):
    env = np.asarray(env, dtype=np.float64)
    if not env.any() or period < 2:
        return np.zeros(0, dtype=np.int64)
    ls32 = local_score(env, period).astype(np.float32)
    return beats_from(ls32, period, tightness, trim)[0]


def chain(env, sr, hop_length=512, start_bpm=120.0, tightness=100.0, trim=True, bpm=None):
    """(tempo, beats): the whole float64 chain of a clip."""
    if bpm is None:
        bpm_, k = tempo(env, sr, hop_length, start_bpm)
        period = k
    else:
        bpm_, period = float(bpm), period_of(bpm, sr, hop_length)
    if not np.asarray(env).any():
        return 0.0, np.zeros(0, dtype=np.int64)
    return bpm_, beat_track(env, period, tightness, trim)


def click_envelope(T, period, phase=0, height=1.0, noise=0.1, seed=0):
    """A click track as an envelope: `height` every `period` frames from `phase`, uniform noise of height * noise."""
    rng = np.random.default_rng(seed)
    env = (rng.random(T) * noise * height).astype(np.float32)
    env[phase::period] += np.float32(height)
    return env
