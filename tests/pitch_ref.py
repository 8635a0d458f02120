"""Float64 restatement of librosa 0.10 `yin` / `pyin` (librosa is not a dependency: this is the parity contract of
syg_pitch_frames_f32 / syg_pyin_viterbi_f32).  Every constant comes from sygnals_amd/_pitch.py."""
from __future__ import annotations

import numpy as np

from sygnals_amd import _pitch as P


def frames(y, frame_length=2048, hop=512, center=True):
    y = np.asarray(y, dtype=np.float64)
    if center:
        y = np.pad(y, frame_length // 2, mode="constant")
    T = 1 + (len(y) - frame_length) // hop
    idx = np.arange(frame_length)[None, :] + hop * np.arange(T)[:, None]
    return y[idx]                                                     # [T, N]


def acf_energy(fr, win_length):
    """[T, N] frames -> (acf, e) [T, N - W] before librosa's |.| < 1e-6 clamps: acf(tau) = sum_{j=1..W} x_j x_{j+tau},
    e(tau) = sum_{j=tau+1..tau+W} x_j^2."""
    N = fr.shape[1]
    W = win_length
    a = np.fft.rfft(fr, N, axis=1)
    b = np.fft.rfft(fr[:, W:0:-1], N, axis=1)
    acf = np.fft.irfft(a * b, N, axis=1)[:, W:]
    en = np.cumsum(fr ** 2, axis=1)
    en = en[:, W:] - en[:, :-W]
    return acf, en


def cmndf(fr, win_length, min_p, max_p):
    """[T, N] frames -> [T, n_lag] cumulative mean normalised difference (librosa's FFT form)."""
    acf, en = acf_energy(fr, win_length)
    acf[np.abs(acf) < 1e-6] = 0
    en[np.abs(en) < 1e-6] = 0
    d = en[:, :1] + en - 2 * acf
    num = d[:, min_p:max_p + 1]
    cm = np.cumsum(d[:, 1:max_p + 1], axis=1) / np.arange(1, max_p + 1)[None, :]
    return num / (cm[:, min_p - 1:max_p] + P.TINY)


def parabolic_shifts(c):
    c = np.asarray(c, dtype=np.float64)
    s = np.zeros_like(c)
    a = c[..., 2:] + c[..., :-2] - 2 * c[..., 1:-1]
    b = (c[..., 2:] - c[..., :-2]) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        s[..., 1:-1] = np.where(np.abs(b) >= np.abs(a), 0, -b / a)
    return s


def troughs(c):
    """localmin (x[i] < x[i-1], x[i] <= x[i+1], edge padding) with trough[0] = c[0] < c[1]; c: [..., n]."""
    xp = np.concatenate([c[..., :1], c, c[..., -1:]], axis=-1)
    tr = (c < xp[..., :-2]) & (c <= xp[..., 2:])
    tr[..., 0] = c[..., 0] < c[..., 1]
    return tr


def yin_from_cmndf(c, sr, min_p, trough_threshold=0.1):
    """-> (period index [T], f0 [T])."""
    sh = parabolic_shifts(c)
    tt = troughs(c) & (c < trough_threshold)
    idx = np.where(tt.any(axis=1), np.argmax(tt, axis=1), np.argmin(c, axis=1))
    per = min_p + idx + sh[np.arange(len(idx)), idx]
    return idx, sr / per


def pyin_frame(c, sr, min_p, fmin, n_bins, shift=None):
    """One frame's emission: (candidate bins, probabilities) in lag order after librosa's assignment rule, and
    voiced_prob.  c: float64 [n_lag]."""
    c = np.asarray(c, dtype=np.float64)
    sh = parabolic_shifts(c) if shift is None else shift
    tr = np.nonzero(troughs(c))[0]
    if len(tr) == 0:
        return np.zeros(0, np.int64), np.zeros(0), 0.0
    h = c[tr]
    thr = P.thresholds()
    below = np.less.outer(h, thr)
    pos = np.cumsum(below, axis=0) - 1
    n = np.count_nonzero(below, axis=0)
    prior = P.boltzmann_pmf(pos, np.broadcast_to(n, pos.shape))
    prior[~below] = 0
    probs = prior.dot(P.beta_probs())
    g = int(np.argmin(h))
    M = np.count_nonzero(~below[g, :])
    probs[g] += P.NO_TROUGH_PROB * np.sum(P.beta_probs()[:M])
    keep = probs > 0
    k = tr[keep]
    p = probs[keep]
    f = sr / (min_p + k + sh[k])
    bins = np.clip(np.round(12 * P.BINS_PER_SEMITONE * np.log2(f / fmin)), 0, n_bins).astype(np.int64)
    col = {}
    for bb, pp in zip(bins, p):                # assignment: the last write (larger lag) wins
        col[int(bb)] = pp
    col.pop(n_bins, None)                      # the first unvoiced row, overwritten afterwards
    ob = np.array([bb for bb in dict.fromkeys(int(x) for x in bins) if bb in col], dtype=np.int64)
    op = np.array([col[bb] for bb in ob], dtype=np.float64)
    obs = np.zeros(n_bins)
    obs[ob] = op
    vp = float(np.clip(np.sum(obs), 0, 1))
    return ob, op, vp


def emission_matrix(cands, vps, n_bins):
    """Candidate lists [(bins, probs)] and voiced_prob [T] -> observation probabilities [2 n_bins, T]."""
    T = len(cands)
    obs = np.zeros((2 * n_bins, T))
    for t, (b, p) in enumerate(cands):
        obs[np.asarray(b, dtype=np.int64), t] = p
    obs[n_bins:, :] = (1 - np.asarray(vps, dtype=np.float64)[None, :]) / n_bins
    return obs


def full_transition(n_bins, width):
    return np.kron(P.switch_matrix(), P.transition_local(n_bins, width))


def viterbi_dense(obs, trans, p_init):
    """librosa.sequence.viterbi (its _viterbi loop), float64."""
    lp = np.log(obs.T + P.TINY)
    lt = np.log(trans + P.TINY)
    li = np.log(p_init + P.TINY)
    Tn, S = lp.shape
    v = lp[0] + li
    ptr = np.zeros((Tn, S), dtype=np.int64)
    gaps = np.full(Tn, np.inf)
    for t in range(1, Tn):
        to = v[None, :] + lt.T                                       # [j, i]
        ptr[t] = np.argmax(to, axis=1)
        best = to[np.arange(S), ptr[t]]
        srt = np.sort(to, axis=1)
        gaps[t] = np.min(srt[:, -1] - srt[:, -2])
        v = lp[t] + best
    st = np.zeros(Tn, dtype=np.int64)
    st[-1] = int(np.argmax(v))
    for t in range(Tn - 2, -1, -1):
        st[t] = ptr[t + 1, st[t + 1]]
    return st, gaps


def viterbi_band(obs, n_bins, width):
    """Band-limited Viterbi with the exact out-of-band candidate (first argmax of v + log(tiny) over every state);
    equal to viterbi_dense state for state."""
    tabs, R, h = P.transition_tables(n_bins, width)
    lc = P.log_consts(n_bins)
    n = n_bins
    S = 2 * n
    lp = np.log(obs.T + P.TINY)
    v = lp[0] + np.concatenate([np.full(n, lc[1]), np.full(n, lc[2])])
    Tn = lp.shape[0]
    jj = np.arange(n)
    if R == n:
        rowmap = np.arange(n)
    else:
        rowmap = np.where(jj < h, jj, np.where(jj > n - 1 - h, jj - (n - 1) + 2 * h, h))
    # slots in increasing predecessor index: block 0 offsets -h..h, then block 1
    cols = []
    for pb in range(2):
        for o in range(-h, h + 1):
            cols.append((pb, o))
    ptr = np.zeros((Tn, S), dtype=np.int64)
    for t in range(1, Tn):
        best = np.full(S, -np.inf)
        bi = np.full(S, -1, dtype=np.int64)
        for bj in range(2):
            sc = np.full((len(cols), n), -np.inf)
            ix = np.zeros((len(cols), n), dtype=np.int64)
            for q, (pb, o) in enumerate(cols):
                ii = jj + o
                ok = (ii >= 0) & (ii < n)
                iic = np.clip(ii, 0, n - 1)
                tab = tabs[0] if pb == bj else tabs[1]
                val = v[pb * n + iic] + tab[rowmap[iic], jj - iic + h]
                sc[q] = np.where(ok, val, -np.inf)
                ix[q] = pb * n + iic
            a = np.argmax(sc, axis=0)
            best[bj * n:(bj + 1) * n] = sc[a, jj]
            bi[bj * n:(bj + 1) * n] = ix[a, jj]
        s = v + lc[0]
        gi = int(np.argmax(s))
        gv = s[gi]
        gj = gi % n
        out = np.abs(gj - np.concatenate([jj, jj])) > h
        take = out & ((gv > best) | ((gv == best) & (gi < bi)))
        best = np.where(take, gv, best)
        bi = np.where(take, gi, bi)
        ptr[t] = bi
        v = lp[t] + best
    st = np.zeros(Tn, dtype=np.int64)
    st[-1] = int(np.argmax(v))
    for t in range(Tn - 2, -1, -1):
        st[t] = ptr[t + 1, st[t + 1]]
    return st


def states_to_f0(st, n_bins, fmin):
    freqs = fmin * 2 ** (np.arange(n_bins) / (12 * P.BINS_PER_SEMITONE))
    f0 = freqs[st % n_bins]
    voiced = st < n_bins
    f0 = np.where(voiced, f0, np.nan)
    return f0, voiced


def pyin(y, sr, fmin=P.C2, fmax=P.C7, frame_length=2048, win_length=None, hop=None, center=True, cm=None):
    """-> dict(f0, voiced, voiced_prob, states, cands, vps, cmndf)."""
    win_length = win_length or frame_length // 2
    hop = hop or frame_length // 4
    min_p, max_p = P.periods(sr, fmin, fmax, frame_length, win_length)
    n = P.n_pitch_bins(fmin, fmax)
    if cm is None:
        cm = cmndf(frames(y, frame_length, hop, center), win_length, min_p, max_p)
    cands, vps = [], []
    for c in cm:
        b, p, vp = pyin_frame(c, sr, min_p, fmin, n)
        cands.append((b, p))
        vps.append(vp)
    vps = np.array(vps)
    obs = emission_matrix(cands, vps, n)
    st = viterbi_band(obs, n, P.transition_width(sr, hop))
    f0, voiced = states_to_f0(st, n, fmin)
    return dict(f0=f0, voiced=voiced, voiced_prob=vps, states=st, cands=cands, vps=vps, cmndf=cm)
