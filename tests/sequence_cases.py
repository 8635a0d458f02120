"""The cases of the Viterbi tests, shared by the CPU file (which checks every case's conditions: margins, sizes) and the
GPU file (which runs them).  Every reference is computed once (lru_cache) and never written to.

Exact tier: log-domain float64 emissions and tables; the device must give the restatement's bits.
Probability tier: float32 probabilities, log(p + eps) taken by the device.  A case is gated only where every decision of
the restatement has an absolute margin above MARGIN_PER_FRAME * T: a score is a sum of up to 2 T + 1 logs of magnitude
at most 88 (|log(FLT_MIN)| = 87.3), each within 2 ulp of float64 (1.1e-16 relative: 88 * 2 * 1.1e-16 = 2e-14 a log, at
most T * 5.7e-14 a score including the additions' own half ulps), and a decision compares two scores: T * 2e-13 covers
twice that.  The 2 ulp of the device's float64 log is taken from its documentation, not measured.
"""
import functools

import numpy as np

from sygnals_amd import _sequence as SQ
from tests import sequence_ref as R

MARGIN_PER_FRAME = 2e-13


def constants():
    from sygnals_amd import ops
    return ops.viterbi_constants()


def forms(S):
    return ("wide", "narrow") if S <= constants()["s_narrow"] else ("wide",)


# ---- exact tier -----------------------------------------------------------------------------------------------------

def exact_shapes():
    """(B, S, T): every S at which the code takes another path (1, the narrow cap and one above, one wave and beyond, the
    LDS-table cap and one above, the byte / two-byte back pointers, the largest), T around the staging tile, B 1, 3, 33."""
    K = constants()
    tile = K["tile"]
    shapes = [(3, S, tile + 1) for S in (1, 2, 3, K["s_narrow"], K["s_narrow"] + 1, 63, 64, 65, K["s_lds"], K["s_lds"] + 1)]
    shapes += [(2, 256, 5), (2, 257, 5), (2, K["s_max"], 5)]
    shapes += [(3, S, T) for S in (2, 25, 65) for T in (1, 2, 3, tile - 1, tile, 2 * tile + 1)]
    shapes += [(B, S, 7) for S in (2, 3, 25) for B in (1, 33)]
    return sorted(set(shapes))


@functools.lru_cache(maxsize=None)
def exact_case(B, S, T, kind, seed=0, per_clip=False):
    """(log_prob [B, S, T] float64, log_trans [S, S] or [B, S, S], log_init [S], states [B, T], logp [B]).
    kind 'normal': standard normals; 'ties': integers in -2 .. 2, so that a large share of the decisions are exact ties
    and every sum is exact."""
    rng = np.random.default_rng([B, S, T, seed, kind == "ties", per_clip])
    tshape = (B, S, S) if per_clip else (S, S)
    if kind == "ties":
        lp, lt, li = (rng.integers(-2, 3, size=s).astype(np.float64) for s in ((B, S, T), tshape, (S,)))
    else:
        lp, lt, li = (rng.standard_normal(s) for s in ((B, S, T), tshape, (S,)))
    states = np.zeros((B, T), dtype=np.int64)
    logp = np.zeros(B)
    for b in range(B):
        states[b], logp[b] = R.viterbi_core(lp[b].T, lt[b] if per_clip else lt, li)
    for a in (lp, lt, li, states, logp):
        a.setflags(write=False)
    return lp, lt, li, states, logp


# ---- probability tier -----------------------------------------------------------------------------------------------

def prob_cases():
    """(S, T, transition kind, variant) of the probability tier."""
    K = constants()
    shapes = [(2, 2000), (3, 1000), (25, 3001), (64, 300), (65, 300), (K["s_lds"], 200), (K["s_lds"] + 1, 200), (600, 60),
              (K["s_max"], 40)]
    cases = [(S, T, "u4", "plain") for S, T in shapes]
    cases += [(S, 300, kind, "plain") for S in (3, 25, 65) for kind in ("loop", "cycle", "local")]
    cases += [(S, 300, "u4", v) for S in (3, 25) for v in ("dbl_min", "zero_prob", "zero_frame", "zero_init", "discriminative")]
    return cases


def _transition(rng, S, kind):
    if kind == "u4":
        u = rng.random((S, S)) ** 4
        return u / u.sum(axis=1, keepdims=True)
    if kind == "loop":                     # one state that is never left: its row holds exact zeros
        stay = 0.5 + 0.45 * rng.random(S)
        stay[S - 1] = 1.0
        return SQ.transition_loop(S, stay)
    if kind == "cycle":
        return SQ.transition_cycle(S, 0.5 + 0.45 * rng.random(S))
    return SQ.transition_local(S, min(S, 5) if S > 3 else 3)


@functools.lru_cache(maxsize=None)
def prob_case(S, T, kind, variant, seed=0):
    """dict(prob [S, T] float32, transition, p_init, p_state, eps, states, logp, margin): the restatement's answer and the
    smallest margin of its decisions."""
    rng = np.random.default_rng([S, T, seed, ("u4", "loop", "cycle", "local").index(kind),
                                 ("plain", "dbl_min", "zero_prob", "zero_frame", "zero_init", "discriminative").index(variant)])
    p = rng.random((S, T)) + 1e-3
    if variant == "zero_prob":
        p[rng.integers(0, S), T // 3] = 0.0
    p = (p / p.sum(axis=0)).astype(np.float32)
    if variant == "zero_frame":
        p[:, T // 2] = 0.0
    tr = _transition(rng, S, kind)
    p_init = p_state = None
    eps = R.tiny(np.float64) if variant == "dbl_min" else R.tiny(np.float32)
    if variant == "zero_init":
        p_init = rng.random(S)
        p_init[0] = 0.0
        p_init /= p_init.sum()
    if variant == "discriminative":
        p_state = rng.random(S) + 0.1
        p_state /= p_state.sum()
        states, logp, margin = R.viterbi_discriminative(p, tr, p_state=p_state, eps=eps, want_margin=True)
    else:
        states, logp, margin = R.viterbi(p, tr, p_init=p_init, eps=eps, want_margin=True)
    for a in (p, tr, states):
        a.setflags(write=False)
    return dict(prob=p, transition=tr, p_init=p_init, p_state=p_state, eps=eps, states=states, logp=logp, margin=margin)


def bound(T):
    return MARGIN_PER_FRAME * T


# ---- mirrors --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mirror_case(which):
    """Inputs of the NumPy mirrors with leading batch axes: float32 prob [2, S, T] (binary: [2, n_labels, T])."""
    rng = np.random.default_rng(["plain", "discriminative", "binary"].index(which) + 40)
    if which == "binary":
        p = rng.random((2, 3, 300)).astype(np.float32)
        tr = np.stack([SQ.transition_loop(2, [a, b]) for a, b in ((0.9, 0.8), (0.7, 0.95), (0.6, 0.6))])
        kw = dict(p_state=np.array([0.4, 0.5, 0.7]), p_init=0.3)
    else:
        p = rng.random((2, 5, 200)) + 1e-3
        p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
        tr = SQ.transition_loop(5, 0.8)
        kw = dict(p_init=np.array([0.1, 0.2, 0.3, 0.15, 0.25]))
        if which == "discriminative":
            kw["p_state"] = np.array([0.3, 0.1, 0.2, 0.25, 0.15])
    p.setflags(write=False)
    return p, tr, kw


def mirror_margin(which):
    """The smallest decision margin over the mirror case's sequences."""
    p, tr, kw = mirror_case(which)
    if which == "binary":
        m = np.inf
        for clip in p:
            em, trs, ps, pi = R.binary_tables(clip, tr, kw["p_state"], kw["p_init"])
            eps = R.tiny(np.float32)
            for l in range(clip.shape[0]):
                m = min(m, R.viterbi_core(R.log_emissions(em[l], eps, ps[l]), np.log(trs[l] + eps), np.log(pi[l] + eps), True)[2])
        return m
    fn = R.viterbi if which == "plain" else R.viterbi_discriminative
    return min(fn(clip, tr, want_margin=True, **kw)[2] for clip in p)
