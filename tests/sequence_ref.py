"""The float64 contract of the Viterbi decoders (ops.viterbi, core/sequence.py): a restatement of librosa 0.10's
librosa.sequence._viterbi and its three callers, written from their definition.  librosa is not a dependency and parity
with it is not pinned here; this file is what the device code is held to.

Core recurrence, all float64, log_prob [T, S], log_trans [S, S] (row = source state), log_p_init [S]:
    value[0]   = log_prob[0] + log_p_init
    ptr[t, j]  = the FIRST i that maximises value[t-1, i] + log_trans[i, j]
    value[t,j] = log_prob[t, j] + (value[t-1, ptr] + log_trans[ptr, j])         (additions in exactly this order)
    state[T-1] = the first argmax of value[T-1];  state[t] = ptr[t+1, state[t+1]];  logp = value[T-1, state[T-1]]
eps is the smallest normal number of prob's dtype; every log is log(p + eps) with p widened to float64 first.
"""
import itertools

import numpy as np


def tiny(dtype) -> float:
    dt = np.dtype(dtype)
    return float(np.finfo(dt if dt.kind == "f" else np.float64).tiny)


def viterbi_core(log_prob, log_trans, log_p_init, want_margin=False):
    """(states [T] int64, logp) and, with want_margin, the smallest absolute margin of any decision: best over runner-up
    predecessor at every (t, j), best over runner-up final state (inf where S = 1)."""
    lp = np.asarray(log_prob, dtype=np.float64)
    lt = np.asarray(log_trans, dtype=np.float64)
    T, S = lp.shape
    assert lt.shape == (S, S)
    cols = np.arange(S)
    value = lp[0] + np.asarray(log_p_init, dtype=np.float64)
    ptr = np.zeros((T, S), dtype=np.int64)
    margin = np.inf
    for t in range(1, T):
        cand = value[:, None] + lt                      # cand[i, j]
        p = np.argmax(cand, axis=0)                     # first maximiser
        best = cand[p, cols]
        if want_margin and S > 1:
            rest = cand.copy()
            rest[p, cols] = -np.inf
            margin = min(margin, float(np.min(best - rest.max(axis=0))))
        ptr[t] = p
        value = lp[t] + best
    states = np.zeros(T, dtype=np.int64)
    states[-1] = int(np.argmax(value))
    if want_margin and S > 1:
        rest = value.copy()
        rest[states[-1]] = -np.inf
        margin = min(margin, float(value[states[-1]] - rest.max()))
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    logp = float(value[states[-1]])
    return (states, logp, margin) if want_margin else (states, logp)


def brute_force(log_prob, log_trans, log_p_init):
    """Exhaustive search over all S^T paths, scored as the recurrence scores them; among equal scores the path the
    recurrence's first-index rules pick: the smallest final state, then (walking back) the smallest predecessor."""
    lp = np.asarray(log_prob, dtype=np.float64)
    T, S = lp.shape
    best, best_paths = -np.inf, []
    for path in itertools.product(range(S), repeat=T):
        v = lp[0, path[0]] + log_p_init[path[0]]
        for t in range(1, T):
            v = lp[t, path[t]] + (v + log_trans[path[t - 1], path[t]])
        if v > best:
            best, best_paths = v, [path]
        elif v == best:
            best_paths.append(path)
    # reversed-lexicographic minimum: last state first, then its predecessor, ...
    pick = min(best_paths, key=lambda p: p[::-1])
    return np.array(pick, dtype=np.int64), float(best), len(best_paths)


def _over_leading(fn, prob, *per_clip):
    """fn over the leading axes of prob [..., S, T]."""
    lead = prob.shape[:-2]
    states = np.zeros(lead + (prob.shape[-1],), dtype=np.int64)
    logp = np.zeros(lead, dtype=np.float64)
    for idx in np.ndindex(*lead):
        states[idx], logp[idx] = fn(prob[idx])
    return states, logp


def log_emissions(prob, eps=None, p_state=None):
    """log_prob [T, S] of prob [S, T]: log(prob + eps), minus log(p_state + eps) where given."""
    prob = np.asarray(prob)
    eps = tiny(prob.dtype) if eps is None else eps
    lp = np.log(prob.astype(np.float64) + eps)
    if p_state is not None:
        lp = lp - np.log(np.asarray(p_state, dtype=np.float64) + eps)[:, None]
    return lp.T


def viterbi(prob, transition, *, p_init=None, return_logp=False, eps=None, want_margin=False):
    prob = np.asarray(prob)
    S = prob.shape[-2]
    eps = tiny(prob.dtype) if eps is None else eps
    lt = np.log(np.asarray(transition, dtype=np.float64) + eps)
    li = np.log((np.full(S, 1.0 / S) if p_init is None else np.asarray(p_init, dtype=np.float64)) + eps)
    if want_margin:
        return viterbi_core(log_emissions(prob, eps), lt, li, True)
    states, logp = _over_leading(lambda p: viterbi_core(log_emissions(p, eps), lt, li), prob)
    return (states, logp) if return_logp else states


def viterbi_discriminative(prob, transition, *, p_state=None, p_init=None, return_logp=False, eps=None, want_margin=False):
    prob = np.asarray(prob)
    S = prob.shape[-2]
    eps = tiny(prob.dtype) if eps is None else eps
    assert np.allclose(prob.sum(axis=-2), 1.0)
    lt = np.log(np.asarray(transition, dtype=np.float64) + eps)
    ps = np.full(S, 1.0 / S) if p_state is None else np.asarray(p_state, dtype=np.float64)
    li = np.log((np.full(S, 1.0 / S) if p_init is None else np.asarray(p_init, dtype=np.float64)) + eps)
    if want_margin:
        return viterbi_core(log_emissions(prob, eps, ps), lt, li, True)
    states, logp = _over_leading(lambda p: viterbi_core(log_emissions(p, eps, ps), lt, li), prob)
    return (states, logp) if return_logp else states


def binary_tables(prob, transition, p_state=None, p_init=None):
    """The two-state problems of viterbi_binary, label by label: prob [n_labels, T] (any float dtype) ->
    (emissions [n_labels, 2, T] float64 = (1 - p, p), transition [n_labels, 2, 2], p_state [n_labels, 2],
    p_init [n_labels, 2]); the complements are formed in float64 from the given value."""
    prob = np.asarray(prob)
    L = prob.shape[0]
    p = prob.astype(np.float64)
    em = np.stack([1.0 - p, p], axis=1)
    tr = np.asarray(transition, dtype=np.float64)
    tr = np.broadcast_to(tr, (L, 2, 2)) if tr.ndim == 2 else tr
    ps = np.broadcast_to(np.asarray(0.5 if p_state is None else p_state, dtype=np.float64), (L,))
    pi = np.broadcast_to(np.asarray(0.5 if p_init is None else p_init, dtype=np.float64), (L,))
    return em, tr, np.stack([1.0 - ps, ps], axis=1), np.stack([1.0 - pi, pi], axis=1)


def viterbi_binary(prob, transition, *, p_state=None, p_init=None, return_logp=False, eps=None):
    prob = np.asarray(prob)
    eps = tiny(prob.dtype) if eps is None else eps
    if prob.ndim > 2:
        st, lg = zip(*(viterbi_binary(p, transition, p_state=p_state, p_init=p_init, return_logp=True, eps=eps) for p in prob))
        return (np.stack(st), np.stack(lg)) if return_logp else np.stack(st)
    em, tr, ps, pi = binary_tables(prob, transition, p_state, p_init)
    states = np.zeros(prob.shape, dtype=np.int64)
    logp = np.zeros(prob.shape[0])
    for l in range(prob.shape[0]):
        states[l], logp[l] = viterbi_core(log_emissions(em[l], eps, ps[l]), np.log(tr[l] + eps), np.log(pi[l] + eps))
    return (states, logp) if return_logp else states
