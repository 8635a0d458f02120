"""Viterbi decoding on the device: librosa.sequence.viterbi, viterbi_discriminative and viterbi_binary with librosa's
signatures (NumPy in and out), their *_batch forms on device tensors, and the transition builders.

The definition is tests/sequence_ref.py, a float64 restatement of librosa 0.10 written from its definition; parity with
librosa itself is not pinned.  eps is the smallest normal number of the caller's dtype; the logs of the transition,
initial and marginal probabilities are taken on the host in float64, log(prob + eps) of the emissions on the device in
float64, and every score, addition and comparison of the recurrence is float64 (ops.viterbi, csrc/sequence.hip).
viterbi_binary forms its complements 1 - p in float64 from the given value (our definition).

Refused with a ValueError that names what is served, before any device work: a transition that is not square, does not
match the number of states, holds a negative entry or rows that do not sum to 1; prob outside [0, 1]; for the
discriminative decoder frames that do not sum to 1; a p_init or p_state that is negative or does not sum to 1.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import ops
from .._sequence import (check_binary_probability, check_distribution, check_prob, check_transition, tiny,  # noqa: F401
                         transition_cycle, transition_local, transition_loop, transition_uniform)

__all__ = ["viterbi", "viterbi_discriminative", "viterbi_binary", "viterbi_batch", "viterbi_discriminative_batch",
           "viterbi_binary_batch", "transition_uniform", "transition_loop", "transition_cycle", "transition_local"]


def _host_prob(who: str, prob, normalised: bool = False) -> np.ndarray:
    p = np.asarray(prob)
    if p.dtype not in (np.float32, np.float64):
        p = p.astype(np.float32 if p.dtype == np.float16 else np.float64)
    check_prob(who, p, normalised)
    return p


def _decode(who: str, prob, transition, p_init, p_state, return_logp: bool, normalised: bool):
    p = _host_prob(who, prob, normalised)
    S, Tn = p.shape[-2:]
    lead = p.shape[:-2]
    B = int(np.prod(lead, dtype=np.int64)) if lead else 1
    # judged on the host first: nothing reaches the device before every argument is accepted
    tr = check_transition(who, transition, S)
    if tr.ndim != 2:
        raise ValueError(f"{who}: transition must be [S, S]; one matrix per clip is served by {who}_batch")
    if p_init is not None:
        check_distribution(who, "p_init", p_init, S)
    if p_state is not None:
        check_distribution(who, "p_state", p_state, S)
    dev = ops.require_gpu()
    x = torch.from_numpy(np.ascontiguousarray(p.reshape(B, S, Tn))).to(dev)
    states, logp = ops.viterbi(x, tr, p_init=p_init, p_state=p_state, eps=tiny(p.dtype), return_logp=True)
    st = states.cpu().numpy().astype(np.uint16).reshape(lead + (Tn,))
    if not return_logp:
        return st
    lg = logp.cpu().numpy().reshape(lead)
    return st, (float(lg) if not lead else lg)


def viterbi(prob, transition, *, p_init=None, return_logp: bool = False):
    """librosa.sequence.viterbi: prob [..., S, T] likelihoods of each frame under each state, transition [S, S] ->
    states [..., T] uint16 (and logp [...], the log-likelihood of the path)."""
    return _decode("viterbi", prob, transition, p_init, None, return_logp, False)


def viterbi_discriminative(prob, transition, *, p_state=None, p_init=None, return_logp: bool = False):
    """librosa.sequence.viterbi_discriminative: prob [..., S, T] are posteriors P(state | frame), each frame summing to
    1; p_state [S] the marginal of each state (default 1 / S)."""
    S = np.asarray(prob).shape[-2] if np.asarray(prob).ndim >= 2 else 1
    ps = np.full(S, 1.0 / S) if p_state is None else p_state
    return _decode("viterbi_discriminative", prob, transition, p_init, ps, return_logp, True)


def _binary_tables(who: str, n_labels: int, transition, p_state, p_init):
    tr = np.asarray(transition, dtype=np.float64)
    if tr.shape == (2, 2):
        tr = np.broadcast_to(tr, (n_labels, 2, 2))
    if tr.shape != (n_labels, 2, 2):
        raise ValueError(f"{who}: transition must be [2, 2] or one per label [{n_labels}, 2, 2], got shape {tr.shape} "
                         "(served: two states a label, square row-stochastic matrices)")
    tr = check_transition(who, tr, 2)
    ps = check_binary_probability(who, "p_state", 0.5 if p_state is None else p_state, n_labels)
    pi = check_binary_probability(who, "p_init", 0.5 if p_init is None else p_init, n_labels)
    return tr, np.stack([1.0 - ps, ps], axis=1), np.stack([1.0 - pi, pi], axis=1)


def viterbi_binary_batch(prob: torch.Tensor, transition, *, p_state=None, p_init=None, return_logp: bool = False,
                         eps: Optional[float] = None, form: Optional[str] = None):
    """viterbi_binary on a device tensor prob [B, n_labels, T] (float32 or float64) -> states [B, n_labels, T] int32 (and
    logp [B, n_labels] float64): every label an independent two-state discriminative decode with emissions (1 - p, p),
    marginals (1 - p_state, p_state) and initials (1 - p_init, p_init), the complements formed in float64."""
    who = "viterbi_binary"
    if not isinstance(prob, torch.Tensor) or prob.dim() != 3 or prob.dtype not in (torch.float32, torch.float64) \
            or min(prob.shape) < 1:
        raise ValueError(f"{who}: prob must be a non-empty float32 or float64 tensor [B, n_labels, T]")
    B, L, Tn = (int(n) for n in prob.shape)
    tr, ps, pi = _binary_tables(who, L, transition, p_state, p_init)
    e = tiny(np.float32 if prob.dtype == torch.float32 else np.float64) if eps is None else float(eps)
    p = prob.reshape(B * L, Tn).to(torch.float64)
    em = torch.stack([1.0 - p, p], dim=1)                                      # [B L, 2, T]
    states, logp = ops.viterbi(em, np.tile(tr, (B, 1, 1)), p_init=np.tile(pi, (B, 1)), p_state=np.tile(ps, (B, 1)), eps=e,
                               form=form, return_logp=True)
    states = states.reshape(B, L, Tn)
    return (states, logp.reshape(B, L)) if return_logp else states


def viterbi_binary(prob, transition, *, p_state=None, p_init=None, return_logp: bool = False):
    """librosa.sequence.viterbi_binary: prob [..., n_labels, T] the probability that each label is active at each frame,
    transition [2, 2] or [n_labels, 2, 2] -> states [..., n_labels, T] uint16 of 0 / 1 (and logp [..., n_labels])."""
    who = "viterbi_binary"
    p = _host_prob(who, np.atleast_2d(np.asarray(prob)))
    L, Tn = p.shape[-2:]
    lead = p.shape[:-2]
    B = int(np.prod(lead, dtype=np.int64)) if lead else 1
    _binary_tables(who, L, transition, p_state, p_init)
    dev = ops.require_gpu()
    x = torch.from_numpy(np.ascontiguousarray(p.reshape(B, L, Tn))).to(dev)
    states, logp = viterbi_binary_batch(x, transition, p_state=p_state, p_init=p_init, return_logp=True, eps=tiny(p.dtype))
    st = states.cpu().numpy().astype(np.uint16).reshape(lead + (L, Tn))
    return (st, logp.cpu().numpy().reshape(lead + (L,))) if return_logp else st


def viterbi_batch(prob: torch.Tensor, transition, *, p_init=None, lengths=None, return_logp: bool = False,
                  form: Optional[str] = None):
    """viterbi on a device tensor prob [B, S, T] (any strides) -> states [B, T] int32 (and logp [B] float64).  transition
    [S, S] or one per clip [B, S, S]; lengths [B]: states past a clip's length are -1.  (ops.viterbi.)"""
    return ops.viterbi(prob, transition, p_init=p_init, lengths=lengths, form=form, return_logp=return_logp)


def viterbi_discriminative_batch(prob: torch.Tensor, transition, *, p_state=None, p_init=None, lengths=None,
                                 return_logp: bool = False, form: Optional[str] = None):
    """viterbi_discriminative on a device tensor prob [B, S, T].  The frames are taken to sum to 1: that is not looked
    for here (it would be a device reduction and a sync); the NumPy form checks it."""
    if isinstance(prob, torch.Tensor) and prob.dim() == 3 and p_state is None:
        p_state = np.full(int(prob.shape[1]), 1.0 / int(prob.shape[1]))
    return ops.viterbi(prob, transition, p_init=p_init, p_state=p_state, lengths=lengths, form=form, return_logp=return_logp)
