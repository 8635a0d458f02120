"""tests/sequence_ref.py, the float64 contract of the Viterbi decoders, against an exhaustive search over all S^T paths;
the three decoders' identities; the transition builders by construction; and the conditions of every GPU case (the
margins the probability tier is gated on).  No device."""
import numpy as np
import pytest

from sygnals_amd import _sequence as SQ
from tests import sequence_cases as SC
from tests import sequence_ref as R


@pytest.mark.parametrize("S,T", [(2, 1), (2, 6), (3, 5), (4, 4)])
def test_restatement_against_exhaustive_search(S, T):
    rng = np.random.default_rng(S * 100 + T)
    for kind in ("normal", "ties"):
        n_tied = 0
        for _ in range(6):
            if kind == "ties":        # small integers: every sum is exact and many paths tie
                lp, lt, li = (rng.integers(-1, 2, size=s).astype(np.float64) for s in ((T, S), (S, S), (S,)))
            else:
                lp, lt, li = (rng.standard_normal(s) for s in ((T, S), (S, S), (S,)))
            states, logp = R.viterbi_core(lp, lt, li)
            want, want_logp, tied = R.brute_force(lp, lt, li)
            n_tied += tied > 1
            assert logp == want_logp
            assert np.array_equal(states, want), (kind, lp, lt, li)
        assert kind == "normal" or T == 1 or n_tied > 0      # the crafted set does hold ties


def test_first_index_rule_on_a_crafted_tie():
    # everything equal: every path ties, the first-index rules give state 0 throughout
    states, logp = R.viterbi_core(np.zeros((5, 3)), np.zeros((3, 3)), np.zeros(3))
    assert np.array_equal(states, np.zeros(5, dtype=np.int64)) and logp == 0.0
    # the final state is the FIRST best one; its predecessor the first best one
    lp = np.zeros((3, 3))
    lp[2] = [0.0, 1.0, 1.0]
    states, _ = R.viterbi_core(lp, np.zeros((3, 3)), np.zeros(3))
    assert states.tolist() == [0, 0, 1]
    lt = np.zeros((3, 3))
    lt[0, 1] = -1.0                   # into state 1, predecessors 1 and 2 tie: 1 is taken
    states, _ = R.viterbi_core(lp, lt, np.zeros(3))
    assert states.tolist() == [1, 1, 1]
    _, _, margin = R.viterbi_core(lp, lt, np.zeros(3), want_margin=True)
    assert margin == 0.0


def test_decoder_identities():
    rng = np.random.default_rng(3)
    S, T = 4, 50
    p = rng.random((S, T)) + 1e-3
    p = (p / p.sum(axis=0)).astype(np.float32)
    tr = SQ.transition_loop(S, 0.7)
    eps = R.tiny(np.float32)
    s0, l0 = R.viterbi(p, tr, return_logp=True)
    s1, l1 = R.viterbi_discriminative(p, tr, return_logp=True)          # uniform p_state
    assert np.array_equal(s0, s1)
    assert abs((l0 - T * np.log(1.0 / S + eps)) - l1) <= 1e-12 * T
    # binary = two-state discriminative decodes, label by label
    pb = rng.random((3, 40)).astype(np.float32)
    trb = np.stack([SQ.transition_loop(2, [a, b]) for a, b in ((0.9, 0.8), (0.7, 0.95), (0.6, 0.6))])
    ps, pi = np.array([0.4, 0.5, 0.7]), np.array([0.3, 0.3, 0.6])
    sb, lb = R.viterbi_binary(pb, trb, p_state=ps, p_init=pi, return_logp=True)
    for l in range(3):
        full = np.stack([1.0 - pb[l].astype(np.float64), pb[l].astype(np.float64)])
        s, lg = R.viterbi_discriminative(full, trb[l], p_state=np.array([1 - ps[l], ps[l]]), p_init=np.array([1 - pi[l], pi[l]]),
                                         return_logp=True, eps=eps)
        assert np.array_equal(s, sb[l]) and lg == lb[l]
    # leading axes are independent decodes
    sl, ll = R.viterbi(np.stack([p, p[::-1]]), tr, return_logp=True)
    assert np.array_equal(sl[0], s0) and ll[0] == l0 and sl.shape == (2, T)


def test_transition_builders_by_construction():
    assert np.array_equal(SQ.transition_uniform(4), np.full((4, 4), 0.25))
    t = SQ.transition_loop(3, [0.5, 0.8, 1.0])
    assert np.allclose(t, [[0.5, 0.25, 0.25], [0.1, 0.8, 0.1], [0.0, 0.0, 1.0]]) and np.allclose(t.sum(1), 1)
    assert np.allclose(SQ.transition_loop(2, 0.9), [[0.9, 0.1], [0.1, 0.9]])
    t = SQ.transition_cycle(4, 0.75)
    assert np.array_equal(t, 0.75 * np.eye(4) + 0.25 * np.roll(np.eye(4), 1, axis=1))
    assert np.array_equal(SQ.transition_cycle(2, [1.0, 0.0]), [[1.0, 0.0], [1.0, 0.0]])
    for who, fn in (("transition_loop", SQ.transition_loop), ("transition_cycle", SQ.transition_cycle)):
        with pytest.raises(ValueError, match="greater than 1"):
            fn(1, 0.5)
        with pytest.raises(ValueError, match=r"must lie in \[0, 1\]"):
            fn(3, 1.5)
        with pytest.raises(ValueError, match="one value per state"):
            fn(3, [0.5, 0.5])
    with pytest.raises(ValueError, match="positive integer"):
        SQ.transition_uniform(0)


@pytest.mark.parametrize("n,width", [(5, 3), (8, 5), (7, 4), (6, 6)])
def test_transition_local_by_construction(n, width):
    t = SQ.transition_local(n, width)
    w = SQ.transition_local(n, width, wrap=True)
    assert np.allclose(t.sum(1), 1) and np.allclose(w.sum(1), 1) and np.all(t >= 0)
    for i in range(n):
        assert np.allclose(w[i], np.roll(w[0], i), rtol=1e-14, atol=0)     # a circular shift of row 0 (the sums may round apart)
        nz = np.flatnonzero(t[i])
        assert nz.min() >= max(0, i - width // 2) and nz.max() <= min(n - 1, i + width // 2)   # the band, on the diagonal
        assert t[i, i] == t[i].max() > 0
    mid = n // 2                                                       # a row that touches no edge is the wrapped one
    if mid - width // 2 >= 0 and mid + width // 2 < n:
        assert np.allclose(t[mid], w[mid])
    assert np.array_equal(SQ.transition_local(n, 1), np.eye(n))
    try:
        from scipy.signal import get_window
    except ImportError:
        return
    row = np.zeros(n)
    row[(n - width) // 2:(n - width) // 2 + width] = get_window("triangle", width, fftbins=False)
    assert np.allclose(w[0], np.roll(row, n // 2 + 1) / row.sum())
    assert np.allclose(SQ.transition_local(n, width, window="hann", wrap=True).sum(1), 1)


def test_transition_local_refusals():
    for bad in (0, 9, 2.5, [3, 3]):
        with pytest.raises(ValueError, match="width="):
            SQ.transition_local(8, bad)
    with pytest.raises(ValueError, match="greater than 1"):
        SQ.transition_local(1, 1)


# ---- the conditions of the GPU cases ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SC.prob_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_probability_tier_margins(case):
    """Every decision of the restatement on this case has a margin above T * 2e-13, so the device's path must equal it."""
    S, T, kind, variant = case
    c = SC.prob_case(S, T, kind, variant)
    assert c["margin"] > SC.bound(T), (c["margin"], SC.bound(T))
    assert np.isfinite(c["logp"]) and c["states"].shape == (T,)
    if variant != "zero_frame":
        assert np.allclose(c["prob"].astype(np.float64).sum(0), 1.0)
    if kind != "u4":
        assert np.any(c["transition"] == 0.0)                          # exact zeros: the log(eps) entries


@pytest.mark.parametrize("which", ["plain", "discriminative", "binary"])
def test_mirror_case_margins(which):
    p, _, _ = SC.mirror_case(which)
    assert SC.mirror_margin(which) > SC.bound(p.shape[-1])


def test_exact_tier_shapes_cover_the_paths():
    K = SC.constants()
    shapes = SC.exact_shapes()
    Ss = {s for _, s, _ in shapes}
    assert {1, 2, 3, K["s_narrow"], K["s_narrow"] + 1, 63, 64, 65, K["s_lds"], K["s_lds"] + 1, K["s_max"]} <= Ss
    assert {1, 2, 3, K["tile"] - 1, K["tile"] + 1} <= {t for _, _, t in shapes} and {1, 3, 33} <= {b for b, _, _ in shapes}
    lp, lt, li, states, logp = SC.exact_case(3, 3, 17, "ties")
    assert np.array_equal(lp, np.round(lp)) and states.shape == (3, 17)
    # the crafted set does tie: a zero margin somewhere
    assert R.viterbi_core(lp[0].T, lt, li, want_margin=True)[2] == 0.0
