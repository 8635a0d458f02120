"""The device Viterbi decoders (ops.viterbi, core.sequence, detect_activity_batch) against tests/sequence_ref.py.

Exact tier: log-domain float64 emissions (normals, and small integers that tie) -- states and logp bit for bit, both forms.
Probability tier: float32 probabilities with the device's own log -- equal states and |logp - ref| <= T * 2e-13 on cases
whose every decision margin is above that bound (tests/sequence_cases.py derives it; tests/test_sequence_ref.py asserts
the margins case by case)."""
import numpy as np
import pytest
import torch

from tests import sequence_cases as SC
from tests import sequence_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    assert hasattr(ops, "viterbi")
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got_states, got_logp, states, logp):
    assert got_states.dtype == torch.int32 and got_logp.dtype == torch.float64
    assert np.array_equal(got_states.cpu().numpy(), states)
    assert np.array_equal(got_logp.cpu().numpy().view(np.int64), np.asarray(logp).view(np.int64))


@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("shape", SC.exact_shapes(), ids=lambda s: "B%d-S%d-T%d" % s)
def test_exact_tier(ops, shape, kind):
    B, S, T = shape
    lp, lt, li, states, logp = SC.exact_case(B, S, T, kind)
    x = dev(lp)
    for form in SC.forms(S):
        st, lg = ops.viterbi(log_prob=x, transition=lt, p_init=li, form=form, return_logp=True)
        same_bits(st, lg, states, logp)
    st, lg = ops.viterbi(log_prob=x, transition=lt, p_init=li, return_logp=True)          # the library's rule
    same_bits(st, lg, states, logp)


def test_long_sequence(ops):
    lp, lt, li, states, logp = SC.exact_case(1, 25, 3001, "normal")
    same_bits(*ops.viterbi(log_prob=dev(lp), transition=lt, p_init=li, return_logp=True), states, logp)
    lp, lt, li, states, logp = SC.exact_case(1, 25, 3001, "ties")
    same_bits(*ops.viterbi(log_prob=dev(lp), transition=lt, p_init=li, return_logp=True), states, logp)


@pytest.mark.parametrize("form", ["wide", "narrow"])
def test_batch_past_the_grid_cap(ops, form):
    """B = 65 537 two-state sequences of 3 frames: the first, the 65 535th and the last row."""
    B = 65537
    rng = np.random.default_rng(11)
    lp, lt, li = rng.standard_normal((B, 2, 3)), rng.standard_normal((2, 2)), rng.standard_normal(2)
    st, lg = ops.viterbi(log_prob=dev(lp), transition=lt, p_init=li, form=form, return_logp=True)
    st, lg = st.cpu().numpy(), lg.cpu().numpy()
    for b in (0, 65534, B - 1):
        s, l = R.viterbi_core(lp[b].T, lt, li)
        assert np.array_equal(st[b], s) and lg[b] == l
    assert st.min() >= 0 and st.max() <= 1 and np.isfinite(lg).all()


@pytest.mark.parametrize("S", [3, 25, 70])
def test_ragged_lengths(ops, S):
    B, T = 6, 37
    lens = np.array([1, T, 7, 16, 17, 33])
    for kind in ("normal", "ties"):
        lp, lt, li, _, _ = SC.exact_case(B, S, T, kind)
        for form in SC.forms(S):
            for lengths in (lens, torch.from_numpy(lens).cuda()):
                st, lg = ops.viterbi(log_prob=dev(lp), transition=lt, p_init=li, lengths=lengths, form=form, return_logp=True)
                st, lg = st.cpu().numpy(), lg.cpu().numpy()
                for b, n in enumerate(lens):
                    s, l = R.viterbi_core(lp[b, :, :n].T, lt, li)
                    assert np.array_equal(st[b, :n], s) and lg[b] == l and np.all(st[b, n:] == -1)


@pytest.mark.parametrize("S", [2, 25, 140])
def test_layouts_and_strides(ops, S):
    """[B, T, S] views, odd batch strides, float32 log-probabilities, a zero batch stride."""
    B, T = 3, 21
    lp, lt, li, states, logp = SC.exact_case(B, S, T, "normal")
    for form in SC.forms(S):
        kw = dict(transition=lt, p_init=li, form=form, return_logp=True)
        bts = dev(lp.transpose(0, 2, 1))                                   # [B, T, S] in memory
        assert bts.is_contiguous()
        same_bits(*ops.viterbi(log_prob=bts.transpose(1, 2), **kw), states, logp)
        buf = torch.full((B, S * T + 7), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :S * T] = dev(lp).reshape(B, S * T)
        view = buf[:, :S * T].view(B, S, T)
        assert view.stride(0) == S * T + 7
        same_bits(*ops.viterbi(log_prob=view, **kw), states, logp)
        big = torch.full((B, S, T + 3), float("nan"), dtype=torch.float64, device="cuda")
        big[:, :, 2:T + 2] = dev(lp)
        same_bits(*ops.viterbi(log_prob=big[:, :, 2:T + 2], **kw), states, logp)
        one = dev(lp[1:2]).expand(B, S, T)                                 # a batch stride of 0
        st, lg = ops.viterbi(log_prob=one, **kw)
        same_bits(st, lg, np.stack([states[1]] * B), np.stack([logp[1]] * B))
        lp32 = lp.astype(np.float32)                                       # float32 logs widen exactly
        want = [R.viterbi_core(lp32[b].astype(np.float64).T, lt, li) for b in range(B)]
        same_bits(*ops.viterbi(log_prob=dev(lp32), **kw), np.stack([w[0] for w in want]), np.array([w[1] for w in want]))


@pytest.mark.parametrize("S", [3, 25])
def test_tables_per_clip_batch_rows_chunks_and_out(ops, S):
    B, T = 5, 19
    lp, lt, li, states, logp = SC.exact_case(B, S, T, "ties", per_clip=True)
    assert lt.shape == (B, S, S)
    x = dev(lp)
    rng = np.random.default_rng(S)
    lis = rng.integers(-2, 3, size=(B, S)).astype(np.float64)              # an initial row per clip as well
    lms = rng.integers(-2, 3, size=(B, S)).astype(np.float64)              # and a marginal row
    want = [R.viterbi_core(lp[b].T - lms[b], lt[b], lis[b]) for b in range(B)]
    ws, wl = np.stack([w[0] for w in want]), np.array([w[1] for w in want])
    for form in SC.forms(S):
        same_bits(*ops.viterbi(log_prob=x, transition=lt, p_init=li, form=form, return_logp=True), states, logp)
        kw = dict(transition=lt, p_init=lis, p_state=lms, form=form, return_logp=True)
        whole = ops.viterbi(log_prob=x, **kw)
        same_bits(*whole, ws, wl)
        for b in range(B):                                                 # a batch equals its rows
            one = ops.viterbi(log_prob=x[b:b + 1], transition=lt[b], p_init=lis[b], p_state=lms[b], form=form, return_logp=True)
            same_bits(*one, ws[b:b + 1], wl[b:b + 1])
        for chunk in (1, 2):                                               # pieces change no bit
            same_bits(*ops.viterbi(log_prob=x, chunk=chunk, **kw), ws, wl)
        again = ops.viterbi(log_prob=x, **kw)                              # the same call gives the same bits
        assert torch.equal(again[0], whole[0]) and torch.equal(again[1], whole[1])
        out = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
        st, lg = ops.viterbi(log_prob=x, out=out, **kw)
        assert st is out and not bool((out == -7).any())
        same_bits(st, lg, ws, wl)


def test_work_bound_chunks_the_batch(ops, monkeypatch):
    B, S, T = 7, 25, 40
    lp, lt, li, states, logp = SC.exact_case(B, S, T, "normal")
    monkeypatch.setattr(ops, "VITERBI_WORK_MAX", 2 * ops.viterbi_work_bytes(1, S, T) + 100)       # two clips a piece
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (calls.append(a[6]), real(name, *a))[1])
    same_bits(*ops.viterbi(log_prob=dev(lp), transition=lt, p_init=li, return_logp=True), states, logp)
    assert calls == [2, 2, 2, 1]


# ---- probability tier ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SC.prob_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_probability_tier(ops, case):
    S, T, kind, variant = case
    c = SC.prob_case(S, T, kind, variant)
    assert c["margin"] > SC.bound(T)
    x = dev(c["prob"])[None]
    assert x.dtype == torch.float32
    eps = c["eps"] if variant == "dbl_min" else None
    for form in SC.forms(S):
        st, lg = ops.viterbi(x, c["transition"], p_init=c["p_init"], p_state=c["p_state"], eps=eps, form=form, return_logp=True)
        err = abs(float(lg[0]) - c["logp"])
        print(f"{case} {form}: |logp - ref| = {err:.3e} (bound {SC.bound(T):.3e}, margin {c['margin']:.3e})")
        assert np.array_equal(st[0].cpu().numpy(), c["states"])
        assert err <= SC.bound(T)


# ---- mirrors and the activity chain -------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["plain", "discriminative", "binary"])
def test_mirrors(which):
    from sygnals_amd.core import sequence as SQ
    p, tr, kw = SC.mirror_case(which)
    T = p.shape[-1]
    assert SC.mirror_margin(which) > SC.bound(T)
    fn, ref = {"plain": (SQ.viterbi, R.viterbi), "discriminative": (SQ.viterbi_discriminative, R.viterbi_discriminative),
               "binary": (SQ.viterbi_binary, R.viterbi_binary)}[which]
    want, want_logp = ref(p, tr, return_logp=True, **kw)
    got, logp = fn(p, tr, return_logp=True, **kw)
    assert got.dtype == np.uint16 and got.shape == want.shape and logp.shape == want_logp.shape
    assert np.array_equal(got, want) and np.max(np.abs(logp - want_logp)) <= SC.bound(T)
    assert np.array_equal(fn(p, tr, **kw), got)                            # without logp: the states alone
    one, one_logp = fn(p[0], tr, return_logp=True, **kw)                   # no leading axis
    assert np.array_equal(one, got[0]) and np.array_equal(np.asarray(one_logp), logp[0])
    x = torch.from_numpy(p).cuda()
    if which == "binary":
        st, lg = SQ.viterbi_binary_batch(x, tr, return_logp=True, **kw)
        for form in ("wide", "narrow"):
            assert torch.equal(SQ.viterbi_binary_batch(x, tr, form=form, **kw), st)
    elif which == "plain":
        st, lg = SQ.viterbi_batch(x, tr, return_logp=True, **kw)
    else:
        st, lg = SQ.viterbi_discriminative_batch(x, tr, return_logp=True, **kw)
    assert st.dtype == torch.int32 and np.array_equal(st.cpu().numpy(), want)
    assert np.array_equal(lg.cpu().numpy(), logp)


def test_float64_probabilities_use_dbl_min(ops):
    c = SC.prob_case(25, 300, "u4", "plain")
    p64 = c["prob"].astype(np.float64)
    states, logp, margin = R.viterbi(p64, c["transition"], want_margin=True)           # eps = DBL_MIN from the dtype
    assert margin > SC.bound(300)
    st, lg = ops.viterbi(dev(p64)[None], c["transition"], return_logp=True)
    assert np.array_equal(st[0].cpu().numpy(), states) and abs(float(lg[0]) - logp) <= SC.bound(300)


def test_activity_chain():
    """A tone gated on and off, L = 32 768: the mask is the restatement's on the device's own RMS, and it is the gate.
    A frame is 2048 samples and a hop 512, so a frame within two hops of an edge of the gate holds both tone and silence
    and may read either way; every other frame must read as its gate.  Threshold 0.1 (the tone's RMS is 0.35): at the
    recipe's default of 0.02 a silent frame's r = -0.02 / std is too close to 0 to outweigh the stay probability 0.6."""
    from sygnals_amd import ops
    from sygnals_amd.core import segmentation as SG
    from sygnals_amd._sequence import transition_loop
    L, sr, hop, frame = 32768, 22050, 512, 2048
    t = np.arange(L)
    gate = ((t >= 6144) & (t < 14336)) | ((t >= 22528) & (t < 28672))
    rng = np.random.default_rng(2)
    y = (0.5 * np.sin(2 * np.pi * 440 * t / sr) * gate + 1e-3 * rng.standard_normal(L)).astype(np.float32)
    clips = np.stack([y, np.zeros(L, dtype=np.float32), np.full(L, 0.25, dtype=np.float32)])
    yd = ops.to_device_f32(clips)
    mask = SG.detect_activity_batch(yd, sr, threshold=0.1).cpu().numpy()
    T = 1 + L // hop
    assert mask.shape == (3, T) and mask.dtype == np.int32
    # the restatement on the device's own RMS
    rms = ops.frame_stats(yd[:1], frame, hop, True, mask=1 << 7)[0, 7].cpu().numpy().astype(np.float64)
    r = (rms - 0.1) / np.std(rms)
    p = 1.0 / (1.0 + np.exp(-r))
    states, _, margin = R.viterbi_discriminative(np.stack([1.0 - p, p]), transition_loop(2, (0.5, 0.6)), want_margin=True)
    assert margin > SC.bound(T)
    assert np.array_equal(mask[0], states)
    centre = np.arange(T) * hop
    want = gate[np.minimum(centre, L - 1)]
    edges = np.array([6144, 14336, 22528, 28672])
    clear = np.min(np.abs(centre[:, None] - edges[None, :]), axis=1) > 2 * hop
    assert clear.sum() > T - 24 and np.array_equal(mask[0][clear] == 1, want[clear])
    # silence has a constant RMS (std = 0): inactive, never NaN; so has a constant signal away from its ends
    assert np.all(mask[1] == 0) and set(np.unique(mask[2])) <= {0, 1}
    segs = SG.segment_by_activity(y, sr, threshold=0.1)
    assert len(segs) == 2 and all(abs(a - e0) <= 3 * hop and abs(b - e1) <= 3 * hop
                                  for (a, b), (e0, e1) in zip(segs, ((6144, 14336), (22528, 28672))))
    assert SG.segment_by_activity(np.zeros(4096, dtype=np.float32), sr) == []
