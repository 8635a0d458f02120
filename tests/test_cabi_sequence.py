"""The Viterbi entries of the C ABI are declared, bound and exported, report their constants, size their workspace and
refuse bad arguments before device work; ops.viterbi and core.sequence refuse what is not served without a device; the
plugin registers the public functions."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_viterbi_constants", "syg_viterbi_form", "syg_viterbi_work_bytes", "syg_viterbi_f32"]


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_double * 4096)()                     # never dereferenced: every call is refused
    return C.cast(buf, C.c_void_p)


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)
    assert h.syg_abi_version() == 1


def test_constants(h):
    from sygnals_amd import ops
    K = ops.viterbi_constants()
    assert set(K) == {"s_max", "s_lds", "s_narrow", "tile", "work_max"}
    assert [h.syg_viterbi_constants(i) for i in range(4)] == [K["s_max"], K["s_lds"], K["s_narrow"], K["tile"]]
    assert h.syg_viterbi_constants(4) == -1 and h.syg_viterbi_constants(-1) == -1
    assert K["s_max"] == 1024 and 1 <= K["s_narrow"] < 64 < K["s_lds"] < K["s_max"] and K["tile"] >= 2
    # the table lives in LDS while 8 S^2 + the two score rows + the emission tile (rows of S | 1) fit 160 KiB
    lds = lambda S: 8 * (S * S + 2 * S + K["tile"] * (S | 1))
    assert lds(K["s_lds"]) <= 160 * 1024 < lds(K["s_lds"] + 1)
    # the launch constants keep exactly their five keys
    assert len(ops.launch_constants()) == 5
    assert ops.viterbi_form(1, 2) == "wide" and ops.viterbi_form(1000, K["s_narrow"] + 1) == "wide"
    assert ops.viterbi_form(1000, 2) in ("wide", "narrow")
    with pytest.raises(ValueError, match="not served"):
        ops.viterbi_form(1, 2000)


def test_work_bytes(h):
    from sygnals_amd import ops
    wb = h.syg_viterbi_work_bytes
    assert wb(1, 1, 1) == 8                                  # one pointer and the narrow form's last word, rounded up
    assert wb(3, 25, 65) == (3 * 25 * 65 + 12 + 7) // 8 * 8  # a byte a pointer up to 256 states
    assert wb(2, 256, 10) == 2 * 256 * 10 + 8 and wb(2, 257, 10) == 2 * 257 * 10 * 2 + 8       # two bytes beyond
    assert wb(1, 1024, 3001) == 1024 * 3001 * 2 + 8
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1025, 1), (1 << 31, 1, 1), (1, 1, 1 << 31), (1 << 20, 1024, 1 << 20)):
        assert wb(*bad) == -1
    assert ops.viterbi_work_bytes(3, 25, 65) == wb(3, 25, 65)
    from sygnals_amd._lib import SygnalsHipError
    with pytest.raises(SygnalsHipError, match="refuses these arguments"):
        ops.viterbi_work_bytes(1, 1025, 1)


def vit_args(p, **kw):
    a = dict(em=p, dtype=0, log_domain=0, sb=50, ss=10, st=1, B=1, S=5, T=10, lengths=None, lt=p, tbs=0, li=p, ibs=0, lm=None,
             mbs=0, eps=1e-38, work=p, work_bytes=4096, states=p, logp=p, form=0)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_entry_refuses_before_device_work(h, p):
    f = h.syg_viterbi_f32
    for kw, msg in ((dict(em=None), b"null pointer"), (dict(lt=None), b"null pointer"), (dict(li=None), b"null pointer"),
                    (dict(work=None), b"null pointer"), (dict(states=None), b"null pointer"), (dict(logp=None), b"null pointer"),
                    (dict(dtype=2), b"dtype 2 is not served"), (dict(S=0), b"outside 1 .. 1024"), (dict(S=1025), b"outside 1 .. 1024"),
                    (dict(B=0), b"bad B / T"), (dict(T=0), b"bad B / T"), (dict(T=1 << 31), b"bad B / T"),
                    (dict(B=1 << 20, S=1024, T=1 << 20, work_bytes=1 << 62), b"2^40 back pointers"),
                    (dict(work_bytes=8), b"syg_viterbi_work_bytes asks for 56"), (dict(ss=-1), b"negative emission stride"),
                    (dict(tbs=5), b"log_trans must be 0"), (dict(ibs=4), b"log_init must be 0"),
                    (dict(lm=p, mbs=3), b"log_marginal must be 0"), (dict(eps=-1.0), b"eps must be finite"),
                    (dict(eps=float("nan")), b"eps must be finite"), (dict(form=3), b"form 3 is not served"),
                    (dict(form=2), b"narrow form serves S <= ")):
        assert f(*vit_args(p, **kw)) == -1, kw
        assert msg in h.syg_last_error(), (kw, h.syg_last_error())


def _prob(B=2, S=3, T=6, dtype=torch.float32):
    return torch.full((B, S, T), 1.0 / S, dtype=dtype)


def test_ops_refuses_without_a_device():
    from sygnals_amd import ops
    x = _prob()
    tr = np.full((3, 3), 1.0 / 3)
    for kw, msg in ((dict(prob=None), "either prob or log_prob"), (dict(log_prob=x), "either prob or log_prob"),
                    (dict(prob=x[0]), r"tensor \[B, S, T\]"), (dict(prob=x.to(torch.float16)), r"tensor \[B, S, T\]"),
                    (dict(prob=np.ones((1, 3, 4), dtype=np.float32)), r"tensor \[B, S, T\]"),
                    (dict(prob=torch.ones(1, 1025, 2)), "above the cap of 1024"),
                    (dict(transition=None), "transition is required"),
                    (dict(transition=np.ones((3, 4)) / 4), "must be square"), (dict(transition=np.ones((2, 2)) / 2), "S = 3 states"),
                    (dict(transition=np.ones((5, 3, 3)) / 3), "5 transition matrices for 2 clips"),
                    (dict(transition=np.array([[1.5, -0.5, 0], [0, 1, 0], [0, 0, 1.0]])), "negative entries"),
                    (dict(transition=np.full((3, 3), 0.3)), "rows of transition must sum to 1"),
                    (dict(p_init=[0.5, 0.6, -0.1]), "p_init must be a probability distribution"),
                    (dict(p_init=[0.5, 0.6, 0.1]), "p_init must be a probability distribution"),
                    (dict(p_init=[0.5, 0.5]), "p_init must hold one value per state"),
                    (dict(p_state=[0.2, 0.2, 0.2]), "p_state must be a probability distribution"),
                    (dict(lengths=[1, 7]), r"lengths must hold one integer in \[1, 6\]"), (dict(lengths=[0, 3]), "lengths must hold"),
                    (dict(lengths=[3]), "lengths must hold"), (dict(lengths=[1.0, 2.0]), "lengths must hold"),
                    (dict(eps=-1e-3), "eps=.* must be finite and not negative"), (dict(form="tall"), "form='tall' is not served"),
                    (dict(form="narrow", prob=_prob(S=9), transition=np.full((9, 9), 1 / 9)), "narrow form serves S <="),
                    (dict(chunk=0), "chunk=0 must be a positive integer"),
                    (dict(out=torch.zeros(2, 6)), r"out must be a int32 tensor \[2, 6\]")):
        a = dict(prob=x, transition=tr)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.viterbi(**a)
    if not torch.cuda.is_available():          # everything is accepted: the next thing asked for is the device
        from sygnals_amd._lib import SygnalsHipError
        with pytest.raises(SygnalsHipError, match="needs an AMD GPU"):
            ops.viterbi(x, tr)


def test_mirrors_refuse_without_a_device():
    from sygnals_amd.core import sequence as SQ
    p = np.full((3, 6), 1.0 / 3, dtype=np.float32)
    tr = SQ.transition_uniform(3)
    for fn in (SQ.viterbi, SQ.viterbi_discriminative):
        with pytest.raises(ValueError, match="must be square"):
            fn(p, np.ones((3, 2)) / 2)
        with pytest.raises(ValueError, match="S = 3 states"):
            fn(p, SQ.transition_uniform(4))
        with pytest.raises(ValueError, match="negative entries"):
            fn(p, np.array([[2.0, -1.0, 0], [0, 1, 0], [0, 0, 1]]))
        with pytest.raises(ValueError, match="rows of transition must sum to 1"):
            fn(p, tr * 0.9)
        with pytest.raises(ValueError, match=r"prob must lie in \[0, 1\]"):
            fn(p * 4, tr)
        with pytest.raises(ValueError, match=r"prob must lie in \[0, 1\]"):
            fn(-p, tr)
        with pytest.raises(ValueError, match="p_init must be a probability distribution"):
            fn(p, tr, p_init=[0.5, 0.25, 0.2])
        with pytest.raises(ValueError, match="at least one state and one frame"):
            fn(p[0], tr)
    with pytest.raises(ValueError, match="sum to 1 over the states"):
        SQ.viterbi_discriminative(p * 0.5, tr)
    with pytest.raises(ValueError, match="p_state must be a probability distribution"):
        SQ.viterbi_discriminative(p, tr, p_state=[0.5, 0.6, -0.1])
    pb = np.full((4, 6), 0.5, dtype=np.float32)
    loop = SQ.transition_loop(2, 0.9)
    with pytest.raises(ValueError, match=r"\[2, 2\] or one per label \[4, 2, 2\]"):
        SQ.viterbi_binary(pb, SQ.transition_uniform(3))
    with pytest.raises(ValueError, match=r"\[2, 2\] or one per label \[4, 2, 2\]"):
        SQ.viterbi_binary(pb, np.stack([loop] * 3))
    with pytest.raises(ValueError, match="rows of transition must sum to 1"):
        SQ.viterbi_binary(pb, loop * 0.5)
    with pytest.raises(ValueError, match=r"prob must lie in \[0, 1\]"):
        SQ.viterbi_binary(pb * 3, loop)
    with pytest.raises(ValueError, match=r"p_state must be a scalar or one value per label \(\[4\]\) in \[0, 1\]"):
        SQ.viterbi_binary(pb, loop, p_state=1.5)
    with pytest.raises(ValueError, match="p_init must be a scalar or one value per label"):
        SQ.viterbi_binary(pb, loop, p_init=[0.5, 0.5])
    with pytest.raises(ValueError, match=r"float32 tensor \[B, L\]"):
        from sygnals_amd.core.segmentation import detect_activity_batch
        detect_activity_batch(np.ones((1, 100), dtype=np.float32), 22050)


def test_plugin_registers_the_sequence_functions():
    from sygnals_amd.core import segmentation as SG
    from sygnals_amd.core import sequence as SQ
    from sygnals_amd.plugins import SygnalsAmdPlugin

    class Reg:
        def __init__(self):
            self.f = {}

        def add_feature(self, name, fn):
            self.f[name] = fn
    r = Reg()
    SygnalsAmdPlugin().register_feature_extractors(r)
    assert r.f["viterbi"] is SQ.viterbi and r.f["segment_by_activity"] is SG.segment_by_activity
    assert set(SQ.__all__) == {"viterbi", "viterbi_discriminative", "viterbi_binary", "viterbi_batch", "viterbi_discriminative_batch",
                               "viterbi_binary_batch", "transition_uniform", "transition_loop", "transition_cycle", "transition_local"}
