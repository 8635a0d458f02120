"""The dynamics entries of the C ABI are declared, bound and exported, and refuse bad arguments before device work; the
ops refuse what is not served without a device; the plugin registers the three transforms; `features post` reports its
usage errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_dynamics_constants", "syg_dynamics_form", "syg_dynamics_work_bytes", "syg_dynamics_f32", "syg_stack_memory_f32"]


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


def test_constants_rule_and_workspace(h):
    from sygnals_amd import _dynamics as DY, ops
    k = ops.dynamics_constants()
    assert k["tile"] == 1024 and k["width_max"] == DY.WIDTH_MAX and k["order_max"] == DY.ORDER_MAX and k["max_out"] == DY.MAX_OUT
    assert k["units"] == 4 and 2 * k["lds_max"] <= 160 * 1024                     # two workgroups a CU at the least
    assert 4 * k["resident_max_t"] * k["units"] <= 64 * 1024
    assert h.syg_dynamics_constants(10) == -1 and h.syg_dynamics_constants(-1) == -1
    f = h.syg_dynamics_form
    assert f(k["resident_max_t"], 0) == 0 and f(k["resident_max_t"] + 1, 0) == 1
    assert f(k["resident_max_t_sliding"], 600) == 0 and f(k["resident_max_t_sliding"] + 1, 600) == 1
    assert f(3001, 4000) == 0                                                     # W >= T is the global form
    assert f(0, 0) == -1 and f(5, -1) == -1
    wb = h.syg_dynamics_work_bytes
    assert wb(2, 13, 1024) == 2 * 13 * 2 * 2 * 8 and wb(2, 13, 1025) == 2 * 13 * 2 * 3 * 8 and wb(0, 1, 1) == -1


def _dyn(h, p, x=True, out="far", B=2, K=3, T=100, sxb=None, sxk=None, sob=None, sok=None, cmvn=0, window=0, variance=1, statics=0,
         n_delta=1, width=9, mode=0, tab=True, form=0, work=None, work_bytes=0):
    sxk = T if sxk is None else sxk
    sxb = K * sxk if sxb is None else sxb
    blocks = statics + n_delta
    sok = T if sok is None else sok
    sob = blocks * K * sok if sob is None else sob
    o = {"far": C.c_void_p(p.value + (1 << 32)), "same": p, "near": C.c_void_p(p.value + 8), None: None}[out]
    return h.syg_dynamics_f32(p if x else None, B, K, T, sxb, sxk, o, sob, sok, cmvn, window, variance, statics, n_delta, width, mode,
                              0.0, p if tab else None, form, work, work_bytes, None)


def test_dynamics_refuses_before_device_work(h, p):
    err = h.syg_last_error
    assert _dyn(h, p, x=False) == -1 and b"null pointer" in err()
    assert _dyn(h, p, out=None) == -1 and b"null pointer" in err()
    assert _dyn(h, p, tab=False) == -1 and b"null pointer argument (tab)" in err()
    for kw in ({"B": 0}, {"K": 0}, {"T": 0}):
        assert _dyn(h, p, **kw) == -1 and b"empty input" in err()
    assert _dyn(h, p, sxk=99) == -1 and b"bad input strides" in err()
    assert _dyn(h, p, sok=99) == -1 and b"bad output strides" in err()
    for kw in ({"n_delta": 3}, {"statics": 0, "n_delta": 0}, {"cmvn": 2}):
        assert _dyn(h, p, **kw) == -1 and b"bad block selection" in err()
    assert _dyn(h, p, form=3) == -1 and b"form must be" in err()
    for w in (8, 1, 257, -9):
        assert _dyn(h, p, width=w) == -1 and b"width must be odd in [3, 255]" in err()
    assert _dyn(h, p, mode=5) == -1 and b"unknown mode" in err()
    assert _dyn(h, p, T=8) == -1 and b"window_length (9) must be less than or equal to the size of x (8)" in err()
    assert _dyn(h, p, B=1 << 11, K=1 << 10, T=(1 << 10) + 1) == -1 and b"is above 2^31" in err()
    for out in ("same", "near"):
        assert _dyn(h, p, out=out) == -1 and b"out overlaps x" in err()
    assert _dyn(h, p, out="near", cmvn=1, statics=1, n_delta=0) == -1 and b"out overlaps x" in err()
    assert _dyn(h, p, cmvn=1, statics=1, n_delta=0, window=-1) == -1 and b"window must be 0" in err()
    k = h.syg_dynamics_constants
    assert _dyn(h, p, T=5000, cmvn=1, statics=1, n_delta=0, window=k(3) + 1) == -1 and b"does not fit beside a tile: the bound is 1024" in err()
    assert _dyn(h, p, out="same", T=5000, cmvn=1, statics=1, n_delta=0, window=600) == -1 and b"cannot write onto its input" in err()
    assert _dyn(h, p, T=5000, cmvn=1, statics=1, n_delta=1, mode=3) == -1 and b"mode wrap with CMVN" in err()
    assert _dyn(h, p, T=5000, cmvn=1, statics=1, n_delta=0) == -1 and b"needs `work`" in err()
    assert _dyn(h, p, T=30000, form=1) == -1 and b"does not fit the resident form" in err()


def test_stack_memory_refuses_before_device_work(h, p):
    f, err = h.syg_stack_memory_f32, h.syg_last_error
    far = C.c_void_p(p.value + (1 << 32))
    assert f(None, 1, 3, 10, 30, 10, far, 2, 1, None) == -1 and b"null pointer" in err()
    assert f(p, 1, 3, 0, 30, 10, far, 2, 1, None) == -1 and b"empty input" in err()
    assert f(p, 1, 3, 10, 30, 10, far, 0, 1, None) == -1 and b"n_steps must be at least 1" in err()
    assert f(p, 1, 3, 10, 30, 10, far, 2, 0, None) == -1 and b"delay must be a non-zero integer" in err()
    assert f(p, 1 << 10, 1 << 10, 1 << 10, 1 << 20, 1 << 10, far, 3, 1, None) == -1 and b"is above 2^31" in err()
    assert f(p, 1, 3, 10, 30, 10, C.c_void_p(p.value + 8), 2, 1, None) == -1 and b"out overlaps x" in err()


def test_ops_refuse_without_a_device():
    from sygnals_amd import ops
    x = torch.zeros(2, 3, 20)
    for w in (8, 2, 1, 257):
        with pytest.raises(ValueError, match="width must be an odd integer in \\[3, 255\\]"):
            ops.delta(x, width=w)
    with pytest.raises(ValueError, match="order must be an integer in \\[1, min\\(4, width - 1\\) = 2\\]"):
        ops.delta(x, width=3, order=3)
    with pytest.raises(ValueError, match="unknown mode 'reflect' \\(served: interp, nearest, mirror, wrap, constant\\)"):
        ops.delta(x, mode="reflect")
    with pytest.raises(ValueError, match="If mode is 'interp', window_length must be less than or equal to the size of x"):
        ops.delta(x, width=21)
    with pytest.raises(ValueError, match="out overlaps x"):
        ops.delta(x, out=x)
    big = torch.zeros(2, 6, 20)
    with pytest.raises(ValueError, match="out overlaps x"):
        ops.delta(big[:, :3], out=big[:, 3:])                # the clips' spans interleave
    with pytest.raises(ValueError, match="out overlaps x"):
        ops.cmvn(big[:, :3], out=big[:, 1:4])
    with pytest.raises(ValueError, match="out overlaps x"):
        ops.feature_post(x, deltas=0, out=x)
    with pytest.raises(ValueError, match="out must be a float32 tensor \\[2, 3, 20\\]"):
        ops.delta(x, out=torch.zeros(2, 3, 21))
    with pytest.raises(ValueError, match="empty input"):
        ops.delta(torch.zeros(2, 0, 20))
    with pytest.raises(ValueError, match="empty input"):
        ops.cmvn(torch.zeros(0, 3, 20))
    with pytest.raises(ValueError, match="x must be a float32 tensor \\[B, K, T\\]"):
        ops.cmvn(torch.zeros(3, 20))
    with pytest.raises(ValueError, match="above 2\\^31"):
        ops.stack_memory(torch.zeros(1, 1, 1 << 20).expand(1 << 6, 1 << 6, 1 << 20), n_steps=2)
    for W in (0, -5, 2.5):
        with pytest.raises(ValueError, match="window must be None"):
            ops.cmvn(x, window=W)
    with pytest.raises(ValueError, match="delay must be a non-zero integer"):
        ops.stack_memory(x, delay=0)
    with pytest.raises(ValueError, match="n_steps must be an integer >= 1"):
        ops.stack_memory(x, n_steps=0)
    with pytest.raises(ValueError, match="deltas must be 0, 1 or 2"):
        ops.feature_post(x, deltas=3)
    with pytest.raises(ValueError, match="cmvn must be None, 'global' or a sliding window"):
        ops.feature_post(x, cmvn="sliding")
    with pytest.raises(ValueError, match="form must be None, 'resident' or 'tiled'"):
        ops.delta(x, form="fused")
    c, E = ops.delta_tables(9, 2)
    assert c.shape == (9,) and E.shape == (9, 9) and c.dtype == np.float32


def test_mirrors_refuse_without_a_device():
    from sygnals_amd.core.features import dynamics as DN
    with pytest.raises(ValueError, match="width must be an odd integer"):
        DN.delta(np.zeros((13, 20)), width=4)
    with pytest.raises(ValueError, match="If mode is 'interp'"):
        DN.delta(np.zeros((13, 5)))
    with pytest.raises(ValueError, match="unknown arguments"):
        DN.delta(np.zeros((13, 20)), trim=True)
    with pytest.raises(ValueError, match="empty input"):
        DN.cmvn(np.zeros((13, 0)))
    with pytest.raises(ValueError, match="must be \\[B, K, T\\]"):
        DN.cmvn_batch(np.zeros((13, 20)))


def test_plugin_registers_the_transforms():
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin
    from sygnals_amd.core.features import dynamics as DN

    class Reg:
        def __init__(self):
            self.t = {}

        def add_transform(self, name, fn):
            self.t[name] = fn
    r = Reg()
    SygnalsAmdPlugin().register_transforms(r)
    assert r.t["delta"] is DN.delta and r.t["cmvn"] is DN.cmvn and r.t["stack_memory"] is DN.stack_memory


def test_features_post_usage_errors(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    src = tmp_path / "f.csv"
    pd.DataFrame({"time": np.arange(5) * 0.01, "mfcc_0": np.arange(5.0), "rms": np.ones(5)}).to_csv(src, index=False)
    run = CliRunner().invoke
    r = run(cli, ["features", "post", str(src), "-o", str(tmp_path / "o.csv"), "--deltas", "2"])
    assert r.exit_code == 2 and "--mode interp" in r.output and "--width" in r.output and "5 frames" in r.output
    r = run(cli, ["features", "post", str(src), "-o", str(tmp_path / "o.csv"), "--deltas", "1", "--width", "4"])
    assert r.exit_code == 2 and "width must be an odd integer" in r.output
    r = run(cli, ["features", "post", str(src), "-o", str(tmp_path / "o.csv"), "--deltas", "1", "--width", "3", "--mode", "reflect"])
    assert r.exit_code == 2 and "unknown mode" in r.output
    r = run(cli, ["features", "post", str(src), "-o", str(tmp_path / "o.csv"), "--deltas", "3"])
    assert r.exit_code == 2
    r = run(cli, ["features", "post", str(src), "-o", str(tmp_path / "o.csv"), "--cmvn", "sliding", "--cmvn-window", "0"])
    assert r.exit_code == 2 and "--cmvn-window must be at least 1" in r.output
    r = run(cli, ["features", "post", str(src), "-o", str(tmp_path / "o.csv"), "--stack", "2", "--delay", "0"])
    assert r.exit_code == 2 and "delay must be a non-zero integer" in r.output
    only_time = tmp_path / "t.csv"
    pd.DataFrame({"time": np.arange(5) * 0.01}).to_csv(only_time, index=False)
    r = run(cli, ["features", "post", str(only_time), "-o", str(tmp_path / "o.csv")])
    assert r.exit_code == 2 and "no feature columns" in r.output
