"""The DTW entries of the C ABI are declared, bound and exported and reject bad arguments before device work; the
workspace rule and the constants agree with ops.dtw_plan; the mirror's refusals name what is served; the CLI reports its
usage errors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_dtw_tile", "syg_dtw_tile_max", "syg_dtw_resident_max_cols", "syg_dtw_run_max", "syg_dtw_cost_tile", "syg_dtw_form",
       "syg_dtw_work_bytes", "syg_dtw_cost_f32", "syg_dtw_f32"]


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_double * 64)()                       # never dereferenced: every call is rejected
    return C.cast(buf, C.c_void_p)


def _lens(*v):
    a = (C.c_int32 * len(v))(*v)
    return C.cast(a, C.c_void_p), a


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)
    assert h.syg_abi_version() == 1


def test_constants_and_plan(h):
    from sygnals_amd import ops
    k = ops.dtw_constants()
    assert k == dict(tile=h.syg_dtw_tile(), tile_max=h.syg_dtw_tile_max(), resident_max_cols=h.syg_dtw_resident_max_cols(),
                     run_max=h.syg_dtw_run_max(), cost_tile=h.syg_dtw_cost_tile())
    assert k["resident_max_cols"] == 64 * k["run_max"] and 1 <= k["tile"] <= k["tile_max"] <= k["resident_max_cols"]
    for B, N, M in ((1, 1, 1), (1024, 94, 94), (256, 1000, 1000), (3, 5000, k["resident_max_cols"]),
                    (1, 7, k["resident_max_cols"] + 1), (1, 16384, 16384), (2, 4097, 3001)):
        pl = ops.dtw_plan(B, N, M)
        tiled = M > k["resident_max_cols"]                            # the rule
        assert pl["form"] == ("tiled" if tiled else "resident") and h.syg_dtw_form(B, N, M, -1) == int(tiled)
        t = k["tile"]
        want = B * (-(-N // t) * M + -(-M // t) * N) * 8 if tiled else 0
        assert pl["work_bytes"] == want == h.syg_dtw_work_bytes(B, N, M, -1, 0)
        assert pl["steps_bytes"] == B * N * M and ops.dtw_plan(B, N, M, want_steps=False)["steps_bytes"] == 0
    # a forced form and a small tile: one row of M per tile row, one column of N per tile column, float64
    assert ops.dtw_plan(2, 17, 9, form="tiled", tile=8) == dict(form="tiled", work_bytes=2 * (3 * 9 + 2 * 17) * 8, steps_bytes=2 * 17 * 9)
    assert ops.dtw_plan(2, 17, 9, form="resident")["work_bytes"] == 0
    with pytest.raises(ValueError):
        ops.dtw_plan(1, 4, 4, form="banded")
    from sygnals_amd._lib import SygnalsHipError
    with pytest.raises(SygnalsHipError, match="pair-resident form serves"):
        ops.dtw_plan(1, 4, k["resident_max_cols"] + 1, form="resident")
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (65536, 4, 4)):
        assert h.syg_dtw_work_bytes(*bad, -1, 0) == -1 and h.syg_dtw_form(*bad, -1) == -1
    assert h.syg_dtw_work_bytes(1, 4, 4, 2, 0) == -1 and h.syg_dtw_work_bytes(1, 4, 4, 1, -1) == -1
    assert h.syg_dtw_work_bytes(1, 4, 4, 1, k["tile_max"] + 1) == -1


def _cost(h, p, X=True, Y=True, B=2, K=3, N=10, M=12, ldx=10, ldy=12, bsx=30, bsy=36, xl=None, yl=None, xlh=None, ylh=None,
          metric=0, Cout=True):
    a = lambda on: p if on else None                                 # noqa: E731
    return h.syg_dtw_cost_f32(a(X), a(Y), B, K, N, M, ldx, ldy, bsx, bsy, xl, yl, xlh, ylh, metric, a(Cout), None)


def _dtw(h, p, Cin=True, B=2, N=10, M=12, ldc=12, bsc=120, xl=None, yl=None, xlh=None, ylh=None, wm=None, wa=None, subseq=0,
         form=-1, tile=0, D=False, steps=False, cost=True, end_col=True, path=False, path_len=False, work=False, work_bytes=0):
    a = lambda on: p if on else None                                 # noqa: E731
    return h.syg_dtw_f32(a(Cin), B, N, M, ldc, bsc, xl, yl, xlh, ylh, wm, wa, subseq, form, tile, a(D), a(steps), a(cost),
                         a(end_col), a(path), a(path_len), a(work), work_bytes, None)


def test_cost_rejects(h, p):
    for kw in ({"X": False}, {"Y": False}, {"Cout": False}):
        assert _cost(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"N": 0}, {"M": 0}, {"N": -3}, {"M": (1 << 30) + 1, "ldy": 1 << 31}):
        assert _cost(h, p, **kw) == -1 and b"must be in [1, 2^30]" in h.syg_last_error()
    for K in (0, -1):
        assert _cost(h, p, K=K) == -1 and b"K=" in h.syg_last_error()
    for B in (0, -1, 65536):
        assert _cost(h, p, B=B) == -1 and b"must be in [1, 65535]" in h.syg_last_error()
    for kw in ({"ldx": 9}, {"ldy": 11}):
        assert _cost(h, p, **kw) == -1 and b"above its row stride" in h.syg_last_error()
    assert _cost(h, p, bsx=-1) == -1 and b"batch strides" in h.syg_last_error()
    for metric in (-1, 4, 99):
        assert _cost(h, p, metric=metric) == -1 and b"metric must be" in h.syg_last_error()
    good, keep = _lens(10, 1)
    for v, name, full in (((0, 5), "x_len", 10), ((11, 5), "x_len", 10), ((5, -2), "x_len", 10)):
        bad, keep2 = _lens(*v)
        assert _cost(h, p, xl=p, xlh=bad) == -1 and b"x_len[" in h.syg_last_error() and b"outside [1, 10]" in h.syg_last_error()
    bad, keep2 = _lens(12, 13)
    assert _cost(h, p, yl=p, ylh=bad) == -1 and b"y_len[1]=13 is outside [1, 12]" in h.syg_last_error()
    assert _cost(h, p, xl=p) == -1 and b"go together" in h.syg_last_error()
    assert _cost(h, p, ylh=good) == -1 and b"go together" in h.syg_last_error()


def test_dtw_rejects(h, p):
    for kw in ({"Cin": False}, {"cost": False}, {"end_col": False}):
        assert _dtw(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"N": 0}, {"M": 0}, {"M": -1}):
        assert _dtw(h, p, **kw) == -1 and b"must be in [1, 2^30]" in h.syg_last_error()
    for B in (0, 65536):
        assert _dtw(h, p, B=B) == -1 and b"must be in [1, 65535]" in h.syg_last_error()
    assert _dtw(h, p, ldc=11) == -1 and b"above the row stride ldc=11" in h.syg_last_error()
    for form in (-2, 2):
        assert _dtw(h, p, form=form) == -1 and b"form must be" in h.syg_last_error()
    for tile in (-1, h.syg_dtw_tile_max() + 1):
        assert _dtw(h, p, form=1, tile=tile) == -1 and b"tile=" in h.syg_last_error()
    wide = h.syg_dtw_resident_max_cols() + 1
    assert _dtw(h, p, M=wide, ldc=wide, form=0) == -1 and b"pair-resident form serves" in h.syg_last_error()
    bad, keep = _lens(10, 11)
    assert _dtw(h, p, xl=p, xlh=bad) == -1 and b"x_len[1]=11 is outside [1, 10]" in h.syg_last_error()
    bad, keep = _lens(0, 3)
    assert _dtw(h, p, yl=p, ylh=bad) == -1 and b"y_len[0]=0 is outside [1, 12]" in h.syg_last_error()
    assert _dtw(h, p, yl=p) == -1 and b"go together" in h.syg_last_error()
    for w in ((1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0)):
        arr = (C.c_double * 3)(*w)
        assert _dtw(h, p, wm=C.cast(arr, C.c_void_p)) == -1 and b"weights must be finite" in h.syg_last_error()
        assert _dtw(h, p, wa=C.cast(arr, C.c_void_p)) == -1 and b"weights must be finite" in h.syg_last_error()
    assert _dtw(h, p, path=True) == -1 and b"path and path_len go together" in h.syg_last_error()
    assert _dtw(h, p, path=True, path_len=True) == -1 and b"path needs steps" in h.syg_last_error()
    # the tiled form: no workspace, or one byte short
    need = h.syg_dtw_work_bytes(2, 10, 12, 1, 4)
    assert need == 2 * (3 * 12 + 3 * 10) * 8
    for kw in ({}, {"work": True, "work_bytes": need - 1}, {"work": True, "work_bytes": 0}):
        assert _dtw(h, p, form=1, tile=4, **kw) == -1
        assert b"needs a workspace of syg_dtw_work_bytes() = %d bytes" % need in h.syg_last_error()


def test_signatures():
    import sygnals_amd.core.alignment as A
    from sygnals_amd import ops
    sig = inspect.signature(A.dtw)
    assert list(sig.parameters) == ["X", "Y", "C", "metric", "step_sizes_sigma", "weights_add", "weights_mul", "subseq", "backtrack",
                                    "global_constraints", "band_rad", "return_steps"]
    assert [sig.parameters[k].default for k in sig.parameters] == [None, None, None, "euclidean", None, None, None, False, True,
                                                                   False, 0.25, False]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert list(inspect.signature(A.dtw_batch).parameters) == ["X", "Y", "C", "metric", "x_len", "y_len", "subseq", "weights_add",
                                                               "weights_mul", "return_D"]
    assert list(inspect.signature(A.dtw_distance_batch).parameters) == ["X", "Y", "C", "metric", "x_len", "y_len", "subseq",
                                                                        "weights_add", "weights_mul"]
    assert list(inspect.signature(ops.dtw_plan).parameters)[:4] == ["B", "N", "M", "want_steps"]
    assert list(inspect.signature(ops.dtw_cost).parameters) == ["X", "Y", "metric", "x_len", "y_len"]
    assert inspect.signature(ops.dtw).parameters["form"].default is None


def test_mirror_refusals_need_no_device():
    import sygnals_amd.core.alignment as A
    x, y = np.zeros((2, 5)), np.zeros((2, 7))
    served = ("euclidean", "sqeuclidean", "cityblock", "cosine", "[[1,1],[0,1],[1,0]]", "subseq")
    for kw in ({"step_sizes_sigma": [[1, 1], [1, 2], [2, 1]]}, {"step_sizes_sigma": [[1, 1], [1, 0], [0, 1]]},
               {"step_sizes_sigma": [[1, 1]]}, {"global_constraints": True}, {"metric": "chebyshev"},
               {"metric": lambda a, b: 0.0}, {"weights_mul": [1.0, 2.0]}, {"weights_add": [0.0, float("inf"), 0.0]}):
        with pytest.raises(ValueError) as e:
            A.dtw(x, y, **kw)
        assert "served" in str(e.value) and all(s in str(e.value) for s in served), kw
    with pytest.raises(ValueError, match="librosa"):
        A.dtw(x, y, global_constraints=True)
    for args, kw in (((), {}), ((x,), {}), ((x, y), {"C": np.zeros((5, 7))}), ((x,), {"C": np.zeros((5, 7))})):
        with pytest.raises(ValueError, match="either X and Y or a cost matrix C"):
            A.dtw(*args, **kw)
    for bad in (np.nan, np.inf, -np.inf):
        Cm = np.ones((4, 4)); Cm[2, 1] = bad
        with pytest.raises(ValueError, match="C must be finite"):
            A.dtw(C=Cm)
    with pytest.raises(ValueError, match="same number of features"):
        A.dtw(np.zeros((2, 5)), np.zeros((3, 5)))
    with pytest.raises(ValueError) as e:
        A.dtw(np.zeros(70000, dtype=np.float32), np.zeros(70000, dtype=np.float32))
    assert "cap" in str(e.value) and str(A.MAX_STEP_CELLS) in str(e.value) and "dtw_distance_batch" in str(e.value)
    t = torch.zeros((2, 3, 8))
    for call in (lambda: A.dtw_batch(t, t, metric="minkowski"), lambda: A.dtw_distance_batch(t, t, metric="minkowski"),
                 lambda: A.dtw_batch(t, t, weights_mul=[1, 2, float("nan")])):
        with pytest.raises(ValueError) as e:
            call()
        assert "served" in str(e.value)
    with pytest.raises(ValueError, match="either X and Y or a cost tensor C"):
        A.dtw_batch(t, t, C=torch.zeros((2, 8, 8)))
    with pytest.raises(ValueError, match="either X and Y or a cost tensor C"):
        A.dtw_distance_batch()


def test_cli_usage_errors(tmp_path):
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli.main import cli
    pcm = (np.sin(np.arange(4000) * 0.05) * 8000).astype(np.int16)
    wavfile.write(tmp_path / "a.wav", 8000, pcm)
    wavfile.write(tmp_path / "b.wav", 16000, pcm)
    r = CliRunner().invoke(cli, ["dsp", "dtw", str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), "-o", str(tmp_path / "p.csv")])
    assert r.exit_code == 2 and "dsp resample" in r.output and "8000" in r.output and "16000" in r.output
    import pandas as pd
    pd.DataFrame({"value": np.arange(8.0)}).to_csv(tmp_path / "x.csv", index=False)
    r = CliRunner().invoke(cli, ["dsp", "dtw", str(tmp_path / "x.csv"), str(tmp_path / "x.csv"), "-o", str(tmp_path / "p.csv"),
                                 "--on", "mfcc"])
    assert r.exit_code == 2 and "--on samples" in r.output
    r = CliRunner().invoke(cli, ["dsp", "dtw", str(tmp_path / "x.csv"), str(tmp_path / "x.csv"), "-o", str(tmp_path / "p.csv"),
                                 "--metric", "chebyshev"])
    assert r.exit_code == 2 and "--metric" in r.output
    r = CliRunner().invoke(cli, ["dsp", "--help"])
    assert r.exit_code == 0 and "dtw" in r.output
