"""The SpecAugment entries of the C ABI are declared, bound and exported and refuse bad arguments before device work; the
op and the public functions refuse what is not served without a device, each with its message; the signatures are the
stated ones; `augment spec-augment` reports its usage errors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from sygnals_amd import _specaug as SA
from tests.test_cabi_symbols import declared_functions

NEW = ["syg_spec_augment_constants", "syg_spec_augment_work_bytes", "syg_spec_augment_f32"]


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


def test_constants_and_workspace(h):
    from sygnals_amd import _rng, ops
    k = ops.spec_augment_constants()
    assert k["stream"] == SA.STREAM_SPEC == 2 and k["max_masks"] == SA.MAX_MASKS == 16 and k["max_elems"] == SA.MAX_ELEMS == 1 << 31
    assert k["stream"] not in (_rng.STREAM_NOISE, _rng.STREAM_ROW)
    assert k["tile"] == 4096 and k["resident_max"] >= k["tile"]
    assert h.syg_spec_augment_constants(5) == -1 and h.syg_spec_augment_constants(-1) == -1
    wb = h.syg_spec_augment_work_bytes
    assert wb(2, 13, 65) == 2 * 1 * 8 + 8 and wb(3, 80, 3001) == 3 * 59 * 8 + 16
    assert wb(0, 1, 1) == -1 and wb(1, 0, 1) == -1 and wb(1 << 11, 1 << 10, (1 << 10) + 1) == -1


def _spec(h, p, x=True, out="far", B=2, K=13, T=100, sxb=None, sxk=None, sob=None, sok=None, first_row=0, nf=2, F=5, nt=2, Wt=10,
          ratio=1.0, W=0, mean=0, value=0.0, form=0, work=None, work_bytes=0):
    sxk = T if sxk is None else sxk
    sxb = K * sxk if sxb is None else sxb
    sok = T if sok is None else sok
    sob = K * sok if sob is None else sob
    o = {"far": C.c_void_p(p.value + (1 << 32)), "same": p, "near": C.c_void_p(p.value + 8), None: None}[out]
    return h.syg_spec_augment_f32(p if x else None, B, K, T, sxb, sxk, o, sob, sok, None, 7, first_row, nf, F, nt, Wt, ratio, W, mean,
                                  value, form, work, work_bytes, None)


def test_entry_refuses_before_device_work(h, p):
    err = h.syg_last_error
    assert _spec(h, p, x=False) == -1 and b"null pointer" in err()
    assert _spec(h, p, out=None) == -1 and b"null pointer" in err()
    for kw in ({"B": 0}, {"K": 0}, {"T": 0}):
        assert _spec(h, p, **kw) == -1 and b"empty input" in err()
    assert _spec(h, p, B=1 << 11, K=1 << 10, T=(1 << 10) + 1, F=0) == -1 and b"above 2^31" in err()
    assert _spec(h, p, sxk=99) == -1 and b"bad input strides" in err()
    assert _spec(h, p, sok=99) == -1 and b"bad output strides" in err()
    for kw in ({"nf": -1}, {"nf": 17}, {"nt": -1}, {"nt": 17}):
        assert _spec(h, p, **kw) == -1 and b"must lie in 0 .. 16" in err()
    for F in (-1, 14):
        assert _spec(h, p, F=F) == -1 and b"freq_width must lie in [0, K = 13]" in err()
    for kw in ({"Wt": -1}, {"W": -1}):
        assert _spec(h, p, **kw) == -1 and b"must not be negative" in err()
    for r in (0.0, -0.5, 1.5, float("nan")):
        assert _spec(h, p, ratio=r) == -1 and b"time_ratio must lie in (0, 1]" in err()
    for v in (float("inf"), float("nan")):
        assert _spec(h, p, value=v) == -1 and b"mask_value must be finite" in err()
    assert _spec(h, p, mean=2) == -1 and b"mean must be 0" in err()
    assert _spec(h, p, first_row=-1) == -1 and b"must lie in [0, 2^31)" in err()
    assert _spec(h, p, first_row=(1 << 31) - 1) == -1 and b"must lie in [0, 2^31)" in err()
    assert _spec(h, p, form=3) == -1 and b"form must be" in err()
    assert _spec(h, p, out="near") == -1 and b"out overlaps x" in err()
    assert _spec(h, p, out="same", W=3) == -1 and b"out overlaps x (with time_warp > 0" in err()
    assert _spec(h, p, out="same", W=80) == -1 and b"out overlaps x (with time_warp > 0" in err()     # though no clip is warped
    assert _spec(h, p, mean=1, form=2) == -1 and b"the mean needs `work`" in err()
    assert _spec(h, p, mean=1, T=5000) == -1 and b"the mean needs `work`" in err()
    assert _spec(h, p, mean=1, out="same") == -1 and b"the mean needs `work`" in err()
    assert _spec(h, p, out="same", nf=0, nt=0) == 0                    # nothing to write, nothing launched


def test_op_refuses_without_a_device():
    from sygnals_amd import ops
    x = torch.zeros(2, 13, 40)
    f = ops.spec_augment
    for kw in ({"freq_masks": 17}, {"freq_masks": -1}, {"time_masks": 17}, {"time_masks": -1}):
        with pytest.raises(ValueError, match="must lie in 0 .. 16"):
            f(x, 1, **kw)
    with pytest.raises(ValueError, match="freq_masks must be an integer"):
        f(x, 1, freq_masks=1.5)
    for F in (14, -1):
        with pytest.raises(ValueError, match="freq_width must lie in \\[0, K = 13\\]"):
            f(x, 1, freq_width=F)
    with pytest.raises(ValueError, match="time_width must not be negative"):
        f(x, 1, freq_width=5, time_width=-1)
    with pytest.raises(ValueError, match="time_warp must not be negative"):
        f(x, 1, freq_width=5, time_warp=-1)
    for r in (0.0, 1.0001, -1, float("nan"), "half"):
        with pytest.raises(ValueError, match="time_ratio must lie in \\(0, 1\\]"):
            f(x, 1, freq_width=5, time_ratio=r)
    for v in (float("inf"), float("nan"), 1e39, "median", None):
        with pytest.raises(ValueError, match="mask_value must be a finite float or 'mean'"):
            f(x, 1, freq_width=5, mask_value=v)
    with pytest.raises(ValueError, match="lengths must be 2 integers, one per clip"):
        f(x, 1, freq_width=5, lengths=[40, 40, 40])
    with pytest.raises(ValueError, match="lengths must be 2 integers, one per clip"):
        f(x, 1, freq_width=5, lengths=[40.0, 3.5])
    for ln in ([0, 40], [1, 41]):
        with pytest.raises(ValueError, match="lengths must lie in \\[1, T = 40\\]"):
            f(x, 1, freq_width=5, lengths=torch.tensor(ln))
    with pytest.raises(ValueError, match="empty input"):
        f(torch.zeros(2, 0, 40), 1, freq_width=0)
    with pytest.raises(ValueError, match="empty input"):
        f(torch.zeros(0, 13, 40), 1, freq_width=5)
    with pytest.raises(ValueError, match="x must be a float32 tensor \\[B, K, T\\]"):
        f(torch.zeros(13, 40), 1)
    with pytest.raises(ValueError, match="above 2\\^31"):
        f(torch.zeros(1, 1, 1 << 20).expand(1 << 6, 1 << 6, 1 << 20), 1)
    with pytest.raises(ValueError, match="rows first_row .. first_row \\+ B - 1 must lie in \\[0, 2\\^31\\)"):
        f(x, 1, first_row=(1 << 31) - 1, freq_width=5)
    with pytest.raises(ValueError, match="seed must be an integer in \\[0, 2\\^64\\)"):
        f(x, -1, freq_width=5)
    with pytest.raises(ValueError, match="out overlaps x"):
        f(x, 1, freq_width=5, time_warp=3, out=x)
    big = torch.zeros(2, 26, 40)
    with pytest.raises(ValueError, match="out overlaps x \\(only out = x itself is served\\)"):
        f(big[:, :13], 1, freq_width=5, out=big[:, 1:14])
    with pytest.raises(ValueError, match="out must be a float32 tensor \\[2, 13, 40\\]"):
        f(x, 1, freq_width=5, out=torch.zeros(2, 13, 41))
    with pytest.raises(ValueError, match="form must be None, 'resident' or 'tiled'"):
        f(x, 1, freq_width=5, mask_value="mean", form="fused")


def test_public_functions_refuse_without_a_device():
    from sygnals_amd.core import augment as A
    x = torch.zeros(2, 13, 40)
    with pytest.raises(ValueError, match="mode 'bicubic' is not served \\(the time warp is piecewise 'linear'\\)"):
        A.spec_augment_batch(x, freq_width=5, mode="bicubic")
    with pytest.raises(ValueError, match="unknown mode 'nearest' \\(served: 'linear'\\)"):
        A.time_warp_batch(x, 3, mode="nearest")
    with pytest.raises(ValueError, match="mode 'bicubic' is not served"):
        A.spec_augment(np.zeros((13, 40)), freq_width=5, mode="bicubic")
    with pytest.raises(ValueError, match="freq_width must lie in \\[0, K = 13\\]"):
        A.spec_augment_batch(x)                                        # the default width 27 needs 27 rows
    with pytest.raises(ValueError, match="freq_width must lie in \\[0, K = 13\\]"):
        A.freq_mask_batch(x, 2, 14)
    with pytest.raises(ValueError, match="time_ratio must lie in \\(0, 1\\]"):
        A.time_mask_batch(x, 2, 10, time_ratio=0.0)
    with pytest.raises(ValueError, match="time_warp must not be negative"):
        A.time_warp_batch(x, -2)
    with pytest.raises(ValueError, match="S must be \\[K, T\\]"):
        A.spec_augment(np.zeros((2, 13, 40)))
    with pytest.raises(ValueError, match="empty input"):
        A.spec_augment(np.zeros((13, 0)))
    with pytest.raises(ValueError, match="mask_value must be a finite float or 'mean'"):
        A.spec_augment(np.zeros((13, 40)), freq_width=5, mask_value="zero")
    with pytest.raises(ValueError, match="lengths must lie in \\[1, T = 40\\]"):
        A.spec_augment_batch(x, freq_width=5, lengths=[0, 1])
    with pytest.raises(ValueError, match="x must be a float32 tensor \\[B, K, T\\]"):
        A.spec_augment_batch(torch.zeros(13, 40), freq_width=5)


def test_signatures_are_the_stated_ones():
    from sygnals_amd import ops
    from sygnals_amd.core import augment as A

    def names(fn):
        return list(inspect.signature(fn).parameters)

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}
    stated = ["x", "seed", "first_row", "freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "time_warp", "mask_value",
              "lengths", "out"]
    assert names(ops.spec_augment)[:len(stated)] == stated
    d = defaults(ops.spec_augment)
    assert (d["first_row"], d["freq_masks"], d["freq_width"], d["time_masks"], d["time_width"], d["time_ratio"], d["time_warp"],
            d["mask_value"], d["lengths"], d["out"]) == (0, 2, 27, 2, 100, 1.0, 0, 0.0, None, None) and "seed" not in d
    d = defaults(A.spec_augment_batch)
    assert names(A.spec_augment_batch)[0] == "x"
    assert (d["seed"], d["first_row"], d["lengths"], d["out"], d["return_seed"], d["return_params"]) == (None, 0, None, None, False, False)
    assert (d["freq_masks"], d["freq_width"], d["time_masks"], d["time_width"], d["time_ratio"], d["time_warp"], d["mask_value"],
            d["mode"]) == (2, 27, 2, 100, 1.0, 0, 0.0, "linear")
    assert names(A.spec_augment)[0] == "S" and defaults(A.spec_augment)["seed"] is None
    for fn in (A.freq_mask_batch, A.time_mask_batch, A.time_warp_batch):
        assert names(fn)[0] == "x" and {"seed", "first_row", "lengths", "out", "return_seed", "return_params"} <= set(names(fn))
    assert set(A.__all__) >= {"spec_augment", "spec_augment_batch", "freq_mask_batch", "time_mask_batch", "time_warp_batch"}
    assert not hasattr(A, "pitch_shift")
    sig = inspect.signature(SA.params)
    assert list(sig.parameters)[:6] == ["seed", "first_row", "B", "K", "T", "lengths"]


def test_cli_usage_errors_and_help(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    src = tmp_path / "f.csv"
    pd.DataFrame({"time": np.arange(5) * 0.01, "mfcc_0": np.arange(5.0), "mfcc_1": np.ones(5), "rms": np.ones(5)}).to_csv(src, index=False)
    run = CliRunner().invoke
    r = run(cli, ["augment", "--help"])
    assert r.exit_code == 0 and "spec-augment" in r.output and "add-noise" in r.output and "pitch-shift" not in r.output
    r = run(cli, ["augment", "spec-augment", "--help"])
    assert r.exit_code == 0 and all(o in r.output for o in ("--freq-masks", "--freq-width", "--time-masks", "--time-width", "--time-ratio",
                                                            "--time-warp", "--mask-value", "--seed", "--output"))
    base = ["augment", "spec-augment", str(src), "-o", str(tmp_path / "o.csv")]
    r = run(cli, base)                                                 # the default width 27 is above 3 rows
    assert r.exit_code == 2 and "--freq-width must be in [0, 3]" in r.output and "3 rows" in r.output
    r = run(cli, base + ["--freq-width", "4"])
    assert r.exit_code == 2 and "--freq-width must be in [0, 3]" in r.output
    for ratio in ("0", "1.5", "-0.1"):
        r = run(cli, base + ["--freq-width", "2", "--time-ratio", ratio])
        assert r.exit_code == 2 and "--time-ratio must be in (0, 1]" in r.output
    for v in ("median", "1.0x"):
        r = run(cli, base + ["--freq-width", "2", "--mask-value", v])
        assert r.exit_code == 2 and "--mask-value must be 'mean' or a float" in r.output
    r = run(cli, base + ["--freq-width", "2", "--freq-masks", "17"])
    assert r.exit_code == 2
    r = run(cli, base + ["--freq-width", "2", "--mask-value", "inf"])
    assert r.exit_code == 2 and "mask_value must be a finite float" in r.output
    assert not (tmp_path / "o.csv").exists()
