"""The PCEN entries of the C ABI are declared, bound and exported, their constants and rule hold together, and they refuse
bad arguments before device work; ops.pcen and the mirrors refuse what is not served without a device; the plugin registers
pcen; `features pcen` reports its usage errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_pcen_constants", "syg_pcen_form", "syg_pcen_work_bytes", "syg_pcen_f32"]


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


def lds_bytes(k, rows, halo, T):
    """What a resident workgroup of `rows` bands takes: S with its halo and the smoother, rows of T | 1 words, and the law."""
    return ((2 * rows + halo) * (T | 1) + rows * 8) * 4


def test_constants_and_rule(h):
    from sygnals_amd import _pcen as PC, ops
    k = ops.pcen_constants()
    assert k["tile"] == 1024 and k["bands"] == 64 and k["units"] == 4 and k["max_out"] == PC.MAX_OUT == 1 << 31
    assert k["table_words"] == PC.TABLE_WORDS and k["grid_max"] >= 1024
    assert 2 * k["lds_max"] <= 160 * 1024                                        # two workgroups a CU
    assert k["units"] * 2 * (k["tile"] + k["tile"] // 16) * 4 <= k["lds_max"]    # the tiled form's static LDS
    lim = k["resident_max_t"]
    assert lds_bytes(k, k["bands"], 0, lim) <= k["lds_max"] < lds_bytes(k, k["bands"], 0, lim + 1)
    assert h.syg_pcen_constants(8) == -1 and h.syg_pcen_constants(-1) == -1
    # the rule steps exactly at the limit, and where not even one band fits beside its halo
    f = h.syg_pcen_form
    assert f(1, 1, 1) == 0 and f(65, 128, 1) == 0 and f(lim, 128, 1) == 0 and f(lim + 1, 128, 1) == 1 and f(1 << 20, 1, 1) == 1
    assert ops.pcen_form(lim, 128) == "resident" and ops.pcen_form(lim + 1, 128, 3) == "tiled"
    for T in (65, lim):
        ms = 1
        while lds_bytes(k, 1, ms - 1, T) <= k["lds_max"]:
            ms += 1
        assert f(T, 4096, ms - 1) == 0 and f(T, 4096, ms) == 1
    assert f(0, 1, 1) == -1 and f(1, 0, 1) == -1 and f(1, 1, 0) == -1 and f(10, 4, 5) == -1
    with pytest.raises(ValueError, match="max_size = 5 exceeds the 4 bands"):
        ops.pcen_form(10, 4, 5)


def test_work_bytes(h):
    wb = h.syg_pcen_work_bytes
    assert wb(3, 5, 1) == 0 and wb(3, 5, 1024) == 0                # one tile a row: one launch, no carries
    assert wb(3, 5, 1025) == 3 * 5 * 2 * 8 and wb(1, 128, 1 << 20) == 128 * 1024 * 8
    assert wb(0, 1, 1) == -1 and wb(1, 0, 1) == -1 and wb(1, 1, 0) == -1


def test_entry_refuses_before_device_work(h, p):
    f, err = h.syg_pcen_f32, h.syg_last_error

    def call(x=p, B=2, M=8, T=65, sxb=8 * 65, sxk=65, out=None, sob=8 * 65, sok=65, gain=0.98, bias=2.0, power=0.5, eps=1e-6, b=0.05,
             tab=None, ms=1, scale=1.0, zi=None, zf=None, form=0, work=None, wbytes=0):
        out = C.c_void_p(p.value + 2 * 8 * 65 * 4) if out is None else out
        return f(x, B, M, T, sxb, sxk, out, sob, sok, gain, bias, power, eps, b, tab, ms, scale, zi, zf, form, work, wbytes, None)
    for kw in ({"x": None}, {"out": C.c_void_p(None)}):
        assert call(**kw) == -1 and b"null pointer" in err()
    for kw in ({"B": 0}, {"M": 0}, {"T": 0}):
        assert call(**kw) == -1 and b"empty input" in err()
    for kw in ({"sxk": 64}, {"sxb": -1}, {"sxk": -65}):
        assert call(**kw) == -1 and b"bad input strides" in err()
    for kw in ({"sok": 64}, {"sob": 7 * 65 + 64}):
        assert call(**kw) == -1 and b"bad output strides" in err()
    assert call(B=1 << 11, M=1 << 10, T=(1 << 10) + 1, sxb=0, sxk=0, sok=1025, sob=1025 << 10) == -1 and b"above 2^31" in err()
    for name, bad in (("gain", -0.1), ("bias", -1.0), ("power", -0.5), ("gain", float("nan")), ("bias", float("inf"))):
        assert call(**{name: bad}) == -1 and f"{name} must be non-negative".encode() in err()
    for bad in (0.0, -1e-6, float("nan")):
        assert call(eps=bad) == -1 and b"eps must be strictly positive" in err()
    for bad in (0.0, -0.1, 1.0000001, float("nan")):
        assert call(b=bad) == -1 and b"b must be in (0, 1]" in err()
    for bad in (0, -1, 9):
        assert call(ms=bad) == -1 and b"max_size must be an integer in [1, M = 8]" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(scale=bad) == -1 and b"scale must be positive and finite" in err()
    for bad in (-1, 3):
        assert call(form=bad) == -1 and b"form must be 0" in err()
    # out over x: only x itself with max_size = 1
    assert call(out=C.c_void_p(p.value + 4)) == -1 and b"out overlaps x" in err()
    assert call(out=p, ms=3) == -1 and b"out overlaps x" in err()
    assert call(out=p, sok=66, sob=8 * 66) == -1 and b"out overlaps x" in err()
    # a forced resident row that does not fit; a tiled row of several tiles without its workspace
    assert call(T=40000, sxk=40000, sxb=8 * 40000, sok=40000, sob=8 * 40000, form=1, out=C.c_void_p(p.value + (1 << 24))) == -1 \
        and b"does not fit the resident form" in err()
    big = dict(T=1025, sxk=1025, sxb=8 * 1025, sok=1025, sob=8 * 1025, out=C.c_void_p(p.value + (1 << 24)))
    assert call(**big) == -1 and b"need `work` of 256 bytes" in err()
    assert call(work=p, wbytes=255, **big) == -1 and b"need `work`" in err()


def test_ops_refuse_without_a_device():
    from sygnals_amd import ops
    S = torch.ones(2, 8, 65)
    for name in ("gain", "bias", "power"):
        with pytest.raises(ValueError, match=f"pcen: {name} must be non-negative .*served: gain >= 0"):
            ops.pcen(S, **{name: -0.5})
        with pytest.raises(ValueError, match=f"pcen: {name} must be non-negative"):
            ops.pcen(S, **{name: np.r_[np.ones(7), -1.0]})
    for bad in (0.0, -1e-6):
        with pytest.raises(ValueError, match="pcen: eps must be strictly positive"):
            ops.pcen(S, eps=bad)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="pcen: time_constant must be strictly positive"):
            ops.pcen(S, time_constant=bad)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="pcen: b must be in \\(0, 1\\] \\(at b = 0 scipy.signal.lfilter_zi is singular\\)"):
            ops.pcen(S, b=bad)
    for bad in (0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="pcen: max_size must be an integer >= 1"):
            ops.pcen(S, max_size=bad)
    with pytest.raises(ValueError, match="pcen: max_size = 9 exceeds the 8 bands"):
        ops.pcen(S, max_size=9)
    for name in ("gain", "bias", "power", "eps", "b"):
        with pytest.raises(ValueError, match=f"pcen: {name} must be a scalar or a vector of one value per band \\(8\\)"):
            ops.pcen(S, **{name: np.full(7, 0.5)})
        with pytest.raises(ValueError, match=f"pcen: {name} must be a scalar or a vector"):
            ops.pcen(S, **{name: np.full((8, 1), 0.5)})
    with pytest.raises(ValueError, match="pcen: gain must be a real number"):
        ops.pcen(S, gain="0.98")
    for bad in (S.double(), torch.complex(S, S), S.numpy(), S[0], S.half()):
        with pytest.raises(ValueError, match="pcen: S must be a float32 tensor \\[B, M, T\\]"):
            ops.pcen(bad)
    for shape in ((0, 8, 65), (2, 0, 65), (2, 8, 0)):
        with pytest.raises(ValueError, match="pcen: empty input"):
            ops.pcen(torch.ones(shape))
    with pytest.raises(ValueError, match="pcen: S must have unit stride along T \\(got 2"):
        ops.pcen(torch.ones(2, 8, 130)[..., ::2])
    with pytest.raises(ValueError, match="pcen: S must have unit stride along T"):
        ops.pcen(torch.ones(2, 65, 8).transpose(1, 2))
    with pytest.raises(ValueError, match="pcen: a result of .* elements is above 2\\^31"):
        ops.pcen(torch.ones(1025).expand(1 << 11, 1 << 10, 1025))
    for bad in (0.0, -2.0, float("inf")):
        with pytest.raises(ValueError, match="pcen: scale must be positive and finite"):
            ops.pcen(S, scale=bad)
    with pytest.raises(ValueError, match="pcen: zi must be \\[B, M\\] = \\[2, 8\\]"):
        ops.pcen(S, zi=np.zeros((8, 1)))
    with pytest.raises(ValueError, match="form must be None, 'resident' or 'tiled'"):
        ops.pcen(S, form="auto")
    buf = torch.ones(2 * 8 * 65 + 8)
    x = buf[:2 * 8 * 65].view(2, 8, 65)
    with pytest.raises(ValueError, match="pcen: out overlaps x \\(only out = x itself is served\\)"):
        ops.pcen(x, out=buf[8:].view(2, 8, 65))
    with pytest.raises(ValueError, match="pcen: out must be a float32 tensor \\[2, 8, 65\\]"):
        ops.pcen(S, out=torch.ones(2, 8, 64))
    with pytest.raises(ValueError, match="pcen: out must be a float32 tensor"):
        ops.pcen(S, out=torch.ones(2, 8, 130)[..., ::2])


def test_mirrors_refuse_without_a_device():
    from sygnals_amd.core.features import pcen as PN
    S = np.ones((8, 65))
    with pytest.raises(ValueError, match="pcen: ref= arrays are not served"):
        PN.pcen(S, ref=S)
    for axis in (0, -2):
        with pytest.raises(ValueError, match=f"pcen: axis = {axis} is not served"):
            PN.pcen(S, axis=axis)
    with pytest.raises(ValueError, match="pcen: max_axis = 1 is not served"):
        PN.pcen(S, max_axis=1)
    with pytest.raises(ValueError, match="pcen: S must be real"):
        PN.pcen(S + 1j)
    with pytest.raises(ValueError, match="pcen: S must be \\[M, T\\] or \\[T\\]"):
        PN.pcen(S[None])
    with pytest.raises(ValueError, match="pcen: max_size > 1 needs a band axis"):
        PN.pcen(S[0], max_size=3)
    with pytest.raises(ValueError, match="pcen: zi must be \\[M, 1\\] = \\[8, 1\\]"):
        PN.pcen(S, zi=np.zeros((1, 8)))
    with pytest.raises(ValueError, match="pcen: empty input"):
        PN.pcen(np.ones((8, 0)))
    with pytest.raises(ValueError, match="pcen_batch: S must be \\[B, M, T\\]"):
        PN.pcen_batch(S)
    with pytest.raises(ValueError, match="pcen_mel_batch: unknown arguments \\['ref'\\]"):
        PN.pcen_mel_batch(np.zeros((1, 4096), dtype=np.float32), ref=1)
    with pytest.raises(ValueError, match="pcen_mel_batch: n_mels must be an integer >= 1"):
        PN.pcen_mel_batch(np.zeros((1, 4096), dtype=np.float32), n_mels=0)
    assert sorted(PN.__all__) == ["pcen", "pcen_batch", "pcen_mel_batch"]


def test_plugin_registers_pcen():
    from sygnals_amd.core.features import pcen as PN
    from sygnals_amd.plugins import SygnalsAmdPlugin

    class Reg:
        def __init__(self):
            self.t = {}

        def add_transform(self, name, fn):
            self.t[name] = fn
    r = Reg()
    SygnalsAmdPlugin().register_transforms(r)
    assert r.t["pcen"] is PN.pcen and "delta" in r.t and "cmvn" in r.t


def test_cli_usage_errors(tmp_path):
    import pandas as pd
    import scipy.io.wavfile
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    wav = tmp_path / "a.wav"
    scipy.io.wavfile.write(wav, 22050, (0.1 * np.sin(np.arange(4096) * 0.1)).astype(np.float32))
    run = CliRunner().invoke
    base = ["features", "pcen", str(wav), "-o", str(tmp_path / "o.csv")]
    for opt, bad, words in (("--gain", "-1", "gain must be non-negative"), ("--bias", "-0.5", "bias must be non-negative"),
                            ("--power", "-2", "power must be non-negative"), ("--eps", "0", "eps must be strictly positive"),
                            ("--time-constant", "0", "--time-constant must be strictly positive"),
                            ("--max-size", "0", "max_size must be an integer >= 1"),
                            ("--max-size", "41", "max_size = 41 exceeds the 40 bands"),
                            ("--scale", "0", "scale must be positive and finite"), ("--n-mels", "0", "--n-mels must be at least 1"),
                            ("--hop-length", "0", "--hop-length must be at least 1"), ("--n-fft", "1", "--n-fft must be at least 2")):
        r = run(cli, base + ["--n-mels", "40"] * (opt != "--n-mels") + [opt, bad])
        assert r.exit_code == 2 and words in r.output, (opt, r.output)
    r = run(cli, base + ["--gain", "much"])
    assert r.exit_code == 2
    series = tmp_path / "s.csv"
    pd.DataFrame({"value": np.arange(50.0)}).to_csv(series, index=False)
    r = run(cli, ["features", "pcen", str(series), "-o", str(tmp_path / "o.csv")])
    assert r.exit_code == 2 and "is not recognized as audio" in r.output
    assert "--max-size" in run(cli, ["features", "pcen", "--help"]).output
