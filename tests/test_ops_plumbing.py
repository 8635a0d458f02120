"""The device plumbing at the top of sygnals_amd/ops.py, checked without a device: the input check's two stages, the output
check, the workspace helper (and the seven functions that used to take whatever their sizing entry answered), the table
cache, the constants reader and the row-block iterator.  Host tensors stand in for device tensors: `Dev` answers is_cuda
with True, require_gpu is patched to name the host, and the library is a spy."""
import numpy as np
import pytest
import torch

from sygnals_amd import _lib, ops
from sygnals_amd._lib import SygnalsHipError


class Dev(torch.Tensor):
    """A host tensor that says it is on the device (views and copies of it say so too)."""
    is_cuda = property(lambda self: True)


def dev(*shape, dtype=torch.float32):
    return torch.arange(int(np.prod(shape)), dtype=dtype).reshape(shape).as_subclass(Dev)


class Spy:
    """Stands in for the library: every entry is recorded; a sizing entry answers `size`, any other entry 0."""

    def __init__(self, size=-1):
        self.size, self.calls = size, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.size if name.endswith("_work_bytes") else 0
        return entry

    def launches(self):
        return [n for n, _ in self.calls if n.endswith(("_f32", "_c64", "_u32"))]


@pytest.fixture
def host(monkeypatch):
    """No device is needed: require_gpu names the host, the current device is 0, the caches start empty and end empty."""
    monkeypatch.setattr(ops, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(ops, "_stream_ptr", lambda: 0)
    ops.clear_caches()
    yield
    ops.clear_caches()


# ---------------------------------------------------------------------------------------------------------- input check
def test_input_check_judges_the_tensor_before_it_asks_for_a_device(monkeypatch):
    def reached():
        raise AssertionError("require_gpu was reached")
    monkeypatch.setattr(ops, "require_gpu", reached)
    D = torch.zeros((2, 3, 1025, 2))
    for bad, dims, tail in ((np.zeros((2, 8), np.float32), 2, ()), (torch.zeros(8), 2, ()), (torch.zeros((2, 8, 1)), 2, ()),
                            (torch.zeros((2, 8), dtype=torch.float64), 2, ()), (D[:, :, :1024], 4, (1025, 2)),
                            (D[..., :1], 4, (1025, 2)), (D.double(), 4, (1025, 2))):
        for check in (ops._f32, ops._f32_in):
            with pytest.raises(ValueError, match="x must be a float32 tensor"):
                check(bad, "x", dims, tail)
    with pytest.raises(ValueError, match=r"D must be a float32 tensor \[\*, \*, 1025, 2\]"):
        ops._f32_in(D[..., :1], "D", 4, (1025, 2))
    with pytest.raises(ValueError, match=r"x must be a float32 tensor \[B, K, T\]"):
        ops._f32(torch.zeros(3), "x", 3, axes="[B, K, T]")
    ops._f32(D, "D", 4, (1025, 2))                                  # a good tensor passes the first stage without a device
    with pytest.raises(AssertionError, match="require_gpu was reached"):
        ops._f32_in(D, "D", 4, (1025, 2))                           # ... and the second stage asks for one


def test_input_check_second_stage_and_unit_stride(host):
    with pytest.raises(ValueError, match="y must be a CUDA tensor"):
        ops._f32_in(torch.zeros((2, 8)), "y", 2)                    # a device, but the tensor is not on it
    x = dev(4, 6)
    assert ops._f32_in(x, "x", 2) is x
    rows = x[:, 1:5]                                                # strided rows with unit stride along a row: no copy
    assert ops._f32_in(rows, "x", 2) is rows
    t = x.t()                                                       # last stride 6
    got = ops._f32_in(t, "x", 2)
    assert got is not t and got.stride(-1) == 1 and torch.equal(got, t)
    one = x[:, ::6]                                                 # one column: its stride does not matter
    assert one.shape == (4, 1) and ops._f32_in(one, "x", 2) is one


# --------------------------------------------------------------------------------------------------------- output check
def test_output_check():
    x = torch.zeros((2, 5))
    new = ops._out(None, (2, 3, 4), x, dtype=torch.float64)
    assert new.shape == (2, 3, 4) and new.dtype == torch.float64 and new.device == x.device
    good = torch.empty((2, 3, 4))
    assert ops._out(good, (2, 3, 4), x) is good and ops._out(good, (2, 3, 4), x, contiguous=True) is good
    with pytest.raises(ValueError, match=r"out must be a float32 tensor \[2, 3, 4\]"):
        ops._out(torch.empty((2, 3, 4), dtype=torch.float64), (2, 3, 4), x)         # the right shape, another dtype
    with pytest.raises(ValueError, match=r"out_k must be a float32 tensor \[2, 3, 4\]"):
        ops._out(torch.empty((2, 4, 3)), (2, 3, 4), x, "out_k")                     # another shape
    with pytest.raises(ValueError, match="out must be a float32 tensor"):
        ops._out(np.zeros((2, 3, 4), np.float32), (2, 3, 4), x)
    rows = torch.empty((2, 3, 8))[:, :, :4]                         # not contiguous, unit stride along the last axis
    assert not rows.is_contiguous() and ops._out(rows, (2, 3, 4), x) is rows
    with pytest.raises(ValueError, match="contiguous"):
        ops._out(rows, (2, 3, 4), x, contiguous=True)
    with pytest.raises(ValueError, match="unit stride along its last axis"):
        ops._out(torch.empty((2, 4, 3)).transpose(1, 2), (2, 3, 4), x)
    with pytest.raises(ValueError, match=r"out must be a complex128 tensor \[2, 3\]"):
        ops._out(torch.empty((2, 3)), (2, 3), x, dtype=torch.complex128, contiguous=True)


# ------------------------------------------------------------------------------------------------------------ workspace
def test_workspace_sizes(monkeypatch):
    cpu = torch.device("cpu")
    spy = Spy()
    monkeypatch.setattr(ops, "lib", lambda: spy)
    # a refusal from an entry that leaves no message names the entry and its arguments; from any other it goes through check
    with pytest.raises(SygnalsHipError, match=r"syg_welch_work_bytes\(3, 256\) refuses these arguments"):
        ops._workspace("syg_welch_work_bytes", 3, 256, dtype=torch.float32, device=cpu)
    with pytest.raises(SygnalsHipError, match=r"syg_laplace_work_bytes failed \(rc=-1\)"):
        ops._workspace("syg_laplace_work_bytes", 1, 2, 16, -1, dtype=torch.float64, device=cpu)
    with pytest.raises(ValueError, match="my own words"):
        ops._workspace("syg_pyin_work_bytes", 1, 1, 1, dtype=torch.uint8, device=cpu, error=ValueError("my own words"))
    assert spy.calls == [("syg_welch_work_bytes", (3, 256)), ("syg_laplace_work_bytes", (1, 2, 16, -1)),
                         ("syg_pyin_work_bytes", (1, 1, 1))]
    spy.size = 0
    assert ops._workspace("syg_dwt_work_bytes", 1, 8, 8, 1, dtype=torch.float32, device=cpu) is None
    assert ops._nbytes(None) == 0
    spy.size = 12
    w = ops._workspace("syg_dtw_work_bytes", 1, 2, 3, -1, 0, dtype=torch.float64, device=cpu)
    assert w.dtype == torch.float64 and w.device == cpu and w.dim() == 1 and ops._nbytes(w) == 16 >= 12
    assert ops._nbytes(ops._workspace("syg_dwt_work_bytes", 1, 8, 8, 1, dtype=torch.float32, device=cpu)) == 12
    spy.size = 16
    for dtype in (torch.float64, torch.float32, torch.int32, torch.uint8):
        w = ops._workspace("syg_csd_work_bytes", 1, 2, 8, dtype=dtype, device=cpu)
        assert w.dtype == dtype and ops._nbytes(w) == 16
    assert ops._work_bytes("syg_sosfilt_work_bytes", 1, 2, 3) == 16


WIN = np.hanning(16).astype(np.float32)
UNCHECKED = {      # the functions whose sizing call used to go unchecked: sizing entry -> a call that reaches it
    "pack_frames": ("syg_pack_rows_work_bytes", lambda: ops.pack_frames(dev(2, 64), 3, 16, 8, 0, 16, detrend="constant")),
    "pack_rows": ("syg_pack_rows_work_bytes", lambda: ops.pack_rows(dev(2, 64), 64, detrend="linear")),
    "welch": ("syg_welch_work_bytes", lambda: ops.welch(dev(2, 64), 16, 8, 16, WIN, "constant", 1.0)),
    "cross_spectrum": ("syg_csd_work_bytes", lambda: ops.cross_spectrum(dev(2, 64), dev(2, 64), 16, 8, 16, WIN, False, 1.0)),
    "onset_strength": ("syg_onset_strength_work_bytes", lambda: ops.onset_strength(dev(2, 8, 20))),
    "dwt": ("syg_dwt_work_bytes", lambda: ops.dwt(dev(2, 64), "db4", 2)),
    "_dynamics": ("syg_dynamics_work_bytes", lambda: ops.cmvn(dev(2, 3, 40), form="tiled")),
}


@pytest.mark.parametrize("name", sorted(UNCHECKED))
def test_a_refused_workspace_raises_before_any_launch(name, host, monkeypatch):
    """All seven can be driven to their sizing call without a device (pack_frames as it stands, the others behind the
    patched require_gpu): a refusal raises SygnalsHipError that names the entry, and no launch entry has been called."""
    entry, call = UNCHECKED[name]
    spy = Spy(-1)
    monkeypatch.setattr(ops, "lib", lambda: spy)
    with pytest.raises(SygnalsHipError, match=entry + r"\(.*\) refuses these arguments"):
        call()
    assert entry in [n for n, _ in spy.calls] and spy.launches() == []


def test_a_granted_workspace_reaches_the_launch(host, monkeypatch):
    """The same calls with a sizing entry that answers 16: the launch entry is called, after the sizing entry."""
    for name, launch in (("pack_rows", "syg_pack_rows_f32"), ("onset_strength", "syg_onset_strength_f32"),
                         ("_dynamics", "syg_dynamics_f32")):
        spy = Spy(16)
        monkeypatch.setattr(ops, "lib", lambda: spy)
        UNCHECKED[name][1]()
        assert [n for n, _ in spy.calls][-2:] == [UNCHECKED[name][0], launch]


# ---------------------------------------------------------------------------------------------------------- table cache
def test_table_cache_limits_families_and_keys_on_the_device(host, monkeypatch):
    built = []

    def get(family, i, limit=None):
        return ops._cached((family, i), lambda: built.append((family, i)) or (family, i, len(built)), limit)

    for i in (0, 1, 2):
        assert get("free", i)[:2] == ("free", i)
    a0 = get("two", 0, 2)
    get("two", 1, 2)
    assert get("two", 0, 2) is a0                                   # a hit makes key 0 the most recently used
    get("two", 2, 2)                                                # ... so the third key evicts key 1
    n = len(built)
    assert get("two", 0, 2) is a0 and get("two", 2, 2)[:2] == ("two", 2) and len(built) == n
    get("two", 1, 2)                                                # rebuilt on the next ask, evicting key 0
    assert built[n:] == [("two", 1)]
    get("two", 0, 2)
    assert built[n:] == [("two", 1), ("two", 0)]
    for i in (0, 1, 2):                                             # the unbounded family kept all three through all that
        get("free", i)
    assert [b for b in built if b[0] == "free"] == [("free", 0), ("free", 1), ("free", 2)]
    # keys are per device
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    assert get("free", 0)[2] == len(built) and built[-1] == ("free", 0)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    n = len(built)
    get("free", 0)
    assert len(built) == n
    # clear_caches empties both kinds, the prepared MFCC calls and the side streams
    ops._mfcc_calls["k"] = object()
    ops._side_streams[0] = object()
    ops.clear_caches()
    assert not ops._dev_cache and not ops._mfcc_calls and not ops._side_streams
    get("free", 0), get("two", 2, 2)
    assert built[-2:] == [("free", 0), ("two", 2)]


def test_the_former_lru_builders_go_through_the_cache(host):
    """Their tables are per device and per key, bounded as before, and clear_caches drops them (host arithmetic only)."""
    s = np.array([0.5 + 1j, 1.0 - 2j])
    p1 = ops.laplace_plan(s, 0.5)
    assert ops.laplace_plan(s, 0.5) is p1 and ops._laplace_anchor_dev(s.tobytes(), 0.5, 100) is ops._laplace_anchor_dev(s.tobytes(), 0.5, 100)
    r1 = ops.resample_plan(3, 2, 100)
    c1 = ops.cwt_plan([1.0, 2.0, 4.0], "morl")
    assert ops.resample_plan(3, 2, 100) is r1 and ops.cwt_plan([1.0, 2.0, 4.0], "morl") is c1
    assert {k[1] for k in ops._dev_cache} == {"laplace_plan", "laplace_anchor", "resample", "cwt_table"}
    for L in range(101, 101 + 70):
        ops.resample_plan(3, 2, L)
    assert sum(k[1] == "resample" for k in ops._dev_cache) == 64
    ops.clear_caches()
    assert ops.laplace_plan(s, 0.5) is not p1


# ------------------------------------------------------------------------------------------------------------ constants
INDEXED = {        # public reader -> (indexed entry, the keys of the parent commit in index order)
    "sosfilt_constants": ("syg_sosfilt_constants", ("chunk", "tile", "chunks_per_wave", "scan_ahead", "group_sections",
                                                    "max_sections", "two_level_chunks")),
    "rng_constants": ("syg_rng_constants", ("rounds", "stream_noise", "stream_row", "row_limit", "colored_max")),
    "cepstrum_constants": ("syg_cepstrum_constants", ("frame", "tile_frames", "waves", "scan", "lds_fixed", "lds_max")),
    "lpc_constants": ("syg_lpc_constants", ("max_frame", "max_order", "waves", "tile_frames", "span_max", "stage_chunk",
                                            "acorr_chunk")),
    "dynamics_constants": ("syg_dynamics_constants", ("tile", "resident_max_t", "resident_max_t_sliding", "window_max",
                                                      "direct_window", "width_max", "order_max", "units", "max_out", "lds_max")),
}
FIGURES = {        # public reader -> the keys of the parent commit and the per-figure entry each was read from
    "laplace_constants": dict(C="syg_laplace_chunk", tile_rows="syg_laplace_tile_rows", tile_cols="syg_laplace_tile_cols",
                              segment="syg_laplace_segment", steep="syg_laplace_steep", fac_stride="syg_laplace_fac_stride"),
    "resample_constants": dict(tile="syg_resample_tile", table_lds_rule="syg_resample_table_lds_rule",
                               table_lds_max="syg_resample_table_lds_max", table_max="syg_resample_table_max",
                               span_max="syg_resample_span_max", rate_max="syg_resample_rate_max"),
    "cwt_constants": dict(tile="syg_cwt_tile", direct_taps_max="syg_cwt_direct_taps_max",
                          scales_per_group="syg_cwt_scales_per_group", span_max="syg_cwt_span_max",
                          taps_lds_max="syg_cwt_taps_lds_max"),
    "dtw_constants": dict(tile="syg_dtw_tile", tile_max="syg_dtw_tile_max", resident_max_cols="syg_dtw_resident_max_cols",
                          run_max="syg_dtw_run_max", cost_tile="syg_dtw_cost_tile"),
}


def test_constants_are_the_parents_dicts():
    h = _lib.lib()
    for reader, (entry, keys) in INDEXED.items():
        want = {k: int(getattr(h, entry)(i)) for i, k in enumerate(keys)}
        got = getattr(ops, reader)()
        assert got == want and list(got) == list(keys) and all(type(v) is int for v in got.values()), reader
    for reader, entries in FIGURES.items():
        want = {k: int(getattr(h, e)()) for k, e in entries.items()}
        got = getattr(ops, reader)()
        assert got == want and list(got) == list(entries) and all(type(v) is int for v in got.values()), reader
    assert len(INDEXED) + len(FIGURES) == 9


def test_constants_are_read_when_asked(monkeypatch):
    spy = Spy()
    monkeypatch.setattr(ops, "lib", lambda: spy)
    assert ops.rng_constants() == dict.fromkeys(("rounds", "stream_noise", "stream_row", "row_limit", "colored_max"), 0)
    assert spy.calls == [("syg_rng_constants", (i,)) for i in range(5)]
    del spy.calls[:]
    assert set(ops.laplace_constants()) == set(FIGURES["laplace_constants"])
    assert [n for n, _ in spy.calls] == list(FIGURES["laplace_constants"].values())


# ----------------------------------------------------------------------------------------------------------- row blocks
def test_row_blocks():
    assert ops.MAX_ROWS == 65535
    assert list(ops._row_blocks(0)) == []
    assert list(ops._row_blocks(1)) == [(0, 1)]
    assert list(ops._row_blocks(65535)) == [(0, 65535)]
    assert list(ops._row_blocks(65536)) == [(0, 65535), (65535, 1)]
    assert list(ops._row_blocks(131071)) == [(0, 65535), (65535, 65535), (131070, 1)]
