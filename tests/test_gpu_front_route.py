"""Which kernels serve a request to the STFT front ends (tests/front_cases.py): every row through its public entry with a
spy on the library, the entry points called -- in order -- against the recorded ones, and the per-kernel wrappers of
sygnals_amd.ops reached against the route the row pins for sygnals_amd._front.front_route
(tests/test_host_logic.py::test_front_route_is_pinned checks the function itself, without a device)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from oracle import cpu_ref as O
from tests.front_cases import CASES, EXPECT, FEATURE_SETS, run, wants

ROWS = ("stft2048_stats", "stft_rows_w1024", "stft_rows_w4096", "stft_rows_wsmall")
MEL = ("stft_mel_w1024_seg", "stft_mel_wseg_small", "stft_mel_w4096", "stft_mel_pow2")
WRAPPERS = ROWS + MEL + ("stft2048_mel", "stft_any")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from sygnals_amd import ops
    ops.require_gpu()


@functools.lru_cache(maxsize=None)
def clips(sr, B, L):
    return O.synth_clips(B, L, sr, seed=L)


def route_taken(c, reached):
    """The (rows, mel) answer of front_route that the wrappers `reached` (names, in call order) stand for; None when the
    request was served without any of them (the MFCC rows straight from a launch)."""
    rows, mel = wants(c)
    if "stft_any" in reached:
        return ("generic" if rows else None, "generic" if mel else None)
    if not reached:
        return None
    by_rows = next((w for w in reached if w in ROWS), "stft2048_mel" if rows else None)
    by_mel = next((w for w in reached if w in MEL), None if rows or not mel else "stft2048_mel")
    assert set(reached) <= {by_rows, by_mel}, reached
    return by_rows, by_mel


class Spy:
    """Records the names of the syg_*_f32 entry points called through lib()."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        real = getattr(self.lib, name)
        if not (name.startswith("syg_") and name.endswith("_f32")):
            return real

        def wrapped(*a):
            self.calls.append(name)
            return real(*a)
        return wrapped


def observe(case, monkeypatch):
    """Runs the row; returns (route taken, entry points called)."""
    from sygnals_amd import _lib, ops
    c = CASES[case]
    y = clips(c.sr, c.B, c.L)
    spy, reached = Spy(_lib.lib()), []
    monkeypatch.setattr(ops, "lib", lambda: spy)
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    for name in WRAPPERS:
        def through(*a, _f=getattr(ops, name), _n=name, **k):
            reached.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, through)
    ops._mfcc_calls.clear()                      # prepared calls hold the library's functions, not the spy's
    try:
        out = run(c, y)
    finally:
        ops._mfcc_calls.clear()
    if c.entry == "extract":
        for f in FEATURE_SETS[c.feats]:          # every feature came out: no failure hides behind the per-feature try
            assert {"mfcc": "mfcc_0", "spectral_contrast": "contrast_delta"}.get(f, f) in out, (f, sorted(out))
    else:
        assert np.isfinite(out.cpu().numpy() if hasattr(out, "cpu") else out).all()
    return route_taken(c, reached), spy.calls


@pytest.mark.parametrize("case", sorted(CASES))
def test_same_launches(case, monkeypatch):
    route, calls = observe(case, monkeypatch)
    want_route, want_calls = EXPECT[case]
    assert calls == want_calls, (calls, want_calls)
    assert route == want_route, (route, want_route)


@pytest.mark.parametrize("case", sorted(k for k, (route, _) in EXPECT.items() if route and route[0] in ROWS and route[1] is None))
def test_stft_front_is_the_rows_wrapper(case):
    """Where one rows wrapper serves the whole request, ops.stft_front returns what that wrapper returns, bit for bit."""
    from sygnals_amd import _tables as T, ops
    c = CASES[case]
    rows, mel = wants(c)
    name = EXPECT[case][0][0]
    y = ops.to_device_f32(clips(c.sr, c.B, c.L))
    plan = T.contrast_plan(np.fft.rfftfreq(c.n_fft, 1.0 / c.sr), c.sr)
    n_mels = c.n_mels if mel else None
    got = ops.stft_front(y, c.sr, c.n_fft, c.hop, True, "hann", None, n_mels, 0.0, None, c.power, 1 | 8, 0.85, 2.0, plan)
    frame = (c.n_fft,) if name == "stft_rows_wsmall" else ()
    stand_in = 16 if name == "stft2048_mel" else None              # (rows alone from the mel launch: 16 bands, discarded)
    bands = () if name in ("stft2048_stats", "stft_rows_wsmall") else (n_mels or stand_in, 0.0, None)
    want = getattr(ops, name)(y, c.sr, *frame, c.hop, True, "hann", 2048 if name.startswith("stft2048") else None, *bands,
                              1 | 8, 0.85, 2.0, plan)
    want = (None,) * (3 - len(want)) + tuple(want)
    if n_mels is None:
        want = (None,) + want[1:]
    assert len(got) == 3 and (got[0] is None) == (n_mels is None)
    for g, w in zip(got, want):
        assert (g is None and w is None) or torch.equal(g, w)
