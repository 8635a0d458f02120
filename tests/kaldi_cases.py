"""The cases of the Kaldi front end's GPU tests (tests/test_gpu_kaldi.py), their inputs and their gates.  No device is
needed here: tests/test_kaldi_ref.py asserts on the CPU the condition every gated case rests on.

Gates (float64, per cell, against tests/kaldi_ref.py):
  energy  |exp(f_dev) - max(E_ref, eps)| <= 1e-5 max_m E_ref of that frame (|E_dev - E_ref| without the logarithm).  It is
          used where every frame has max_m E_ref > 1e6 eps = 0.119, so that the floor at eps lies five decades below the
          tolerance.  A noise clip of amplitude 1e-3 has frame peaks near 1e-3 and cannot carry it: the 1e-3 case is a tone
          in a 1200-sample window whose band passes, and the DC-heavy clip with DC removal is taken with three wide bands.
  log     on cells with E_ref >= 1e-2 max_m E_ref: |f_dev - f_ref| <= 2e-3; at least one cell a frame (the peak cell)."""
import numpy as np

from sygnals_amd import _kaldi as KD
from tests import kaldi_ref as KR

ENERGY_TOL = 1e-5
LOG_TOL = 2e-3
DOMINANT = 1e-2
SCALE_MIN = 1e6 * KD.EPS

# (sr, frame_length ms, frame_shift ms) -> (wl, hop, N)
SIZES = {"16k": (16000.0, 25.0, 10.0), "8k": (8000.0, 25.0, 10.0), "22k": (22050.0, 25.0, 10.0), "48k": (48000.0, 25.0, 10.0),
         "16k_full": (16000.0, 32.0, 10.0)}
EXPECTED_SIZES = {"16k": (400, 160, 512), "8k": (200, 80, 256), "22k": (551, 220, 1024), "48k": (1200, 480, 2048),
                  "16k_full": (512, 160, 512)}


def length_for(T: int, wl: int, hop: int, snip_edges: bool) -> int:
    """A clip length with exactly T frames (the shortest; T = 0: the longest)."""
    if snip_edges:
        return wl - 1 if T == 0 else wl + (T - 1) * hop
    return hop - hop // 2 - 1 if T == 0 else T * hop - hop // 2


def signal(kind: str, B: int, L: int, amp: float, sr: float, seed: int, freq: float = 0.0) -> np.ndarray:
    """float32 [B, L]: noise (white), tone (a cosine at freq plus noise 40 dB below), brown (integrated noise), dc
    (0.9 + 1e-3 noise), const (amp)."""
    g = np.random.default_rng(seed)
    n = np.arange(L, dtype=np.float64)[None, :]
    if kind == "noise":
        x = amp * g.standard_normal((B, L))
    elif kind == "tone":
        ph = g.uniform(0, 2 * np.pi, (B, 1))
        x = amp * (np.cos(2 * np.pi * freq * n / sr + ph) + 0.01 * g.standard_normal((B, L)))
    elif kind == "brown":
        x = np.cumsum(g.standard_normal((B, L)), axis=1)
        x = amp * x / np.maximum(np.abs(x).max(axis=1, keepdims=True), 1e-30)
    elif kind == "dc":
        x = 0.9 + 1e-3 * g.standard_normal((B, L))
    elif kind == "const":
        x = np.full((B, L), amp)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def _case(cid, size="16k", T=3, B=1, snip=True, kind="noise", amp=1.0, freq=0.0, L=None, layout="ct", strided=False, **kw):
    sr, fl, fs = SIZES[size]
    fl, fs = kw.pop("frame_length", fl), kw.pop("frame_shift", fs)
    wl, hop, _ = KD.sizes(sr, fl, fs)
    L = length_for(T, wl, hop, snip) if L is None else L
    kw = dict(kw, frame_length=fl, frame_shift=fs, snip_edges=snip)
    return dict(id=cid, sr=sr, kw=kw, L=L, B=B, kind=kind, amp=amp, freq=freq, layout=layout, strided=strided)


def cases():
    out = []
    for size in SIZES:                                                   # every size, both framings, two tiles, a partial one
        for snip in (True, False):
            out.append(_case(f"{size}-{'snip' if snip else 'reflect'}-T17-B3", size, T=17, B=3, snip=snip,
                             kind="tone" if size == "22k" else "noise", freq=3000.0))
    for T in (1, 2, 15, 16, 33):                                         # the frame counts around the tile
        for snip in (True, False):
            out.append(_case(f"16k-{'snip' if snip else 'reflect'}-T{T}", T=T, snip=snip, kind="brown" if T == 15 else "noise"))
    # frames that leave the clip on both sides: L = hop / 2, wl - 1, and L = 1 (a shift of one sample: T = 1)
    out.append(_case("reflect-L80", snip=False, L=80))
    out.append(_case("reflect-L399", snip=False, L=399))
    out.append(_case("reflect-L1-hop1", snip=False, L=1, frame_shift=0.0625, kind="const", remove_dc_offset=False))
    out.append(_case("reflect-L5-hop1", snip=False, L=5, frame_shift=0.0625))
    out.append(_case("8k-B33", "8k", T=2, B=33))
    out.append(_case("16k-strided-ct", T=5, B=3, strided=True))
    out.append(_case("16k-strided-tc", T=5, B=3, strided=True, layout="tc"))
    out.append(_case("48k-tc", "48k", T=3, B=2, layout="tc"))
    for M in (3, 16, 17, 23, 80, 128, 256):
        out.append(_case(f"16k-M{M}", num_mel_bins=M))
    out.append(_case("48k-M256", "48k", T=2, num_mel_bins=256))
    out.append(_case("8k-M80-T18", "8k", T=18, num_mel_bins=80))
    for w in KD.WINDOWS:
        out.append(_case(f"window-{w}", window_type=w, kind="tone", freq=1234.0))
    out.append(_case("blackman-coeff", window_type="blackman", blackman_coeff=0.3))
    out.append(_case("no-dc-removal", remove_dc_offset=False))
    out.append(_case("no-preemphasis", preemphasis_coefficient=0.0))
    out.append(_case("preemphasis-1", preemphasis_coefficient=1.0))
    out.append(_case("magnitude", use_power=False))
    out.append(_case("linear", use_log_fbank=False))
    out.append(_case("linear-magnitude", use_log_fbank=False, use_power=False))
    out.append(_case("band-limits", low_freq=300.0, high_freq=-400.0, num_mel_bins=40))
    out.append(_case("energy-first", use_energy=True, energy_floor=0.0))
    out.append(_case("energy-last", use_energy=True, htk_compat=True, raw_energy=False, layout="tc"))
    out.append(_case("amp-1e-3-tone", "48k", T=2, kind="tone", amp=1e-3, freq=16000.0))
    out.append(_case("amp-32768", kind="noise", amp=32768.0, T=4))
    out.append(_case("amp-32768-brown", "22k", kind="brown", amp=32768.0, T=2))
    out.append(_case("dc-heavy-kept", kind="dc", remove_dc_offset=False))
    out.append(_case("dc-heavy-removed", "48k", T=2, kind="dc", num_mel_bins=3))
    return out


def case_input(c) -> np.ndarray:
    seed = sum(map(ord, c["id"]))
    return signal(c["kind"], c["B"], c["L"], c["amp"], c["sr"], seed, c["freq"])


def reference(c, x: np.ndarray):
    """(E [B, T, M] mel energies before the logarithm, e [B, T] log-energies, f [B, T, C] the contract's result)."""
    kw = {k: v for k, v in c["kw"].items() if k not in ("use_energy", "htk_compat", "use_log_fbank", "subtract_mean")}
    E, e, f = [], [], []
    for row in x:
        Eb, eb = KR.mel_energies(row.astype(np.float64), c["sr"], **kw)
        E.append(Eb)
        e.append(eb)
        f.append(KR.fbank(row.astype(np.float64), c["sr"], **c["kw"]))
    return np.stack(E), np.stack(e), np.stack(f)


def mel_columns(c):
    """Slice of the mel columns in the result [.., C]."""
    M = c["kw"].get("num_mel_bins", 23)
    off = 1 if (c["kw"].get("use_energy", False) and not c["kw"].get("htk_compat", False)) else 0
    return slice(off, off + M)


def gates(f_mel: np.ndarray, E_ref: np.ndarray, use_log: bool = True, use_floor: bool = True):
    """(worst energy error / frame peak, worst log error on the dominant cells, dominant cells of the poorest frame) of
    the mel columns f_mel [..., T, M] against E_ref (before the logarithm)."""
    f = np.asarray(f_mel, dtype=np.float64)
    peak = E_ref.max(axis=-1, keepdims=True)
    Ef = np.maximum(E_ref, KD.EPS) if use_log else E_ref
    Ed = np.exp(f) if use_log else f
    e_err = float(np.max(np.abs(Ed - Ef) / peak))
    dom = E_ref >= DOMINANT * peak
    if use_log:
        l_err = float(np.max(np.where(dom, np.abs(f - np.log(Ef)), 0.0)))
    else:
        l_err = float(np.max(np.where(dom, np.abs(np.log(np.maximum(f, 1e-300)) - np.log(Ef)), 0.0)))
    return e_err, l_err, int(dom.sum(axis=-1).min())


def band_centres(M: int, sr: float, low: float = 20.0, high: float = 0.0) -> np.ndarray:
    """Centre frequencies (Hz) of the M triangles."""
    if high <= 0:
        high += sr / 2
    ml, mh = KR.mel(low), KR.mel(high)
    c = ml + (np.arange(M) + 1.0) * (mh - ml) / (M + 1)
    return 700.0 * (np.exp(c / 1127.0) - 1.0)
