"""Host plan of the continuous wavelet transform (csrc/cwt.hip; include/sygnals_hip.h states the tables' layout): the
arithmetic of PyWavelets 1.x pywt.cwt turned into a bank of FIR filters.  pywt.cwt computes, per scale s,
-sqrt(s) diff(convolve(data, k_s)) with k_s the integrated wavelet resampled to the scale and reversed; here the
difference is taken on the filter, h_s = -sqrt(s) d(k_s) with d(k)[0] = k[0], d(k)[i] = k[i] - k[i - 1], d(k)[n] = -k[n - 1],
in float64, and rounded once to float32, so the cancellation never happens in float32 and the device runs
W[t] = sum_j h_s[j] x[t + shift_s - j].  Pure NumPy, no device and no library here, so the plan is tested on the CPU
(the independent conv-then-diff restatement is tests/cwt_ref.py).  PyWavelets itself is not a dependency: parity with it
is unpinned."""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass

import numpy as np

SERVED = ("morl", "mexh", "gaus1", "cmorB-C")
PRECISION = 10                      # pywt.cwt samples the wavelet at 2^10 points
PAIR_RATIO = 4.0                    # two scales share a filter row of the spectral form only within this factor
OUTPUTS = {"coef": 0, "magnitude": 1, "power": 2}
_CMOR = re.compile(r"^cmor(\d+\.?\d*|\.\d+)-(\d+\.?\d*|\.\d+)$")


@dataclass(frozen=True)
class Wavelet:
    name: str
    kind: str             # morl | mexh | gaus1 | cmor
    lo: float
    hi: float
    complex: bool
    B: float = 0.0        # cmor: bandwidth
    C: float = 0.0        # cmor: centre frequency


def served_message(wavelet) -> str:
    return (f"wavelet {wavelet!r} is not served; served: morl, mexh, gaus1 and cmorB-C with positive floats B and C "
            "(e.g. cmor1.5-1.0)")


@functools.lru_cache(maxsize=64)
def parse_wavelet(wavelet) -> Wavelet:
    if not isinstance(wavelet, str):
        raise ValueError(served_message(wavelet))
    if wavelet == "morl":
        return Wavelet(wavelet, "morl", -8.0, 8.0, False)
    if wavelet == "mexh":
        return Wavelet(wavelet, "mexh", -8.0, 8.0, False)
    if wavelet == "gaus1":
        return Wavelet(wavelet, "gaus1", -5.0, 5.0, False)
    m = _CMOR.match(wavelet)
    if m and float(m.group(1)) > 0 and float(m.group(2)) > 0:
        return Wavelet(wavelet, "cmor", -8.0, 8.0, True, float(m.group(1)), float(m.group(2)))
    raise ValueError(served_message(wavelet))


def psi(w: Wavelet, x: np.ndarray) -> np.ndarray:
    if w.kind == "morl":
        return np.exp(-x * x / 2.0) * np.cos(5.0 * x)
    if w.kind == "mexh":
        return 2.0 / (np.sqrt(3.0) * np.pi ** 0.25) * (1.0 - x * x) * np.exp(-x * x / 2.0)
    if w.kind == "gaus1":
        return -2.0 * x * np.exp(-x * x) / (np.pi / 2.0) ** 0.25
    return (np.pi * w.B) ** -0.5 * np.exp(-x * x / w.B) * np.exp(2j * np.pi * w.C * x)


@functools.lru_cache(maxsize=16)
def _integrated(w: Wavelet):
    """(int_psi, x, step) of pywt.integrate_wavelet at 2^PRECISION points (conjugated for a complex wavelet, as pywt.cwt does)."""
    x = np.linspace(w.lo, w.hi, 2 ** PRECISION)
    step = x[1] - x[0]
    ip = np.cumsum(psi(w, x)) * step
    return (np.conj(ip) if w.complex else ip), x, step


def scale_filter(w: Wavelet, s: float):
    """(h_s in float64 or complex128, crop offset floor(d)) of one scale; ValueError in pywt's words where it is too small."""
    ip, x, step = _integrated(w)
    j = (np.arange(s * (x[-1] - x[0]) + 1) / (s * step)).astype(int)
    if j[-1] >= ip.size:
        j = np.extract(j < ip.size, j)
    k = ip[j][::-1]
    n = k.size
    if n < 2:                                              # d = (len(coef) - L) / 2 = (n - 2) / 2 < 0
        raise ValueError(f"Selected scale of {s} too small.")
    dk = np.empty(n + 1, dtype=k.dtype)
    dk[0] = k[0]
    dk[1:n] = k[1:] - k[:-1]
    dk[n] = -k[n - 1]
    return -np.sqrt(s) * dk, (n - 2) // 2


def check_scales(scales) -> np.ndarray:
    try:
        s = np.atleast_1d(np.asarray(scales, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("Scales array must not be empty and contain only positive values.") from None
    if s.ndim != 1 or s.size == 0 or not np.all(np.isfinite(s)) or np.any(s <= 0):
        raise ValueError("Scales array must not be empty and contain only positive values.")
    return s


def central_frequency(wavelet, precision: int = 8) -> float:
    """pywt.central_frequency: the strongest bin of the wavelet sampled at 2^precision points over its support."""
    w = parse_wavelet(wavelet)
    x = np.linspace(w.lo, w.hi, 2 ** precision)
    p = psi(w, x)
    domain = float(x[-1] - x[0])
    index = int(np.argmax(np.abs(np.fft.fft(p)[1:]))) + 2
    if index > len(p) / 2:
        index = len(p) - index + 2
    return 1.0 / (domain / (index - 1))


def scale2frequency(wavelet, scales, precision: int = 8) -> np.ndarray:
    """pywt.scale2frequency: central_frequency / scale, in cycles per sample."""
    return central_frequency(wavelet, precision) / np.asarray(scales, dtype=np.float64)


def scalogram_scales(num, L) -> np.ndarray:
    """The scale grid the reference's plot_scalogram makes from a count: geomspace(1, max(2, L / 8), max(1, num))."""
    return np.geomspace(1.0, max(2.0, L / 8.0), num=max(1, int(num)))


@dataclass(frozen=True)
class CwtPlan:
    wavelet: Wavelet
    scales: np.ndarray     # [S] float64, the caller's order
    table: np.ndarray      # float32: every filter in turn; a complex one is its re plane, then its im plane
    table64: tuple         # the filters before rounding (float64 / complex128), one array per scale
    tab_off: np.ndarray    # [S] int64: where filter s starts in table
    taps: np.ndarray       # [S] int32: len(h_s) = len(k_s) + 1
    offset: np.ndarray     # [S] int32: floor(d), pywt.cwt's crop; the device's shift is offset + 1
    l1: np.ndarray         # [S] float64: ||h_s||_1 (of the float64 filter); A_s = l1 max|x|

    @property
    def S(self) -> int:
        return int(self.scales.size)

    @property
    def planes(self) -> int:
        return 2 if self.wavelet.complex else 1

    def filter32(self, i: int) -> np.ndarray:
        """Filter i as the device holds it: float32, or complex64 for a complex wavelet."""
        o, n = int(self.tab_off[i]), int(self.taps[i])
        if self.wavelet.complex:
            return self.table[o:o + n] + 1j * self.table[o + n:o + 2 * n]
        return self.table[o:o + n]

    def meta(self, idx) -> np.ndarray:
        """[len(idx), 4] int32 of syg_cwt_f32: {offset in table, taps, shift, index of the scale in y}."""
        idx = np.asarray(idx, dtype=np.int64)
        return np.ascontiguousarray(np.stack([self.tab_off[idx], self.taps[idx], self.offset[idx] + 1, idx], axis=1).astype(np.int32))

    def reach(self, idx, group: int) -> int:
        """The widest input span, at one output column, of the groups of `group` consecutive entries of idx."""
        idx = np.asarray(idx, dtype=np.int64)
        shift, taps = self.offset[idx].astype(np.int64) + 1, self.taps[idx].astype(np.int64)
        best = 1
        for g in range(0, idx.size, group):
            sh, tp = shift[g:g + group], taps[g:g + group]
            best = max(best, int(sh.max() - (sh - tp + 1).min() + 1))
        return best


@functools.lru_cache(maxsize=32)
def _plan(name: str, s_bytes: bytes) -> CwtPlan:
    w = parse_wavelet(name)
    scales = np.frombuffer(s_bytes, dtype=np.float64).copy()
    hs, offs = zip(*(scale_filter(w, float(s)) for s in scales))
    taps = np.array([h.size for h in hs], dtype=np.int64)
    planes = 2 if w.complex else 1
    tab_off = np.concatenate([[0], np.cumsum(taps * planes)[:-1]]).astype(np.int64)
    if int(taps.sum()) * planes >= 2 ** 31:
        raise ValueError(f"cwt: the filter table of these scales takes {int(taps.sum()) * planes} floats, above the bound of 2^31")
    parts = []
    for h in hs:
        parts += [h.real.astype(np.float32), h.imag.astype(np.float32)] if w.complex else [h.astype(np.float32)]
    l1 = np.array([np.abs(h).sum() for h in hs])
    scales.setflags(write=False)
    return CwtPlan(w, scales, np.concatenate(parts), tuple(hs), tab_off, taps.astype(np.int32), np.array(offs, dtype=np.int32), l1)


def cwt_plan(scales, wavelet="morl") -> CwtPlan:
    """The filters of a scale list (independent of the row length), cached per wavelet and scale list."""
    w = parse_wavelet(wavelet)
    return _plan(w.name, check_scales(scales).tobytes())


def split_forms(plan: CwtPlan, direct_taps_max: int, form):
    """(direct, spectral): the indices of the scales each path takes.  form None is the rule: a filter of at most
    direct_taps_max taps runs direct."""
    idx = np.arange(plan.S)
    if form == "direct":
        return idx, idx[:0]
    if form == "spectral":
        return idx[:0], idx
    short = plan.taps <= direct_taps_max
    return idx[short], idx[~short]


def spectral_rows(plan: CwtPlan, idx):
    """Filter rows of the spectral form over the scales idx: [(a, b or -1)].  A complex wavelet's row is one scale.  A real
    wavelet's row carries two, h_a + i h_b: neighbours in sorted order, and only within PAIR_RATIO of each other (A_s goes
    as sqrt(s), so the partner's rounding leaks in at no more than twice the scale's own); a scale without such a
    neighbour runs alone."""
    idx = [int(i) for i in idx]
    if plan.wavelet.complex:
        return [(i, -1) for i in idx]
    order = sorted(idx, key=lambda i: (plan.scales[i], i))
    rows, p = [], 0
    while p < len(order):
        a = order[p]
        if p + 1 < len(order) and plan.scales[order[p + 1]] <= PAIR_RATIO * plan.scales[a]:
            rows.append((a, order[p + 1]))
            p += 2
        else:
            rows.append((a, -1))
            p += 1
    return rows


def spectral_tables(plan: CwtPlan, rows, M: int):
    """(h [R, M, 2] float32, zero-padded filter rows whose transforms the device takes once; rmeta [R, 4] int32 of
    syg_cwt_crop_f32: {shift_a, index_a, shift_b, index_b})."""
    h = np.zeros((len(rows), M, 2), dtype=np.float32)
    rmeta = np.zeros((len(rows), 4), dtype=np.int32)
    for r, (a, b) in enumerate(rows):
        fa = plan.filter32(a)
        if plan.wavelet.complex:
            h[r, :fa.size, 0], h[r, :fa.size, 1] = fa.real, fa.imag
            rmeta[r] = (plan.offset[a] + 1, a, 0, -1)
        else:
            h[r, :fa.size, 0] = fa
            rmeta[r] = (plan.offset[a] + 1, a, 0, -1)
            if b >= 0:
                fb = plan.filter32(b)
                h[r, :fb.size, 1] = fb
                rmeta[r, 2:] = (plan.offset[b] + 1, b)
    return h, rmeta
