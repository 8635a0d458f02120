"""Host tables of syg_laplace_f32 (csrc/laplace.hip; the layout is the one include/sygnals_hip.h documents): pure NumPy,
float64 throughout, the float32 table rounded once.  No device and no library here: the constants come in as arguments
(ops.laplace reads them from the library), so the builder is tested on the CPU."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

STEEP_LOG = 40.0          # a column is steep where |Re(s) t_step| (C - 1) exceeds this: exp(-40) keeps the table normal
DOMAIN = 700.0            # -Re(s) t_step (L - 1) beyond this overflows the reference's own exp


@dataclass(frozen=True)
class LaplacePlan:
    table: np.ndarray     # [C, 2, S16] float32
    fac: np.ndarray       # [Sc, fac_stride] float64
    col: np.ndarray       # [Sc] int32, -1 in padding
    s_t: np.ndarray       # [Sc] complex128: s t_step per column (0 in padding)
    rev: np.ndarray       # [Sc] bool: served as the transform of the reversed row
    S: int
    S_fwd: int            # padded
    S_rev: int            # padded
    S_steep_fwd: int
    S_steep_rev: int

    @property
    def S16(self) -> int:
        return self.S_fwd + self.S_rev


def check_s_values(s_values, t_step) -> np.ndarray:
    s = np.asarray(s_values, dtype=np.complex128)
    if s.ndim != 1:
        raise ValueError("s_values must be 1D.")
    if not np.isfinite(t_step):
        raise ValueError(f"t_step must be finite, got {t_step}.")
    bad = np.flatnonzero(~np.isfinite(s))
    if bad.size:
        raise ValueError(f"s_values[{bad[0]}] = {s[bad[0]]} is not finite.")
    return s


def check_domain(s: np.ndarray, t_step: float, L: int) -> None:
    """The served domain: -Re(s) t_step (L - 1) <= 700 for every s (beyond it the reference's exp gives inf / nan)."""
    g = -s.real * float(t_step) * max(L - 1, 0)
    bad = np.flatnonzero(g > DOMAIN * (1.0 + 1e-12))                 # a bound written as -700 / ((L - 1) t_step) rounds to 700 + 1 ulp
    if bad.size:
        i = bad[0]
        raise ValueError(f"s_values[{i}] = {s[i]} is outside the served domain: -Re(s) * t_step * (L - 1) = {g[i]:.6g} "
                         f"exceeds {DOMAIN:g} (exp overflows float64 there)")


def plan(s_values, t_step: float, C: int, tile_cols: int, segment: int, steep: int, fac_stride: int) -> LaplacePlan:
    s = check_s_values(s_values, t_step)
    S = s.size
    if STEEP_LOG / (C - 1) * steep < 746.0 or fac_stride != 38 or segment % C:
        raise ValueError("laplace plan: the library's constants do not fit this table builder")
    st = s * float(t_step)
    a = st.real
    is_steep = np.abs(a) * (C - 1) > STEEP_LOG
    is_rev = a < 0
    groups = [np.flatnonzero(~is_steep & ~is_rev), np.flatnonzero(~is_steep & is_rev),
              np.flatnonzero(is_steep & ~is_rev), np.flatnonzero(is_steep & is_rev)]
    pad = [(-len(groups[0])) % tile_cols, (-len(groups[1])) % tile_cols, 0, 0]
    col = np.concatenate([np.concatenate([g, np.full(p, -1, dtype=np.int64)]) for g, p in zip(groups, pad)]).astype(np.int32)
    live = col >= 0
    Sc = col.size
    s_t = np.zeros(Sc, dtype=np.complex128)
    s_t[live] = st[col[live]]
    rev = np.zeros(Sc, dtype=bool)
    rev[live] = is_rev[col[live]]
    e = np.where(rev, s_t, -s_t)                                     # z = exp(e), |z| <= 1
    S_fwd, S_rev = len(groups[0]) + pad[0], len(groups[1]) + pad[1]
    S16 = S_fwd + S_rev
    i = np.arange(C, dtype=np.float64)[:, None]
    power = np.where(rev[None, :S16], C - 1 - i, i)                  # forward z^i, reversed z^(C - 1 - i)
    tab = np.exp(e[None, :S16] * power) * live[None, :S16]
    table = np.stack([tab.real, tab.imag], axis=1).astype(np.float32)          # [C, 2, S16]
    powers = np.concatenate([np.arange(16) * C, [16 * C, segment, 1]]).astype(np.float64)
    z = np.exp(e[:, None] * powers[None, :]) * live[:, None]
    fac = np.stack([z.real, z.imag], axis=2).reshape(Sc, fac_stride)
    return LaplacePlan(np.ascontiguousarray(table), np.ascontiguousarray(fac), col, s_t, rev, S, S_fwd, S_rev,
                       len(groups[2]), len(groups[3]))


def anchors(p: LaplacePlan, L: int) -> np.ndarray:
    """[Sc, 2] float64: 1 for a forward column, exp(-s (L - 1) t_step) for a reversed one (finite inside the domain)."""
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.where(p.rev, np.exp(-p.s_t * float(L - 1)), 1.0 + 0.0j) * (p.col >= 0)
    return np.ascontiguousarray(np.stack([a.real, a.imag], axis=1))
