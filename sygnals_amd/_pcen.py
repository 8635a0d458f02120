"""Host side of PCEN (csrc/pcen.hip): the argument rules, the time_constant -> b rule and the per-band parameter table.

pcen(S) is librosa 0.10's: with ref = S (or its running maximum over max_size bands),
    M, zf = scipy.signal.lfilter([b], [1, b - 1], ref, zi=zi)        (zi None: lfilter_zi = 1 - b, not scaled by S[..., 0])
    smooth = exp(-gain (log(eps) + log1p(M / eps)))
    power == 0: log1p(S smooth);  bias == 0: exp(power (log S + log smooth));  else bias**power expm1(power log1p(S smooth / bias))
gain, bias, power, eps and b may each be a scalar or a vector with one value per band.  No device is needed here."""
from __future__ import annotations

import numpy as np

MAX_OUT = 1 << 31
TABLE_WORDS = 8          # SYG_PCEN_TABLE_WORDS: b, (1 - b)^tile, eps, gain, power, bias, bias^power, the case
LAW_GENERAL, LAW_POWER0, LAW_BIAS0 = 0, 1, 2
SERVED = ("gain >= 0, bias >= 0, power >= 0, eps > 0, time_constant > 0, 0 < b <= 1 (scalars or one value per band), "
          "1 <= max_size <= bands")


def b_from_time_constant(time_constant, sr, hop_length, who: str = "pcen") -> float:
    """librosa's rule: b = (sqrt(1 + 4 t^2) - 1) / (2 t^2) with t = time_constant sr / hop_length."""
    tc = _number(time_constant, "time_constant", who)
    if not tc > 0:
        raise ValueError(f"{who}: time_constant must be strictly positive (got {time_constant!r}; served: {SERVED})")
    if not (_number(sr, "sr", who) > 0 and _number(hop_length, "hop_length", who) > 0):
        raise ValueError(f"{who}: sr and hop_length must be positive (got {sr!r}, {hop_length!r})")
    t = tc * float(sr) / float(hop_length)
    return float((np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t))


def _number(v, name: str, who: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{who}: {name} must be a real number (got {v!r})")
    return float(v)


def check_max_size(max_size, M: int, who: str = "pcen") -> int:
    if isinstance(max_size, bool) or not isinstance(max_size, (int, np.integer)) or max_size < 1:
        raise ValueError(f"{who}: max_size must be an integer >= 1 (got {max_size!r})")
    if max_size > M:
        raise ValueError(f"{who}: max_size = {max_size} exceeds the {M} bands (served: 1 <= max_size <= bands)")
    return int(max_size)


def check_scale(scale, who: str = "pcen") -> float:
    s = _number(scale, "scale", who)
    if not (s > 0 and np.isfinite(s)):
        raise ValueError(f"{who}: scale must be positive and finite (got {scale!r})")
    return s


def check_size(who: str, B: int, M: int, T: int) -> None:
    if min(B, M, T) < 1:
        raise ValueError(f"{who}: empty input (shape [{B}, {M}, {T}])")
    if B * M * T > MAX_OUT:
        raise ValueError(f"{who}: a result of {B * M * T} elements is above 2^31 = {MAX_OUT}")


_RULES = {"gain": (lambda v: v >= 0, "non-negative"), "bias": (lambda v: v >= 0, "non-negative"),
          "power": (lambda v: v >= 0, "non-negative"), "eps": (lambda v: v > 0, "strictly positive"),
          "b": (lambda v: (v > 0) & (v <= 1), "in (0, 1] (at b = 0 scipy.signal.lfilter_zi is singular)")}


def check_params(M: int, gain, bias, power, eps, b, who: str = "pcen"):
    """(values, per_band): the five parameters in the order gain, bias, power, eps, b as float64 scalars, or, where any of
    them is a vector, as five float64 [M] arrays."""
    vals, per_band = [], False
    for name, v in (("gain", gain), ("bias", bias), ("power", power), ("eps", eps), ("b", b)):
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        a = np.asarray(v)
        if a.dtype == bool or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
            raise ValueError(f"{who}: {name} must be a real number or one per band (got {v!r})")
        a = a.astype(np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != M):
            raise ValueError(f"{who}: {name} must be a scalar or a vector of one value per band ({M}); got shape {list(a.shape)}")
        ok, words = _RULES[name]
        if not (np.all(np.isfinite(a)) and np.all(ok(a))):
            raise ValueError(f"{who}: {name} must be {words} (got {v!r}; served: {SERVED})")
        per_band = per_band or a.ndim == 1
        vals.append(a)
    if per_band:
        return [np.broadcast_to(a, (M,)).copy() for a in vals], True
    return [float(a) for a in vals], False


def pack_table(vals, tile: int) -> np.ndarray:
    """The device table [M, TABLE_WORDS] float64 of per-band parameters (every derived figure is made here, in float64)."""
    gain, bias, power, eps, b = (np.asarray(v, dtype=np.float64) for v in vals)
    tab = np.empty((b.shape[0], TABLE_WORDS), dtype=np.float64)
    tab[:, 0] = b
    tab[:, 1] = (1.0 - b) ** tile
    tab[:, 2], tab[:, 3], tab[:, 4], tab[:, 5] = eps, gain, power, bias
    tab[:, 6] = bias ** power
    tab[:, 7] = np.where(power == 0, LAW_POWER0, np.where(bias == 0, LAW_BIAS0, LAW_GENERAL))
    return tab


def check_zi(zi, B: int, M: int, who: str = "pcen"):
    """zi as a float64 array or tensor [B, M] (scipy's state z = (1 - b) M of every row), or None."""
    if zi is None:
        return None
    shape = tuple(zi.shape) if hasattr(zi, "shape") else np.shape(zi)
    if shape != (B, M):
        raise ValueError(f"{who}: zi must be [B, M] = [{B}, {M}] (the filter state of every row; got shape {list(shape)})")
    return zi
