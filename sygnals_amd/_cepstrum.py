"""Host side of the cepstral analysis (csrc/cepstrum.hip; the float64 restatement is tests/cepstrum_ref.py): the defaults,
the argument rules and the quefrency range of the cepstral pitch method.  No device work."""
from __future__ import annotations

import math

AMIN = 1e-5                 # floor of |X|: the square root of the 1e-10 power floor of the dB code
THRESHOLD = 0.13            # voicing threshold of the cepstral peak (2048-sample hann frames at 22 050 Hz: white noise
#                             peaks at most 0.095, harmonic complexes from 82 to 1000 Hz at least 0.186)
MAX_N = 1 << 26             # the longest row (the longest transform plan)
MAX_ELEMS = 1 << 31         # elements of one result at most


def check_amin(amin) -> float:
    a = float(amin)
    if not math.isfinite(a) or a < 0.0:
        raise ValueError(f"amin must be finite and >= 0, got {amin}")
    return a


def check_n_ceps(n_ceps, n_fft: int) -> int:
    """Q: n_ceps, or n_fft // 2 + 1 when it is None; 1 <= Q <= n_fft."""
    if n_ceps is None:
        return n_fft // 2 + 1
    if isinstance(n_ceps, bool) or int(n_ceps) != n_ceps or not 1 <= n_ceps <= n_fft:
        raise ValueError(f"n_ceps={n_ceps} is outside 1 ... n_fft = {n_fft}")
    return int(n_ceps)


def check_size(what: str, dims, names) -> None:
    total = 1
    for d in dims:
        total *= int(d)
    if total > MAX_ELEMS:
        shape = " x ".join(f"{int(d)} {n}" for d, n in zip(dims, names))
        raise ValueError(f"{what}: the result of {shape} has {total} elements, above the bound of 2^31; take fewer rows a call")


def row_length(n, L: int, n_min: int = 1) -> int:
    """The transform length of a whole-row cepstrum: n, or the row's length."""
    if n is None:
        n = L
    if isinstance(n, bool) or int(n) != n or n < n_min:
        raise ValueError(f"n must be an integer >= {n_min}, got {n}")
    if n > MAX_N:
        raise ValueError(f"n={n} is above the longest transform, 2^26")
    return int(n)


def quefrency_range(sr, fmin, fmax, n_fft: int):
    """(qmin, qmax) = (ceil(sr / fmax), min(floor(sr / fmin), n_fft // 2 - 1)); refused when empty."""
    sr, fmin, fmax = float(sr), float(fmin), float(fmax)
    if not (sr > 0 and fmin > 0 and fmax > 0 and math.isfinite(sr) and math.isfinite(fmin) and math.isfinite(fmax)):
        raise ValueError(f"cepstral pitch: fmin={fmin}, fmax={fmax} and sr={sr} must be positive and finite")
    qmin = int(math.ceil(sr / fmax))
    qmax = min(int(math.floor(sr / fmin)), n_fft // 2 - 1)
    if qmin < 1 or qmin > qmax:
        raise ValueError(f"cepstral pitch: fmin={fmin}, fmax={fmax} at sr={sr} leave no quefrency range in frames of {n_fft} "
                         f"samples (qmin={qmin}, qmax={qmax})")
    return qmin, qmax
