"""The cases that pin the strided FFT path bit for bit (tests/golden/fft_strided_before.json, recorded from the code before
the two kernel pairs, the two launchers and the Python compositions were given one home): the smallest lengths at which
each kernel and each launch rule is reached.  Inputs come from numpy's default_rng(seed) on the host, so they do not depend
on the device; the kernels have no atomics, so a result is a function of its input alone.

    name -> (op, seed, args)        run(name) -> the result as a contiguous float32 host array
"""
import hashlib

import numpy as np

CASES = {}


def _add(op, *args):
    CASES["%s-%s" % (op, "-".join(str(a) for a in args))] = (op, 1000 + len(CASES), args)


# fft_any(x [rows, n, 2], inverse):
#   6000          mixed row kernel, one launch              2025, 1009   Bluestein over a mixed length
#   16384         power-of-two tiles of 16 columns          65536        the 40 KB rule: 8 columns
#   2^19          8 and 4 columns                           2^21         pass B has n2 = 2048: power-of-two row kernel
#   48000         mixed tiles 8 wide, once by the LDS rule (n = 200) and once by divisibility (batch 200)
#   44100         batch 210 divides by no tile: both passes in the mixed row kernel
#   3 * 2^20      mixed, n2 = 2048 (1 row)                  2^25         bign > 2^24: the double twiddle (1 row, forward)
for _n in (6000, 2025, 1009, 16384, 65536, 1 << 19, 1 << 21, 48000, 44100):
    for _inv in (0, 1):
        _add("fft_any", _n, 3, _inv)
for _inv in (0, 1):
    _add("fft_any", 3 << 20, 1, _inv)
_add("fft_any", 1 << 25, 1, 0)
# analytic_fused(x [rows, n], magnitude): the fused ends, one launch (16, 250, 4096, 6000) and two
for _n in (16, 250, 4096, 6000, 16384, 44100, 48000):
    for _mag in (0, 1):
        _add("analytic_fused", _n, 3, _mag)
# fft_pair_rows(x [rows, 2 H - 3], H): the zero fill of the pair load is read
for _H in (256, 6000, 16384, 24000):
    _add("fft_pair_rows", _H, 3)
# rfft_conv(x [rows, n], k [1, taps])
_add("rfft_conv", 48000, 3, 512)


def run(name):
    import torch
    from sygnals_amd import ops
    op, seed, args = CASES[name]
    rng = np.random.default_rng(seed)
    dev = lambda shape: torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).cuda()
    if op == "fft_any":
        n, rows, inv = args
        out = ops.fft_any(dev((rows, n, 2)), bool(inv))
    elif op == "analytic_fused":
        n, rows, mag = args
        out = ops.analytic_fused(dev((rows, n)), bool(mag))
    elif op == "fft_pair_rows":
        H, rows = args
        out = ops.fft_pair_rows(dev((rows, 2 * H - 3)), H)
    else:
        n, rows, taps = args
        x = dev((rows, n))
        out = ops.rfft_conv(x, dev((1, taps)))
    assert out is not None and out.dtype == torch.float32, name
    return np.ascontiguousarray(out.contiguous().cpu().numpy())


def digest(a):
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "first8": [float(v) for v in a.ravel()[:8]]}
