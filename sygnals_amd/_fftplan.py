"""Which launches serve a complex transform of length n: fft_plan.  Every "do the kernels take this length directly?"
question -- fft_any's dispatch, the Bluestein and convolution length searches, the fused real-input and analytic forms --
is asked here and nowhere else.  Pure host logic: no torch, no library (tests/test_host_logic.py pins the answers).
sygnals_amd.ops runs a plan (ops._run_plan)."""

MAX_LDS_FFT = 8192        # longest power-of-two transform of one workgroup (syg_fft_pow2_*)
MAX_MIXED_FFT = 8192      # longest mixed-radix one (syg_fft_mixed_*)
MAX_ROWS = 65535          # rows of one launch: the four-step passes put them on a grid axis


def is_pow2(n: int) -> bool:
    return n >= 2 and (n & (n - 1)) == 0


def _is_smooth(n: int) -> bool:
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def smooth_split(n: int):
    """None when n has a prime factor other than 2, 3, 5, 7 (or is too long); (n, 1) when one mixed-radix launch
    takes it; else the most balanced (n1, n2), n1 * n2 = n, both <= 8192 -- the four-step factors."""
    if n < 2 or not _is_smooth(n):
        return None
    if n <= MAX_MIXED_FFT:
        return n, 1
    best = None
    d = 1
    while d * d <= n:
        if n % d == 0 and n // d <= MAX_MIXED_FFT:
            best = (d, n // d)                       # d <= sqrt(n): the largest such d is the most balanced split
        d += 1
    return best


def fft_plan(n: int):
    """(kind, n1, n2) of a length-n complex transform the kernels take directly -- kind "pow2" or "mixed" names the
    engine, n2 == 1 is one launch of length n1 = n, otherwise the four-step passes A (n2 transforms of length n1) and B
    (n1 of length n2) -- or None: powers of two above 2^26, 7-smooth lengths without a split into two factors <= 8192,
    and every other length (Bluestein)."""
    if is_pow2(n):
        if n <= MAX_LDS_FFT:
            return "pow2", n, 1
        n1 = 1 << ((n.bit_length() - 1) // 2)
        return ("pow2", n1, n // n1) if n // n1 <= MAX_LDS_FFT else None
    split = smooth_split(n)
    return None if split is None else ("mixed",) + split


def next_direct_len(m: int) -> int:
    """The smallest length >= m that has a plan.  A power of two beyond the longest plan ends the search as well: the
    transform then reports that length as unsupported."""
    while fft_plan(m) is None and not is_pow2(m):
        m += 1
    return m


def conv_fft_len(n_out: int) -> int:
    """Transform length (in real samples, even) for a linear convolution with n_out output samples: the smallest
    M >= n_out, M >= 16, whose half M/2 is a product of 2, 3, 5, 7 that the FFT kernels take directly -- what
    scipy.fft.next_fast_len does for fftconvolve.  (A power of two can be up to twice the needed length.)"""
    return 2 * next_direct_len(max(16, n_out + (n_out & 1)) // 2)
