"""The CQT parameter table shared by the host tests (plan against the oracle, routing) and the device tests
(tests/test_gpu_cqt_params.py): every row is one call of ops.cqt / compute_cqt away from the single point
(bins_per_octave 12, tuning 0, filter_scale 1, sparsity 0.01, whole octaves) the older tests sit on.  ROUTES pins what
sygnals_amd._cqt.cqt_route answers for it, so that the claim "this row runs that kernel" stays true."""
from collections import namedtuple

Case = namedtuple("Case", "sr hop fmin n_bins bpo tuning filter_scale sparsity")


def _c(sr, hop, fmin, n_bins, bpo=12, tuning=0.0, filter_scale=1.0, sparsity=0.01):
    return Case(sr, hop, fmin, n_bins, bpo, tuning, filter_scale, sparsity)


CASES = {
    "default": _c(48000, 512, None, 84),
    "fs0.5": _c(48000, 512, None, 84, filter_scale=0.5),
    "fs2": _c(48000, 512, None, 84, filter_scale=2.0),
    "dense": _c(48000, 512, None, 84, sparsity=0.0),
    "tune+.37": _c(48000, 512, None, 84, tuning=0.37),
    "tune-.5": _c(48000, 512, None, 84, tuning=-0.5),
    "bins80": _c(48000, 512, None, 80),
    "bins77": _c(48000, 512, None, 77),
    "bins7": _c(48000, 512, None, 7),
    "bins1": _c(48000, 512, None, 1),
    "bpo8": _c(48000, 512, None, 56, 8),
    "bpo8-fs0.9": _c(48000, 512, None, 56, 8, filter_scale=0.9),
    "bpo16": _c(48000, 512, None, 112, 16),
    "bpo16-fs0.5": _c(48000, 512, None, 112, 16, filter_scale=0.5),
    "bpo24": _c(48000, 512, None, 168, 24),
    "bpo24-fs0.5": _c(48000, 512, None, 168, 24, filter_scale=0.5),
    "bpo24-fs0.25": _c(48000, 512, None, 160, 24, filter_scale=0.25),
    "bpo36": _c(48000, 512, None, 252, 36),
    "bpo36-fs0.25": _c(48000, 512, None, 252, 36, filter_scale=0.25),
    "bpo3": _c(48000, 512, None, 21, 3),
    "bpo1": _c(48000, 512, None, 7, 1),
    "22k": _c(22050, 256, None, 72),
    "16k": _c(16000, 256, 65.4, 60),
    "16k-hop160": _c(16000, 160, 100.0, 48),
    "hop192": _c(48000, 192, 130.8, 60),
    "hop96": _c(48000, 96, 261.6, 48),
    "hop100": _c(48000, 100, 1046.5, 24),
    "hop1": _c(48000, 1, 4186.0, 12),
    "8k": _c(8000, 512, None, 72),
    "96k": _c(96000, 512, None, 96),
}


def kwargs(c: Case) -> dict:
    """Keyword arguments of ops.cqt / oracle.cpu_ref.cqt (both take these names)."""
    return dict(hop_length=c.hop, fmin=c.fmin, n_bins=c.n_bins, bins_per_octave=c.bpo, tuning=c.tuning,
                filter_scale=c.filter_scale, sparsity=c.sparsity)


def B(n_fft, n_filt, tiles):
    return ("syg_cqt_octave_bf16x3_f32", n_fft, n_filt, tiles)


def G(n_fft, n_filt, tiles):
    return ("syg_cqt_octave_gemm_f32", n_fft, n_filt, tiles)


def F(n_fft, n_filt, groups):
    return ("syg_cqt_octave_f32", n_fft, n_filt, groups)


MODES = ("bf16x3", "gemm", "fft")
# case -> (the default mode takes the one-launch form, early decimations, the level-by-level calls per octave (top octave
# first) in the modes bf16x3, gemm, fft).  Fourth field: 16-row tiles of the matrix forms -- two tiles, or an even count at
# n_fft <= 256 for the gemm form, run as the kernels' <N, 2> instantiation, everything else as <N, 1> -- and the number
# of calls (row groups of <= 24 filters) for syg_cqt_octave_f32.
ROUTES = {
    "default": (True, 1,
        7 * [B(256, 12, 2)],
        7 * [G(256, 12, 2)],
        7 * [F(256, 12, 1)]),
    "fs0.5": (False, 1,
        7 * [B(128, 12, 2)],
        7 * [G(128, 12, 2)],
        7 * [F(128, 12, 1)]),
    "fs2": (False, 1,
        7 * [G(512, 12, 2)],
        7 * [G(512, 12, 2)],
        7 * [F(512, 12, 1)]),
    "dense": (True, 1,
        7 * [B(256, 12, 2)],
        7 * [G(256, 12, 2)],
        7 * [F(256, 12, 1)]),
    "tune+.37": (True, 1,
        7 * [B(256, 12, 2)],
        7 * [G(256, 12, 2)],
        7 * [F(256, 12, 1)]),
    "tune-.5": (True, 1,
        7 * [B(256, 12, 2)],
        7 * [G(256, 12, 2)],
        7 * [F(256, 12, 1)]),
    "bins80": (False, 1,
        6 * [B(256, 12, 2)] + 1 * [B(256, 8, 1)],
        6 * [G(256, 12, 2)] + 1 * [G(256, 8, 1)],
        6 * [F(256, 12, 1)] + 1 * [F(256, 8, 1)]),
    "bins77": (False, 2,
        6 * [B(256, 12, 2)] + 1 * [B(128, 5, 1)],
        6 * [G(256, 12, 2)] + 1 * [G(128, 5, 1)],
        6 * [F(256, 12, 1)] + 1 * [F(128, 5, 1)]),
    "bins7": (False, 7,
        1 * [B(256, 7, 1)],
        1 * [G(256, 7, 1)],
        1 * [F(256, 7, 1)]),
    "bins1": (False, 8,
        1 * [B(128, 1, 1)],
        1 * [G(128, 1, 1)],
        1 * [F(128, 1, 1)]),
    "bpo8": (True, 1,
        7 * [B(256, 8, 1)],
        7 * [G(256, 8, 1)],
        7 * [F(256, 8, 1)]),
    "bpo8-fs0.9": (False, 1,
        7 * [B(128, 8, 1)],
        7 * [G(128, 8, 1)],
        7 * [F(128, 8, 1)]),
    "bpo16": (False, 1,
        7 * [G(512, 16, 2)],
        7 * [G(512, 16, 2)],
        7 * [F(512, 16, 1)]),
    "bpo16-fs0.5": (True, 1,
        7 * [B(256, 16, 2)],
        7 * [G(256, 16, 2)],
        7 * [F(256, 16, 1)]),
    "bpo24": (False, 1,
        7 * [G(512, 24, 3)],
        7 * [G(512, 24, 3)],
        7 * [F(512, 24, 1)]),
    "bpo24-fs0.5": (False, 1,
        7 * [G(256, 24, 3)],
        7 * [G(256, 24, 3)],
        7 * [F(256, 24, 1)]),
    "bpo24-fs0.25": (False, 1,
        6 * [G(128, 24, 3)] + 1 * [B(128, 16, 2)],
        6 * [G(128, 24, 3)] + 1 * [G(128, 16, 2)],
        6 * [F(128, 24, 1)] + 1 * [F(128, 16, 1)]),
    "bpo36": (False, 1,
        7 * [F(1024, 36, 2)],
        7 * [F(1024, 36, 2)],
        7 * [F(1024, 36, 2)]),
    "bpo36-fs0.25": (False, 1,
        7 * [G(256, 36, 5)],
        7 * [G(256, 36, 5)],
        7 * [F(256, 36, 2)]),
    "bpo3": (False, 1,
        7 * [F(64, 3, 1)],
        7 * [F(64, 3, 1)],
        7 * [F(64, 3, 1)]),
    "bpo1": (False, 1,
        7 * [F(32, 1, 1)],
        7 * [F(32, 1, 1)],
        7 * [F(32, 1, 1)]),
    "22k": (False, 1,
        6 * [B(256, 12, 2)],
        6 * [G(256, 12, 2)],
        6 * [F(256, 12, 1)]),
    "16k": (False, 0,
        5 * [G(512, 12, 2)],
        5 * [G(512, 12, 2)],
        5 * [F(512, 12, 1)]),
    "16k-hop160": (False, 1,
        4 * [B(256, 12, 2)],
        4 * [G(256, 12, 2)],
        4 * [F(256, 12, 1)]),
    "hop192": (False, 1,
        5 * [B(256, 12, 2)],
        5 * [G(256, 12, 2)],
        5 * [F(256, 12, 1)]),
    "hop96": (False, 1,
        4 * [B(256, 12, 2)],
        4 * [G(256, 12, 2)],
        4 * [F(256, 12, 1)]),
    "hop100": (False, 1,
        2 * [B(256, 12, 2)],
        2 * [G(256, 12, 2)],
        2 * [F(256, 12, 1)]),
    "hop1": (False, 0,
        1 * [B(256, 12, 2)],
        1 * [G(256, 12, 2)],
        1 * [F(256, 12, 1)]),
    "8k": (False, 0,
        6 * [B(256, 12, 2)],
        6 * [G(256, 12, 2)],
        6 * [F(256, 12, 1)]),
    "96k": (False, 1,
        8 * [B(256, 12, 2)],
        8 * [G(256, 12, 2)],
        8 * [F(256, 12, 1)]),
}
