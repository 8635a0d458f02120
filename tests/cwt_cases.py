"""The continuous-wavelet case table shared by the host checks (tests/test_cwt_cases.py: every case reaches the inner
forms and the transform lengths it names) and the device tests (tests/test_gpu_cwt_params.py).  Plain data and host
arithmetic, no device.

`route` restates the launch rules of syg_cwt_f32 and cwt_direct_kernel (sygnals_amd/csrc/cwt.hip) on the host: the
tap-count sort of ops._cwt_direct_dev, the plan's reach, the staged words of the span and of the taps, and per block the
choice between the three inner forms
    vec      cw_scale_vec: stride 1, staged span, staged taps
    staged   cw_scale<., true>: staged span, taps from global memory
    global   cw_scale<., false>: nothing staged.
Its constants are the library's (ops.cwt_constants()), so a changed constant fails the table instead of silently testing
something else."""
from collections import namedtuple

import numpy as np

from sygnals_amd import _cwt as CW

CMOR = "cmor1.5-1.0"
WAVELETS = ("morl", "mexh", "gaus1", CMOR)

Routed = namedtuple("Routed", "group tile scale form taps delta cnt")


def constants():
    """ops.cwt_constants(): the library's own figures (no device is needed for them)."""
    from sygnals_amd import ops
    return ops.cwt_constants()


def route(L, stride, scales, wavelet, idx=None, k=None):
    """[Routed] in launch order: per (scale group, tile, entry of the sorted meta) the caller's index of the scale, the
    inner form the block takes for it, its tap count, the zero taps cw_scale_vec puts in front (delta) and the tile's
    column count.  idx: the scales that run direct (default: all of them, form="direct")."""
    k = constants() if k is None else k
    tile, spg, span_max, taps_max = k["tile"], k["scales_per_group"], k["span_max"], k["taps_lds_max"]
    plan = CW.cwt_plan(scales, wavelet)
    idx = np.arange(plan.S) if idx is None else np.asarray(idx, dtype=np.int64)
    idx = idx[np.argsort(plan.taps[idx], kind="stable")]
    reach = plan.reach(idx, spg)
    n_out = -(-L // stride)
    xs_words = min(((tile - 1) * stride + reach + 12 + 3) & ~3, span_max + 12)
    hs_words = min(plan.planes * ((reach + 6 + 3) & ~3), taps_max) if stride == 1 else 0
    out = []
    for g in range(0, idx.size, spg):
        members = idx[g:g + spg]
        shift, taps = plan.offset[members].astype(np.int64) + 1, plan.taps[members].astype(np.int64)
        lo_rel, hi_rel = int((shift - (taps - 1)).min()), int(shift.max())
        for t in range(-(-n_out // tile)):
            cnt = min(tile, n_out - t * tile)
            stage = (cnt - 1) * stride + (hi_rel - lo_rel) + 1 + 12 <= xs_words
            for s, sh, tp in zip(members, shift, taps):
                if stage and stride == 1 and plan.planes * (tp + 6) <= hs_words:
                    form = "vec"
                else:
                    form = "staged" if stage else "global"
                out.append(Routed(g // spg, t, int(s), form, int(tp), (4 - ((int(sh) - lo_rel) & 3)) & 3, cnt))
    return out


def sorted_order(scales, wavelet):
    """The order in which the direct launch takes the caller's scales (ops._cwt_direct_dev)."""
    return [int(i) for i in np.argsort(CW.cwt_plan(scales, wavelet).taps, kind="stable")]


def first_scale(wavelet, taps):
    """The first scale on the grid 0.005, 0.010, ... whose filter has `taps` taps."""
    w = CW.parse_wavelet(wavelet)
    for n in range(1, 400):
        s = round(0.005 * n, 3)
        try:
            if CW.scale_filter(w, s)[0].size == taps:
                return s
        except ValueError:                               # too small a scale
            pass
    raise ValueError(f"no scale up to 2 gives {taps} taps of {wavelet}")


SMALL_TAPS = (3, 4, 5, 6, 7)
SMALL_L = (1, 5, 1027)


def small_scales(wavelet):
    """The first scales of 3 ... 7 taps and one of about 1000 taps (16 s + 2; 10 s + 2 for gaus1): the long filter sets
    the group's earliest sample, so that the short ones start at every residue of four words."""
    w = CW.parse_wavelet(wavelet)
    return tuple(first_scale(wavelet, t) for t in SMALL_TAPS) + (round(992.0 / (w.hi - w.lo), 3),)


# ---------------------------------------------------------------------------- the direct form
# must: {(tile, form)} the launch takes, exactly; per_scale: {index in scales: the forms that scale takes, exactly}
DirectCase = namedtuple("DirectCase", "name wavelet scales L stride B groups tiles must per_scale")
SIX = (1, 1.5, 2, 7.3, 32, 64.5)
SHUFFLED = (40, 1, 7.3, 64, 2, 1, 33.3, 5, 12, 3, 50, 9)          # two groups; scale 1 twice; no order


def _both(*forms):
    return frozenset((t, f) for t, fs in enumerate(forms) for f in fs)


def direct_cases():
    out = [
        # taps 8194, 9602, 14402 in both planes: the first fits the staged taps to the word, the others do not
        DirectCase("long-complex", CMOR, (512, 600, 900), 1500, 1, 3, 1, 2, _both(("vec", "staged"), ("vec", "staged")),
                   {0: {"vec"}, 1: {"staged"}, 2: {"staged"}}),
        DirectCase("at-the-bound", CMOR, (512,), 1025, 1, 3, 1, 2, _both(("vec",), ("vec",)), {0: {"vec"}}),
        DirectCase("past-the-bound", CMOR, (513,), 1025, 1, 3, 1, 2, _both(("staged",), ("staged",)), {0: {"staged"}}),
        # 16002 taps: a full tile's span is too long, the last tile of 76 columns fits
        DirectCase("unstaged-then-vec", "morl", (1000,), 1100, 1, 3, 1, 2, _both(("global",), ("vec",)), {}),
        # 17 x 1024 + 5 samples at stride 17: 1025 columns, the last of them the tile of its own
        DirectCase("stride-17", "morl", (1, 2, 7.3, 32), 17 * 1024 + 5, 17, 3, 1, 2, _both(("global",), ("staged",)), {}),
    ]
    for w in ("morl", CMOR):
        tag = "cmor" if w == CMOR else w
        out += [
            DirectCase(f"stride-3-{tag}", w, SIX, 5000, 3, 3, 1, 2, _both(("staged",), ("staged",)), {}),
            # a full tile spans 1023 x 16 + 1034 samples, the last tile's 226 columns 225 x 16 + 1034
            DirectCase(f"stride-16-{tag}", w, SIX, 20000, 16, 3, 1, 2, _both(("global",), ("staged",)), {}),
            DirectCase(f"shuffled-{tag}", w, SHUFFLED, 2100, 1, 3, 2, 3, _both(("vec",), ("vec",), ("vec",)), {}),
        ]
    for w in WAVELETS:
        tag = "cmor" if w == CMOR else w
        for L in SMALL_L:
            tiles = -(-L // 1024)
            out.append(DirectCase(f"small-{tag}-L{L}", w, small_scales(w), L, 1, 3, 1, tiles, _both(*[("vec",)] * tiles), {}))
            out.append(DirectCase(f"small-{tag}-L{L}-stride-2", w, small_scales(w), L, 2, 3, 1, 1, _both(("staged",)), {}))
    return out


def case_id(c):
    return c.name


# ---------------------------------------------------------------------------- the spectral form's lengths
# slack = M - (L + taps - 1); plan = ops.fft_plan(M)
SpecCase = namedtuple("SpecCase", "name scale taps L M plan B")
SPECTRAL_CASES = (
    SpecCase("pow2-one-launch-tight", 200, 3202, 895, 4096, ("pow2", 4096, 1), 3),
    SpecCase("pow2-one-launch-plus-1", 200, 3202, 896, 4116, ("mixed", 4116, 1), 3),
    SpecCase("mixed-tight", 200, 3202, 1503, 4704, ("mixed", 4704, 1), 3),
    SpecCase("pow2-four-step-tight", 300, 4802, 60735, 65536, ("pow2", 256, 256), 1),
    SpecCase("pow2-four-step-plus-1", 300, 4802, 60736, 65610, ("mixed", 243, 270), 1),
)
TIGHT = ("pow2-one-launch-tight", "mixed-tight", "pow2-four-step-tight")


def spectral_scales(c):
    """The case's scale and one half its size: the longer one sets M, and for a real wavelet the two share a filter row."""
    return (c.scale / 2, c.scale)


# ---------------------------------------------------------------------------- scale order, pairing, other parameters
# direct (2, 1, 7.3, 2: at most 1024 taps) and spectral scales interleaved, scale 2 twice, no order; scale 64 has 1026 taps
MIXED_ORDER = (300, 2, 700, 1, 100, 64, 65, 7.3, 150, 2)
MIXED_L = 1500
PAIR_S = 80                                                       # (s, 4 s): exactly PAIR_RATIO apart
PAIR_L = 3000
LAYOUT_SCALES = (1, 2, 7.3, 32, 64.5, 200)                        # 3202 taps over rows of 1500: past both ends of the row
LAYOUT_L = 1500
OTHER_CMOR = ("cmor0.5-2.0", "cmor2.0-0.5")
OTHER_CMOR_SCALES = (1, 7.3, 70)
OTHER_CMOR_L = 1027


def every_scale_list():
    """[(wavelet, scales)] of every list the device tests pass: the host check pins the plan's filters for all of them."""
    out = [(c.wavelet, tuple(c.scales)) for c in direct_cases()]
    for w in ("morl", "mexh", CMOR):
        out += [(w, spectral_scales(c)) for c in SPECTRAL_CASES]
    for w in ("morl", CMOR):
        out += [(w, MIXED_ORDER), (w, LAYOUT_SCALES), (w, (PAIR_S, 4 * PAIR_S))]
    out += [(w, OTHER_CMOR_SCALES) for w in OTHER_CMOR]
    out += [(w, (first_scale(w, 3),)) for w in ("morl", CMOR)]
    return sorted(set(out))
