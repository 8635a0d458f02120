"""The launch-cap case table shared by the host checks (tests/test_launch_cap_cases.py: every case crosses the cap it names
at every CU count, under 1 GiB of device buffers) and the device tests (tests/test_gpu_launch_caps.py).  Plain data and
host arithmetic, no device.

A case is a function of the CU count `cu` and of the library's constants `k` (constants(): what ops.*_constants() and
ops.fx_add_noise_resident_max() expose).  The grid caps are the library's too (LAUNCH_NAMES: read at every use, never
assigned here); geometry that exists only in a .hip file is restated once below, each with the file that owns it.
`crosses(cu, k)` recomputes the launch plan from the kernel's own rule and is true only if the path the case names is
taken; the device tests assert it with the device's own CU count, so that a changed cap fails the test instead of
silently emptying it.  `bytes(cu, k)` is the sum of the device buffers the device test holds at once (inputs,
the result, the expected result gathered from the eight-row call, the workspace)."""
from collections import namedtuple

CU_COUNTS = (64, 104, 228, 256, 304, 320)
GIB = 1 << 30

# ---------------------------------------------------------------------------- caps restated from the kernels' files
FX_TREM_ROWS = 8               # effects.hip: rows a tremolo workgroup serves (TREM_ROWS); it has no row loop
FX_AN_SEG = 4096               # effects.hip: samples of a mix segment (AN_SEG = 256 threads x 16)
FX_ANG_BLOCKS = 2048           # effects.hip: workgroups of the generating mix's power pass over the batch
FX_SCALE_LANES = 64            # effects.hip: lanes of noise_gen_scale_kernel; more slices than that: runs per lane
LPC_ENV_THREADS = 256          # lpc.hip: threads of lpc_envelope_kernel, one element each per pass
PITCH_WAVES = 2                # pitch.hip: frames (waves) of a workgroup of pitch_frames_kernel

# ---------------------------------------------------------------------------- caps the library reports (ops.launch_constants)
LAUNCH_NAMES = {                       # the name the cases and the device tests use -> the library's figure
    "FX_MAX_ROWS_Y": "max_grid_y",                       # effects.hip: rows of the grid's y dimension (mix, compress, midside)
    "RNG_MAX_ROWS_Y": "max_grid_y",                      # rng.hip: the same of rng_normal_kernel, unpack_pairs_kernel
    "LOUD_MAX_GRID_Y": "max_grid_y",                     # loudness.hip: channel rows of one launch (clips_per_launch)
    "SOS_MAX_GRID_Y": "max_grid_y",                      # sosfilt_causal.hip: rows of one launch of launch_group
    "STACK_MAX_ROWS_Y": "max_grid_y",                    # dynamics.hip: output rows of stack_memory_kernel's grid
    "FX_NOISE_WGS_PER_CU": "noise_wgs_per_cu",           # effects.hip: the resident mixes and noise_gen_scale_kernel
    "LPC_WGS_PER_CU": "lpc_frames_wgs_per_cu",           # lpc.hip: lpc_frames_kernel
    "LPC_ENV_WGS_PER_CU": "lpc_envelope_wgs_per_cu",     # lpc.hip: lpc_envelope_kernel
    "PITCH_WGS_PER_CU": "pitch_frames_wgs_per_cu",       # pitch.hip: pitch_frames_kernel
}


def launch(k, name):
    """The cap `name` of LAUNCH_NAMES among the constants k."""
    return k["launch"][LAUNCH_NAMES[name]]


def __getattr__(name):
    """LC.FX_MAX_ROWS_Y and its like, for the device tests: the library's figure, read now."""
    if name in LAUNCH_NAMES:
        return launch(constants(), name)
    raise AttributeError(name)


ROWS8 = 8                      # distinct rows of every case: the large batch is rows8[arange(B) % 8]


def constants():
    """The library's own figures (no device is needed for them)."""
    from sygnals_amd import ops
    return {"resident_max": ops.fx_add_noise_resident_max(), "max_rows": ops.MAX_ROWS, "lpc": ops.lpc_constants(),
            "sosfilt": ops.sosfilt_constants(), "loudness": ops.loudness_constants(), "launch": ops.launch_constants()}


def ceil_div(a, b):
    return -(-a // b)


def noise_gen_slices(B, L):
    """(S, slen) of effects.hip's noise_gen_slices: the slices of a row in the generating mix's power pass."""
    s = min(ceil_div(FX_ANG_BLOCKS, B), ceil_div(L, FX_AN_SEG))
    slen = ceil_div(ceil_div(L, s), FX_AN_SEG) * FX_AN_SEG
    return ceil_div(L, slen), slen


Case = namedtuple("Case", "name where cap shape crosses bytes")
F32 = 4


def _rows_case(name, where, cap_text, cap, shape, nbytes, rows=lambda s: s["B"]):
    """A case whose path is `more rows than the grid's y dimension holds`."""
    return Case(name, where, cap_text, shape, lambda cu, k: rows(shape(cu, k)) > launch(k, cap), lambda cu, k: nbytes(shape(cu, k)))


def _cap8(cu, k):
    return launch(k, "FX_NOISE_WGS_PER_CU") * cu


# ---------------------------------------------------------------------------- effects.hip: pointwise
B_ROWS = 65537 + 3


def _mix_shape(cu, k):
    return dict(B=B_ROWS, Lx=3, L=5, Ly=7)


def _point_shape(cu, k):
    return dict(B=B_ROWS, L=5)


def _tremolo_shape(cu, k):
    return dict(B=FX_TREM_ROWS * launch(k, "FX_MAX_ROWS_Y"), L=3)


def _tremolo_crosses(cu, k):
    """The largest accepted batch: its grid is the cap itself, one row more is refused."""
    B = _tremolo_shape(cu, k)["B"]
    return ceil_div(B, FX_TREM_ROWS) == launch(k, "FX_MAX_ROWS_Y") and ceil_div(B + 1, FX_TREM_ROWS) > launch(k, "FX_MAX_ROWS_Y")


# ---------------------------------------------------------------------------- effects.hip: add_noise
def _noise_shape(L):
    return lambda cu, k: dict(B=_cap8(cu, k) + 5, L=L)


def _noise_resident_crosses(L):
    def crosses(cu, k):
        s = _noise_shape(L)(cu, k)
        return s["L"] <= k["resident_max"] and s["B"] > _cap8(cu, k)
    return crosses


GEN_FIRST_ROW = 11
GEN_HEAD = 2048                # rows of the first of the two smaller calls of the three-launch case


def _gen_long_shape(cu, k):
    """cap8 + 2048 rows where cap8 >= 2048 (256 CUs and up); below that 2048 + 2048, so that the second piece [2048, B) too
    has the 2048 rows from which noise_gen_slices gives one slice a row."""
    return dict(B=max(_cap8(cu, k), GEN_HEAD) + GEN_HEAD, L=k["resident_max"] + 1, head=GEN_HEAD)


def _gen_long_crosses(cu, k):
    """Three launches, the scale kernel's grid capped, and one slice a row in the whole call and in both of its pieces (so
    that the sums of the three calls have one order)."""
    s = _gen_long_shape(cu, k)
    one = all(noise_gen_slices(b, s["L"])[0] == 1 for b in (s["B"], s["head"], s["B"] - s["head"]))
    return s["L"] > k["resident_max"] and s["B"] > _cap8(cu, k) and one


GEN_SLICE_CASES = ((1, 64 * FX_AN_SEG + 1, 2), (3, 64 * FX_AN_SEG + 1, 2), (1, 130 * FX_AN_SEG + 5, 3),
                   (3, 130 * FX_AN_SEG + 5, 3))                       # (B, L, slices a lane)


def _gen_slices_shape(B, L, per):
    return lambda cu, k: dict(B=B, L=L, per=per)


def _gen_slices_crosses(B, L, per):
    def crosses(cu, k):
        S = noise_gen_slices(B, L)[0]
        got = ceil_div(S, FX_SCALE_LANES)
        empty = FX_SCALE_LANES * got - S >= got                       # at least one lane past the last slice
        return L > k["resident_max"] and S > FX_SCALE_LANES and got == per and (per < 3 or empty)
    return crosses


# ---------------------------------------------------------------------------- rng.hip
RANDN_B, RANDN_FIRST_ROW = 65540, 3
COLORED_B, COLORED_L, COLORED_FIRST_ROW = 65539, 4, 7


def colored_pairs(first_row, B):
    """(first pair, pairs) that hold the rows first_row .. first_row + B - 1 (pairs by absolute row index)."""
    p0, p1 = first_row >> 1, (first_row + B - 1) >> 1
    return p0, p1 - p0 + 1


def colored_piece_rows(L, k):
    """Rows of the largest piece ops.colored_noise hands to the pair kernels: it cuts a batch at MAX_ROWS div 2 pairs, so
    through ops.colored_noise no launch ever holds more rows than the grid (the device test drives the entries directly)."""
    M = 1 << max(1, (int(L) - 1).bit_length())
    return 2 * max(1, min(k["max_rows"] // 2, (1 << 26) // M))


def _colored_crosses(cu, k):
    P = colored_pairs(COLORED_FIRST_ROW, COLORED_B)[1]
    return 2 * P > launch(k, "RNG_MAX_ROWS_Y") and COLORED_B > launch(k, "RNG_MAX_ROWS_Y") and COLORED_FIRST_ROW % 2 == 1


# ---------------------------------------------------------------------------- loudness.hip
def _loud_shape(C, L, fs):
    return lambda cu, k: dict(B=launch(k, "LOUD_MAX_GRID_Y") // C + 2, C=C, L=L, fs=fs)


def _loud_crosses(C, L, fs, segments=False):
    def crosses(cu, k):
        s = _loud_shape(C, L, fs)(cu, k)
        per = min(s["B"], launch(k, "LOUD_MAX_GRID_Y") // C)    # clips_per_launch
        ok = s["B"] > per and s["B"] - per < per                      # a second, shorter piece
        if segments:
            n_seg = 10 * L // fs                                        # whole segments; they end at sample n_seg fs div 10
            ok = ok and n_seg == 2 and ceil_div(n_seg * fs // 10, k["loudness"]["chunk"]) == 7
        return ok
    return crosses


def _loud_bytes(C, L, fs, segments=False):
    def nbytes(cu, k):
        s = _loud_shape(C, L, fs)(cu, k)
        n = (1 if segments else 3) * s["B"] * C * (L + 3) * F32        # the clips; gain_rows: its result and the expected one
        if segments:
            rows, nch = min(s["B"], launch(k, "LOUD_MAX_GRID_Y") // C) * C, ceil_div(L, k["loudness"]["chunk"])
            n += rows * (nch * 10 + 2 * nch * 4) * 8 + 2 * s["B"] * C * (10 * L // fs) * 8
        return n + 3 * s["B"] * 8
    return nbytes


# ---------------------------------------------------------------------------- sosfilt_causal.hip
SOS_L = 257


def _sos_shape(sections):
    return lambda cu, k: dict(B=B_ROWS, L=SOS_L, sections=sections)


def _sos_crosses(sections):
    def crosses(cu, k):
        s = _sos_shape(sections)(cu, k)
        scan = ceil_div(s["L"], k["sosfilt"]["chunk"]) == 2          # two chunks: the scan runs, the workspace is used
        groups = ceil_div(sections, k["sosfilt"]["group_sections"])
        return s["B"] > launch(k, "SOS_MAX_GRID_Y") and scan and groups == (2 if sections > 8 else 1)
    return crosses


def _sos_bytes(sections):
    def nbytes(cu, k):
        s = _sos_shape(sections)(cu, k)
        nch = ceil_div(s["L"], k["sosfilt"]["chunk"])
        S = min(sections, k["sosfilt"]["group_sections"])
        work = 2 * min(s["B"], launch(k, "SOS_MAX_GRID_Y")) * (nch + ceil_div(nch, k["sosfilt"]["scan_ahead"])) * 2 * S * 8
        return 3 * s["B"] * s["L"] * F32 + 3 * s["B"] * sections * 2 * 8 + work
    return nbytes


# ---------------------------------------------------------------------------- dynamics.hip
def _stack_shape(cu, k):
    return dict(B=1, K=8200, n_steps=8, delay=1, T=5)


# ---------------------------------------------------------------------------- lpc.hip
def _lpc_clip_shape(hop, frames):
    return lambda cu, k: dict(B=launch(k, "LPC_WGS_PER_CU") * cu + 5, N=64, order=2, hop=hop, center=False, L=64 + (frames - 1) * hop, T=frames)


def _lpc_clip_crosses(hop, frames, staged):
    def crosses(cu, k):
        s = _lpc_clip_shape(hop, frames)(cu, k)
        tile = k["lpc"]["tile_frames"]
        span = (tile - 1) * s["hop"] + s["N"]
        T = 1 + (s["L"] - s["N"]) // s["hop"]
        tiles = s["B"] * ceil_div(T, tile)
        return T == frames and ceil_div(T, tile) == 1 and (span <= k["lpc"]["span_max"]) == staged and tiles > launch(k, "LPC_WGS_PER_CU") * cu
    return crosses


def _lpc_long_shape(cu, k):
    L = 128 * cu + 300
    return dict(B=1, N=3, order=1, hop=1, center=True, L=L, T=1 + (L + 2 * (3 // 2) - 3) // 1)


def _lpc_long_crosses(cu, k):
    s = _lpc_long_shape(cu, k)
    tile = k["lpc"]["tile_frames"]
    tiles = ceil_div(s["T"], tile)
    return tile == 16 and tiles > launch(k, "LPC_WGS_PER_CU") * cu + 1 and s["T"] % tile != 0


def lpc_long_tiles(cu, k):
    """First frames of the three tiles the device test checks: the first, one a workgroup takes on its second turn, the
    last (partial) one."""
    s = _lpc_long_shape(cu, k)
    tile = k["lpc"]["tile_frames"]
    return 0, (launch(k, "LPC_WGS_PER_CU") * cu + 1) * tile, (ceil_div(s["T"], tile) - 1) * tile


ENV_NFFT = 4096


def _env_shape(order):
    return lambda cu, k: dict(B=1, order=order, n_fft=ENV_NFFT, T=cu * launch(k, "LPC_ENV_WGS_PER_CU") * LPC_ENV_THREADS // (ENV_NFFT // 2 + 1) + 3)


def _env_crosses(order):
    def crosses(cu, k):
        s = _env_shape(order)(cu, k)
        total = s["B"] * (s["n_fft"] // 2 + 1) * s["T"]
        return ceil_div(total, LPC_ENV_THREADS) > launch(k, "LPC_ENV_WGS_PER_CU") * cu
    return crosses


# ---------------------------------------------------------------------------- pitch.hip
PITCH_SR, PITCH_WIN, PITCH_HOP, PITCH_NF = 22050, 1024, 512, 2048


def _pitch_shape(cu, k):
    return dict(B=8 * cu + 8, L=PITCH_NF + 3 * PITCH_HOP, T=4)


def _pitch_crosses(cu, k):
    s = _pitch_shape(cu, k)
    T = 1 + (s["L"] - PITCH_NF) // PITCH_HOP
    return T == s["T"] and ceil_div(s["B"] * T, PITCH_WAVES) > launch(k, "PITCH_WGS_PER_CU") * cu


def _pitch_bytes(cu, k):
    from sygnals_amd import _pitch as P
    s = _pitch_shape(cu, k)
    min_p, max_p = P.periods(PITCH_SR, P.C2, P.C7, PITCH_NF, PITCH_WIN)
    n_lag = max_p - min_p + 1
    frames = s["B"] * s["T"]
    per_frame = 2 * P.cand_stride(n_lag) * 4 + 3 * 4 + n_lag * 4      # candidates (bin, prob), f0 / count / vp, CMNDF
    return s["B"] * s["L"] * F32 + 2 * 2 * frames * per_frame        # both modes, the result and the expected one


def cases():
    out = [
        _rows_case("fx_mix", "effects.hip", "mix_kernel: r += gridDim.y past 65535 rows", "FX_MAX_ROWS_Y", _mix_shape,
                   lambda s: s["B"] * (s["Lx"] + s["Ly"] + 2 * s["L"] + 3) * F32),
        _rows_case("fx_compress", "effects.hip", "compress_kernel: r += gridDim.y past 65535 rows", "FX_MAX_ROWS_Y", _point_shape,
                   lambda s: 3 * s["B"] * (s["L"] + 3) * F32),
        _rows_case("fx_midside", "effects.hip", "midside_kernel: r += gridDim.y past 65535 stereo pairs", "FX_MAX_ROWS_Y", _point_shape,
                   lambda s: 3 * 2 * s["B"] * s["L"] * F32),
        Case("fx_tremolo", "effects.hip", "syg_fx_tremolo_f32: at most 8 x 65535 rows", _tremolo_shape, _tremolo_crosses,
             lambda cu, k: 3 * (_tremolo_shape(cu, k)["B"] + 1) * (_tremolo_shape(cu, k)["L"] + 3) * F32),
    ]
    for L in (7, 1000):
        nb = lambda cu, k, L=L: _noise_shape(L)(cu, k)["B"] * (4 * (L + 3) * F32 + 8)
        out.append(Case(f"fx_add_noise-L{L}", "effects.hip", "noise_resident_kernel: row loop past cu x 8 workgroups",
                        _noise_shape(L), _noise_resident_crosses(L), nb))
        out.append(Case(f"fx_add_noise_gen-L{L}", "effects.hip", "noise_gen_resident_kernel: row loop past cu x 8 workgroups",
                        _noise_shape(L), _noise_resident_crosses(L), lambda cu, k, nb=nb: 2 * nb(cu, k)))
    out.append(Case("fx_add_noise_gen-long", "effects.hip", "noise_gen_scale_kernel: row loop past cu x 8 workgroups",
                    _gen_long_shape, _gen_long_crosses,
                    lambda cu, k: _gen_long_shape(cu, k)["B"] * (3 * _gen_long_shape(cu, k)["L"] * F32 + 8 + 32)))
    for B, L, per in GEN_SLICE_CASES:
        out.append(Case(f"fx_add_noise_gen-B{B}-L{L}", "effects.hip", f"noise_gen_scale_kernel: {per} slices a lane",
                        _gen_slices_shape(B, L, per), _gen_slices_crosses(B, L, per),
                        lambda cu, k, B=B, L=L: B * (5 * L * F32 + 8 + 16 * (noise_gen_slices(B, L)[0] + 1))))
    for L in (5, 1025):
        out.append(_rows_case(f"randn-L{L}", "rng.hip", "rng_normal_kernel: b += gridDim.y past 65535 rows", "RNG_MAX_ROWS_Y",
                              lambda cu, k, L=L: dict(B=RANDN_B, L=L, first_row=RANDN_FIRST_ROW), lambda s: 2 * s["B"] * s["L"] * F32))
    out.append(Case("colored_noise", "rng.hip", "rng_normal_kernel (pair rows), unpack_pairs_kernel: b += gridDim.y past 65535 rows",
                    lambda cu, k: dict(B=COLORED_B, L=COLORED_L, first_row=COLORED_FIRST_ROW), _colored_crosses,
                    lambda cu, k: 3 * (COLORED_B + 1) * COLORED_L * 2 * F32 + 3 * COLORED_B * COLORED_L * F32))
    for name, fs in (("true_peak", 48000), ("true_peak-sample", 192000), ("gain_rows", 48000)):
        out.append(Case(name, "loudness.hip", f"syg_{name.split('-')[0]}_f32: the clips_per_launch split at 65535 div C clips",
                        _loud_shape(3, 5, fs), _loud_crosses(3, 5, fs), _loud_bytes(3, 5, fs)))
    for C in (3, 2):
        out.append(Case(f"loudness_segments-C{C}", "loudness.hip", "syg_loudness_segments_f32: the clips_per_launch split at 65535 div C clips",
                        _loud_shape(C, 1601, 8000), _loud_crosses(C, 1601, 8000, True), _loud_bytes(C, 1601, 8000, True)))
    for sections in (2, 10):
        out.append(Case(f"sosfilt-S{sections}", "sosfilt_causal.hip", "launch_group: split at 65535 rows", _sos_shape(sections),
                        _sos_crosses(sections), _sos_bytes(sections)))
    out.append(_rows_case("stack_memory", "dynamics.hip", "stack_memory_kernel: r += gridDim.y past 65535 output rows", "STACK_MAX_ROWS_Y",
                          _stack_shape, lambda s: (s["B"] * s["K"] * s["T"] + 2 * s["B"] * s["K"] * s["n_steps"] * s["T"]) * F32,
                          rows=lambda s: s["B"] * s["K"] * s["n_steps"]))
    lpc_bytes = lambda shape: (lambda cu, k: shape(cu, k)["B"] * (shape(cu, k)["L"] + 2 * 3 * (2 * shape(cu, k)["order"] + 2) * shape(cu, k)["T"]) * F32)
    out.append(Case("lpc_frames-staged", "lpc.hip", "lpc_frames_kernel: tile loop past cu x 8 workgroups, span staged",
                    _lpc_clip_shape(64, 5), _lpc_clip_crosses(64, 5, True), lpc_bytes(_lpc_clip_shape(64, 5))))
    out.append(Case("lpc_frames-unstaged", "lpc.hip", "lpc_frames_kernel: tile loop past cu x 8 workgroups, span not staged",
                    _lpc_clip_shape(816, 3), _lpc_clip_crosses(816, 3, False), lpc_bytes(_lpc_clip_shape(816, 3))))
    out.append(Case("lpc_frames-long", "lpc.hip", "lpc_frames_kernel: tile loop past cu x 8 workgroups over one clip",
                    _lpc_long_shape, _lpc_long_crosses, lpc_bytes(_lpc_long_shape)))
    for order in (1, 64):
        out.append(Case(f"lpc_envelope-p{order}", "lpc.hip", "lpc_envelope_kernel: grid stride past cu x 32 x 256 elements",
                        _env_shape(order), _env_crosses(order),
                        lambda cu, k, order=order: _env_shape(order)(cu, k)["T"] * ((order + 2) + 4 * (ENV_NFFT // 2 + 1)) * F32))
    out.append(Case("pitch_frames", "pitch.hip", "pitch_frames_kernel: frame loop past cu x 16 workgroups of two waves",
                    _pitch_shape, _pitch_crosses, _pitch_bytes))
    return out


def case(name):
    """The case of this name."""
    return {c.name: c for c in cases()}[name]


def case_id(c):
    return c.name
