"""Designs, inputs and references shared by the causal IIR tests (test_iir_ref.py on the CPU, test_gpu_iir.py on the GPU).

The reference of the GPU tests is scipy.signal.sosfilt in float64 on the float32 input.  The CPU tests hold that reference
itself to a long-double sample loop (sosfilt_longdouble), for every design and input the GPU tests use, so a bad reference
cannot pass for a good kernel.  Designs come straight from SciPy, not from the project's designers."""
from collections import namedtuple

import numpy as np
from scipy import signal

FS = 48000.0
GATE = 1e-5                    # the project's gate: |y - y_ref| <= GATE * max|y_ref| per row, and the same for zf


def eq_peak(freq, gain_db, q, fs=FS):
    """Audio EQ Cookbook peaking biquad, written out here independently of the package."""
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * np.pi * freq / fs
    al = np.sin(w0) / (2.0 * q)
    b = np.array([1.0 + al * A, -2.0 * np.cos(w0), 1.0 - al * A])
    a = np.array([1.0 + al / A, -2.0 * np.cos(w0), 1.0 - al / A])
    return np.concatenate([b / a[0], a / a[0]])


GRAPHIC_BANDS = [(31.25 * 2 ** i, -6.0 if i % 2 == 0 else 6.0) for i in range(10)]      # 31.25 Hz ... 16 kHz, -+6 dB
GRAPHIC_Q = 1.414


def _designs():
    d = {}
    d["preemph"] = np.array([[1.0, -0.97, 0.0, 1.0, 0.0, 0.0]])
    d["bessel4_lp"] = signal.bessel(4, 2000.0, "lowpass", fs=FS, output="sos")
    d["cheby1_5_lp"] = signal.cheby1(5, 1.0, 3000.0, "lowpass", fs=FS, output="sos")
    d["cheby2_6_hp"] = signal.cheby2(6, 40.0, 500.0, "highpass", fs=FS, output="sos")
    d["butter4_bp"] = signal.butter(4, (300.0, 3400.0), "bandpass", fs=FS, output="sos")
    d["ellip8_bp"] = signal.ellip(8, 0.5, 60.0, (300.0, 3400.0), "bandpass", fs=FS, output="sos")
    d["ellip10_bs"] = signal.ellip(10, 0.5, 60.0, (1000.0, 2000.0), "bandstop", fs=FS, output="sos")
    d["butter10_bp"] = signal.butter(10, (300.0, 3400.0), "bandpass", fs=FS, output="sos")
    d["eq10"] = np.stack([eq_peak(f, g, GRAPHIC_Q) for f, g in GRAPHIC_BANDS])
    long = np.concatenate([d["eq10"], d["ellip10_bs"], d["butter10_bp"], d["eq10"]])
    d["cat17"] = long[:17].copy()              # groups 8 | 8 | 1
    d["cat32"] = long[:32].copy()              # four full groups
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in d.items()}


DESIGNS = _designs()
SECTIONS = {k: v.shape[0] for k, v in DESIGNS.items()}
assert [SECTIONS[k] for k in DESIGNS] == [1, 2, 3, 3, 4, 8, 10, 10, 10, 17, 32]

ZI_MODES = ("none", "zero", "steady", "random")
Case = namedtuple("Case", "design B L zi")


def case_id(c):
    return f"{c.design}-B{c.B}-L{c.L}-{c.zi}"


def boundary_lengths(k):
    """The lengths at which the kernels take another path, from the library's own constants: one chunk, the scan's
    look-ahead, one wave of chunks and the longest row whose scan is one launch, each +- 1, in front of them the shortest rows."""
    chunk = k["chunk"]
    out = [1, 2, 3]
    for n in (chunk, k["scan_ahead"] * chunk, k["chunks_per_wave"] * chunk, k["two_level_chunks"] * chunk):
        out += [n - 1, n, n + 1]
    return out


def sweep_cases(k):
    """(design, B, L, zi) of the GPU sweep by group; the CPU test holds SciPy to long double on exactly these."""
    g = {"lengths": [], "designs": [], "batches": [], "long": []}
    for i, L in enumerate(boundary_lengths(k)):                       # every length, two designs, zi modes in turn
        g["lengths"].append(Case("butter4_bp", 3, L, ZI_MODES[i % 4]))
        g["lengths"].append(Case("eq10", 2, L, ZI_MODES[(i + 1) % 4]))
    for name in DESIGNS:                                              # every design, every zi mode, rows of 5+ odd chunks
        for zi in ZI_MODES:
            g["designs"].append(Case(name, 3, 5 * k["chunk"] + 3, zi))
    for B in (1, 3, 16, 17, 33):                                      # batches (odd length: rows off 16-byte boundaries)
        g["batches"].append(Case("ellip8_bp", B, 3 * k["chunk"] + 9, "random"))
        g["batches"].append(Case("cat17", B, k["chunk"] + 1, "random"))
    g["long"].append(Case("butter4_bp", 1, 1 << 20, "random"))        # one long row
    return g


def make_input(c, constant=False):
    """x [B, L] float32 and zi [B, S, 2] float64 (None for 'none') of a case: seeded by the case itself."""
    S = SECTIONS[c.design]
    rng = np.random.default_rng([c.B, c.L, S, ZI_MODES.index(c.zi)])
    x = rng.standard_normal((c.B, c.L)).astype(np.float32)
    if constant:
        x[:] = rng.uniform(0.5, 1.5, (c.B, 1)).astype(np.float32)
    if c.zi == "none":
        zi = None
    elif c.zi == "zero":
        zi = np.zeros((c.B, S, 2))
    elif c.zi == "steady":
        zi = signal.sosfilt_zi(DESIGNS[c.design])[None] * x[:, :1, None].astype(np.float64)
    else:
        zi = rng.normal(0.0, 0.3, (c.B, S, 2))
    return x, zi


def scipy_ref(sos, x, zi):
    """y [B, L], zf [B, S, 2] in float64: scipy.signal.sosfilt on the float32 input, row by row states."""
    B = x.shape[0]
    z = np.zeros((B, sos.shape[0], 2)) if zi is None else zi
    y, zf = signal.sosfilt(sos, x.astype(np.float64), axis=-1, zi=np.ascontiguousarray(np.moveaxis(z, 0, 1)))
    return y, np.moveaxis(zf, 1, 0)


def sosfilt_longdouble(sos, x, zi):
    """The direct-form-II-transposed cascade as a sample loop in long double, vectorised over rows only.
    x [R, n], zi [R, S, 2] -> y [R, n], zf [R, S, 2] (long double)."""
    ld = np.longdouble
    c = sos.astype(ld)
    c = c / c[:, 3:4]
    u = x.astype(ld)
    z = zi.astype(ld).copy()
    for s in range(c.shape[0]):
        b0, b1, b2, _, a1, a2 = c[s]
        z0, z1 = z[:, s, 0].copy(), z[:, s, 1].copy()
        out = np.empty_like(u)
        for n in range(u.shape[1]):
            xn = u[:, n]
            yn = b0 * xn + z0
            z0 = b1 * xn - a1 * yn + z1
            z1 = b2 * xn - a2 * yn
            out[:, n] = yn
        z[:, s, 0], z[:, s, 1] = z0, z1
        u = out
    return u, z


SEG = 2048


def reference_error(sos, x, zi):
    """How far SciPy's float64 sosfilt is from long double on x [B, L]: (worst |dy| / row peak, worst |dzf| / row's largest
    state).  Rows longer than SEG are checked segment by segment: SciPy's run is cut into blocks that carry its own
    state (bit-identical to the whole-row call), and every block is held to a long-double loop that starts from the
    state SciPy carried in, for the block's output AND for the state it hands on -- so every sample and every carried
    state of the long row is checked, at the cost of a short loop."""
    B, L = x.shape
    S = sos.shape[0]
    y_ref, zf_ref = scipy_ref(sos, x, zi)
    state = np.zeros((B, S, 2)) if zi is None else zi.copy()
    ey = ez = 0.0
    nseg = -(-L // SEG)
    Lp = nseg * SEG
    xp = np.zeros((B, Lp), dtype=np.float64)
    xp[:, :L] = x
    # SciPy's states at every segment start, by carrying them (and the outputs must equal the whole-row call's bits)
    starts = np.empty((B, nseg, S, 2))
    y_blocks = np.empty((B, Lp))
    for g in range(nseg):
        starts[:, g] = state
        n = min(SEG, L - g * SEG)
        yb, state = scipy_ref(sos, xp[:, g * SEG:g * SEG + n], state)
        y_blocks[:, g * SEG:g * SEG + n] = yb
    assert np.array_equal(y_blocks[:, :L], y_ref) and np.array_equal(state, zf_ref)
    ends = np.concatenate([starts[:, 1:], zf_ref[:, None]], axis=1)                    # the state each segment hands on
    last = L - (nseg - 1) * SEG
    ypk = np.max(np.abs(y_ref), axis=1)
    ypk[ypk == 0] = 1.0
    for sel, n in ((slice(0, nseg - 1), SEG), (slice(nseg - 1, nseg), last)):          # full segments, then the last one
        R = starts[:, sel].shape[1]
        if R == 0:
            continue
        seg0 = sel.start * SEG
        xs = xp[:, seg0:seg0 + R * SEG].reshape(B * R, SEG)[:, :n] if n == SEG else xp[:, seg0:seg0 + n].reshape(B, n)
        yl, zl = sosfilt_longdouble(sos, xs, starts[:, sel].reshape(B * R, S, 2))
        ys = y_ref[:, seg0:seg0 + R * n].reshape(B * R, n) if n == SEG else y_ref[:, seg0:seg0 + n]
        ey = max(ey, float(np.max(np.abs(yl - ys).max(axis=1) / np.repeat(ypk, R))))
        ze = ends[:, sel].reshape(B * R, 2 * S)
        zpk = np.maximum(np.max(np.abs(ze), axis=1), 1e-300)                            # each handed-on state's own peak
        ez = max(ez, float(np.max(np.abs(zl.reshape(B * R, 2 * S) - ze).max(axis=1) / zpk)))
    return ey, ez


# ---- the inputs of the GPU tests outside the sweep (the CPU test holds SciPy to long double on these too)
IMPULSE_L = 600
IMPULSE_AT = (0, 255, 256, IMPULSE_L - 1)
IMPULSE_DESIGNS = ("butter4_bp", "eq10", "cat17")
CONSTANT_DESIGNS = ("bessel4_lp", "cheby1_5_lp", "ellip10_bs", "eq10")       # designs with a gain at 0 Hz to settle on
STREAM_L = 20000
STREAM_CUTS = (1, 2, 257, 1000, 16385)
STREAM_DESIGNS = ("butter4_bp", "eq10")
STRIDED = Case("ellip8_bp", 3, 1500, "random")                               # rows 1540 floats apart, 7 floats in
ALIAS = Case("cat17", 3, 4099, "random")
E2E_DESIGNS = ("cheby1_5_lp", "ellip8_bp", "bessel4_lp")
E2E_L = 3000


def impulses():
    x = np.zeros((len(IMPULSE_AT), IMPULSE_L), dtype=np.float32)
    for r, n in enumerate(IMPULSE_AT):
        x[r, n] = 1.0
    return x


def constant_case(name):
    return Case(name, 3, 1283, "steady")


def stream_input(name):
    rng = np.random.default_rng([STREAM_L, SECTIONS[name]])
    return rng.standard_normal((1, STREAM_L)).astype(np.float32)


def e2e_input(name):
    rng = np.random.default_rng([E2E_L, SECTIONS[name], 7])
    return rng.standard_normal((2, E2E_L)).astype(np.float32)


def special_inputs():
    out = [(name, impulses(), None) for name in IMPULSE_DESIGNS]
    out += [(name,) + make_input(constant_case(name), constant=True) for name in CONSTANT_DESIGNS]
    out += [(name, stream_input(name), None) for name in STREAM_DESIGNS]
    out += [(c.design,) + make_input(c) for c in (STRIDED, ALIAS)]
    out += [(name, e2e_input(name), None) for name in E2E_DESIGNS]
    return out
