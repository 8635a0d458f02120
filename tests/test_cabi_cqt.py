"""The six entry points of the constant-Q transform (cqt.hip, cqt_fused.hip) reject bad arguments before any device work:
every case below is an otherwise valid call with ONE thing wrong, and pins the return code, the prefix that names the entry
point and a distinguishing part of syg_last_error().  No GPU is needed: nothing here reaches a device call."""
import ctypes as C
import os

import pytest

INVALID = -1
P, PMIS = "<buffer>", "<buffer + 4 bytes>"
HULL, ROW0, YS, LDS = "<hull>", "<row0>", "<level pointers>", "<level strides>"

# 24000 samples at hop 64: 1 + 24000 // 64 = 376 centred frames; rows 72 .. 83 of an 84-row transform
OCT = [("y", P), ("B", 2), ("L", 24000), ("ldy", 24000), ("n_fft", 256), ("hop", 64), ("T", 376)]
OUT = [("out", P), ("out_bstride", 84 * 376), ("row0", 72), ("stream", None)]
DEC = [("x", P), ("B", 2), ("L", 24000), ("ldx", 24000), ("taps", P), ("ntaps", 41), ("scale", 1.4142135)]

# name -> (prefix of its messages, arguments in ABI order with valid values)
ENTRIES = {
    "syg_cqt_octave_f32": ("cqt_octave: ", OCT + [("twiddle", P), ("basis", P), ("n_filt", 12), ("hull_host", HULL)] + OUT),
    "syg_cqt_octave_gemm_f32": ("cqt_octave_gemm: ", OCT + [("gpacked", P), ("n_filt", 12)] + OUT),
    "syg_cqt_octave_bf16x3_f32": ("cqt_octave_bf16x3: ", OCT + [("gsplit", P), ("n_filt", 12)] + OUT),
    # 48000 samples: every one of the seven octaves has 1 + (48000 >> (o + 1)) // (256 >> o) = 94 frames
    "syg_cqt_fused_f32": ("cqt_fused: ", [("y", P), ("B", 2), ("L", 48000), ("ldy", 48000), ("taps", P), ("ntaps", 41),
                                         ("scale", 1.4142135), ("gsplit", P), ("n_filt", 12), ("n_oct", 7), ("row0_host", ROW0),
                                         ("T", 94), ("out", P), ("out_bstride", 84 * 94), ("stream", None)]),
    "syg_decimate2_f32": ("decimate2: ", DEC + [("y", P), ("ldy", 12000), ("stream", None)]),
    "syg_decimate2_chain_f32": ("decimate2_chain: ", DEC + [("levels", 3), ("y", YS), ("ldy", LDS), ("stream", None)]),
}
ALL = sorted(ENTRIES)
OCTAVE = [n for n in ALL if "octave" in n]
FRAMED = OCTAVE + ["syg_cqt_fused_f32"]
MAXFILT = {"syg_cqt_octave_f32": 24, "syg_cqt_octave_gemm_f32": 64, "syg_cqt_octave_bf16x3_f32": 16, "syg_cqt_fused_f32": 16}
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def hull(k0=10, length=20, n=12):
    """HOST int32 [2 n]: first non-zero bin and run length of every filter's row (129 bins at frame length 256)."""
    return (C.c_int32 * (2 * n))(*([k0] * n + [length] * n))


def row0s(first=72, step=12, n=7):
    return (C.c_int32 * n)(*[first - step * o for o in range(n)])


class Caller:
    def __init__(self, h):
        self.h = h
        raw = (C.c_float * 72)()                                 # a 64-float dummy buffer, 16-byte aligned
        self.keep = [raw]
        self.p = (C.addressof(raw) + 15) // 16 * 16

    def __call__(self, name, **wrong):
        """Call `name` with its valid arguments and `wrong` on top; returns (rc, last error)."""
        names = [n for n, _ in ENTRIES[name][1]]
        assert set(wrong) <= set(names), (name, wrong)
        std = {P: lambda: self.p, PMIS: lambda: self.p + 4, HULL: hull, ROW0: row0s,
               YS: lambda: (C.c_void_p * 4)(self.p, self.p, self.p, self.p),
               LDS: lambda: (C.c_int64 * 4)(12000, 6000, 3000, 1500)}
        vals = []
        for n, v in ENTRIES[name][1]:
            v = wrong.get(n, v)
            if isinstance(v, str):
                v = std[v]()
            if isinstance(v, C.Array):
                self.keep.append(v)
                v = C.addressof(v)
            vals.append(v)
        rc = getattr(self.h, name)(*vals)
        return rc, self.h.syg_last_error().decode()


@pytest.fixture()
def call(h):
    return Caller(h)


def rejected(res, prefix, part, rc=INVALID):
    got, msg = res
    assert got == rc, (got, msg)
    assert msg.startswith(prefix) and part in msg, msg


def test_all_six_are_bound(h):
    from sygnals_amd import _lib
    assert len(ALL) == 6
    for name in ALL:
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(ENTRIES[name][1]), name


@pytest.mark.parametrize("name", ALL)
def test_null_pointers(call, name):
    own, args = ENTRIES[name]
    optional = {"stream", "hull_host"}                            # (no hull: the rows are dense)
    for ptr in [n for n, v in args if (isinstance(v, str) or v is None) and n not in optional]:
        rejected(call(name, **{ptr: None}), own, "null pointer argument")


@pytest.mark.parametrize("name", FRAMED)
def test_clip_and_frame_count(call, name):
    own, args = ENTRIES[name]
    a = dict(args)
    bad = "bad B/L/ldy" + ("" if name == "syg_cqt_fused_f32" else "/hop")
    rejected(call(name, B=0), own, bad)
    rejected(call(name, L=0, ldy=0), own, bad)
    rejected(call(name, ldy=a["L"] - 1), own, bad)
    if name in OCTAVE:
        rejected(call(name, B=65536), own, bad)
        rejected(call(name, hop=0), own, bad)
        rejected(call(name, hop=-64), own, bad)
    # T beyond the centred frame count (and none at all)
    for T in (a["T"] + 1, 0, -1):
        rejected(call(name, T=T, out_bstride=84 * max(T, 1)), own, "exceeds the centred frame count %d" % a["T"])


def test_one_launch_frame_count_is_the_smallest_over_the_octaves(call):
    # 49150 samples: 24575 after the early decimation, 1 + 24575 // 256 = 96 frames in octave 0; the next level rounds up to
    # 12288 samples = 1 + 12288 // 128 = 97 frames, which the transform as a whole does not have
    rejected(call("syg_cqt_fused_f32", L=49150, ldy=49150, T=97, out_bstride=84 * 97), "cqt_fused: ",
             "T=97 exceeds the centred frame count 96")


@pytest.mark.parametrize("name,taken", [("syg_cqt_octave_f32", (8, 32, 64, 128, 256, 512, 1024)),
                                        ("syg_cqt_octave_gemm_f32", (128, 256, 512)),
                                        ("syg_cqt_octave_bf16x3_f32", (128, 256))])
def test_frame_lengths_an_entry_does_not_take(call, name, taken):
    own, args = ENTRIES[name]
    for n_fft in (0, 4, 96, 192, 2048, 4096, 8192, -256) + tuple(n for n in (64, 512, 1024) if n not in taken):
        rejected(call(name, n_fft=n_fft), own, "n_fft must be")
    # (a frame length it takes fails at the NEXT wrong thing)
    for n_fft in taken:
        rejected(call(name, n_fft=n_fft, n_filt=0), own, "n_filt must be in [1, %d]" % MAXFILT[name])


@pytest.mark.parametrize("name", FRAMED)
def test_filter_count(call, name):
    own, args = ENTRIES[name]
    for n_filt in (0, -1, MAXFILT[name] + 1):
        rejected(call(name, n_filt=n_filt), own, "n_filt")
    # the limit itself passes this check: rows 72 .. 72 + limit - 1 no longer fit the 84-row output
    rejected(call(name, n_filt=MAXFILT[name], **({"hull_host": hull(n=24)} if name == "syg_cqt_octave_f32" else {})), own,
             "output rows out of range")


@pytest.mark.parametrize("name", FRAMED)
def test_output_rows(call, name):
    own, args = ENTRIES[name]
    a = dict(args)
    rejected(call(name, out_bstride=a["out_bstride"] - 1), own, "output rows out of range")
    rejected(call(name, out_bstride=0), own, "output rows out of range")
    if name in OCTAVE:
        rejected(call(name, row0=-1), own, "output rows out of range")
        rejected(call(name, row0=73), own, "output rows out of range")
        rejected(call(name, row0=INT_MAX), own, "output rows out of range")      # (row0 + n_filt must not wrap)
        rejected(call(name, row0=INT_MAX - 11), own, "output rows out of range")
    else:
        rejected(call(name, row0_host=row0s(first=71)), own, "output rows out of range")          # the last octave: row -1
        rejected(call(name, row0_host=row0s(first=73)), own, "output rows out of range")
        rejected(call(name, row0_host=row0s(first=INT_MAX, step=0)), own, "output rows out of range")
        # only the first n_oct entries are read
        rejected(call(name, n_oct=6, row0_host=row0s(first=72, step=12, n=6), out_bstride=0), own, "output rows out of range")


@pytest.mark.parametrize("name", ["syg_cqt_octave_bf16x3_f32", "syg_cqt_fused_f32"])
def test_operand_table_alignment(call, name):
    rejected(call(name, gsplit=PMIS), ENTRIES[name][0], "operand table must be 16-byte aligned")


def test_hull_that_leaves_the_spectrum(call):
    name, own = "syg_cqt_octave_f32", "cqt_octave: "
    rejected(call(name, hull_host=hull(k0=110, length=20)), own, "non-zero run of filter 0 out of range (k0=110 len=20)")
    rejected(call(name, hull_host=hull(k0=-1)), own, "non-zero run of filter 0 out of range")
    rejected(call(name, hull_host=hull(length=-1)), own, "non-zero run of filter 0 out of range")
    rejected(call(name, hull_host=hull(k0=130, length=0)), own, "non-zero run of filter 0 out of range")
    rejected(call(name, hull_host=hull(k0=INT_MAX, length=INT_MAX)), own, "non-zero run of filter 0 out of range")
    a = hull()
    a[5], a[12 + 5] = 100, 30                                      # 100 + 30 > 129 bins
    rejected(call(name, hull_host=a), own, "non-zero run of filter 5 out of range (k0=100 len=30)")
    # at another frame length the spectrum is shorter: 65 bins at 128
    rejected(call(name, n_fft=128, hull_host=hull(k0=50, length=20)), own, "non-zero run of filter 0 out of range")


def test_one_launch_decimator_and_octave_count(call):
    name, own = "syg_cqt_fused_f32", "cqt_fused: "
    for ntaps in (0, 39, 40, 43, 1025):
        rejected(call(name, ntaps=ntaps), own, "the decimator must have 41 taps (got %d)" % ntaps)
    for n_oct in (0, 8, -1):
        rejected(call(name, n_oct=n_oct), own, "n_oct must be in [1, 7]")


@pytest.mark.parametrize("name", ["syg_decimate2_f32", "syg_decimate2_chain_f32"])
def test_decimator_checks(call, name):
    own, args = ENTRIES[name]
    rejected(call(name, B=0), own, "bad B/L/ldx")
    rejected(call(name, B=65536), own, "bad B/L/ldx")
    rejected(call(name, L=0, ldx=0), own, "bad B/L/ldx")
    rejected(call(name, ldx=23999), own, "bad B/L/ldx")
    for ntaps in (0, -1, 40, 1027):
        rejected(call(name, ntaps=ntaps), own, "ntaps must be odd and <= 1025")


def test_decimate2_output_stride(call):
    rejected(call("syg_decimate2_f32", ldy=11999), "decimate2: ", "ldy too small")
    rejected(call("syg_decimate2_f32", L=24001, ldx=24001), "decimate2: ", "ldy too small")       # ceil(24001 / 2) = 12001


def test_decimate2_chain_levels_and_buffers(call):
    name, own = "syg_decimate2_chain_f32", "decimate2_chain: "
    for levels in (0, 5, -1):
        rejected(call(name, levels=levels), own, "levels must be 1 ... 4 (got %d)" % levels)
    p = call.p
    rejected(call(name, y=(C.c_void_p * 3)(p, p, None)), own, "the last level needs an output buffer")
    rejected(call(name, ldy=(C.c_int64 * 3)(12000, 5999, 3000)), own, "ldy[1] too small")
    rejected(call(name, ldy=(C.c_int64 * 3)(11999, 6000, 3000)), own, "ldy[0] too small")
    # a level that is not wanted needs no stride ...
    rejected(call(name, y=(C.c_void_p * 3)(None, p, p), ldy=(C.c_int64 * 3)(0, 6000, 2999)), own, "ldy[2] too small")
    # ... except where every level is written: another filter length goes level by level
    rejected(call(name, ntaps=21, y=(C.c_void_p * 3)(None, p, p)), own, "with 21 taps every level needs an output buffer")
