"""The fifteen entry points of the fused STFT front ends (stft_mel.hip, stft_mel_pow2.hip, stft_mel_w1024_seg.hip,
stft_mel_w4096.hip, stft_mel_wseg_small.hip) reject bad arguments before any device work: every case below is an otherwise
valid call with ONE thing wrong, and pins the return code, the prefix that names the entry point (the 2048 file reports its
clip checks as "stft2048") and a distinguishing part of syg_last_error().  The answers of the 2048 file's two `fits` functions
are pinned at the end.  No GPU is needed: nothing here reaches a device call."""
import ctypes as C
import os

import pytest

from sygnals_amd._tables import MAX_BANDS

INVALID = -1
P, PMIS, CP, PLAN = "<buffer>", "<buffer + 4 bytes>", "<contrast plan>", "<mel plan>"

CLIP = [("y", P), ("B", 2), ("L", 48000), ("ldy", 48000), ("hop", 512), ("center", 1), ("T", 94), ("window", P), ("twiddle", P)]
CLIPN = CLIP[:4] + [("n_fft", 512)] + CLIP[4:]
STATS = [("sr", 48000.0), ("roll", 0.85), ("bw_p", 2.0), ("smask", 31), ("stats_out", P), ("cplan", CP), ("contrast_out", P)]
MFCC = [("dct", P), ("n_mfcc", 13), ("lifter", None), ("amin", 1e-10), ("top_db", 80.0), ("ref_is_max", 1), ("ref_value", 1.0)]
STREAM = [("stream", None)]


def SEG(words):
    return [("segtab", P), ("n_segtab", words), ("n_mels", 40)]


# name -> (prefix of its own messages, prefix of its clip checks, arguments in ABI order with valid values)
ENTRIES = {
    "syg_stft2048_mel_f32": ("stft2048_mel: ", "stft2048: ", CLIP + [("wpacked", P), ("plan", PLAN), ("n_mels", 40), ("mel_out", P)]
                             + STATS + STREAM),
    "syg_stft2048_mfcc_f32": ("stft2048_mfcc: ", "stft2048: ", CLIP + [("wpacked", P), ("plan", PLAN), ("n_mels", 40)] + MFCC
                              + [("mel_out", None), ("mfcc_out", P)] + STREAM),
    "syg_stft2048_mfcc_tri_f32": ("stft2048_mfcc_tri: ", "stft2048: ", CLIP + SEG(1024) + MFCC + [("mfcc_out", P)] + STREAM),
    "syg_stft2048_features_tri_f32": ("stft2048_features_tri: ", "stft2048: ", CLIP + SEG(1024) + MFCC + STATS
                                      + [("mfcc_out", P), ("mfcc_rows", 13)] + STREAM),
    "syg_stft2048_mel_tri_f32": ("stft2048_mel_tri: ", "stft2048: ", CLIP + SEG(2048) + [("mel_out", P)] + STATS + [("waves", 16)]
                                 + STREAM),
    "syg_stft2048_stats_f32": ("stft2048_stats: ", "stft2048: ", CLIP + STATS + STREAM),
    "syg_stft2048_c2c_f32": ("stft2048_c2c: ", "stft2048: ", CLIP + [("out", P)] + STREAM),
    "syg_stft_mel_pow2_f32": ("stft_mel_pow2: ", "stft_mel_pow2: ", CLIPN + [("basis_p", P), ("Fp", 272), ("n_mels", 40), ("power", 2),
                                                                           ("mel_out", P)] + STREAM),
    "syg_stft_mfcc_pow2_f32": ("stft_mfcc_pow2: ", "stft_mfcc_pow2: ", CLIPN + [("basis_p", P), ("Fp", 272), ("n_mels", 40)] + MFCC
                               + [("mel_out", None), ("mfcc_out", P)] + STREAM),
    "syg_stft_mel_w1024_seg_f32": ("stft_mel_w1024_seg: ", "stft_mel_w1024_seg: ", CLIP + SEG(2048) + [("mel_out", P)] + STREAM),
    "syg_stft_rows_w1024_f32": ("stft_rows_w1024: ", "stft_rows_w1024: ", CLIP + SEG(2048) + [("mel_out", P)] + STATS + STREAM),
    "syg_stft_mel_w4096_f32": ("stft_mel_w4096: ", "stft_mel_w4096: ", CLIP + SEG(2048) + [("mel_out", P)] + STREAM),
    "syg_stft_rows_w4096_f32": ("stft_rows_w4096: ", "stft_rows_w4096: ", CLIP + SEG(2048) + [("mel_out", P)] + STATS + STREAM),
    "syg_stft_mel_wseg_small_f32": ("stft_mel_wseg_small: ", "stft_mel_wseg_small: ", CLIPN + SEG(2048) + [("mel_out", P)] + STREAM),
    "syg_stft_rows_wsmall_f32": ("stft_rows_wsmall: ", "stft_rows_wsmall: ", CLIPN + STATS + STREAM),
}
ALL = sorted(ENTRIES)
SEGMENT = {  # entries that read a piece table -> the largest n_mels they take
    "syg_stft2048_mfcc_tri_f32": 127, "syg_stft2048_features_tri_f32": 127, "syg_stft2048_mel_tri_f32": 255,
    "syg_stft_mel_w1024_seg_f32": 255, "syg_stft_rows_w1024_f32": 255, "syg_stft_mel_w4096_f32": 255,
    "syg_stft_rows_w4096_f32": 255, "syg_stft_mel_wseg_small_f32": 48,
}
ROWS = {  # entries with statistics / contrast rows -> (the rows are optional, number of bins of a row)
    "syg_stft2048_mel_f32": (True, 1025), "syg_stft2048_features_tri_f32": (False, 1025), "syg_stft2048_mel_tri_f32": (True, 1025),
    "syg_stft2048_stats_f32": (False, 1025), "syg_stft_rows_w1024_f32": (False, 513), "syg_stft_rows_w4096_f32": (False, 2049),
    "syg_stft_rows_wsmall_f32": (False, 257),
}


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def cplan(n_rows=2, lo=(0, 100), hi=(100, 120), k=(2, 2)):
    """HOST int32 [1 + 3 * MAX_BANDS] {n_rows, lo[], hi[], k[]} (valid for every frame length here: 129 bins and more)."""
    a = (C.c_int32 * (1 + 3 * MAX_BANDS))()
    a[0] = n_rows
    for r in range(len(lo)):
        a[1 + r], a[1 + MAX_BANDS + r], a[1 + 2 * MAX_BANDS + r] = lo[r], hi[r], k[r]
    return a


class Caller:
    def __init__(self, h):
        self.h = h
        raw = (C.c_float * 72)()                                 # a 64-float dummy buffer, 16-byte aligned
        self.keep = [raw, cplan(), (C.c_int32 * 5)(2, 16, 28, 10, 16 * 28 * 64)]      # mel plan: layout 2, 16 waves, 40 bands
        self.p = (C.addressof(raw) + 15) // 16 * 16

    def __call__(self, name, **wrong):
        """Call `name` with its valid arguments and `wrong` on top; returns (rc, last error)."""
        names = [n for n, _ in ENTRIES[name][2]]
        assert set(wrong) <= set(names), (name, wrong)
        vals = []
        for n, v in ENTRIES[name][2]:
            v = wrong.get(n, v)
            if isinstance(v, C.Array):
                self.keep.append(v)
                v = C.addressof(v)
            vals.append({P: self.p, PMIS: self.p + 4, CP: C.addressof(self.keep[1]), PLAN: C.addressof(self.keep[2])}.get(v, v)
                        if isinstance(v, str) else v)
        rc = getattr(self.h, name)(*vals)
        return rc, self.h.syg_last_error().decode()


@pytest.fixture()
def call(h):
    return Caller(h)


def rejected(res, prefix, part, rc=INVALID):
    got, msg = res
    assert got == rc, (got, msg)
    assert msg.startswith(prefix) and part in msg, msg


def test_all_fifteen_are_bound(h):
    from sygnals_amd import _lib
    assert len(ALL) == 15
    for name in ALL:
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(ENTRIES[name][2]), name


@pytest.mark.parametrize("name", ALL)
def test_clip_checks(call, name):
    own, clip, args = ENTRIES[name]
    for ptr in ("y", "window", "twiddle"):
        rejected(call(name, **{ptr: None}), clip, "null pointer argument")
    rejected(call(name, B=0), clip, "need B >= 1, L >= 1, ldy >= L")
    rejected(call(name, L=0, ldy=0), clip, "need B >= 1, L >= 1, ldy >= L")
    rejected(call(name, ldy=47999), clip, "need B >= 1, L >= 1, ldy >= L")
    rejected(call(name, hop=0), clip, "hop must be >= 1")
    rejected(call(name, hop=-512), clip, "hop must be >= 1")
    for T in (93, 95, 0):
        rejected(call(name, T=T), clip, "does not match the framing rule")
    # center = 0: 1 + (L - n_fft) / hop frames
    n_fft = dict(args).get("n_fft", 1024 if "w1024" in name else 4096 if "w4096" in name else 2048)
    rejected(call(name, center=0, T=94), clip, "does not match the framing rule")
    rejected(call(name, center=0, T=(48000 - n_fft) // 512), clip, "does not match the framing rule")
    rejected(call(name, center=0, L=n_fft - 1, ldy=n_fft - 1, T=1), clip, "does not match the framing rule")


@pytest.mark.parametrize("name", ALL)
def test_output_and_table_pointers(call, name):
    own, clip, args = ENTRIES[name]
    required = {"wpacked", "plan", "segtab", "dct", "mel_out", "mfcc_out", "out", "basis_p"} & {n for n, _ in args}
    if name in ("syg_stft2048_mfcc_f32", "syg_stft_mfcc_pow2_f32"):
        required.discard("mel_out")                               # optional there
    if name in ("syg_stft_rows_w1024_f32", "syg_stft_rows_w4096_f32"):
        required -= {"segtab", "mel_out"}                        # the mel block is optional (see test_rows_family_rules)
    if name == "syg_stft2048_features_tri_f32":
        required.discard("mel_out")
    for ptr in sorted(required):
        rejected(call(name, **{ptr: None}), clip if ptr == "basis_p" else own, "null")


@pytest.mark.parametrize("name", sorted(SEGMENT))
def test_piece_table_checks(call, name):
    own, clip, args = ENTRIES[name]
    words = dict(args)["n_segtab"]
    for n in (words - 1, words + 4, 0, 4096):
        rejected(call(name, n_segtab=n), own, "the piece table has %d words" % n)
    rejected(call(name, segtab=PMIS), own, "16-byte aligned")
    for n_mels in (0, -1, SEGMENT[name] + 1):
        rejected(call(name, n_mels=n_mels), own, "n_mels")


def test_mel_tri_takes_both_table_sizes(call):
    # (1024 words: the two-pass table; the call then fails at the NEXT wrong thing)
    rejected(call("syg_stft2048_mel_tri_f32", n_segtab=1024, waves=4), "stft2048_mel_tri: ", "waves must be 8 or 16")


@pytest.mark.parametrize("name", sorted(ROWS))
def test_rows_checks(call, name):
    own, clip, args = ENTRIES[name]
    optional, n_bins = ROWS[name]
    plan_who = "stft2048: " if clip == "stft2048: " else own
    if not optional:
        rejected(call(name, stats_out=None, contrast_out=None), own, "no statistics requested")
    for bad in (dict(smask=0), dict(smask=32), dict(smask=64), dict(smask=-1), dict(roll=1.5), dict(roll=-0.1), dict(sr=0.0),
                dict(bw_p=0.0)):
        rejected(call(name, **bad), own, "invalid statistics parameters")
    rejected(call(name, cplan=None), plan_who, "contrast_out given without cplan_host")
    for n_rows in (0, -1, MAX_BANDS + 1):
        rejected(call(name, cplan=cplan(n_rows=n_rows)), plan_who, "contrast rows must be in [1, %d]" % MAX_BANDS)
    rejected(call(name, cplan=cplan(hi=(100, n_bins + 1))), plan_who, "contrast band 1 invalid")
    rejected(call(name, cplan=cplan(hi=(n_bins + 1, n_bins + 2))), plan_who, "contrast band 0 invalid")
    rejected(call(name, cplan=cplan(k=(2, 21))), plan_who, "contrast band 1 invalid")       # k > hi - lo
    rejected(call(name, cplan=cplan(k=(0, 2))), plan_who, "contrast band 0 invalid")
    rejected(call(name, cplan=cplan(lo=(-1, 100))), plan_who, "contrast band 0 invalid")
    rejected(call(name, cplan=cplan(lo=(0, 120))), plan_who, "contrast band 1 invalid")     # lo == hi
    # without the output that reads them, the parameters are not looked at: the call gets as far as its next wrong thing
    rejected(call(name, stats_out=None, smask=0, hop=0), clip, "hop must be >= 1")
    rejected(call(name, contrast_out=None, cplan=None, hop=0), clip, "hop must be >= 1")


def test_rows_frames_per_clip_limit(call):
    """2^27 frames per clip and more are refused by every rows form (hop 1, L = 2^27 - 1: T = 2^27).  The parent's wording
    differs between siblings and is plainly wrong in two of them -- syg_stft_rows_wsmall_f32 reports the framing rule,
    syg_stft2048_mel_f32 'invalid statistics parameters' -- so those two pin the return code alone, and w1024 ('clip too
    long' where w4096 says 'too many frames per clip') the return code and the prefix."""
    big = dict(hop=1, L=(1 << 27) - 1, ldy=(1 << 27) - 1, T=1 << 27)
    rejected(call("syg_stft_rows_w4096_f32", **big), "stft_rows_w4096: ", "too many frames per clip")
    rejected(call("syg_stft_rows_w1024_f32", **big), "stft_rows_w1024: ", "")
    assert call("syg_stft_rows_wsmall_f32", **big)[0] == INVALID
    assert call("syg_stft2048_mel_f32", **big)[0] == INVALID
    # the 2048 forms that keep results in 24-bit frame indices / 32-bit offsets have limits of their own
    rejected(call("syg_stft2048_stats_f32", **big), "stft2048_stats: ", "clip too long")
    rejected(call("syg_stft2048_features_tri_f32", **big), "stft2048_features_tri: ", "clip too long")
    rejected(call("syg_stft2048_mel_tri_f32", **big), "stft2048_mel_tri: ", "clip too long")


def test_rows_family_rules(call):
    rejected(call("syg_stft_rows_wsmall_f32", n_fft=1024), "stft_rows_wsmall: ", "n_fft must be 512 or 256 (got 1024)")
    rejected(call("syg_stft_mel_wseg_small_f32", n_fft=1024), "stft_mel_wseg_small: ", "n_fft must be 512 or 256 (got 1024)")
    rejected(call("syg_stft_rows_wsmall_f32", n_fft=128), "stft_rows_wsmall: ", "n_fft must be 512 or 256 (got 128)")
    rejected(call("syg_stft_rows_w1024_f32", segtab=None), "stft_rows_w1024: ", "segtab and mel_out come together")
    rejected(call("syg_stft_rows_w1024_f32", mel_out=None), "stft_rows_w1024: ", "segtab and mel_out come together")
    rejected(call("syg_stft_rows_w4096_f32", mel_out=None), "stft_rows_w4096: ", "a piece table without mel_out")
    rejected(call("syg_stft2048_stats_f32", hop=1024, T=47), "stft2048_stats: ", "needs hop <= 512")
    # statistics only (no piece table): the table's arguments are then not looked at
    for name in ("syg_stft_rows_w1024_f32", "syg_stft_rows_w4096_f32"):
        rejected(call(name, segtab=None, mel_out=None, n_segtab=0, n_mels=0, hop=0), ENTRIES[name][0], "hop must be >= 1")


def test_other_family_rules(call):
    rejected(call("syg_stft2048_mfcc_f32", plan=(C.c_int32 * 5)(2, 8, 28, 10, 8 * 28 * 64)), "stft2048_mfcc: ", "needs a 16-wave plan")
    rejected(call("syg_stft2048_mel_f32", plan=(C.c_int32 * 5)(1, 16, 28, 10, 16 * 28 * 64)), "stft2048_mel: ", "mel plan layout 1")
    rejected(call("syg_stft2048_mel_f32", n_mels=41), "stft2048_mel: ", "groups of four mel rows")
    rejected(call("syg_stft2048_mel_tri_f32", waves=4), "stft2048_mel_tri: ", "waves must be 8 or 16")
    for name, own in (("syg_stft2048_mfcc_f32", "stft2048_mfcc: "), ("syg_stft2048_mfcc_tri_f32", "stft2048_mfcc_tri: "),
                      ("syg_stft2048_features_tri_f32", "stft2048_features_tri: "), ("syg_stft_mfcc_pow2_f32", "stft_mfcc_pow2: ")):
        rejected(call(name, n_mfcc=0), own, "n_mfcc")
        rejected(call(name, n_mfcc=41), own, "n_mfcc")
        rejected(call(name, amin=0.0), own, "amin must be strictly positive")
        rejected(call(name, ref_is_max=2), own, "ref_is_max must be 0 or 1")
    rejected(call("syg_stft2048_features_tri_f32", mfcc_rows=12), "stft2048_features_tri: ", "mfcc_rows_per_clip >= n_mfcc")
    for name in ("syg_stft_mel_pow2_f32", "syg_stft_mfcc_pow2_f32"):
        own = ENTRIES[name][0]
        rejected(call(name, n_fft=1000), own, "n_fft must be a power of two in [64, 4096] (got 1000)")
        rejected(call(name, n_fft=8192, Fp=4112), own, "n_fft must be a power of two in [64, 4096] (got 8192)")
        rejected(call(name, Fp=257), own, "Fp must be 1 + n_fft/2 rounded up to a multiple of 16 (got 257)")
        rejected(call(name, n_mels=0), own, "n_mels must be in [1, 256]")
        rejected(call(name, n_mels=257), own, "n_mels must be in [1, 256]")
        rejected(call(name, basis_p=PMIS), own, "the padded filterbank must be 16-byte aligned")
    rejected(call("syg_stft_mel_pow2_f32", power=3), "stft_mel_pow2: ", "power must be 1 or 2")
    rejected(call("syg_stft_rows_w4096_f32", window=PMIS), "stft_rows_w4096: ", "16-byte aligned")
    rejected(call("syg_stft_mel_w4096_f32", window=PMIS), "stft_mel_w4096: ", "16-byte aligned")


# (n_mels, n_mfcc) -> [(first T, value)]: the value holds from that frame count up to the next entry's (the last one up to 400)
FITS = {
    "syg_stft2048_mfcc_fits": {(40, 13): [(1, 2), (113, 1), (353, 0)], (64, 13): [(1, 2), (65, 1), (209, 0)],
                               (128, 13): [(1, 2), (17, 1), (97, 0)], (127, 20): [(1, 2), (17, 1), (97, 0)], (1, 1): [(1, 2)]},
    "syg_stft2048_mfcc_tri_fits": {(40, 13): [(1, 1), (97, 0)], (64, 13): [(1, 1), (49, 0)], (128, 13): [(1, 0)],
                                   (127, 20): [(1, 1), (17, 0)], (1, 1): [(1, 1)]},
}


@pytest.mark.parametrize("name", sorted(FITS))
def test_clip_resident_fits(h, name):
    """syg_stft2048_mfcc_fits (2: the clip's mel matrix, DCT rows and lifter fit beside the stage buffer, 1: in its place, 0:
    not at all) and syg_stft2048_mfcc_tri_fits (1: two mel matrices fit beside the stage buffer) for T = 1 ... 400: the frame
    counts at which the answer changes (the padded frame count is a multiple of 16, so they are 16 k + 1) and the value on
    each side, as the library gave them before the LDS accounting was moved into one place."""
    fits = getattr(h, name)
    for (n_mels, n_mfcc), steps in FITS[name].items():
        want = []
        for (t0, v), t1 in zip(steps, [t for t, _ in steps[1:]] + [401]):
            want += [v] * (t1 - t0)
        got = [fits(n_mels, T, n_mfcc) for T in range(1, 401)]
        assert got == want, (n_mels, n_mfcc, [T for T in range(1, 401) if got[T - 1] != want[T - 1]][:8])
    for bad in ((0, 94, 13), (40, 0, 13), (40, 94, 0), (40, 94, 41), (257 if name == "syg_stft2048_mfcc_fits" else 128, 94, 13)):
        assert fits(*bad) == 0, bad
    # what tests/test_gpu_fused.py relies on
    assert [h.syg_stft2048_mfcc_fits(n, T, 13) for n, T in ((40, 94), (64, 94), (128, 94), (128, 120))] == [2, 1, 1, 0]
