"""The frame-count rules of the entry points outside the fused STFT front ends (those are in test_cabi_stft.py): an
otherwise valid call with a wrong T is refused with the entry's own prefix, the one wording "does not match the framing
rule" and the count the rule expects in parentheses.  Two rules exist: 1 + L / hop for centred frames (frame_stats,
stft_pow2, pitch_frames) and librosa.feature.rms's count on the padded signal (hnr_rows), which is one less for an odd
frame length when hop divides L.  Their Python mirrors (ops.num_frames, ops.num_frames_padded) and the one call helper
of ops (_call) are pinned here too.  No GPU is needed: nothing here reaches a device call."""
import ctypes as C
import os

import pytest

INVALID = -1
P = "<buffer>"

# name -> (prefix of its messages, name of its frame-length argument, arguments in ABI order with valid values:
#          L = 22016 = 86 * 256, hop 256, centred: 87 frames under both rules for an even frame length)
ENTRIES = {
    "syg_frame_stats_f32": ("frame_stats: ", "frame_length", [
        ("y", P), ("B", 2), ("L", 22016), ("ldy", 22016), ("frame_length", 1024), ("hop", 256), ("center", 1), ("T", 87),
        ("num_bins", 10), ("mask", 1), ("out", P), ("stream", None)]),
    "syg_stft_pow2_c2c_f32": ("stft_pow2: ", "n_fft", [
        ("y", P), ("B", 2), ("L", 22016), ("ldy", 22016), ("n_fft", 1024), ("hop", 256), ("center", 1), ("T", 87),
        ("window", P), ("twiddle", P), ("out", P), ("stream", None)]),
    "syg_pitch_frames_f32": ("pitch_frames: ", "frame_length", [
        ("y", P), ("B", 2), ("L", 22016), ("ldy", 22016), ("frame_length", 2048), ("win_length", 1024), ("hop", 256),
        ("center", 1), ("T", 87), ("sr", 22050.0), ("min_period", 10), ("max_period", 500), ("mode", 0),
        ("trough_threshold", 0.1), ("fmin", 65.0), ("n_bins", 0), ("ptab", None), ("K", 0), ("twiddle", P), ("f0_out", P),
        ("cand_bin", None), ("cand_prob", None), ("cand_count", None), ("voiced_prob", None), ("cmndf_out", None),
        ("stream", None)]),
    "syg_hnr_rows_f32": ("hnr_rows: ", "frame_length", [
        ("y_harm", P), ("y_perc", P), ("B", 2), ("L", 22016), ("ldy", 22016), ("frame_length", 1024), ("hop", 256),
        ("center", 1), ("T", 87), ("hnr_out", P), ("rms_harm_out", None), ("rms_perc_out", None), ("stream", None)]),
}
ALL = sorted(ENTRIES)


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def call(h):
    buf = (C.c_float * 64)()

    def go(name, **wrong):
        """Call `name` with its valid arguments and `wrong` on top; returns (rc, last error)."""
        args = ENTRIES[name][2]
        assert set(wrong) <= {n for n, _ in args}, (name, wrong)
        vals = [wrong.get(n, v) for n, v in args]
        rc = getattr(h, name)(*[C.addressof(buf) if v == P else v for v in vals])
        return rc, h.syg_last_error().decode()
    return go


def refused(res, prefix, T, expected):
    rc, msg = res
    assert rc == INVALID, (rc, msg)
    assert msg.startswith(prefix), msg
    assert "T=%d does not match the framing rule (%d)" % (T, expected) in msg, msg


def test_all_four_are_bound(h):
    from sygnals_amd import _lib
    for name in ALL:
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(ENTRIES[name][2]), name


@pytest.mark.parametrize("name", ALL)
def test_wrong_T_reports_the_expected_count(call, name):
    prefix, flen, args = ENTRIES[name]
    frame = dict(args)[flen]
    # center = 1: 1 + 22016 / 256 = 87 frames
    for T in (86, 88, 0):
        refused(call(name, T=T), prefix, T, 87)
    # center = 0, L >= frame: 1 + (22016 - frame) / 256 = 83 frames of 1024, 79 of 2048
    full = {1024: 83, 2048: 79}[frame]
    for T in (87, full - 1, full + 1):
        refused(call(name, center=0, T=T), prefix, T, full)
    # center = 0, L = frame - 1: no frame at all, so T = 1 is refused
    refused(call(name, center=0, L=frame - 1, ldy=frame - 1, T=1), prefix, 1, 0)
    # center = 0, L = frame: exactly one frame
    refused(call(name, center=0, L=frame, ldy=frame, T=2), prefix, 2, 1)


def test_odd_frame_length_separates_the_two_rules(call):
    """frame_length 1025, hop 256, L = 86 * 256, centred: 1 + L / hop = 87, but the signal padded by 512 on both sides
    holds 1 + (22016 + 1024 - 1025) / 256 = 86 frames."""
    refused(call("syg_hnr_rows_f32", frame_length=1025, T=87), "hnr_rows: ", 87, 86)
    refused(call("syg_frame_stats_f32", frame_length=1025, T=86), "frame_stats: ", 86, 87)
    # the even frame length 1024: 87 under both rules
    refused(call("syg_hnr_rows_f32", T=86), "hnr_rows: ", 86, 87)
    refused(call("syg_frame_stats_f32", T=86), "frame_stats: ", 86, 87)
    # not centred, the rules agree for an odd frame length as well: 1 + (22016 - 1025) / 256 = 82
    refused(call("syg_hnr_rows_f32", frame_length=1025, center=0, T=83), "hnr_rows: ", 83, 82)
    refused(call("syg_frame_stats_f32", frame_length=1025, center=0, T=83), "frame_stats: ", 83, 82)


RULES = [  # (L, frame, hop, center) -> (num_frames, num_frames_padded)
    ((22016, 1025, 256, True), (87, 86)),
    ((22016, 1024, 256, True), (87, 87)),
    ((100, 2048, 512, False), (0, 0)),
    ((22016, 1025, 256, False), (82, 82)),
    ((2047, 2048, 512, True), (4, 4)),
]


@pytest.mark.parametrize("shape,counts", RULES)
def test_python_mirrors(shape, counts):
    from sygnals_amd import _pitch, ops
    assert (ops.num_frames(*shape), ops.num_frames_padded(*shape)) == counts
    assert _pitch.num_frames(*shape) == counts[0]


def test_pitch_rule_is_the_one_rule():
    from sygnals_amd import _pitch, ops
    assert _pitch.num_frames is ops.num_frames


class FakeLib:
    def __init__(self, status):
        self.status, self.calls = status, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.status
        return entry


def test_call_appends_the_stream_and_checks_under_the_entry_name(h, monkeypatch):
    from sygnals_amd import ops
    from sygnals_amd._lib import SygnalsHipError
    monkeypatch.setattr(ops, "_stream_ptr", lambda: 0x5EED)
    ok = FakeLib(0)
    monkeypatch.setattr(ops, "lib", lambda: ok)                  # a replaced ops.lib is looked up at call time
    assert ops._call("syg_some_entry_f32", 1, 2.5, None) is None
    (name, args), = ok.calls
    assert name == "syg_some_entry_f32" and args[:3] == (1, 2.5, None) and len(args) == 4
    assert isinstance(args[3], C.c_void_p) and args[3].value == 0x5EED
    bad = FakeLib(-2)
    monkeypatch.setattr(ops, "lib", lambda: bad)
    with pytest.raises(SygnalsHipError, match=r"syg_other_entry_f32 failed \(rc=-2\)"):
        ops._call("syg_other_entry_f32", 7)
    assert [n for n, _ in bad.calls] == ["syg_other_entry_f32"] and not ok.calls[1:]
