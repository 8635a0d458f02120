"""The onset parameter tables shared by the host checks (tests/test_onset_ref.py: every fixture is within its cap by the
restatement alone, every boundary is in the table) and the device tests (tests/test_gpu_onset_params.py).  Plain data and
seeded generators, no device: both sides build the exact same inputs from a case.

The sizes are the switches of sygnals_amd/csrc/onset.hip: the flux kernel splits M mel rows over four waves, walks 64
frames a step, runs as one workgroup a clip up to T_ONE = 2048 frames and as slices of FSL = 256 output frames over partial
maxima of MSL = 1024 frames beyond; the peaks kernel takes 256 threads up to 256 frames, stages a halo of PHALO = 256
frames a side, runs fused up to P_ONE = 4096 frames and packs 64 * PW = 131072 flags a pass of the greedy walk."""
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------------------- A. the flux kernel alone
FLUX_M = (1, 2, 3, 5, 7, 40, 127, 130, 256)
FLUX_T = (2, 3, 63, 64, 65, 300, 2047, 2048, 2049, 2303, 2304, 2305, 3071, 3072, 3073)
FLUX_LAGK = ((1, 1), (2, 3), (1, 4), (3, 2), (64, 1), (65, 3), ("T-1", 1), (1, "M"), (1, "M+5"))
FLUX_TOP_DB = (80.0, 20.0, None)
FLUX_AMIN = (1e-10, 1e-5)
# (zeros in front beyond the lag, T_out): centre padding cut to T and uncut, no centre padding uncut and cut by a frame
FLUX_PAD = (("centre-cut", 2, "T"), ("centre-full", 2, None), ("plain-full", 0, None), ("plain-cut", 0, "T-1"))
FLUX_SLICED_FROM = 2049                 # T_ONE + 1

FluxCase = namedtuple("FluxCase", "M T lag max_size top_db amin pad T_out detrend B seed")


def _resolve(v, M, T):
    return {"T-1": T - 1, "T": T, "M": M, "M+5": M + 5}.get(v, v)


def _flux_case(M, T, lagk, top_db, amin, padmode, detrend, seed):
    lag, k = _resolve(lagk[0], M, T), _resolve(lagk[1], M, T)
    if not 1 <= lag < T:
        return None
    _, extra, cut = padmode
    T_out = _resolve(cut, M, T)
    if T_out is not None and T_out <= lag + extra:      # the cut would leave the padding alone: such a case runs uncut
        T_out = None
    # three different clips a call on the sliced sizes (the workspace is indexed by clip) and under detrend
    B = 3 if (T >= FLUX_SLICED_FROM or detrend) else 1
    return FluxCase(M, T, lag, k, top_db, amin, lag + extra, T_out, detrend, B, seed)


def flux_cases():
    """A seeded subset of the product: every T with every (lag, max_size), every M with every T, every M with every
    (lag, max_size), every sliced T with every padding and detrend both ways; the other axes cycle through shuffled lists
    so that each value of each axis occurs many times."""
    rng = np.random.default_rng(20240)
    out, seen = [], set()

    def cyc(values):
        while True:
            for i in rng.permutation(len(values)):
                yield values[i]
    m_, t_, lk_, db_, am_, pd_, dt_ = (cyc(v) for v in (FLUX_M, FLUX_T, FLUX_LAGK, FLUX_TOP_DB, FLUX_AMIN, FLUX_PAD,
                                                       (False, True)))

    def add(M=None, T=None, lagk=None, padmode=None, detrend=None):
        M, T = next(m_) if M is None else M, next(t_) if T is None else T
        for _ in range(1 if lagk is not None else 4 * len(FLUX_LAGK)):     # (a drawn lag the clip is too short for: draw again)
            c = _flux_case(M, T, next(lk_) if lagk is None else lagk, next(db_), next(am_),
                           next(pd_) if padmode is None else padmode, next(dt_) if detrend is None else detrend, len(out))
            if c is not None and c[:9] not in seen:
                seen.add(c[:9])
                out.append(c)
                return
    for T in FLUX_T:
        for lagk in FLUX_LAGK:
            add(T=T, lagk=lagk)
    for M in FLUX_M:
        for T in FLUX_T:
            add(M=M, T=T)
    for M in FLUX_M:
        for lagk in FLUX_LAGK:
            add(M=M, lagk=lagk)
    for T in FLUX_T:
        if T >= 63:
            for padmode in FLUX_PAD:
                for detrend in (False, True):
                    add(T=T, padmode=padmode, detrend=detrend)
    return out


def flux_id(c):
    return (f"M{c.M}-T{c.T}-lag{c.lag}-k{c.max_size}-db{c.top_db:g}" if c.top_db is not None else
            f"M{c.M}-T{c.T}-lag{c.lag}-k{c.max_size}-dbNone") + \
        f"-amin{c.amin:g}-pad{c.pad}-out{c.T_out}-{'detrend' if c.detrend else 'raw'}-B{c.B}"


def flux_power(c):
    """[B, M, T] float32 mel POWER: sparse values over eight decades, a different clip per row."""
    rng = np.random.default_rng(7000 + c.seed)
    out = []
    for _ in range(c.B):
        scale = 10.0 ** rng.uniform(-6, 2, size=(1, c.T))
        if c.lag == c.T - 1:            # one valid frame: make its pair a rise near the clip's maximum, or any top_db floors both
            scale[0, 0], scale[0, -1] = 1e-2, 10.0 ** rng.uniform(1.5, 2.5)
        out.append((rng.random((c.M, c.T)) ** 8 * scale).astype(np.float32))
    return np.stack(out)


def flux_flat_power(c):
    """[2, M, T]: an all-zero clip and a constant clip.  Their envelope is exactly 0."""
    return np.stack([np.zeros((c.M, c.T), np.float32), np.full((c.M, c.T), 0.0123, np.float32)])


# ---------------------------------------------------------------------------- B. the envelope through the mirrors
# front end -> the function of sygnals_amd.ops that manager.mel_power_batch must reach for it
FRONT_ENDS = {"fused2048": "stft2048_mel", "seg1024": "stft_mel_w1024_seg", "seg512": "stft_mel_wseg_small",
              "seg256": "stft_mel_wseg_small", "seg4096": "stft_mel_w4096", "pow2": "stft_mel_pow2", "generic": "mel_dense"}
MirrorCase = namedtuple("MirrorCase", "front sr n_fft hop n_mels fmin fmax opt")
_MIRROR_FRAMES = (("fused2048", 22050, 2048), ("seg1024", 16000, 1024), ("seg512", 16000, 512), ("seg256", 8000, 256),
                  ("seg4096", 32000, 4096), ("pow2", 8000, 128), ("generic", 16000, 1000))
_MIRROR_OPTS = (dict(), dict(lag=2), dict(max_size=3), dict(center=False), dict(detrend=True),
                dict(lag=2, max_size=3, detrend=True))
# the segment-sum kernels of 1024 / 512 / 256 hold a 40-band filterbank, not a 128-band one; a 128-band filterbank at
# those frame lengths is the fused power-of-two kernel's (pinned below and by the host check)
_SEG_40_ONLY = ("seg1024", "seg512", "seg256")


def mirror_cases():
    out = []
    for fi, (front, sr, n_fft) in enumerate(_MIRROR_FRAMES):
        # (n_fft // (2 hop), n_mels, fmin, fmax): the four paddings, both filterbanks, one band-limited filterbank
        rows = [(2, 128, 0.0, None), (2, 40, 0.0, None), (0, 128, 0.0, None), (1, 40, 0.0, None), (16, 128, 0.0, None),
                (16, 40, 0.0, None), (2, 40, 60.0, 0.4 * sr)]
        for ri, (r, n_mels, fmin, fmax) in enumerate(rows):
            hop = n_fft if r == 0 else n_fft // (2 * r)
            assert n_fft // (2 * hop) == r
            served = "pow2" if (front in _SEG_40_ONLY and n_mels == 128) else front
            out.append(MirrorCase(served, sr, n_fft, hop, n_mels, fmin, fmax, _MIRROR_OPTS[(fi + ri) % len(_MIRROR_OPTS)]))
    return out


def mirror_id(c):
    opt = "+".join(f"{k}{v}" for k, v in c.opt.items()) or "default"
    return f"{c.front}-sr{c.sr}-n{c.n_fft}-hop{c.hop}-mel{c.n_mels}-fmin{c.fmin:g}-{opt}"


# ---------------------------------------------------------------------------- C. the peaks kernel alone
PEAK_T = (1, 2, 255, 256, 257, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 131072, 131073)
PEAK_WAIT = (0, 1, 62, 63, 64, 65, 200, "T+1")
PEAK_HALO = (1, 255, 256, 257)          # max(pre) and max(post): the staged tile holds 256 frames a side
PEAK_WIDE_T_MAX = 8193                  # a window costs T loads per frame
GRID_KINDS = ("plateau", "stairs", "negative", "zero-run", "random", "ramp-up", "ramp-down")
GRID = 2.0 ** -10

PeakCase = namedtuple("PeakCase", "T pre_max post_max pre_avg post_avg delta wait kind seed")


def peak_windows(c):
    return dict(pre_max=c.pre_max, post_max=c.post_max, pre_avg=c.pre_avg, post_avg=c.post_avg, delta=c.delta, wait=c.wait)


def _halo_windows(hl, hr, flip_l, flip_r):
    """(pre_max, post_max, pre_avg, post_avg) with max(pre) = hl and max(post) = hr; the flips say whether the max window
    or the mean window carries that side, the other one stays narrow (0 or 3 frames before, 1 after)."""
    pre = (hl, 0 if hl == 1 else 3)
    post = (hr, 1)
    pre_max, pre_avg = pre if flip_l else pre[::-1]
    post_max, post_avg = post if flip_r else post[::-1]
    return pre_max, post_max, pre_avg, post_avg


def peak_cases():
    """Narrow windows: every T with every wait.  Wide windows (T <= 8193): every pair of halos with every T.  The kind of
    envelope cycles; `smooth` rows (normalised, under the unsure-frame rule) sit on every other case up to 8193 frames and
    on four of the long ones."""
    out = []
    narrow = ((1, 1, 4, 5), (0, 1, 0, 1), (3, 2, 0, 1), (2, 1, 9, 10))
    kinds = GRID_KINDS
    n = 0
    for T in PEAK_T:
        for wait in PEAK_WAIT:
            w = narrow[(n + n // 8) % len(narrow)]
            kind = kinds[n % len(kinds)]
            delta = 0.0 if kind == "plateau" or n % 3 == 0 else 0.07
            wt = T + 1 if wait == "T+1" else wait
            out.append(PeakCase(T, *w, delta, wt, kind, n))
            if (T <= PEAK_WIDE_T_MAX and n % 2 == 0) or (T > PEAK_WIDE_T_MAX and wait in (0, 63)):
                out.append(PeakCase(T, *w, 0.07, wt, "smooth", n))
            n += 1
    for T in PEAK_T:
        if not 255 <= T <= PEAK_WIDE_T_MAX:
            continue
        for hl in PEAK_HALO:
            for hr in PEAK_HALO:
                if hl == 1 and hr == 1:
                    continue
                w = _halo_windows(hl, hr, n % 2 == 1, (n // 2) % 2 == 1)
                kind = kinds[n % len(kinds)]
                delta = 0.0 if kind == "plateau" or n % 3 == 0 else 0.07
                wait = (0, 1, 62, 63, 64, 65, 200, T + 1)[n % 8]
                out.append(PeakCase(T, *w, delta, wait, kind, n))
                if n % 2 == 0:
                    out.append(PeakCase(T, *w, 0.05, wait, "smooth", n))
                n += 1
    # what the cycling must not be trusted to hit: every frame a candidate, kept and compacted across the fused / sliced
    # switch and across a 131072-frame segment of the greedy walk
    for T in (4096, 4097, 131072, 131073):
        out.append(PeakCase(T, 1, 1, 4, 5, 0.0, 0, "plateau", n))
        out.append(PeakCase(T, 0, 1, 0, 1, 0.0, 63, "plateau", n + 1))
        n += 2
    return out


def peak_id(c):
    return f"T{c.T}-w{c.pre_max}.{c.post_max}.{c.pre_avg}.{c.post_avg}-d{c.delta:g}-wait{c.wait}-{c.kind}-{c.seed}"


def smooth_envelope(T, seed):
    """The envelope of tests/test_gpu_onset.py::_envelope: rectified, smoothed noise over a small random floor."""
    rng = np.random.default_rng(seed)
    e = np.convolve(np.maximum(rng.standard_normal(T + 4), 0.0) ** 2, np.hanning(5), mode="valid")
    return (e + 0.01 * rng.random(T)).astype(np.float32)


def grid_envelope(kind, T, seed):
    """float32 [T], every value an integer multiple of 2^-10 in [-1, 1]: a window sum of such values is exact in float64 in
    any order, so the device and the restatement must agree on every comparison, ties included."""
    rng = np.random.default_rng(9000 + seed)
    if kind == "plateau":
        e = np.full(T, 384)
    elif kind == "stairs":              # runs of 1 ... 7 equal frames over nine levels: ties and repeated maxima in a window
        levels = rng.integers(-4, 5, size=T) * 128
        e = np.repeat(levels, rng.integers(1, 8, size=T))[:T]
    elif kind == "negative":
        e = -rng.integers(1, 1025, size=T)
    elif kind == "zero-run":            # zero runs inside a non-zero envelope: a zero that wins both tests is still no peak
        e = np.repeat(rng.integers(-3, 4, size=T) * 200, rng.integers(1, 12, size=T))[:T]
        e[0] = 200
    elif kind == "random":
        e = rng.integers(-1024, 1025, size=T)
    elif kind in ("ramp-up", "ramp-down"):   # saw teeth of 1000 frames: the last (first) frame is a peak of the clip
        e = np.arange(T) % 1000 - 500 + (np.arange(T) % 1000 >= 500)     # never 0
        if kind == "ramp-down":
            e = e[::-1]
    else:
        raise ValueError(kind)
    return (np.asarray(e, dtype=np.float64) * GRID).astype(np.float32)


# smooth rows whose first seed (31000 + n) left a frame within (W + 4) 2^-24 of the mean test's threshold in the restatement:
# 19 of 123, more than the one case in ten the rule allows, so these take the next clear seed.  Rows 122 and 164 keep
# theirs (one unsure frame each): they are the rows that run the sure-frames branch of the comparison.
SMOOTH_SEEDS = {96: 32096, 107: 32107, 188: 34188, 192: 32192, 196: 33196, 198: 32198, 200: 32200, 212: 32212, 226: 32226,
                230: 32230, 240: 32240, 242: 32242, 244: 37244, 248: 32248, 252: 37252, 254: 32254, 256: 34256}


def peak_envelope(c):
    """(float32 envelope, normalize)."""
    if c.kind == "smooth":
        return smooth_envelope(c.T, SMOOTH_SEEDS.get(c.seed, 31000 + c.seed)), True
    return grid_envelope(c.kind, c.T, c.seed), False


# ---------------------------------------------------------------------------- D. end to end
E2E_CASES = ((22050, 256, 22050), (44100, 512, 44100), (8000, 128, 12000), (48000, 1024, 96000), (16000, 160, 24000),
             (22050, 64, 11025), (32000, 441, 40001))                      # sr, hop, clip length
E2E_PEAK_ARGS = (dict(), dict(delta=0.03), dict(delta=0.2, wait=0), dict(pre_max=10, post_max=10))
E2E_BACKTRACK = ((22050, 256, 22050), (16000, 160, 24000))                 # these two also run with backtrack=True


def e2e_cases():
    out = [(sr, hop, L, ai, False) for (sr, hop, L) in E2E_CASES for ai in range(len(E2E_PEAK_ARGS))]
    out += [(sr, hop, L, ai, True) for (sr, hop, L) in E2E_BACKTRACK for ai in range(len(E2E_PEAK_ARGS))]
    return out


def e2e_id(c):
    sr, hop, L, ai, bt = c
    args = "+".join(f"{k}{v}" for k, v in E2E_PEAK_ARGS[ai].items()) or "defaults"
    return f"sr{sr}-hop{hop}-L{L}-{args}{'-backtrack' if bt else ''}"


# ---------------------------------------------------------------------------- E. short clips, metrics, silence
SHORT_SR_HOP = ((22050, 512), (16000, 256))
SHORT_LAGS = (1, 3)


def short_lengths(hop):
    return (1, 100, hop - 1, hop, 2 * hop - 1)


METRIC_L = (1, 63, 1023, 1024, 1025, 100001)
METRIC_B = (1, 5)

# segment_by_silence on onset_ref.silence_clip (noise passages of 0.50 / 0.35 / 0.45 s, gaps of 0.40 and 0.25 s)
SILENCE_CASES = (
    dict(sr=22050, frame_length=1024, hop_length=None, threshold_db=-20.0),
    dict(sr=22050, frame_length=400, hop_length=100, threshold_db=-60.0),
    dict(sr=22050, frame_length=512, hop_length=128, threshold_db=-60.0, min_silence_duration_sec=0.3),   # 0.25 s gap stays
    dict(sr=22050, frame_length=1024, hop_length=None, threshold_db=-20.0, padding_sec=0.15),             # 0.25 s gap merges
    dict(sr=16000, frame_length=400, hop_length=100, threshold_db=-20.0, min_silence_duration_sec=0.3, padding_sec=0.22),
)
# segments expected from each (the three passages; two of them joined; ...): pinned so that a parameter set cannot quietly
# stop removing its gap
SILENCE_SEGMENTS = (3, 3, 2, 2, 1)


def silence_kwargs(c):
    return {k: v for k, v in c.items() if k not in ("sr", "frame_length", "hop_length")}
