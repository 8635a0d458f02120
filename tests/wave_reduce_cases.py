"""The cases that pin the float64 wave sums and the (value, index) picks bit for bit (tests/golden/wave_reduce_before.json,
recorded from the code before every feature's private wave reduction was replaced by the shared ones of csrc/common.h):
the smallest shapes that reach each converted site.  Inputs come from numpy's default_rng(seed) on the host, so they do
not depend on the device; the kernels have no atomics, so a result is a function of its input alone.

    name -> (op, seed, args)        run(name) -> the results as a list of contiguous host arrays
"""
import hashlib

import numpy as np

CASES = {}


def _add(op, *args):
    CASES["%s-%s" % (op, "-".join(str(a) for a in args))] = (op, 2000 + len(CASES), args)


# frame_stats(y [2, 4000], frame, hop), centred: 1024 / 256 is the staged + vector load, 600 / 250 the scalar one
_add("frame_stats", 1024, 256)
_add("frame_stats", 600, 250)
# hnr_rows(yh, yp [2, L], 1024, 256), centred, a wave a frame, four to a workgroup: 24 frames fill the last workgroup, 26
# leave two of its waves idle
_add("hnr_rows", 3000, 1024, 256)
_add("hnr_rows", 3300, 1024, 256)
# fx_add_noise(y [2, L], noise, snr per row): L = resident_max + d, one launch (d < 0) and the partial-sum form (d > 0)
_add("fx_add_noise", -37)
_add("fx_add_noise", 1000)
# spec_augment(x [2, 20, 150], mask_value="mean", lengths (150, 97)): both forms of the mean's sums, a partial last chunk
_add("spec_augment", "resident")
_add("spec_augment", "tiled")
# cmvn(x [2, 13, 300], window, variance=True, form): the sliding window, and the whole row with its chunk sums of x and of
# (x - m)^2 out of LDS (resident) and from the two passes of the statistics kernel (tiled)
_add("cmvn", 51, None)
_add("cmvn", None, "resident")
_add("cmvn", None, "tiled")
# chroma_fold(x [2, 37, 129], table [12, 129], "rows", norm)
for _norm in (1, 2, "inf"):
    _add("chroma_fold", _norm)
# tuning_hist and piptrack of one small spectrogram [2, 5, 1025]: the float maximum behind the threshold
_add("tuning_hist", 1025)
# lpc_frames(y [2, 6000], 8, 2048, 512, burg); lpc_rows(y [2, L], 8, burg) above the stage chunk: three workgroups a row
_add("lpc_frames", 6000, 2048, 512)
_add("lpc_rows", 13001)
# pitch_pyin / pitch_yin(y [1, 8192]) at the default frame sizes: both float64 sums, the Viterbi arg-max, YIN's first minimum
_add("pitch_pyin", 8192)
_add("pitch_yin", 8192)
# beat_dp(ls [2, 400], periods, period_max): the three tiers (one wave with 2 and with 9 offsets a lane, four waves with 13),
# rows full of equal local scores
_add("beat_dp", 23, 40, 40)
_add("beat_dp", 150, 301, 301)
_add("beat_dp", 100, 130, 400)
# dtw(C [1, 70, 200], subseq=True): two zero-cost diagonals, so the last row's minimum stands in two columns
_add("dtw", 70, 200)


def _harmonic(rng, B, L, sr):
    """a few decaying partials over noise: voiced frames for the pitch trackers"""
    t = np.arange(L) / sr
    y = np.zeros((B, L))
    for b in range(B):
        f0 = 110.0 * (1 + b) * (1 + 0.1 * t)
        ph = 2 * np.pi * np.cumsum(f0) / sr
        y[b] = sum(np.sin(h * ph) / h for h in (1, 2, 3, 4)) + 0.05 * rng.standard_normal(L)
    return y.astype(np.float32)


def run(name):
    import torch
    from sygnals_amd import _pitch as P
    from sygnals_amd import ops
    op, seed, args = CASES[name]
    rng = np.random.default_rng(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    normal = lambda *shape: dev(rng.standard_normal(shape, dtype=np.float32))
    if op == "frame_stats":
        out = ops.frame_stats(normal(2, 4000), args[0], args[1], True)
    elif op == "hnr_rows":
        L, N, hop = args
        out = ops.hnr_rows(normal(2, L), normal(2, L), N, hop, True, rms=True)
    elif op == "fx_add_noise":
        L = ops.fx_add_noise_resident_max() + args[0]
        out = ops.fx_add_noise(normal(2, L), normal(2, L), np.array([3.0, 12.5]))
    elif op == "spec_augment":
        out = ops.spec_augment(normal(2, 20, 150), 11, freq_masks=2, freq_width=5, time_masks=2, time_width=20,
                               mask_value="mean", lengths=[150, 97], form=args[0])
    elif op == "cmvn":
        out = ops.cmvn(normal(2, 13, 300), args[0], True, form=args[1])
    elif op == "chroma_fold":
        x = np.abs(rng.standard_normal((2, 37, 129), dtype=np.float32))
        tab = np.abs(rng.standard_normal((12, 129), dtype=np.float32))
        out = ops.chroma_fold(dev(x), tab, "rows", 2, None, np.inf if args[0] == "inf" else args[0])
    elif op == "tuning_hist":
        S = dev(np.abs(rng.standard_normal((2, 5, 1025), dtype=np.float32)))
        out = tuple(ops.tuning_hist(S, 22050, 2048)) + tuple(ops.piptrack(S, 22050, 2048))
    elif op == "lpc_frames":
        L, N, hop = args
        out = ops.lpc_frames(normal(2, L), 8, N, hop, True, "burg", None, True, True)
    elif op == "lpc_rows":
        out = ops.lpc_rows(normal(2, args[0]), 8, "burg", None, None, True, True)
    elif op == "pitch_pyin":
        out = ops.pitch_pyin(dev(_harmonic(rng, 1, args[0], 22050)), 22050, P.C2, P.C7)
    elif op == "pitch_yin":
        out = ops.pitch_yin(dev(_harmonic(rng, 1, args[0], 22050)), 22050, P.C2, P.C7)
    elif op == "beat_dp":
        ls = rng.integers(0, 4, size=(2, 400)).astype(np.float32)            # small integers: equal candidates abound
        ls[:, ::50] += 3.0
        lsd = dev(ls)
        out = ops.beat_dp(lsd, lsd.max(dim=1).values, [args[0], args[1]], period_max=args[2])
    else:
        N, M = args
        C = rng.integers(1, 5, size=(N, M)).astype(np.float32)
        i = np.arange(N)
        C[i, 20 + i] = 0.0
        C[i, 110 + i] = 0.0
        r = ops.dtw(dev(C[None]), subseq=True, want_D=True)
        assert int(r["end_col"][0]) == 20 + N - 1 and float(r["cost"][0]) == 0.0, name       # the tie rule decided
        out = [r[k] for k in sorted(r) if r[k] is not None]
    out = [out] if isinstance(out, torch.Tensor) else list(out)
    assert out and all(isinstance(t, torch.Tensor) for t in out), name
    return [np.ascontiguousarray(t.contiguous().cpu().numpy()) for t in out]


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return {"sha256": h.hexdigest(), "first8": [repr(float(v)) for v in arrays[0].ravel()[:8]]}
