"""Restatement of SpecAugment in Python integers and float64 NumPy: the contract of sygnals_amd/csrc/spec_augment.hip and
sygnals_amd/_specaug.py, with which it shares no code (the Philox words come from tests/rng_ref.py).

Clip b: row r = first_row + b, T_b valid frames.  Item q = one call words(seed, r, q, stream=2), words w0 and w1.
draw(w, n) = (w n) >> 32.
  warp, q = 0, only if W > 0 and T_b > 2 W:  c = W + draw(w0, T_b - 2 W), w' = c - W + 1 + draw(w1, 2 W); [0, c) -> w' frames,
    [c, T_b) -> T_b - w' frames, each torch's linear interpolate with align_corners=False by the integer position rule.
  frequency mask i, q = 1 + i:  f = draw(w0, F + 1), f0 = draw(w1, K - f + 1): rows [f0, f0 + f).
  time mask j, q = 17 + j:  We = min(Wt, floor(p T_b)), t = draw(w0, We + 1), t0 = draw(w1, T_b - t + 1): frames [t0, t0 + t).
Order: warp, then the union of the masks; frames t >= T_b are copied.  "mean": the float64 mean of x[b, :, :T_b] before
the warp."""
import math

import numpy as np

from tests import rng_ref

STREAM = 2


def draw(w, n):
    return (int(w) * int(n)) >> 32


def _w01(seed, row, q):
    w = rng_ref.words(seed, row, [q], stream=STREAM)[0]
    return int(w[0]), int(w[1])


def clip_draws(seed, row, K, Tb, nf, F, nt, Wt, p, W):
    """The draws of one clip in Python integers: dict(c, w, f [nf], f0 [nf], t [nt], t0 [nt]); c = w = -1 for no warp."""
    d = {"c": -1, "w": -1, "f": [], "f0": [], "t": [], "t0": []}
    if W > 0 and Tb > 2 * W:
        w0, w1 = _w01(seed, row, 0)
        d["c"] = W + draw(w0, Tb - 2 * W)
        d["w"] = d["c"] - W + 1 + draw(w1, 2 * W)
    for i in range(nf):
        w0, w1 = _w01(seed, row, 1 + i)
        f = draw(w0, F + 1)
        d["f"].append(f)
        d["f0"].append(draw(w1, K - f + 1))
    We = min(Wt, math.floor(float(p) * float(Tb)))
    for j in range(nt):
        w0, w1 = _w01(seed, row, 17 + j)
        t = draw(w0, We + 1)
        d["t"].append(t)
        d["t0"].append(draw(w1, Tb - t + 1))
    return d


def draws(seed, first_row, B, K, T, lengths=None, nf=2, F=27, nt=2, Wt=100, p=1.0, W=0):
    lengths = [T] * B if lengths is None else [int(v) for v in lengths]
    return [clip_draws(seed, first_row + b, K, lengths[b], nf, F, nt, Wt, p, W) for b in range(B)]


def resize(seg, n_out):
    """seg [..., n_in] float64 -> [..., n_out]: linear, align_corners=False, the position by integer quotient / remainder."""
    seg = np.asarray(seg, dtype=np.float64)
    n_in = seg.shape[-1]
    assert n_in < 2 ** 31 and n_out < 2 ** 31                       # (2u + 1) n_in stays inside int64
    u = np.arange(n_out, dtype=np.int64)
    den = 2 * n_out
    num = np.maximum((2 * u + 1) * n_in - n_out, 0)                  # s = max(0, num / den)
    q, r = num // den, num % den
    i0 = np.minimum(q, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    a, b = seg[..., i0], seg[..., i1]
    return a + (r.astype(np.float64) / float(den)) * (b - a)


def warp(x, c, wp, Tb):
    """x [K, T] float64 -> the warped clip; frames >= Tb are kept."""
    y = np.array(x, dtype=np.float64)
    y[:, :wp] = resize(x[:, :c], wp)
    y[:, wp:Tb] = resize(x[:, c:Tb], Tb - wp)
    return y


def mask_of(d, K, T, Tb):
    """bool [K, T]: the union of the clip's masks (inside [0, Tb) only)."""
    m = np.zeros((K, T), dtype=bool)
    for f, f0 in zip(d["f"], d["f0"]):
        m[f0:f0 + f, :Tb] = True
    for t, t0 in zip(d["t"], d["t0"]):
        m[:, t0:t0 + t] = True
    return m


def clip_mean(x, Tb):
    return float(np.mean(np.asarray(x, dtype=np.float64)[:, :Tb]))


def apply(x, seed, first_row=0, nf=2, F=27, nt=2, Wt=100, p=1.0, W=0, mask_value=0.0, lengths=None):
    """x [B, K, T] -> (y float64 [B, K, T], mask bool [B, K, T], the clips' draws)."""
    x = np.asarray(x, dtype=np.float64)
    B, K, T = x.shape
    lengths = [T] * B if lengths is None else [int(v) for v in lengths]
    ds = draws(seed, first_row, B, K, T, lengths, nf, F, nt, Wt, p, W)
    y = x.copy()
    masks = np.zeros(x.shape, dtype=bool)
    for b, d in enumerate(ds):
        Tb = lengths[b]
        if d["c"] >= 0:
            y[b] = warp(x[b], d["c"], d["w"], Tb)
        masks[b] = mask_of(d, K, T, Tb)
        value = clip_mean(x[b], Tb) if isinstance(mask_value, str) else float(mask_value)
        y[b][masks[b]] = value
    return y, masks, ds


def stack_params(ds, key):
    return np.array([d[key] for d in ds], dtype=np.int64).reshape(len(ds), -1)
