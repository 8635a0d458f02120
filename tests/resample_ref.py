"""float64 restatement of scipy.signal.resample_poly in the index form the device uses (tests/test_resample_ref.py holds it
to scipy within 1e-12 of the peak):
    t = (n + n_pre_remove) down,  p = t mod up,  q = t div up,   y[n] = sum_{j < Kp} tab[p][j] x~[q - j].
Written from scipy's documented arithmetic, independent of sygnals_amd/_resample.py (n_post_pad is found by scipy's own
loop here, in closed form there)."""
from math import gcd

import numpy as np
from scipy.signal import firwin

SERVED = ("constant", "mean", "minimum", "maximum", "edge", "wrap", "symmetric", "reflect")


def plan(L, up, down, window=("kaiser", 5.0)):
    """(up, down, n_out, n_pre_remove, Kp, tab [up, Kp] float64) with up / down reduced."""
    g = gcd(up, down)
    up, down = up // g, down // g
    n_out = -(-(L * up) // down)
    if isinstance(window, (list, np.ndarray)):
        h = np.array(window, dtype=np.float64)
        half_len = (h.size - 1) // 2
    else:
        half_len = 10 * max(up, down)
        h = firwin(2 * half_len + 1, 1.0 / max(up, down), window=window)
    h = h * up
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    n_post_pad = 0
    while ((L - 1) * up + h.size + n_pre_pad + n_post_pad - 1) // down + 1 < n_out + n_pre_remove:
        n_post_pad += 1
    hp = np.concatenate([np.zeros(n_pre_pad), h, np.zeros(n_post_pad)])
    Kp = -(-hp.size // up)
    tab = np.zeros((up, Kp))
    for p in range(up):
        v = hp[p::up]
        tab[p, :v.size] = v
    return up, down, n_out, n_pre_remove, Kp, tab


def pad_index(i, L, padtype):
    """Index map of the pad rule: (index into x, inside?) for integer positions i of any sign and size."""
    i = np.asarray(i, dtype=np.int64)
    inside = (i >= 0) & (i < L)
    if padtype == "edge":
        m = np.clip(i, 0, L - 1)
    elif padtype == "wrap":
        m = np.mod(i, L)
    elif padtype == "symmetric":
        m = np.mod(i, 2 * L)
        m = np.where(m < L, m, 2 * L - 1 - m)
    elif padtype == "reflect":
        m = np.mod(i, 2 * L - 2)
        m = np.where(m < L, m, 2 * L - 2 - m)
    else:
        m = np.clip(i, 0, L - 1)
    return m, inside


def resample_poly(x, up, down, window=("kaiser", 5.0), padtype="constant", cval=None):
    x = np.asarray(x, dtype=np.float64)
    L = x.size
    if padtype not in SERVED:
        raise ValueError(padtype)
    if padtype == "reflect" and L < 2:
        raise ValueError("reflect needs two samples")
    if up == down:
        return x.copy()
    up, down, n_out, npr, Kp, tab = plan(L, up, down, window)
    back = 0.0
    if padtype in ("mean", "minimum", "maximum"):
        back = {"mean": np.mean, "minimum": np.amin, "maximum": np.amax}[padtype](x)
        x, padtype, cval = x - back, "constant", 0.0
    fill = 0.0 if cval is None else float(cval)
    t = (np.arange(n_out, dtype=np.int64) + npr) * down
    p, q = t % up, t // up
    y = np.zeros(n_out)
    for j in range(Kp):
        m, inside = pad_index(q - j, L, padtype)
        v = x[m]
        if padtype == "constant":
            v = np.where(inside, v, fill)
        y += tab[p, j] * v
    return y + back
