"""NumPy walk of syg_laplace_f32's arithmetic from the host tables alone (sygnals_amd/_laplace.plan / anchors): the
float32 chunk contraction, the float64 Horner over tiles and segments, the reversed rows, the steep recurrence.  It pins
what the tables MEAN on a machine without a device; the kernel's own lane maps are tested on the GPU."""
import numpy as np


def run(x, p, anchor, t_step, C, tile_rows, segment, steep, segmented):
    x = np.asarray(x, dtype=np.float32)
    L = x.size
    K = -(-L // C)
    out = np.full(p.S, np.nan, dtype=np.complex128)
    fac = p.fac.reshape(p.fac.shape[0], -1, 2)
    fac = fac[..., 0] + 1j * fac[..., 1]                             # [Sc, 19]: Z^0..15, Z^16, Z^seg, z
    anc = anchor[:, 0] + 1j * anchor[:, 1]
    seg_ch = segment // C if segmented else K
    for c in range(p.S16):
        rev = c >= p.S_fwd
        tab = p.table[:, 0, c].astype(np.float32), p.table[:, 1, c].astype(np.float32)
        pad = np.zeros(K * C, dtype=np.float32)
        if rev:
            pad[K * C - L:] = x                                      # end-aligned grid: chunk k is pad[(K-1-k)C : (K-k)C]
            chunks = pad.reshape(K, C)[::-1]
        else:
            pad[:L] = x
            chunks = pad.reshape(K, C)
        P = (chunks @ tab[0]).astype(np.float64) + 1j * (chunks @ tab[1]).astype(np.float64)      # [K]
        segs = []
        for k_lo in range(0, K, seg_ch):
            k_hi = min(K, k_lo + seg_ch)
            h = 0j
            for k0 in range(k_lo + ((k_hi - k_lo - 1) // tile_rows) * tile_rows, k_lo - 1, -tile_rows):
                r = np.arange(min(tile_rows, k_hi - k0))
                h = h * fac[c, 16] + np.sum(fac[c, r] * P[k0 + r])
            segs.append(h)
        h = 0j
        for v in segs[::-1]:
            h = h * fac[c, 17] + v
        if p.col[c] >= 0:
            out[p.col[c]] = t_step * (anc[c] * h)
    for c in range(p.S16, p.col.size):
        xs = (x[::-1] if p.rev[c] else x)[:steep].astype(np.float64)
        e = np.cumprod(np.concatenate([[1.0 + 0j], np.full(max(xs.size - 1, 0), fac[c, 18])]))[:xs.size]   # the recurrence
        h = np.sum(xs * e)
        out[p.col[c]] = t_step * (anc[c] * h)
    return out
