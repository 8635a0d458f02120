"""NumPy lane/register model of the wave FFT of stft_mel.hip with lane-indexed exchanges (ds_write_addtid_b32:
every store writes one 64-float row, float L from lane L; re and im are separate rows).  Checks the index maps
against np.fft.rfft and the bank behaviour of every LDS access of the transform under the per-instruction banking
of MI355X_MICROARCH.md (ds_read_b64: 32-lane groups on 64 banks; ds_write_b32: 32-lane groups on 32 banks, where
2-way costs nothing).  Development aid only; tools/wave_fft_model_v4.py is the model of the row-store exchanges.

Maps (see wave_rfft2048):
  pass 1   lane l holds column b = sig(l) = 4 (l & 15) + bp, bp = (l >> 4) ^ ((l >> 2) & 2)
  exch. 1  row r of round h, plane p at float X1_ROW r + 64 p (skew of one 8-byte slot per row); lane (c7, bp, hi)
           reads slot i of its half: floats 2 (4 hi + i) + 16 (bp ^ 2 hi) of row c7
  pass 2   lane L = 32 hi + 16 (bp >> 1) + 2 rho + (bp & 1), c = 8 hi + c7, rho = ((c7 & 3) << 1) | (c7 >> 2)
  exch. 2  row r (c' & 7), plane p at float X2_ROW r + 64 p; group (c, c') read as the lane pairs (bp 0, 1), (2, 3)
  units    u = lane + 64 j: c = UNIT_C[(u >> 3)], c' = u & 7 -- each 32-lane group holds a set of c closed under the
           mirror c -> 16 - c and under c -> c + 8
"""
import numpy as np

M = 1024
X1_ROW, X2_ROW = 130, 132
UNIT_C = [0, 4, 8, 12, 1, 7, 9, 15, 2, 6, 10, 14, 3, 5, 11, 13]


def W(N, e):
    return np.exp(-2j * np.pi * e / N)


def sig(l):
    return 4 * (l & 15) + ((l >> 4) ^ ((l >> 2) & 2))


def p2(L):
    """pass-2 lane -> (c, bp)"""
    hi, rho = L >> 5, (L >> 1) & 7
    c7 = (rho >> 1) | ((rho & 1) << 2)
    return 8 * hi + c7, ((L >> 3) & 2) | (L & 1)


def unit(u):
    c, cp = UNIT_C[u >> 3], u & 7
    if c != 0:
        return c, cp, 16 - c, 15 - cp
    if cp != 0:
        return 0, cp, 0, 16 - cp
    return 0, 0, 0, 8


def rho_of(c7):
    return ((c7 & 3) << 1) | (c7 >> 2)


lane = np.arange(64)


def model(x, win):
    xw = x * win
    z = xw[0::2] + 1j * xw[1::2]
    s = sig(lane)
    v = np.stack([z[64 * a + s] for a in range(16)], 0)
    y = np.stack([sum(v[a] * W(16, a * c) for a in range(16)) for c in range(16)], 0)
    y = y * np.stack([W(1024, s * c) for c in range(16)], 0)
    c2, bp = p2(lane)
    c7, hi = c2 & 7, lane >> 5
    base1 = X1_ROW * c7 + 8 * hi + 16 * (bp ^ (2 * hi))
    tt = np.zeros((2, 8, 64), complex)
    for h in (0, 1):
        buf = np.full(1056, np.nan)
        for r in range(8):
            buf[X1_ROW * r + lane] = y[8 * h + r].real
            buf[X1_ROW * r + 64 + lane] = y[8 * h + r].imag
        for i in range(4):
            for e in (0, 1):
                tt[h, 2 * i + e] = buf[base1 + 2 * i + e] + 1j * buf[base1 + 64 + 2 * i + e]
    for i in range(8):
        a0, a1 = tt[0, i].copy(), tt[1, i].copy()
        tt[0, i, 32:] = a1[:32]
        tt[1, i, :32] = a0[32:]
    u_ = np.concatenate([tt[0], tt[1]], 0)
    # reader lane (c, bp) must now hold y[c][4 a + bp] in u_[a]
    for a in range(16):
        assert np.allclose(u_[a], y[c2, [list(s).index(4 * a + b) for b in bp]]), a
    t = np.stack([sum(u_[a] * W(16, a * cp) for a in range(16)) for cp in range(16)], 0)
    t = t * np.stack([W(64, bp * cp) for cp in range(16)], 0)
    G = np.zeros((2, 4, 64), complex); H = np.zeros((2, 4, 64), complex)
    for h in (0, 1):
        buf = np.full(1056, np.nan)
        for r in range(8):
            buf[X2_ROW * r + lane] = t[8 * h + r].real
            buf[X2_ROW * r + 64 + lane] = t[8 * h + r].imag
        for j in (0, 1):
            for l in range(64):
                c, cp, cm, cmp_ = unit(l + 64 * j)
                gc, gcp = (c, cp) if h == 0 else (cm, cmp_)
                a = X2_ROW * (gcp & 7) + 32 * (gc >> 3) + 2 * rho_of(gc & 7)
                for b in range(4):
                    f = a + 16 * (b >> 1) + (b & 1)
                    val = buf[f] + 1j * buf[f + 64]
                    (G if h == 0 else H)[j, b, l] = val
    X = np.full(1025, np.nan + 0j)
    for j in (0, 1):
        for l in range(64):
            u = l + 64 * j
            c, cp, cm, cmp_ = unit(u)
            g = np.array([sum(G[j, b, l] * W(4, b * d) for b in range(4)) for d in range(4)])
            hh = np.array([sum(H[j, b, l] * W(4, b * d) for b in range(4)) for d in range(4)])
            k = c + 16 * cp + 256 * np.arange(4)
            if u == 0:
                pairs = [(g[0], g[0], 0), (g[1], g[3], 256), (hh[0], hh[3], 128), (hh[1], hh[2], 384), (g[2], g[2], 512)]
            else:
                km = cm + 16 * cmp_ + 256 * np.arange(4)
                assert all((k[d] + km[3 - d]) % 1024 == 0 for d in range(4))
                pairs = [(g[d], hh[3 - d], k[d]) for d in range(4)]
            for zk, zm, kk in pairs:
                E = 0.5 * (zk + np.conj(zm)); O = -0.5j * (zk - np.conj(zm))
                w = np.exp(-1j * np.pi * kk / M)
                X[kk] = E + w * O
                X[M - kk] = np.conj(E - w * O)
    return X


def worst(addr_floats, width_floats, modfloats):
    """largest number of distinct addresses on one bank slot, over the two 32-lane groups"""
    out = 0
    for g in (lane[:32], lane[32:]):
        a = np.unique(addr_floats[g])
        out = max(out, np.bincount((a // width_floats) % (modfloats // width_floats)).max())
    return out


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    x = rng.normal(size=2048)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(2048) / 2048)
    X = model(x, win)
    print("max err", np.abs(X - np.fft.rfft(x * win)).max(), "nan:", np.isnan(X).any())
    s = sig(lane)
    assert sorted(s) == list(range(64))
    print("stage / window / tw1 reads (b64):", worst(2 * (64 * 3 + s), 2, 64))
    c2, bp = p2(lane)
    assert sorted(zip(c2, bp)) == [(c, b) for c in range(16) for b in range(4)]
    assert all(c2[l + 32] == c2[l] + 8 and bp[l + 32] == bp[l] for l in range(32))
    c7, hi = c2 & 7, lane >> 5
    base1 = X1_ROW * c7 + 8 * hi + 16 * (bp ^ (2 * hi))
    print("x1 reads:", [worst(base1 + 2 * i + 64 * p, 2, 64) for i in range(4) for p in (0, 1)])
    for j in (0, 1):
        for h in (0, 1):
            a = []
            for l in lane:
                c, cp, cm, cmp_ = unit(l + 64 * j)
                gc, gcp = (c, cp) if h == 0 else (cm, cmp_)
                a.append(X2_ROW * (gcp & 7) + 32 * (gc >> 3) + 2 * rho_of(gc & 7))
            a = np.array(a)
            print(f"x2 reads j{j} h{h}:", [worst(a + 16 * k + 64 * p, 2, 64) for k in (0, 1) for p in (0, 1)])
    def pos(k): return k + (k >> 4)
    for j in (0, 1):
        res = []
        for d in range(4):
            kk = []
            for l in lane:
                c, cp, cm, cmp_ = unit(l + 64 * j); k = c + 16 * cp + 256 * d
                if l + 64 * j == 0: k = [0, 256, 128, 384][d]
                kk.append(k)
            kk = np.array(kk)
            res.append((worst(pos(kk), 1, 32), worst(pos(1024 - kk), 1, 32)))
        print("power-row stores (b32, 2-way free) unit", j, res)
