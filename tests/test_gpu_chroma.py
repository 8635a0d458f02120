"""The tonal kernels on the device (syg_chroma_fold_rows_f32, syg_chroma_fold_bins_f32, syg_chroma_cens_f32,
syg_tuning_hist_f32) and the chains over them against the float64 restatement of tests/chroma_ref.py.

G1 (folds) and G2 (CENS) are 1e-5 gates on crafted input, the restatement fed the same float32 numbers.  G3 (tuning) is
exact: counts, peak count and tuning, on inputs whose every decision has a relative margin of at least 1e-9 in float64.
G4 (end to end) is gated at the larger of 1e-5 and twice the floor: what the restatement itself moves by when it is fed the
device's own STFT / CQT in place of the oracle's.  Every device call writes into a NaN-filled `out`; every test prints its
worst fraction of its gate.  Worst figures measured on MI355X: see README.md, "Chroma, CENS, tonnetz and tuning"."""
import warnings

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from sygnals_amd import _chroma as CH
from sygnals_amd import ops
from sygnals_amd.core.features import tonal as TN
from tests import chroma_cases as K
from tests import chroma_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
WORST = {}


def _note(key, frac):
    WORST[key] = max(WORST.get(key, 0.0), float(frac))
    print(f"{key}: fraction of the gate {float(frac):.3e}, worst so far {WORST[key]:.3e}")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _power(x, cplx, power):
    """float64 |x|^power of an interleaved complex float32 array, or the real array itself."""
    x = x.astype(np.float64)
    if not cplx:
        return x
    p = x[..., 0] ** 2 + x[..., 1] ** 2
    return p if power == 2 else np.sqrt(p)


def _gate_frames(got, ref, raw, norm, key, what):
    """got, ref [n, T]; raw: the unnormalised reference.  |got - ref| <= 1e-5 of the frame's own norm (1 after normalising;
    the raw maximum without a norm)."""
    assert np.isfinite(got).all(), what
    scale = np.ones(ref.shape[-1]) if norm is not None else np.max(np.abs(raw), axis=0)
    err = np.max(np.abs(got - ref), axis=0)
    frac = np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1) / TOL, np.where(err > 0, np.inf, 0)))
    _note(key, frac)
    assert frac <= 1.0, f"{what}: {frac:.3e} of the gate"


def _fold_rows(x, tab, cplx, power, norm, threshold=None):
    B, T = x.shape[:2]
    out = _nan(B, tab.shape[0], T)
    got = ops.chroma_fold(_dev(x), tab, "rows", power, threshold, norm, out=out)
    assert got is out
    return got.cpu().numpy()


def _ref_fold(P, tab, norm, threshold=None):
    """P float64 [cols, T] in librosa's layout -> (normalised, raw)."""
    raw = tab.astype(np.float64) @ P
    if threshold is not None:
        raw = np.where(raw < threshold, 0.0, raw)
    return R.normalize(raw, norm, axis=0), raw


# ----------------------------------------------------------------------------------------------------- G1: frame-major fold
@pytest.mark.parametrize("cplx", [False, True])
def test_fold_rows_sizes(cplx):
    for F in K.ROWS_F:
        tab = R.filters_chroma(22050, 2 * (F - 1))
        for i, T in enumerate(K.ROWS_T):
            x = K.complex_pairs((2, T, F), 31 * F + T) if cplx else K.positive((2, T, F), 31 * F + T)
            norm, power = K.NORMS[i % 4], 1 + (i + F) % 2
            got = _fold_rows(x, tab, cplx, power, norm)
            for b in range(2):
                ref, raw = _ref_fold(_power(x[b], cplx, power).T, tab, norm)
                _gate_frames(got[b], ref, raw, norm, "G1 rows", f"fold_rows F={F} T={T} cplx={cplx} norm={norm}")


@pytest.mark.parametrize("nc,F", K.ROWS_TABLES)
def test_fold_rows_tables_and_norms(nc, F):
    tab = R.filters_chroma(16000, 2 * (F - 1), n_chroma=nc, tuning=0.2) if nc % 12 == 0 else K.positive((nc, F), nc * F, lo=0.0)
    x = K.positive((1, 33, F), F + nc)
    for norm in K.NORMS:
        got = _fold_rows(x, tab, False, 2, norm)
        ref, raw = _ref_fold(x[0].astype(np.float64).T, tab, norm)
        _gate_frames(got[0], ref, raw, norm, "G1 rows", f"fold_rows table {nc} x {F} norm={norm}")
    assert np.array_equal(_fold_rows(x, _dev(tab), False, 2, np.inf), _fold_rows(x, tab, False, 2, np.inf))     # a device table


def test_fold_rows_batch_equals_rows_and_repeats():
    tab = R.filters_chroma(22050, 256)
    x = K.complex_pairs((33, 65, 129), 5)
    full = _fold_rows(x, tab, True, 2, np.inf)
    assert np.array_equal(full, _fold_rows(x, tab, True, 2, np.inf))
    assert np.array_equal(full[:3], _fold_rows(x[:3], tab, True, 2, np.inf))
    for b in (0, 1, 16, 32):
        assert np.array_equal(full[b:b + 1], _fold_rows(x[b:b + 1], tab, True, 2, np.inf))


def test_fold_rows_threshold_and_edge_frames():
    F, nc = 129, 12
    tab = np.zeros((nc, F), dtype=np.float32)
    tab[np.arange(nc), 5 * np.arange(nc) + 3] = 1.0                              # one bin a row: every sum is exact
    x = np.zeros((1, 6, F), dtype=np.float32)
    thr = np.float32(0.375)
    x[0, 0, 5 * np.arange(nc) + 3] = np.where(np.arange(nc) % 2 == 0, thr, np.nextafter(thr, np.float32(0)))
    x[0, 1, 5 * np.arange(nc) + 3] = 0.25                                        # every entry below the threshold
    x[0, 3, 5 * np.arange(nc) + 3] = (np.arange(nc) + 1) * np.float32(1e-40)     # a frame below float32 tiny in every norm
    x[0, 4, 5 * np.arange(nc) + 3] = np.arange(nc) + 1.0
    x[0, 5, 10] = 7.0                                                            # energy that no row takes
    for norm in K.NORMS:
        got = _fold_rows(x, tab, False, 2, norm, threshold=float(thr))[0]
        keep = np.where(np.arange(nc) % 2 == 0, thr, 0.0)
        assert np.array_equal(got[:, 0] != 0, keep != 0), "entries equal to the threshold stay, those below go"
        assert not got[:, 1].any() and not got[:, 2].any() and not got[:, 5].any() and np.isfinite(got).all()
        plain = _fold_rows(x, tab, False, 2, norm)[0]
        assert np.array_equal(plain[:, 3], x[0, 3, 5 * np.arange(nc) + 3]), "below tiny: returned unnormalised, exactly"
        assert not plain[:, 2].any()
        ref, raw = _ref_fold(x[0].astype(np.float64).T, tab, norm)
        _gate_frames(plain[:, [0, 1, 4]], ref[:, [0, 1, 4]], raw[:, [0, 1, 4]], norm, "G1 rows", f"edge frames norm={norm}")


# ------------------------------------------------------------------------------------------------------- G1: bin-major fold
def _fold_bins(x, tab, power, norm, threshold=None, transform=None, strided=False):
    """x [B, Kb, T(, 2)] host array; strided: rows inside a larger allocation whose row and batch strides are odd numbers of
    floats for a real input (a complex input's strides are pairs of floats, so even, with an odd number of pairs)."""
    B, Kb, T = x.shape[:3]
    d = _dev(x)
    if strided:
        tail = x.shape[3:]
        Tp = T + 1 + T % 2                                                       # odd
        Kp = Kb + 1 + Kb % 2                                                     # odd: the batch stride Kp Tp is odd too
        big = torch.zeros((B, Kp, Tp) + tail, dtype=torch.float32, device="cuda")
        big[:, :Kb, :T] = d
        d = big[:, :Kb, :T]
        assert not d.is_contiguous() and (d.stride(1) // (2 if tail else 1)) % 2 == 1 and (d.stride(0) // (2 if tail else 1)) % 2 == 1
    rows = tab.shape[0] if transform is None else transform.shape[0]
    out = _nan(B, rows, T)
    got = ops.chroma_fold(d, tab, "bins", power, threshold, norm, transform, out=out)
    assert got is out
    return got.cpu().numpy()


@pytest.mark.parametrize("Kb,bpo,nc,window", K.BINS_TABLES)
def test_fold_bins_sizes(Kb, bpo, nc, window):
    tab = R.cq_to_chroma(Kb, bpo, nc, window=None if window is None else np.array(window)).astype(np.float32)
    for i, T in enumerate(K.BINS_T):
        cplx = i % 2 == 0
        x = K.complex_pairs((2, Kb, T), Kb + T) if cplx else K.positive((2, Kb, T), Kb + T)
        norm, power = K.NORMS[(i + nc) % 4], 1 + i % 2
        got = _fold_bins(x, tab, power, norm, threshold=0.0, strided=i != 2)       # odd strides: real input at T = 63 and 65, complex at 1 and 1000
        for b in range(2):
            ref, raw = _ref_fold(_power(x[b], cplx, power), tab, norm, 0.0)
            _gate_frames(got[b], ref, raw, norm, "G1 bins", f"fold_bins K={Kb} nc={nc} T={T} cplx={cplx} norm={norm}")


def test_fold_bins_every_norm_batches_and_repeats():
    tab = R.cq_to_chroma(252, 36, 12)
    x = K.complex_pairs((33, 252, 65), 11)
    for norm in K.NORMS:
        got = _fold_bins(x[:2], tab, 1, norm, threshold=0.0)
        ref, raw = _ref_fold(_power(x[1], True, 1), tab, norm, 0.0)
        _gate_frames(got[1], ref, raw, norm, "G1 bins", f"fold_bins norm={norm}")
    full = _fold_bins(x, tab, 1, np.inf, 0.0)
    assert np.array_equal(full, _fold_bins(x, tab, 1, np.inf, 0.0))
    assert np.array_equal(full[:3], _fold_bins(x[:3], tab, 1, np.inf, 0.0))
    assert np.array_equal(full, _fold_bins(x, tab, 1, np.inf, 0.0, strided=True))
    for b in (0, 7, 32):
        assert np.array_equal(full[b:b + 1], _fold_bins(x[b:b + 1], tab, 1, np.inf, 0.0))


def test_fold_bins_threshold_identity_and_edge_frames():
    nc = 12
    eye = np.eye(nc, dtype=np.float32)
    thr = np.float32(0.375)
    x = np.zeros((1, nc, 5), dtype=np.float32)
    x[0, :, 0] = np.where(np.arange(nc) % 2 == 0, thr, np.nextafter(thr, np.float32(0)))
    x[0, :, 1] = 0.25
    x[0, :, 3] = (np.arange(nc) + 1) * np.float32(1e-40)
    x[0, :, 4] = np.arange(nc) + 1.0
    for norm in K.NORMS:
        got = _fold_bins(x, eye, 1, norm, threshold=float(thr))[0]
        assert np.array_equal(got[:, 0] != 0, np.arange(nc) % 2 == 0), "entries equal to the threshold stay, those below go"
        assert not got[:, 1].any() and not got[:, 2].any() and np.isfinite(got).all()
        plain = _fold_bins(x, eye, 1, norm)[0]
        assert np.array_equal(plain[:, 3], x[0, :, 3]) and not plain[:, 2].any()
        ref, raw = _ref_fold(x[0].astype(np.float64), eye, norm)
        _gate_frames(plain[:, [0, 1, 4]], ref[:, [0, 1, 4]], raw[:, [0, 1, 4]], norm, "G1 bins", f"identity fold norm={norm}")
    assert np.array_equal(_fold_bins(x, eye, 1, None)[0], x[0]), "the identity fold without a norm is a copy"


@pytest.mark.parametrize("nc", [12, 24, 36])
def test_fold_bins_tonnetz_transform(nc):
    phi = CH.tonnetz_phi(nc)
    ch = K.positive((3, nc, 130), nc)
    ch[1, :, 7] = 0.0
    got = _fold_bins(ch, np.eye(nc, dtype=np.float32), 1, None, transform=phi)
    for b in range(3):
        ref = phi.astype(np.float64) @ R.normalize(ch[b].astype(np.float64), 1, axis=0)
        _gate_frames(got[b], ref, ref, 1, "G1 tonnetz", f"tonnetz transform nc={nc}")
        assert np.max(np.abs(ref - R.tonnetz(ch[b]))) < 1e-6                     # (float32 phi against the float64 one)
    assert not got[1, :, 7].any()
    tab = R.cq_to_chroma(36 * 3, 36, nc) if 36 % nc == 0 else R.cq_to_chroma(72 * 2, 72, nc)
    C = K.complex_pairs((2, tab.shape[1], 70), 3)
    got = _fold_bins(C, tab, 1, np.inf, threshold=0.0, transform=phi)
    for b in range(2):
        chroma, _ = _ref_fold(_power(C[b], True, 1), tab, np.inf, 0.0)
        ref = phi.astype(np.float64) @ R.normalize(chroma, 1, axis=0)
        _gate_frames(got[b], ref, ref, 1, "G1 tonnetz", f"tonnetz after the fold nc={nc}")


# ------------------------------------------------------------------------------------------------------------------ G2: CENS
def test_cens_windows_and_lengths():
    tile = ops.chroma_constants()["cens_tile"]
    for T in K.cens_T(tile):
        ch = np.stack([K.cens_chroma(12, T, 7 * T + b) for b in range(2)])
        for b in range(2):
            live = ch[b][:, ch[b].any(axis=0)]
            assert live.size == 0 or R.cens_margin(live) >= 1e-4
        d = _dev(ch)
        for wl in K.CENS_WIN:
            out = _nan(2, 12, T)
            got = ops.chroma_cens(d, wl, "hann", out=out)
            assert got is out and np.isfinite(got.cpu().numpy()).all()
            for b in range(2):
                ref = R.cens_from_chroma(ch[b], 2, wl, "hann")
                err = np.max(np.abs(got[b].cpu().numpy() - ref))
                _note("G2 cens", err / TOL)
                assert err <= TOL, f"cens T={T} win_len_smooth={wl}"


@pytest.mark.parametrize("name", K.CENS_WINDOWS)
def test_cens_window_names_norms_and_strides(name):
    T, nc = 300, 24
    ch = np.stack([K.cens_chroma(nc, T, 100 + b) for b in range(3)])
    big = torch.zeros((3, nc + 2, T + 5), dtype=torch.float32, device="cuda")
    big[:, :nc, :T] = _dev(ch)
    for wl in (2, 41):
        for norm in (2, 1, np.inf, None):
            got = ops.chroma_cens(big[:, :nc, :T], wl, name, norm, out=_nan(3, nc, T)).cpu().numpy()
            assert np.array_equal(got, ops.chroma_cens(_dev(ch), wl, name, norm).cpu().numpy())
            assert np.array_equal(got[1:2], ops.chroma_cens(_dev(ch[1:2]), wl, name, norm).cpu().numpy())
            for b in range(3):
                ref = R.cens_from_chroma(ch[b], norm, wl, name)
                scale = 1.0 if norm is not None else max(np.max(np.abs(ref)), 1e-30)
                err = np.max(np.abs(got[b] - ref)) / scale
                _note("G2 cens", err / TOL)
                assert err <= TOL, f"cens window={name} win_len_smooth={wl} norm={norm}"


# ---------------------------------------------------------------------------------------------------- G3: tuning histogram
SR, NFFT, F = 22050, 2048, 1025
K_LO, K_HI = 14, 372                                                            # 150 Hz <= k sr / n_fft < 4000 Hz


def _tuning_case(S_list, bpo=12, resolution=0.01):
    """S_list: float32 [F, T] magnitude spectrograms, one per clip (librosa's layout).  The restatement's decisions are
    checked for their margins, then counts, peak count and tuning must be the restatement's exactly."""
    want = []
    for S in S_list:
        d = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = R.estimate_tuning(S, SR, NFFT, resolution, bpo, detail=d)
        assert d["worst_margin"] >= 1e-9, f"a decision of the restatement has a margin of {d['worst_margin']:.2e}"
        want.append((t, d))
    X = _dev(np.stack([S.T for S in S_list]))
    B, nb = len(S_list), int(np.ceil(1.0 / resolution))
    counts = torch.full((B, nb), -1, dtype=torch.int32, device="cuda")
    npk = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    c, n = ops.tuning_hist(X, SR, NFFT, 1, resolution=resolution, bins_per_octave=bpo, out=(counts, npk))
    assert c is counts and n is npk
    c, n = c.cpu().numpy(), n.cpu().numpy()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tun = ops.estimate_tuning(X, SR, NFFT, 1, resolution, bpo)
    for b, (t, d) in enumerate(want):
        assert n[b] == d["n_peaks"] and np.array_equal(c[b], d["counts"]), f"clip {b}: {n[b]} peaks against {d['n_peaks']}"
        assert tun[b] == t
    if any(d["n_peaks"] == 0 for _, d in want):
        assert any("empty frequency set" in str(m.message) for m in w)
    _note("G3 tuning (exact)", 0.0)
    return want


def test_tuning_no_peak_one_peak_even_and_odd():
    zero = np.zeros((F, 3), dtype=np.float32)
    one = K.bumps(F, 1, [(100.3, 1.0)], 1)
    odd = K.bumps(F, 1, [(100.3, 1.0), (150.6, 0.7), (220.1, 0.5)], 2)
    even = K.bumps(F, 2, [(100.3, 1.0), (150.6, 0.7), (220.1, 0.5), (301.4, 0.8)], 3)
    for S in (zero, one, odd, even):
        want = _tuning_case([S])
    assert want[0][1]["n_peaks"] == 8
    got = _tuning_case([zero[:, :2], even, one.repeat(2, axis=1), odd.repeat(2, axis=1)])        # clips that differ in peak count
    assert [d["n_peaks"] for _, d in got] == [0, 8, 2, 6]


def test_tuning_first_and_last_admissible_bin():
    S = K.bumps(F, 2, [(K_LO + 0.2, 1.0), (K_HI - 1.2, 0.9), (5.0, 2.0), (K_HI + 6.3, 1.5), (600.0, 3.0)], 4)
    (t, d), = _tuning_case([S])
    p, _ = R.piptrack(S, SR, NFFT)
    ks = sorted(set(np.nonzero(p)[0].tolist()))
    assert ks == [K_LO, K_HI - 1] and d["n_peaks"] == 4


@pytest.mark.parametrize("bpo,resolution", [(12, 0.01), (36, 0.01), (12, 0.05), (36, 0.05)])
def test_tuning_many_frames(bpo, resolution):
    peaks = [(30.4 + 17.3 * i, 1.0 / (1 + 0.37 * i)) for i in range(12)]
    for T in (1, 2, 65):
        _tuning_case([K.bumps(F, T, peaks, T), K.bumps(F, T, peaks[:5], T + 1)], bpo=bpo, resolution=resolution)


@pytest.mark.parametrize("power", [1, 2])
def test_tuning_complex_input(power):
    """The complex STFT with |X|^power on load: the restatement is fed S as the device itself forms it (cabs_pow)."""
    peaks = [(30.4 + 17.3 * i, 1.0 / (1 + 0.37 * i)) for i in range(9)]
    mag = np.stack([K.bumps(F, 5, peaks, 9 + b).T for b in range(2)]).astype(np.float64)      # [B, T, F]
    ph = np.random.default_rng(1).uniform(0, 2 * np.pi, mag.shape)
    X = _dev(np.stack([mag * np.cos(ph), mag * np.sin(ph)], axis=-1).astype(np.float32))
    S = ops.cabs_pow(X, power).cpu().numpy()
    want = []
    for b in range(2):
        d = {}
        t = R.estimate_tuning(S[b].T, SR, NFFT, detail=d)
        assert d["worst_margin"] >= 1e-9
        want.append((t, d))
    counts = torch.full((2, 100), -1, dtype=torch.int32, device="cuda")
    npk = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    c, n = ops.tuning_hist(X, SR, NFFT, power, out=(counts, npk))
    tun = ops.estimate_tuning(X, SR, NFFT, power)
    for b, (t, d) in enumerate(want):
        assert int(n[b]) == d["n_peaks"] and np.array_equal(c[b].cpu().numpy(), d["counts"]) and tun[b] == t
    assert np.array_equal(c.cpu().numpy(), ops.tuning_hist(_dev(S), SR, NFFT)[0].cpu().numpy())
    _note("G3 tuning (exact)", 0.0)


def test_piptrack_dense_pair():
    S = K.bumps(F, 3, [(100.3, 1.0), (150.6, 0.7), (220.1, 0.5), (5.0, 2.0)], 12)
    p_ref, m_ref = R.piptrack(S, SR, NFFT)
    pitch, mag = ops.piptrack(_dev(S.T[None]), SR, NFFT, out=(_nan(1, 3, F), _nan(1, 3, F)))
    pitch, mag = pitch[0].cpu().numpy().T, mag[0].cpu().numpy().T
    assert np.array_equal(pitch != 0, p_ref != 0) and np.array_equal(mag != 0, m_ref != 0)
    # float64 values rounded once to float32: half an ulp, 6e-8 relative; the gate is 2e-7
    for got, ref in ((pitch, p_ref), (mag, m_ref)):
        frac = np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)) / 2e-7
        _note("G3 piptrack", frac)
        assert frac <= 1.0
    pm, mm = TN.piptrack(S=S, sr=SR)
    assert np.array_equal(pm, pitch) and np.array_equal(mm, mag)


# ------------------------------------------------------------------------------------------------------------ G4: end to end
def _gate_e2e(got, ref, floor_ref, key, what):
    """got against ref at max(1e-5, 2 floor), floor = |floor_ref - ref|: what the restatement moves by on the device's own
    transform."""
    floor = float(np.max(np.abs(floor_ref - ref)))
    gate = max(TOL, 2 * floor)
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: device {err:.3e}, floor {floor:.3e}, gate {gate:.3e} ({'1e-5' if gate == TOL else 'twice the floor'} applied)")
    _note(key, err / gate)
    assert np.isfinite(got).all() and err <= gate, what


@pytest.mark.parametrize("sr,L,n_fft,hop,tuning", K.E2E_STFT)
def test_chroma_stft_end_to_end(sr, L, n_fft, hop, tuning):
    y = K.chord(sr, L, cents=100 * tuning, harmonics=2, seed=L)
    S = np.abs(O.stft(y, n_fft, hop)) ** 2
    Xd = ops.stft_any(_dev(y[None]), n_fft, hop)
    Sd = (Xd[0].cpu().numpy().astype(np.float64) ** 2).sum(axis=-1).T
    assert Sd.shape == S.shape
    for norm in (np.inf, 2):
        ref = R.chroma_stft(S, sr, norm, n_fft, tuning)
        got = TN.chroma_stft_batch(_dev(y[None]), sr, None, norm, n_fft, hop, tuning=tuning, out=_nan(1, 12, S.shape[1]))[0].cpu().numpy()
        _gate_e2e(got, ref, R.chroma_stft(Sd, sr, norm, n_fft, tuning), "G4 chroma_stft", f"chroma_stft sr={sr} n_fft={n_fft} norm={norm}")
    one = TN.chroma_stft(y, sr, n_fft=n_fft, hop_length=hop, tuning=tuning)
    assert one.shape == ref.shape and one.dtype == np.float32
    S32 = S.astype(np.float32)
    fromS = TN.chroma_stft(S=S32, sr=sr, n_fft=n_fft, tuning=tuning, norm=2)
    _gate_e2e(fromS, R.chroma_stft(S32, sr, 2, n_fft, tuning), R.chroma_stft(S32, sr, 2, n_fft, tuning), "G4 chroma_stft",
              f"chroma_stft from S sr={sr} n_fft={n_fft}")


@pytest.mark.parametrize("sr,L,tuning", K.E2E_CQT)
def test_chroma_cqt_cens_tonnetz_end_to_end(sr, L, tuning):
    y = K.chord(sr, L, cents=100 * tuning / 3, harmonics=2, seed=L + 1)
    C = np.abs(O.cqt(y, sr, 512, None, 252, 36, tuning=tuning))
    Cd = ops.cqt(_dev(y[None]), sr, 512, None, 252, 36, tuning)
    Cdm = np.sqrt((Cd[0].cpu().numpy().astype(np.float64) ** 2).sum(axis=-1))
    assert Cdm.shape == C.shape
    T = C.shape[1]
    d = _dev(y[None])
    got = TN.chroma_cqt_batch(d, sr, tuning=tuning, out=_nan(1, 12, T))[0].cpu().numpy()
    _gate_e2e(got, R.chroma_cqt(C), R.chroma_cqt(Cdm), "G4 chroma_cqt", f"chroma_cqt sr={sr} L={L}")
    got = TN.chroma_cqt_batch(d, sr, tuning=tuning, norm=2, threshold=None, n_chroma=36)[0].cpu().numpy()
    _gate_e2e(got, R.chroma_cqt(C, 2, None, 36), R.chroma_cqt(Cdm, 2, None, 36), "G4 chroma_cqt", f"chroma_cqt 36 rows sr={sr}")
    got = TN.tonnetz_batch(d, sr, tuning=tuning, out=_nan(1, 6, T))[0].cpu().numpy()
    _gate_e2e(got, R.tonnetz(R.chroma_cqt(C)), R.tonnetz(R.chroma_cqt(Cdm)), "G4 tonnetz", f"tonnetz sr={sr} L={L}")
    assert np.array_equal(TN.tonnetz(y, sr, tuning=tuning), got)
    ch32 = R.chroma_cqt(C).astype(np.float32)
    _gate_e2e(TN.tonnetz(chroma=ch32), R.tonnetz(ch32), R.tonnetz(ch32), "G4 tonnetz", "tonnetz of a given chroma")
    for wl in (41, None):
        got = TN.chroma_cens_batch(d, sr, tuning=tuning, win_len_smooth=wl, out=_nan(1, 12, T))[0].cpu().numpy()
        _gate_e2e(got, R.chroma_cens(C, win_len_smooth=wl), R.chroma_cens(Cdm, win_len_smooth=wl), "G4 chroma_cens",
                  f"chroma_cens sr={sr} L={L} win_len_smooth={wl}")
    C32 = C.astype(np.float32)
    _gate_e2e(TN.chroma_cqt(C=C32), R.chroma_cqt(C32), R.chroma_cqt(C32), "G4 chroma_cqt", "chroma_cqt of a given C")


def _qualifies(S, bpo, what):
    """The issue's two checks on the restatement alone (S float64 [F, T]): the top count leads the runner-up by more than
    twice the fragile decisions, and the float32-rounded S gives the same estimate."""
    d = {}
    t = R.estimate_tuning(S, 22050, 2048, bins_per_octave=bpo, detail=d)
    top = np.sort(d["counts"])[::-1]
    assert top[0] - top[1] > 2 * d["fragile"], f"{what}: counts {top[:3]} with {d['fragile']} fragile decisions do not qualify"
    assert R.estimate_tuning(S.astype(np.float32), 22050, 2048, bins_per_octave=bpo) == t, f"{what}: unstable under float32 rounding"
    return t


@pytest.mark.parametrize("cents,harmonics,seconds", K.E2E_AUTO)
def test_tuning_none_end_to_end(cents, harmonics, seconds):
    sr = 22050
    y = K.chord(sr, seconds * sr, cents=cents, harmonics=harmonics)
    M = np.abs(O.stft(y, 2048, 512))
    t_mag = _qualifies(M, 12, "magnitude, 12 bins")
    t_mag36 = _qualifies(M, 36, "magnitude, 36 bins")
    t_pow = _qualifies(M ** 2, 12, "power, 12 bins")
    assert abs(t_mag - cents / 100.0) <= 0.05
    assert TN.estimate_tuning(y, sr) == t_mag
    assert TN.estimate_tuning(y, sr, bins_per_octave=36) == t_mag36
    ref = R.chroma_stft(M ** 2, sr, np.inf, 2048, None)
    Xd = ops.stft_any(_dev(y[None]), 2048, 512)
    Sd = (Xd[0].cpu().numpy().astype(np.float64) ** 2).sum(axis=-1).T
    got = TN.chroma_stft(y, sr)
    _gate_e2e(got, ref, R.chroma_stft(Sd, sr, np.inf, 2048, t_pow), "G4 tuning=None", f"chroma_stft tuning=None at {cents} cents")
    C = np.abs(O.cqt(y, sr, 512, None, 252, 36, tuning=t_mag36))
    Cd = ops.cqt(_dev(y[None]), sr, 512, None, 252, 36, t_mag36)
    Cdm = np.sqrt((Cd[0].cpu().numpy().astype(np.float64) ** 2).sum(axis=-1))
    _gate_e2e(TN.chroma_cqt(y, sr), R.chroma_cqt(C), R.chroma_cqt(Cdm), "G4 tuning=None", f"chroma_cqt tuning=None at {cents} cents")


def test_tuning_none_groups_clips_by_estimate():
    sr = 22050
    ys = np.stack([K.chord(sr, sr, cents=-35), K.chord(sr, sr, cents=-20, harmonics=3), K.chord(sr, sr, cents=0, harmonics=3),
                   K.chord(sr, sr, cents=-35, seed=1)])
    est = TN.estimate_tuning_batch(ys, sr)
    assert len(set(est.tolist())) == 3 and est[0] == est[3]
    got = TN.chroma_stft_batch(ys, sr, out=_nan(4, 12, 44)).cpu().numpy()
    for b in range(4):
        assert np.array_equal(got[b], TN.chroma_stft(ys[b], sr))
    got = TN.chroma_cqt_batch(ys, sr).cpu().numpy()
    for b in (0, 1):
        assert np.array_equal(got[b], TN.chroma_cqt(ys[b], sr))


# ------------------------------------------------------------------------------------------------------------------ the CLI
def test_features_chroma_round_trip(tmp_path):
    import pandas as pd
    import scipy.io.wavfile
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    sr = 22050
    y = K.chord(sr, sr, cents=0, harmonics=3)
    wav = tmp_path / "a.wav"
    scipy.io.wavfile.write(wav, sr, y)
    run = CliRunner().invoke
    for kind, fn in (("stft", TN.chroma_stft), ("cqt", TN.chroma_cqt), ("cens", TN.chroma_cens), ("tonnetz", TN.tonnetz)):
        want = fn(y, sr)
        r = run(cli, ["features", "chroma", str(wav), "-o", str(tmp_path / f"{kind}.npz"), "--kind", kind])
        assert r.exit_code == 0, r.output
        z = np.load(tmp_path / f"{kind}.npz")
        name = "tonnetz" if kind == "tonnetz" else "chroma"
        assert np.array_equal(z[name], want) and z["time"].shape == (want.shape[1],) and abs(float(z["tuning"])) <= 0.5
        assert np.allclose(z["time"], np.arange(want.shape[1]) * 512 / sr)
        r = run(cli, ["features", "chroma", str(wav), "-o", str(tmp_path / f"{kind}.csv"), "--kind", kind])
        assert r.exit_code == 0, r.output
        t = pd.read_csv(tmp_path / f"{kind}.csv")
        assert list(t.columns) == ["time"] + [f"{name}_{i}" for i in range(want.shape[0])]
        assert np.allclose(t[[f"{name}_{i}" for i in range(want.shape[0])]].to_numpy().T, want, atol=1e-6)
    r = run(cli, ["features", "chroma", str(wav), "-o", str(tmp_path / "g.npz"), "--kind", "cqt", "--tuning", "0.25", "--norm", "2",
                  "--hop-length", "256"])
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "g.npz")
    assert float(z["tuning"]) == 0.25 and np.array_equal(z["chroma"], TN.chroma_cqt(y, sr, hop_length=256, norm=2, tuning=0.25))


def test_dtw_on_chroma_follows_a_shift(tmp_path):
    import scipy.io.wavfile
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    sr, shift = 22050, 4
    y = K.melody(sr, 3 * sr)
    y2 = np.concatenate([K.melody(sr, shift * 512, seed=9) * 0.01, y])[:len(y)].astype(np.float32)
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    scipy.io.wavfile.write(a, sr, y)
    scipy.io.wavfile.write(b, sr, y2)
    r = CliRunner().invoke(cli, ["dsp", "dtw", str(a), str(b), "-o", str(tmp_path / "p.npz"), "--on", "chroma"])
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "p.npz")
    wp = z["path"]
    off = wp[:, 1] - wp[:, 0]
    assert int(z["hop_length"]) == 512 and int(np.median(off)) == shift
    inner = off[(wp[:, 0] > 8) & (wp[:, 1] < wp[:, 1].max() - 8)]
    assert np.mean(inner == shift) >= 0.9, f"{np.mean(inner == shift):.2f} of the path runs parallel to the diagonal"
