"""GPU tests of the HPSS kernels (syg_hpss_masks_f32, syg_istft2048_f32, syg_hnr_rows_f32) on what tests/test_gpu_hpss.py
leaves alone, which feeds them almost only the device STFT of noise or a tone: median windows holding equal values, zeros
and +inf at every size class of the runtime network and at clips far shorter than the window; magnitudes whose squares are
denormal or overflow; the `powf` powers and a single margin above 1 of the soft masks; the inverse STFT of a crafted D
(imaginary parts in the two real bins, fewer or more frames than the length asks, the lengths at which the segment count
steps, more waves than the grid holds); and ops.hnr_rows called directly (uncentred, odd and short frames, a frame longer
than the clip, strided rows, the rms outputs, every class of the +-80 / NaN rule).

Inputs and tables: tests/hpss_cases.py (tests/test_hpss_cases.py holds them to their purpose on the CPU).  The reference is
the float64 restatement of tests/hpss_ref.py; the gates are those of tests/test_gpu_hpss.py (medians bit for bit, masks
1e-6 absolute, audio 1e-5 of the peak) and, for the HNR rows, one float32 spacing of the float64 value, which is what a
float64 sum rounded once promises.  Each group prints its worst figure.

Worst figures measured on MI355X: see README.md, the HNR paragraph."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import hpss_cases as K
from tests import hpss_ref as R
from tests.gpu_util import assert_parity, peak_rel

F32_TINY = float(np.finfo(np.float32).tiny)
MASK_GATE = 1e-6


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops
    ops.require_gpu()
    return ops


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda")          # (a copy: the shared inputs are read-only)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- a. medians, bit for bit
@functools.lru_cache(maxsize=None)
def _tie(B, T):
    """(D, |D| as the kernel states it) of the tie input: built once, shared, never written to."""
    D = K.tie_spectrum(B, T)
    S = K.mag32(D)
    D.setflags(write=False)
    S.setflags(write=False)
    return D, S


@functools.lru_cache(maxsize=None)
def _tie_median(B, T, k, axis):
    M = R.median_filter_axis(_tie(B, T)[1], k, axis=axis)
    M.setflags(write=False)
    return M


def _where(a, b):
    return f"differs at {np.argwhere(a != b)[:5].tolist()}"


@pytest.mark.parametrize("T", K.MEDIAN_T)
@pytest.mark.parametrize("win", K.MEDIAN_WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_medians_exact_under_ties(ops, win, T):
    D, _ = _tie(3, T)
    Dd = _dev(D)
    Mh, Mp, H, P = ops.hpss_masks(Dd, win, 2.0, 1.0, medians=True)
    Hh, Ph = H.cpu().numpy(), P.cpu().numpy()
    Hr, Pr = _tie_median(3, T, win[0], 1), _tie_median(3, T, win[1], 2)
    assert Hh.shape == Hr.shape == (3, T, K.NB)
    assert np.array_equal(Hh, Hr), f"H {_where(Hh, Hr)}"
    assert np.array_equal(Ph, Pr), f"P {_where(Ph, Pr)}"
    assert bool(torch.isfinite(Mh).all()) and bool(torch.isfinite(Mp).all())
    for b in range(3):                                   # the clip offset: a batch row is its single call, masks included
        one = ops.hpss_masks(Dd[b:b + 1], win, 2.0, 1.0, medians=True)
        for got, want in zip(one, (Mh, Mp, H, P)):
            assert torch.equal(got[0], want[b])


@pytest.mark.parametrize("win", K.EDGE_WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_medians_exact_on_denormal_squares_overflow_and_zeros(ops, win):
    D = K.edge_spectrum(K.EDGE_T)
    S = K.mag32(D)
    _, _, H, P = ops.hpss_masks(_dev(D), win, 2.0, 1.0, medians=True)
    Hh, Ph = H.cpu().numpy(), P.cpu().numpy()
    Hr = R.median_filter_axis(S, win[0], axis=1)
    Pr = R.median_filter_axis(S, win[1], axis=2)
    # bit patterns: +inf equals +inf, and a magnitude rebuilt from denormal squares must come out to the last bit
    assert np.array_equal(_bits(Hh), _bits(Hr)), f"H {_where(_bits(Hh), _bits(Hr))}"
    assert np.array_equal(_bits(Ph), _bits(Pr)), f"P {_where(_bits(Ph), _bits(Pr))}"
    out = np.concatenate([Hh.ravel(), Ph.ravel()])
    assert np.isposinf(out).any() and (out == 0).any() and ((out > 0) & (out < 1e-18)).any()
    assert not np.isnan(out).any()


# ---------------------------------------------------------------------------- b. soft masks
@functools.lru_cache(maxsize=None)
def _softmask_input(kind):
    D = _tie(2, 33)[0] if kind == "tie" else K.noise_spectrum(2, 33)
    D.setflags(write=False)
    return D


@pytest.mark.parametrize("margin", K.SOFTMASK_MARGINS, ids=lambda m: f"m{m[0]}-{m[1]}")
@pytest.mark.parametrize("power", K.SOFTMASK_POWERS, ids=lambda p: f"p{p}")
def test_soft_masks_at_every_power_and_margin(ops, power, margin):
    split = margin == (1.0, 1.0)
    worst = 0.0
    for kind in ("tie", "noise"):
        Mh, Mp, H, P = (t.cpu().numpy() for t in
                        ops.hpss_masks(_dev(_softmask_input(kind)), K.SOFTMASK_WINDOWS, power, margin, medians=True))
        rh = R.softmask(H, P.astype(np.float64) * margin[0], power, split, tiny=F32_TINY)
        rp = R.softmask(P, H.astype(np.float64) * margin[1], power, split, tiny=F32_TINY)
        assert np.isfinite(Mh).all() and np.isfinite(Mp).all()
        err = max(float(np.abs(Mh - rh).max()), float(np.abs(Mp - rp).max()))
        worst = max(worst, err)
        # gate: the project's 1e-6 absolute.  A float32 emulation of the kernel's softmask1 on 200 000 random pairs over
        # six decades stays within 2.3e-7 of float64 at each of these powers and margins
        assert err <= MASK_GATE, (kind, err)
        bad = np.maximum(H, P) < F32_TINY
        eq = (H == P) & (H > 0)
        if kind == "tie":
            assert bad.sum() >= 1000 and eq.sum() >= 1000, (bad.sum(), eq.sum())
        want = 0.5 if split and np.isfinite(power) else 0.0                  # the hard mask never splits
        assert (Mh[bad] == want).all() and (Mp[bad] == want).all()
        if split and np.isfinite(power):
            assert (Mh[eq] == 0.5).all() and (Mp[eq] == 0.5).all()
        if np.isinf(power):
            assert (Mh[eq] == 0.0).all() and (Mp[eq] == 0.0).all()
            assert np.isin(Mh, (0.0, 1.0)).all() and np.isin(Mp, (0.0, 1.0)).all()
    print(f"hpss masks power={power} margin={margin}: worst {worst:.2e} absolute (gate {MASK_GATE:g})")


# ---------------------------------------------------------------------------- c. inverse STFT on crafted D
def _istft_ref(D, L, mask=None):
    """R.istft of every clip of D [B, T, 1025, 2] (times mask [B, T, 1025]) -> [B, L] float64."""
    Dc = K.to_complex(D)
    if mask is not None:
        Dc = Dc * np.swapaxes(np.asarray(mask, dtype=np.float64), -1, -2)
    return np.stack([R.istft(Dc[b], L) for b in range(Dc.shape[0])])


def _parity(got, want, what):
    worst = 0.0
    for b in range(want.shape[0]):
        assert_parity(got[b].cpu().numpy(), want[b], what=f"{what}, clip {b}")
        worst = max(worst, peak_rel(got[b].cpu().numpy().astype(np.float64), want[b]))
    return worst


def test_istft_ignores_imaginary_parts_of_the_real_bins(ops):
    B, T, L = 2, 9, 4096
    D = K.noise_spectrum(B, T)
    assert np.abs(D[..., 0, 1]).min() > 1e-4 and np.abs(D[..., 1024, 1]).min() > 1e-4 and np.abs(D[..., 0, 1]).max() > 1
    D0 = D.copy()
    D0[..., 0, 1] = 0.0
    D0[..., 1024, 1] = 0.0
    want = _istft_ref(D, L)
    assert np.array_equal(want, _istft_ref(D0, L))
    Ma, Mb = K.unit_masks(B, T)
    got = ops.istft2048(_dev(D), 512, L)
    assert torch.equal(got, ops.istft2048(_dev(D0), 512, L))
    worst = _parity(got, want, "istft")
    ya, yb = ops.istft2048(_dev(D), 512, L, mask=(_dev(Ma), _dev(Mb)))
    za, zb = ops.istft2048(_dev(D0), 512, L, mask=(_dev(Ma), _dev(Mb)))
    assert torch.equal(ya, za) and torch.equal(yb, zb)
    worst = max(worst, _parity(ya, _istft_ref(D, L, Ma), "istft mask a"), _parity(yb, _istft_ref(D, L, Mb), "istft mask b"))
    print(f"istft crafted D, Im X[0] and Im X[1024] of order 1: worst {worst:.2e} of the peak")


@pytest.mark.parametrize("L", K.ISTFT_SEAMS)
def test_istft_segment_seams(ops, L):
    B, T = 2, 1 + L // 512
    D = K.noise_spectrum(B, T, seed=L)
    Ma, Mb = K.unit_masks(B, T, seed=L)
    Dd, Mad, Mbd = _dev(D), _dev(Ma), _dev(Mb)
    plain = ops.istft2048(Dd, 512, L)
    one = ops.istft2048(Dd, 512, L, mask=Mad)
    ya, yb = ops.istft2048(Dd, 512, L, mask=(Mad, Mbd))
    assert plain.shape == one.shape == ya.shape == yb.shape == (B, L)
    worst = max(_parity(plain, _istft_ref(D, L), f"istft L={L}"), _parity(ya, _istft_ref(D, L, Ma), f"istft L={L} mask a"),
                _parity(yb, _istft_ref(D, L, Mb), f"istft L={L} mask b"))
    assert torch.equal(one, ya)                                              # one component or two: the same bits
    sa, sb = ops.istft2048(Dd, 512, L, mask=(Mad, Mbd), ldy=L + 37)
    assert sa.stride(0) == L + 37 and torch.equal(sa, ya) and torch.equal(sb, yb)
    assert torch.equal(ops.istft2048(Dd, 512, L, ldy=L + 37), plain)
    for b in range(B):                                                       # a batch row is its single call
        ra, rb = ops.istft2048(Dd[b:b + 1], 512, L, mask=(Mad[b:b + 1], Mbd[b:b + 1]))
        assert torch.equal(ra[0], ya[b]) and torch.equal(rb[0], yb[b])
        assert torch.equal(ops.istft2048(Dd[b:b + 1], 512, L)[0], plain[b])
    print(f"istft L={L} ({K.istft_segments(L)} segments a clip), plain and two masks: worst {worst:.2e} of the peak")


@pytest.mark.parametrize("T,L,last", [(5, 8000, 3071), (1, 5000, 1023)])
def test_istft_of_fewer_frames_than_the_length_asks(ops, T, L, last):
    B = 2
    D = K.noise_spectrum(B, T, seed=L)
    Ma, Mb = K.unit_masks(B, T, seed=L)
    want = _istft_ref(D, L)
    assert not want[:, last + 1:].any() and want[:, last].all()
    plain = ops.istft2048(_dev(D), 512, L)
    ya, yb = ops.istft2048(_dev(D), 512, L, mask=(_dev(Ma), _dev(Mb)))
    worst = max(_parity(plain, want, "istft short D"), _parity(ya, _istft_ref(D, L, Ma), "istft short D mask a"),
                _parity(yb, _istft_ref(D, L, Mb), "istft short D mask b"))
    for y in (plain, ya, yb):                                                # no frame reaches there: exactly zero
        assert not bool(y[:, last + 1:].any())
        assert bool((y[:, last] != 0).all())
    print(f"istft of {T} frames at length {L}: worst {worst:.2e} of the peak, zero from sample {last + 1} on")


def test_istft_of_more_frames_than_the_length_needs(ops):
    B, T, L, need = 2, 40, 3000, 10
    D = K.noise_spectrum(B, T, seed=L)
    Ma, Mb = K.unit_masks(B, T, seed=L)
    for a in (D, Ma, Mb):
        a[:, need:] = np.nan
    Dd, Mad, Mbd = _dev(D), _dev(Ma), _dev(Mb)
    plain = ops.istft2048(Dd, 512, L)
    ya, yb = ops.istft2048(Dd, 512, L, mask=(Mad, Mbd))
    worst = max(_parity(plain, _istft_ref(D[:, :need], L), "istft long D"),
                _parity(ya, _istft_ref(D[:, :need], L, Ma[:, :need]), "istft long D mask a"),
                _parity(yb, _istft_ref(D[:, :need], L, Mb[:, :need]), "istft long D mask b"))
    assert np.array_equal(_istft_ref(D, L), _istft_ref(D[:, :need], L))      # the reference does not read them either
    cut = lambda t: t[:, :need].contiguous()                                 # noqa: E731
    assert torch.equal(plain, ops.istft2048(cut(Dd), 512, L))
    ca, cb = ops.istft2048(cut(Dd), 512, L, mask=(cut(Mad), cut(Mbd)))
    assert torch.equal(ya, ca) and torch.equal(yb, cb)
    print(f"istft of {T} frames (NaN from frame {need} on) at length {L}: worst {worst:.2e} of the peak")


def test_istft_more_waves_than_the_grid_holds(ops):
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    B, T, L = cu * 128 + 8, 2, 600
    assert K.istft_segments(L) == 1 and 2 * B > cu * 256                     # two waves a clip: past the cap of cu * 64 workgroups
    D8 = K.noise_spectrum(8, T, seed=L)
    Ma8, Mb8 = K.unit_masks(8, T, seed=L)
    D8d, Ma8d, Mb8d = _dev(D8), _dev(Ma8), _dev(Mb8)
    ya8, yb8 = ops.istft2048(D8d, 512, L, mask=(Ma8d, Mb8d))
    worst = max(_parity(ya8, _istft_ref(D8, L, Ma8), "istft 8 clips mask a"),
                _parity(yb8, _istft_ref(D8, L, Mb8), "istft 8 clips mask b"))
    idx = torch.arange(B, device="cuda") % 8
    ya, yb = ops.istft2048(D8d[idx], 512, L, mask=(Ma8d[idx], Mb8d[idx]))
    assert ya.shape == yb.shape == (B, L)
    assert torch.equal(ya, ya8[idx]) and torch.equal(yb, yb8[idx])
    print(f"istft of {B} clips x 2 components on {cu} CUs (cap {cu * 256} waves): every row equals its 8-clip call; "
          f"those worst {worst:.2e} of the peak")


# ---------------------------------------------------------------------------- d. HNR rows, direct
def _cls(v):
    return np.where(np.isnan(v), 0, np.where(v == 80, 1, np.where(v == -80, 2, 3)))


def _ulps(got, ref):
    """|got - ref| in float32 spacings of |ref| (0 where both are exactly equal)."""
    got = got.astype(np.float64)
    sp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.where(got == ref, 0.0, np.abs(got - ref) / sp)


@pytest.mark.parametrize("c", K.HNR_CASES, ids=lambda c: c.id)
def test_hnr_rows_direct(ops, c):
    yh, yp = K.hnr_rows_input(c)
    T = ops.num_frames_padded(c.L, c.fl, c.hop, bool(c.center))
    if c.pad:                                            # rows ld apart in a buffer of NaN: a read past a row's end shows
        bufs = [torch.full((c.B, c.ld), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
        yhd, ypd = (b[:, :c.L] for b in bufs)
        yhd.copy_(_dev(yh))
        ypd.copy_(_dev(yp))
        assert yhd.stride(0) == ypd.stride(0) == c.ld and not yhd.is_contiguous()
    else:
        yhd, ypd = _dev(yh), _dev(yp)
    hnr, rh, rp = (t.cpu().numpy() for t in ops.hnr_rows(yhd, ypd, c.fl, c.hop, bool(c.center), rms=True))
    assert hnr.shape == rh.shape == rp.shape == (c.B, T) and hnr.dtype == np.float32
    ref = [R.hnr_from_components(yh[r], yp[r], c.fl, c.hop, bool(c.center)) for r in range(c.B)]
    want, ph, pp = (np.stack([x[i] for x in ref]) for i in range(3))
    assert want.shape == (c.B, T)
    near = (np.abs(ph / R.EPSILON - 1) < 0.01) | (np.abs(pp / R.EPSILON - 1) < 0.01)
    assert near.sum() <= 0.02 * near.size
    assert np.array_equal(_cls(hnr)[~near], _cls(want)[~near]), np.argwhere((_cls(hnr) != _cls(want)) & ~near)[:5]
    row_class = {0: 3, 1: 1, 2: 2, 3: 0, 4: 1}           # what the row kinds of hnr_rows_input are there to reach
    assert set(np.unique(_cls(want)[~near]).tolist()) >= {row_class[r % 5] for r in range(c.B)}
    # one float32 spacing: the kernel sums in float64 and rounds once
    val = (_cls(want) == 3) & (_cls(hnr) == 3)
    u_hnr = float(_ulps(hnr[val], want[val]).max()) if val.any() else 0.0
    u_rh = float(_ulps(rh, np.sqrt(ph)).max())
    u_rp = float(_ulps(rp, np.sqrt(pp)).max())
    print(f"hnr rows {c.id}: {T} frames, {int(near.sum())} near the threshold; worst hnr {u_hnr:.2f}, rms_harm {u_rh:.2f}, "
          f"rms_perc {u_rp:.2f} float32 spacings")
    assert u_hnr <= 1.0 and u_rh <= 1.0 and u_rp <= 1.0
    if c.pad:
        assert all(bool(torch.isnan(b[:, c.L:]).all()) for b in bufs)
