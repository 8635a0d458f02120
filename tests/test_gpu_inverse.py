"""Griffin-Lim and the mel / MFCC inversions on the device (csrc/griffinlim.hip with the forward and inverse STFT, through
sygnals_amd.ops and sygnals_amd.core.features.inverse) against the float64 restatement tests/inverse_ref.py fed
the same float32 inputs.  The contract is staged, because the phase normalisation amplifies the STFT's rounding from
iteration to iteration whatever computes it (float32 against float64 on these signals: 8e-7 of the peak after one
iteration, 7e-5 after 32 at momentum 0.99):

  G1  the projection alone: 1e-5 max S; crafted cells keep |D| <= S (1 + 1e-6); sums to 1e-12 relative, bit-repeatable
  G2  one whole iteration (project, inverse, forward): 1e-5 of the rebuilt spectrum's peak (the inverse STFT that
      projected on its load measured slower than the two launches and was not kept, so there is no second form to match)
  G3  end to end: 0, 1 and 2 iterations gated at 1e-5 of the output's peak; 32 iterations measured, and properties gated
      there (trace at momentum 0, final convergence, zero input, chunk independence, seeds)

Bounds this file sets itself, with their reasons:
  TRACE_SLACK  a float32 FFT of 2048 points rounds once in each of its log2(2048) = 11 stages, so a rebuilt spectrum is
      off by at most about 11 eps32 of its norm, and so is the inverse before it; the trace is a relative distance in that
      norm, and a step compares two spectra: 4 * 11 * eps32 = 2.6e-6.  The restatement with float32 spectra never rose on
      these signals, nor did the device (the largest step of both is -1.0e-3, printed).
  CONV_TOL     the final convergence against the float64 restatement's: 1e-5 relative, the project's parity gate.  The
      restatement with float32 spectra sits within 1.7e-7 of it and the device within 1.9e-6 (momentum 0.99; 1.6e-8 at
      momentum 0), both printed.
  32 iterations, measured and not gated: the device's clip is 5.9e-6 of the peak from the float64 restatement's at
      momentum 0 and 1.1e-4 at 0.99 (the restatement with float32 spectra alone: 8.3e-8 and 7.1e-7).
  dense        |out - ref| <= 1e-5 sum_m |W| |pre(X)| before `post`, which is float32 accumulation of 128 terms
      (128 * 2^-24 = 7.6e-6); `post` adds its own rounding, relative to its own value: 8 eps32 for the root and the
      power, and for db_to_power the bound on the exponent carried through the exponential.
Every test prints its figures; those measured on MI355X are in README.md, "Feature inversion"."""
import numpy as np
import pytest
import torch

from sygnals_amd import _tables as T
from sygnals_amd import ops
from sygnals_amd.core.features import inverse as IV
from tests import inverse_ref as R

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
TOL = 1e-5
TRACE_SLACK = 4 * 11 * EPS32
CONV_TOL = 1e-5
NB = 1025


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _c(t):
    """Device spectrum [..., 2] float32 -> complex128 host array."""
    a = t.cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def _spectra(B, Tn, seed):
    rng = np.random.default_rng(seed)
    Rr = rng.standard_normal((B, Tn, NB, 2)).astype(np.float32)
    P = rng.standard_normal((B, Tn, NB, 2)).astype(np.float32)
    S = np.abs(rng.standard_normal((B, Tn, NB))).astype(np.float32)
    return Rr, P, S


def _cx(a):
    a = a.astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


# ------------------------------------------------------------------ G1
@pytest.mark.parametrize("Tn", [1, 2, 5, 40])
def test_g1_projection(Tn):
    Rr, P, S = _spectra(3, Tn, Tn)
    Rd, Pd, Sd = _dev(Rr), _dev(P), _dev(S)
    for momentum, Pq in ((0.0, P), (0.99, P), (0.99, None)):
        alpha = ops.gl_alpha(momentum)
        D = _c(ops.gl_project(Rd, Sd, Pd if Pq is not None else None, alpha))
        ref = R.project(_cx(Rr), _cx(Pq) if Pq is not None else None, S, alpha)
        err = np.max(np.abs(D - ref)) / S.max()
        print(f"T={Tn} momentum={momentum} P={'yes' if Pq is not None else 'no'}: {err:.3e} of max S ({err / EPS32:.1f} eps32)")
        assert np.isfinite(D).all() and err <= TOL
    # in place, and batch rows that are not contiguous (made contiguous, as istft2048 does)
    alpha = ops.gl_alpha(0.99)
    want = ops.gl_project(Rd, Sd, Pd, alpha)
    big = torch.zeros((6,) + tuple(Rd.shape[1:]), device="cuda")
    big[::2] = Rd
    assert torch.equal(ops.gl_project(big[::2], Sd, Pd, alpha), want)
    # a clip's bits do not depend on where it lies (at odd T the second clip starts 8 bytes off a 16-byte line)
    assert torch.equal(ops.gl_project(Rd[1:], Sd[1:], Pd[1:], alpha), want[1:])
    inplace = Rd.clone()
    assert ops.gl_project(inplace, Sd, Pd, alpha, out=inplace) is inplace and torch.equal(inplace, want)


def test_g1_crafted_cells():
    """What a naive sqrtf(re^2 + im^2) fails: a component of 1e-25 squares to zero and the quotient by tiny is 1e13 S, one
    of 1e30 squares to +inf and zeroes the bin."""
    alpha = ops.gl_alpha(0.99)
    a32 = np.float32(alpha)
    cells = [(1e-25, 1e-25), (-1e-25, 1e-25), (1e-25, 0.0), (0.0, -1e-25), (1e-40, -1e-40), (1e-40, 0.0), (1e30, 1e30),
             (-1e30, 1e-25), (0.0, 1e30), (3e38, 3e38), (1e-25, 1e30), (3.0, 4.0)]
    Rr = np.zeros((1, 2, NB, 2), dtype=np.float32)
    P = np.zeros_like(Rr)
    S = np.zeros((1, 2, NB), dtype=np.float32)
    for j, (re, im) in enumerate(cells):
        for t in (0, 1):
            Rr[0, t, 10 + j] = (re, im)
            S[0, t, 10 + j] = 1.0 + j
    zero_a, zero_s = 40, 41
    P[0, :, zero_a] = (4.0, -2.0)                                     # alpha * 2^k is exact: A = R - alpha P = 0
    Rr[0, :, zero_a] = (a32 * np.float32(4.0), a32 * np.float32(-2.0))
    S[0, :, zero_a] = 5.0
    Rr[0, :, zero_s] = (0.3, -0.7)                                    # S = 0
    Rr[0, :, 0] = (1.0, 2.0)                                          # Im parts in bins 0 and 1024
    Rr[0, :, 1024] = (-3.0, 0.5)
    S[0, :, 0] = 2.0
    S[0, :, 1024] = 6.0
    assert np.float64(a32) * 4.0 == np.float64(Rr[0, 0, zero_a, 0])
    for Pq in (None, P):
        D = _c(ops.gl_project(_dev(Rr), _dev(S), _dev(Pq) if Pq is not None else None, alpha))
        assert np.isfinite(D).all()
        assert np.all(np.abs(D) <= S.astype(np.float64) * (1 + 1e-6))
        assert np.all(D[0, :, zero_s] == 0)
        ref = R.project(_cx(Rr), _cx(Pq) if Pq is not None else None, S, alpha)
        err = np.max(np.abs(D - ref)) / S.max()
        print(f"crafted cells, P={'yes' if Pq is not None else 'no'}: {err:.3e} of max S")
        assert err <= TOL
        if Pq is not None:
            assert np.all(D[0, :, zero_a] == 0)
        # the phase survives every exponent: |D| = S wherever |A| is far above tiny
        far = [10 + j for j, c in enumerate(cells) if max(abs(c[0]), abs(c[1])) > 1e-30]
        assert np.allclose(np.abs(D[0, :, far]), S[0, :, far], rtol=1e-6)
        assert np.allclose(D[0, :, 0], 2.0 * (1 + 2j) / np.sqrt(5.0), rtol=1e-6)


@pytest.mark.parametrize("Tn", [1, 2, 40, 2100])
def test_g1_sums(Tn):
    """(sum (|R| - S)^2, sum S^2) per clip in float64; T = 2100 is past the cap of 1024 workgroups a clip."""
    B = 3 if Tn < 100 else 2
    Rr, P, S = _spectra(B, Tn, 100 + Tn)
    Rd, Pd, Sd = _dev(Rr), _dev(P), _dev(S)
    D, sums = ops.gl_project(Rd, Sd, Pd, ops.gl_alpha(0.99), return_sums=True)
    D2, sums2 = ops.gl_project(Rd, Sd, Pd, ops.gl_alpha(0.99), return_sums=True)
    assert torch.equal(sums, sums2) and torch.equal(D, D2) and torch.equal(D, ops.gl_project(Rd, Sd, Pd, ops.gl_alpha(0.99)))
    got = sums.cpu().numpy()
    want = np.array([R.sums(_cx(Rr[b]), S[b]) for b in range(B)])
    rel = np.max(np.abs(got - want) / want)
    print(f"T={Tn}: sums {rel:.3e} relative")
    assert got.shape == (B, 2) and rel <= 1e-12
    # a clip's figures do not depend on the batch it sits in
    _, one = ops.gl_project(Rd[1:2], Sd[1:2], Pd[1:2], ops.gl_alpha(0.99), return_sums=True)
    assert torch.equal(one[0], sums[1])


# ------------------------------------------------------------------ G2
def _signals(B, L):
    return np.stack([R.tones_noise(L, k) for k in range(B)])


def _mags(y):
    """float32 magnitudes [B, T, 1025] of the float64 STFT of the clips y."""
    return np.stack([np.abs(R.stft(v)) for v in y]).astype(np.float32)


@pytest.mark.parametrize("L", [512, 8192, 8193, 16384, 16385])
def test_g2_one_iteration(L):
    """Lengths where the inverse's wave count steps (8192 | 8193, 16384 | 16385) and two frames."""
    B = 3
    Tn = 1 + L // 512
    S = _mags(_signals(B, L))
    Rr, P, _ = _spectra(B, Tn, L)
    Rd, Pd, Sd = _dev(Rr), _dev(P), _dev(S)
    alpha = ops.gl_alpha(0.99)
    for Pq, Pdq in ((P, Pd), (None, None)):
        D = ops.gl_project(Rd, Sd, Pdq, alpha)
        y = ops.istft2048(D, length=L)
        Rn = _c(ops.stft2048_c2c(y.contiguous()))
        for b in range(B):
            D64 = R.project(_cx(Rr[b]), _cx(Pq[b]) if Pq is not None else None, S[b], alpha)
            y64 = R.istft(D64, L)
            R64 = R.stft(y64)
            ey = np.max(np.abs(y[b].cpu().numpy() - y64)) / np.max(np.abs(y64))
            er = np.max(np.abs(Rn[b] - R64)) / np.max(np.abs(R64))
            print(f"L={L} clip {b} P={'yes' if Pq is not None else 'no'}: y {ey:.3e} of its peak, rebuilt spectrum {er:.3e} of its peak")
            assert ey <= TOL and er <= TOL


# ------------------------------------------------------------------ G3
L3, B3 = 8192, 3
T3 = 1 + L3 // 512


@pytest.fixture(scope="module")
def case3():
    """The experiment's signals (tones plus noise, 17 frames), their float32 magnitudes, the device's starting spectrum of
    seed 7, and the restatement's runs at 32 iterations in float64 and with float32 spectra."""
    S = _mags(_signals(B3, L3))
    R0 = _cx(ops.randn(B3, T3 * NB * 2, 7).cpu().numpy().reshape(B3, T3, NB, 2))
    runs = {}
    for momentum in (0.0, 0.99):
        for s32 in (False, True):
            runs[momentum, s32] = [R.griffinlim(S[b], 32, momentum, R0[b], L3, stft32=s32) for b in range(B3)]
    for v in (S, R0):
        v.setflags(write=False)
    return S, R0, runs


@pytest.mark.parametrize("n_iter,momentum", [(0, 0.99), (1, 0.99), (2, 0.99), (2, 0.0)])
def test_g3_first_iterations(case3, n_iter, momentum):
    S, R0, _ = case3
    y, trace = ops.griffinlim(_dev(S), n_iter, momentum, "random", 7, return_trace=True)
    assert y.shape == (B3, L3) and trace.shape == (B3, n_iter) and trace.dtype == torch.float64
    assert torch.equal(ops.griffinlim(_dev(S), n_iter, momentum, "random", 7), y), "traced and untraced runs differ"
    for b in range(B3):
        want, tr = R.griffinlim(S[b], n_iter, momentum, R0[b], L3)
        e = np.max(np.abs(y[b].cpu().numpy() - want)) / np.max(np.abs(want))
        et = np.max(np.abs(trace[b].cpu().numpy() - tr) / tr) if n_iter else 0.0
        print(f"n_iter={n_iter} momentum={momentum} clip {b}: {e:.3e} of the output's peak, trace {et:.3e} relative")
        assert e <= TOL and et <= TOL


def test_g3_other_starts(case3):
    """init=None (phases of 1) and caller's angles (any modulus), one iteration each."""
    S, R0, _ = case3
    y = ops.griffinlim(_dev(S), 1, 0.99, None).cpu().numpy()
    ang = np.stack([R0.real, R0.imag], axis=-1).astype(np.float32) * 3.0
    ya = ops.griffinlim(_dev(S), 1, 0.99, angles=_dev(ang)).cpu().numpy()
    for b in range(B3):
        want, _ = R.griffinlim(S[b], 1, 0.99, None, L3)
        wa, _ = R.griffinlim(S[b], 1, 0.99, _cx(ang[b]), L3)
        e, ea = (np.max(np.abs(g - w)) / np.max(np.abs(w)) for g, w in ((y[b], want), (ya[b], wa)))
        print(f"clip {b}: init=None {e:.3e}, angles {ea:.3e} of the output's peak")
        assert e <= TOL and ea <= TOL
    # the true phases are a fixed point: the clip comes back
    sig = _signals(1, L3)
    D = R.stft(sig[0])
    back = ops.griffinlim(_dev(np.abs(D).astype(np.float32)[None]), 4, 0.99,
                          angles=_dev(np.stack([D.real, D.imag], axis=-1).astype(np.float32)[None]))[0].cpu().numpy()
    e = np.max(np.abs(back - sig[0])) / np.max(np.abs(sig[0]))
    print(f"true phases, 4 iterations: {e:.3e} of the peak")
    assert e <= TOL


def test_g3_at_32_iterations(case3):
    """Measured, not gated: the output against the float64 restatement, beside the restatement's own shift when its
    spectra are rounded to float32.  Gated: the trace at momentum 0 and the final convergence."""
    S, R0, runs = case3
    for momentum in (0.0, 0.99):
        y, trace = ops.griffinlim(_dev(S), 32, momentum, "random", 7, return_trace=True)
        y, trace = y.cpu().numpy(), trace.cpu().numpy()
        assert np.isfinite(y).all() and np.isfinite(trace).all()
        for b in range(B3):
            y64, t64 = runs[momentum, False][b]
            y32, t32 = runs[momentum, True][b]
            pk = np.max(np.abs(y64))
            print(f"32 iterations, momentum {momentum}, clip {b}: device {np.max(np.abs(y[b] - y64)) / pk:.3e} of the peak, "
                  f"restatement with float32 spectra {np.max(np.abs(y32 - y64)) / pk:.3e}")
            d_dev, d_32 = abs(trace[b, -1] - t64[-1]) / t64[-1], abs(t32[-1] - t64[-1]) / t64[-1]
            print(f"    final convergence {trace[b, -1]:.6e} (float64 {t64[-1]:.6e}): device {d_dev:.3e} relative, "
                  f"float32 spectra {d_32:.3e}")
            assert d_dev <= CONV_TOL
            if momentum == 0.0:
                rise, rise32 = np.max(np.diff(trace[b])), np.max(np.diff(t32))
                print(f"    largest step of the trace: device {rise:.3e}, float32 spectra {rise32:.3e} (slack {TRACE_SLACK:.2e})")
                assert rise <= TRACE_SLACK and trace[b, -1] < trace[b, 0]


def test_g3_zero_input_chunks_and_seeds(case3):
    S, _, _ = case3
    Sd = _dev(S)
    assert torch.count_nonzero(ops.griffinlim(torch.zeros(2, T3, NB, device="cuda"), 32)) == 0
    y, trace = ops.griffinlim(Sd, 32, 0.99, "random", 11, return_trace=True)
    for chunk in (1, 2, B3):
        yc, tc = ops.griffinlim(Sd, 32, 0.99, "random", 11, return_trace=True, chunk=chunk)
        assert torch.equal(yc, y) and torch.equal(tc, trace), f"chunk={chunk} changes the bits"
        assert torch.equal(ops.griffinlim(Sd, 32, 0.99, "random", 11, chunk=chunk), y), f"chunk={chunk}, untraced"
    assert torch.equal(ops.griffinlim(Sd, 32, 0.99, "random", 11), y)
    assert not torch.equal(ops.griffinlim(Sd, 32, 0.99, "random", 12), y)
    for r in range(B3):
        assert torch.equal(ops.griffinlim(Sd[r:r + 1], 32, 0.99, "random", 11, first_row=r)[0], y[r])
    # the mirror: librosa's orientation in, the same clip out
    one = IV.griffinlim(S[1].T, 32, 0.99, seed=11)
    assert one.dtype == np.float32 and np.array_equal(one, ops.griffinlim(Sd[1:2], 32, 0.99, "random", 11)[0].cpu().numpy())
    assert torch.equal(IV.griffinlim_batch(Sd, 2, seed=11), ops.griffinlim(Sd, 2, seed=11))


# ------------------------------------------------------------------ dense inversions
def _dense_check(X, W, pre_ref, post, power=2.0, ref=1.0, mel_major=False, what=""):
    out = ops.inv_dense(_dev(X), _dev(W), pre_ref, post, power, ref, mel_major).cpu().numpy().astype(np.float64)
    if mel_major:
        out = out.transpose(0, 2, 1)
    worst = 0.0
    for b in range(X.shape[0]):
        lin, scale = R.inv_dense(X[b], W, pre_ref)
        bound = TOL * scale
        if post is None:
            err, allow = np.abs(out[b] - lin), bound
        elif post == "root":
            # judged before the root: out^power against max(lin, 0); the root's own rounding is relative to its value
            err = np.abs(out[b] ** power - np.maximum(lin, 0.0))
            allow = bound + 8 * EPS32 * power * np.maximum(lin, 0.0)
            assert np.all(out[b][lin < -bound] == 0), f"{what}: a negative sum is not clipped to zero"
            assert np.all(out[b] >= 0)
        else:
            # out = ref 10^(lin / 10): an error e in the exponent is a relative error ln(10) / 10 e of the power
            want = R.db_to_power(lin, ref)
            err, allow = np.abs(out[b] - want), want * (np.log(10.0) / 10.0 * bound + 8 * EPS32)
        fin = np.isfinite(allow)
        assert np.isfinite(out[b][fin]).all(), f"{what}: non-finite output"
        ratio = np.max(err[fin] / np.maximum(allow[fin], 1e-300))
        worst = max(worst, ratio)
        assert np.all(err[fin] <= allow[fin]), f"{what}: {ratio:.3f} of the bound"
    print(f"{what}: worst {worst:.3f} of the bound")


@pytest.mark.parametrize("M", [1, 13, 40, 128])
@pytest.mark.parametrize("Tn", [1, 63, 65])
def test_dense_shapes_and_modes(M, Tn):
    rng = np.random.default_rng(M * 100 + Tn)
    F = 1025 if M == 128 else 70
    W = rng.standard_normal((F, M)).astype(np.float32)
    X = rng.standard_normal((3, M, Tn)).astype(np.float32)
    Xdb = rng.uniform(-80.0, 10.0, (3, M, Tn)).astype(np.float32)
    _dense_check(X, W, None, None, what=f"M={M} T={Tn} plain")
    _dense_check(X, W, None, None, mel_major=True, what=f"M={M} T={Tn} plain, mel-major out")
    for power in (1.0, 2.0, 3.0):
        _dense_check(X, W, None, "root", power, what=f"M={M} T={Tn} root {power:g}")
    _dense_check(Xdb, W, 2.5, None, what=f"M={M} T={Tn} dB in")
    _dense_check(Xdb, W, 1.0, "root", 2.0, what=f"M={M} T={Tn} dB in, root 2")
    _dense_check((X * 3).astype(np.float32), (W / np.sqrt(M)).astype(np.float32), None, "db", ref=0.5, what=f"M={M} T={Tn} dB out")


def test_dense_edges():
    """-inf dB is power 0, +200 dB is 1e20 and keeps float32's relative precision, all-negative sums clip to exactly 0."""
    rng = np.random.default_rng(5)
    M, Tn = 40, 65
    W = rng.standard_normal((70, M)).astype(np.float32)
    X = rng.uniform(-80.0, 10.0, (3, M, Tn)).astype(np.float32)
    X[0, 3, :] = -np.inf
    X[1, :, 7] = -np.inf                                     # a whole frame of silence: every sum is 0
    X[2, 5, 11] = 200.0
    X[2, :, 12] = rng.uniform(190.0, 200.0, M)
    _dense_check(X, W, 1.0, None, what="edges, dB in")
    _dense_check(X, W, 1.0, "root", 2.0, what="edges, dB in, root")
    out = ops.inv_dense(_dev(X), _dev(W), 1.0).cpu().numpy()
    assert np.all(out[1, 7] == 0) and np.isfinite(out).all() and np.max(np.abs(out[2, 12])) > 1e18
    neg = ops.inv_dense(_dev(np.abs(X[:, :, :5]) + 1), _dev(-np.abs(W)), None, "root").cpu().numpy()
    assert np.all(neg == 0)


@pytest.mark.parametrize("M,power", [(128, 2.0), (40, 1.0)])
def test_mel_to_stft(M, power):
    rng = np.random.default_rng(M)
    B = T.mel_filterbank(22050, 2048, M).astype(np.float64)
    P = rng.random((2, NB, 9)) ** 4
    mel = np.einsum("mf,bft->bmt", B, P).astype(np.float32)
    S = ops.mel_to_stft(_dev(mel), 22050, power=power)
    assert S.shape == (2, 9, NB) and S.dtype == torch.float32 and float(S.min()) >= 0 and int((S == 0).sum()) > 0
    W = ops.mel_pinv_table(22050, 2048, M)
    _dense_check(mel, W, None, "root", power, what=f"mel_to_stft M={M} power={power:g}")
    assert torch.equal(S, ops.inv_dense(_dev(mel), _dev(W), None, "root", power))
    # against the restatement's own pseudo-inverse (float64, not rounded to float32): the table's rounding is inside the bound
    for b in range(2):
        lin = (R.mel_pinv(B) @ mel[b].astype(np.float64)).T
        bound = TOL * (np.abs(W.astype(np.float64)) @ np.abs(mel[b].astype(np.float64))).T
        got = S[b].cpu().numpy().astype(np.float64) ** power
        assert np.all(np.abs(got - np.maximum(lin, 0)) <= bound + 8 * EPS32 * power * np.maximum(lin, 0))
    assert np.array_equal(IV.mel_to_stft(mel[0], 22050, power=power), S[0].cpu().numpy().T)


@pytest.mark.parametrize("K,M,lifter", [(13, 128, 0), (40, 40, 22), (1, 40, 0)])
def test_mfcc_to_mel(K, M, lifter):
    rng = np.random.default_rng(K)
    mfcc = (rng.standard_normal((3, K, 63)) * 20.0 / np.sqrt(K)).astype(np.float32)
    mel = ops.mfcc_to_mel(_dev(mfcc), M, ref=2.0, lifter=lifter)
    assert mel.shape == (3, M, 63)
    W = ops.idct_lifter_table(K, M, 2, "ortho", lifter)
    _dense_check(mfcc, W, None, "db", ref=2.0, mel_major=True, what=f"mfcc_to_mel K={K} M={M} lifter={lifter}")
    assert torch.equal(mel, ops.inv_dense(_dev(mfcc), _dev(W), None, "db", ref=2.0, mel_major_out=True))
    want = R.mfcc_to_mel(mfcc[1], M, 2, 2.0, lifter)
    rel = np.max(np.abs(mel[1].cpu().numpy() - want) / want)
    print(f"against the restatement's own matrix: {rel:.3e} relative")
    assert rel <= np.log(10.0) / 10.0 * TOL * np.max(np.abs(R.idct_matrix(K, M, 2, lifter)) @ np.abs(mfcc[1].astype(np.float64))) + 8 * EPS32
    db = ops.mfcc_to_mel(_dev(mfcc), M, ref=2.0, lifter=lifter, as_db=True)
    assert torch.equal(db, ops.inv_dense(_dev(mfcc), _dev(W), mel_major_out=True))
    assert np.array_equal(IV.mfcc_to_mel(mfcc[0], M, ref=2.0, lifter=lifter), mel[0].cpu().numpy())


def test_audio_compositions():
    """mel_to_audio and mfcc_to_audio compose the ops: one call each, against the composition written out."""
    y = _signals(2, 4096)
    S = _dev(_mags(y))
    mel = ops.mel_dense(S * S, _dev(T.mel_filterbank(22050, 2048, 128)))
    a = ops.mel_to_audio(mel, 22050, n_iter=2, seed=3)
    assert a.shape == (2, 4096) and torch.equal(a, ops.griffinlim(ops.mel_to_stft(mel, 22050), 2, seed=3))
    assert np.array_equal(IV.mel_to_audio(mel[1].cpu().numpy(), 22050, n_iter=2, seed=3),
                          ops.mel_to_audio(mel[1:2], 22050, n_iter=2, seed=3)[0].cpu().numpy())
    mfcc = ops.mel_mfcc(mel.clone(), 20, top_db=None, ref=1.0)
    b = ops.mfcc_to_audio(mfcc, 128, n_iter=2, seed=3)
    logmel = ops.mfcc_to_mel(mfcc, 128, as_db=True)
    assert torch.equal(b, ops.griffinlim(ops.mel_to_stft(logmel, 22050, db_ref=1.0), 2, seed=3))
    # converting on the second's load is the same map as converting in the first: the magnitudes agree to the dense bound
    S1 = ops.mel_to_stft(ops.mfcc_to_mel(mfcc, 128), 22050).cpu().numpy().astype(np.float64)
    S2 = ops.mel_to_stft(logmel, 22050, db_ref=1.0).cpu().numpy().astype(np.float64)
    W = np.abs(ops.mel_pinv_table(22050, 2048, 128).astype(np.float64))
    scale = np.einsum("fm,bmt->btf", W, ops.mfcc_to_mel(mfcc, 128).cpu().numpy().astype(np.float64))
    assert np.all(np.abs(S1 ** 2 - S2 ** 2) <= 2 * TOL * scale + 16 * EPS32 * S1 ** 2)
    assert np.array_equal(IV.mfcc_to_audio(mfcc[0].cpu().numpy(), 128, n_iter=2, seed=3),
                          ops.mfcc_to_audio(mfcc[0:1], 128, n_iter=2, seed=3)[0].cpu().numpy())
    assert torch.equal(IV.mfcc_to_audio_batch(mfcc, 128, n_iter=2, seed=3), b)
    assert torch.equal(IV.mel_to_audio_batch(mel, 22050, n_iter=2, seed=3), a)
