"""The device NMF (ops.nmf, nmf_divergence, nmf_masks, core.decompose) against the float64 restatement tests/nmf_ref.py.
Gates: 1e-5 of each factor's peak for one step, one half step and the iterated cases of tests/nmf_cases.py (each
conditioned on the CPU: tests/test_nmf_ref.py); exact properties are compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import nmf_cases as NC
from tests import nmf_ref as R

pytestmark = pytest.mark.gpu
GATE = NC.GATE


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops as o
    o.require_gpu()
    return o


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def run(ops, V, A0, C0, n_iter, loss, **kw):
    A, C = ops.nmf(dev(V)[None], A0=dev(A0)[None], C0=dev(C0)[None], n_iter=n_iter, beta_loss=loss, **kw)
    return A[0].cpu().numpy(), C[0].cpu().numpy()


def check(got, want, what):
    for g, w, name in zip(got, want, "AC"):
        assert np.isfinite(g).all(), (what, name)
        e = R.rel_peak(g, w)
        print(f"{what} {name}: {e:.2e} of the peak")
        assert e <= GATE, (what, name, e)


@pytest.mark.parametrize("loss", NC.LOSSES)
@pytest.mark.parametrize("kind", NC.KINDS)
@pytest.mark.parametrize("shape", NC.SHAPES, ids=str)
def test_one_step_and_half_steps(ops, shape, kind, loss):
    V, A0, C0 = NC.inputs(shape, kind)
    check(run(ops, V, A0, C0, 1, loss), NC.reference(shape, kind, loss, 1), "step")
    a, c = run(ops, V, A0, C0, 1, loss, update_C=False)
    check((a, c), NC.reference(shape, kind, loss, 1, True, False), "A half")
    assert np.array_equal(c, C0)
    # the C half from the stepped A, so that both halves see factors that are not the start
    A1 = NC.reference(shape, kind, loss, 1, True, False)[0].astype(np.float32)
    a, c = run(ops, V, A1, C0, 1, loss, update_A=False)
    check((a, c), R.nmf(V, A1, C0, 1, loss, False, True), "C half")
    assert np.array_equal(a, A1)


@pytest.mark.parametrize("shape,kind,loss,n_iter", NC.ITERATED, ids=str)
def test_iterated(ops, shape, kind, loss, n_iter):
    V, A0, C0 = NC.inputs(shape, kind)
    check(run(ops, V, A0, C0, n_iter, loss), NC.reference(shape, kind, loss, n_iter), f"{n_iter} iterations")


@pytest.mark.parametrize("form", ["fma", "mfma"])
@pytest.mark.parametrize("loss", NC.LOSSES)
@pytest.mark.parametrize("shape", NC.SHAPES, ids=str)
def test_both_forms_of_the_contractions(ops, shape, loss, form):
    """The FMA and the MFMA form at every shape (the default takes one of them by K): one step, each half, 10 iterations,
    and the exact properties of the frozen factor and of the zero frame and bin."""
    for kind in NC.KINDS:
        V, A0, C0 = NC.inputs(shape, kind)
        check(run(ops, V, A0, C0, 1, loss, form=form), NC.reference(shape, kind, loss, 1), f"{form} step")
        a, c = run(ops, V, A0, C0, 1, loss, update_C=False, form=form)
        check((a, c), NC.reference(shape, kind, loss, 1, True, False), f"{form} A half")
        assert np.array_equal(c, C0)
        a, c = run(ops, V, A0, C0, 1, loss, update_A=False, form=form)
        check((a, c), NC.reference(shape, kind, loss, 1, False, True), f"{form} C half")
        assert np.array_equal(a, A0)
        got = run(ops, V, A0, C0, 10, loss, form=form)
        check(got, NC.reference(shape, kind, loss, 10), f"{form} 10 iterations")
        if kind == "sparse" and shape[0] > 1 and shape[1] > 1:
            assert not got[0][shape[0] // 2].any() and not got[1][:, shape[1] // 3].any()


@pytest.mark.parametrize("loss", NC.LOSSES)
def test_zeros_stay_and_eps_branch(ops, loss):
    shape = (17, 65, 5)
    V, A0, C0 = (np.array(x) for x in NC.inputs(shape, "sparse"))
    A0[3, 1] = 0.0
    C0[2, 7] = 0.0
    C0[4, :] = 0.0                       # sum_f C = 0 under KL, a zero row and column of C C^T under Frobenius
    for form in ("fma", "mfma"):
        A, C = run(ops, V, A0, C0, 3, loss, form=form)
        assert A[3, 1] == 0 and C[2, 7] == 0 and not C[4].any() and np.isfinite(A).all() and np.isfinite(C).all()
    got = run(ops, V, A0, C0, 3, loss)
    A, C = got
    assert A[3, 1] == 0 and C[2, 7] == 0 and not C[4].any()
    assert not A[17 // 2].any() and not C[:, 65 // 3].any()          # the all-zero frame and bin of V
    check(got, R.nmf(V, A0, C0, 3, loss), "crafted zeros")
    ones, za, zc = np.ones((4, 6), np.float32), np.zeros((4, 3), np.float32), np.zeros((3, 6), np.float32)
    A, C = run(ops, ones, za, zc, 2, loss)                           # every denominator is zero
    assert not A.any() and not C.any()
    A, C = run(ops, ones, np.ones((4, 3), np.float32), zc, 2, loss)
    wa, wc = R.nmf(ones, np.ones((4, 3)), zc, 2, loss)
    assert np.isfinite(A).all() and np.isfinite(C).all() and np.allclose(A, wa, rtol=1e-5, atol=0) and np.allclose(C, wc, rtol=1e-5, atol=0)


@pytest.mark.parametrize("loss", NC.LOSSES)
def test_shared_dictionary_and_batch(ops, loss):
    shapes = (33, 130, 33)
    Vs = np.stack([NC.inputs(shapes, k)[0] for k in NC.KINDS])
    As = np.stack([NC.inputs(shapes, k)[1] for k in NC.KINDS])
    Cs = np.stack([NC.inputs(shapes, k)[2] for k in NC.KINDS])
    A, C = ops.nmf(dev(Vs), A0=dev(As), C0=dev(Cs), n_iter=4, beta_loss=loss)
    for b in range(3):                                               # three different clips equal three single calls
        a1, c1 = ops.nmf(dev(Vs[b:b + 1]), A0=dev(As[b:b + 1]), C0=dev(Cs[b:b + 1]), n_iter=4, beta_loss=loss)
        assert torch.equal(A[b], a1[0]) and torch.equal(C[b], c1[0])
    As1, Cd = ops.nmf(dev(Vs), A0=dev(As), C0=dev(Cs[:1]), n_iter=4, beta_loss=loss, update_C=False)
    As2, Cr = ops.nmf(dev(Vs), A0=dev(As), C0=dev(np.repeat(Cs[:1], 3, 0)), n_iter=4, beta_loss=loss, update_C=False)
    assert torch.equal(As1, As2) and torch.equal(Cd, dev(Cs[:1])) and torch.equal(Cr[2], dev(Cs[0]))
    shared = dev(Cs[:1])
    assert ops.nmf(dev(Vs), A0=dev(As), C0=shared, n_iter=1, beta_loss=loss, update_C=False)[1].data_ptr() != shared.data_ptr()
    with pytest.raises(ValueError, match="shared dictionary"):
        ops.nmf(dev(Vs), A0=dev(As), C0=dev(Cs[:1]), n_iter=1, beta_loss=loss)


@pytest.mark.parametrize("loss", NC.LOSSES)
def test_batch_past_the_grid_cap(ops, loss):
    B, (T, F, K) = 65537, (2, 3, 2)
    g = np.random.default_rng(11)
    V = (g.standard_normal((B, T, F)) ** 2).astype(np.float32)
    A0 = np.abs(g.standard_normal((B, T, K))).astype(np.float32)
    C0 = np.abs(g.standard_normal((B, K, F))).astype(np.float32)
    assert B > ops.launch_constants()["max_grid_y"]
    A, C, tr = ops.nmf(dev(V), A0=dev(A0), C0=dev(C0), n_iter=3, beta_loss=loss, return_trace=True)
    A, C, tr = A.cpu().numpy(), C.cpu().numpy(), tr.cpu().numpy()
    for b in (0, 65534, 65535, 65536):
        check((A[b], C[b]), R.nmf(V[b], A0[b], C0[b], 3, loss), f"clip {b}")
        want = R.divergence(V[b], A[b], C[b], loss)
        assert abs(tr[b, -1] - want) <= 1e-6 * abs(want) + 1e-300


@pytest.mark.parametrize("loss", NC.LOSSES)
def test_divergence_at_the_workgroup_cap(ops, loss):
    """T F = 2 253 900 bins: ceil(T F / 8192) = 276 is past the 256 workgroups a clip is cut into."""
    T, F, K = 1100, 2049, 2
    g = np.random.default_rng(8)
    V = (g.standard_normal((T, F)) ** 2).astype(np.float32)
    A, C = R.init_factors(V, K, g.standard_normal(K * F + T * K))
    V[7, 5] = 0.0
    d = ops.nmf_divergence(dev(V)[None], dev(A)[None], dev(C)[None], loss)
    want = R.divergence(V, A, C, loss)
    assert d.shape == (1,) and abs(float(d[0]) - want) <= 1e-6 * abs(want)
    assert torch.equal(d, ops.nmf_divergence(dev(V)[None], dev(A)[None], dev(C)[None], loss))


def test_factors_on_another_device_are_refused(ops):
    V, A, C = torch.ones(1, 5, 33).cuda(), torch.ones(1, 5, 3), torch.ones(1, 3, 33)
    with pytest.raises(ValueError, match="A0 must be on the device of V"):
        ops.nmf(V, A0=A, C0=C.cuda())
    with pytest.raises(ValueError, match="C0 must be on the device of V"):
        ops.nmf(V, A0=A.cuda(), C0=C)
    with pytest.raises(ValueError, match="C must be on the device of V"):
        ops.nmf_divergence(V, A.cuda(), C)
    with pytest.raises(ValueError, match="G must be on the device of V"):
        ops.nmf_masks(torch.ones(1, 5, 33, 2).cuda(), A.cuda(), C.cuda(), torch.ones(2, 3))


@pytest.mark.parametrize("loss", NC.LOSSES)
@pytest.mark.parametrize("shape", [(5, 33, 3), (65, 129, 17), (300, 12, 4), (40, 1025, 8), (3, 2049, 5)], ids=str)
def test_divergence_and_trace(ops, shape, loss):
    for kind in NC.KINDS:
        V, A0, C0 = NC.inputs(shape, kind)
        A, C, tr = ops.nmf(dev(V)[None], A0=dev(A0)[None], C0=dev(C0)[None], n_iter=30, beta_loss=loss, return_trace=True)
        A2, C2 = ops.nmf(dev(V)[None], A0=dev(A0)[None], C0=dev(C0)[None], n_iter=30, beta_loss=loss)
        assert torch.equal(A, A2) and torch.equal(C, C2)             # the trace changes no bit of the factors
        tr = tr[0].cpu().numpy()
        assert tr.shape == (31,) and tr.dtype == np.float64
        for d, (a, c) in ((tr[0], (A0, C0)), (tr[-1], (A[0].cpu().numpy(), C[0].cpu().numpy()))):
            want = R.divergence(V, a, c, loss)
            print(f"divergence {shape} {kind} {loss}: {abs(d - want) / max(abs(want), 1e-300):.2e} relative")
            assert abs(d - want) <= 1e-6 * abs(want)
        rise = float(np.max(np.diff(tr)))
        print(f"trace {shape} {kind} {loss}: largest step {rise / tr[0]:.2e} of the first value")
        assert rise <= 1e-5 * tr[0]


def test_initialisation(ops):
    T, F, K = 17, 65, 5
    V = np.stack([NC.inputs((17, 65, 5), k)[0] for k in NC.KINDS])
    A, C = ops.nmf(dev(V), K, n_iter=0, seed=7, first_row=2)
    z = ops.randn(3, K * F + T * K, 7, 2).cpu().numpy()
    for b in range(3):
        wa, wc = R.init_factors(V[b], K, z[b])
        sp = np.spacing(np.maximum(np.abs(wa), np.float32(1e-30)))
        assert np.all(np.abs(A[b].cpu().numpy() - wa) <= sp)
        assert np.all(np.abs(C[b].cpu().numpy() - wc) <= np.spacing(np.maximum(np.abs(wc), np.float32(1e-30))))
        a1, c1 = ops.nmf(dev(V[b:b + 1]), K, n_iter=2, seed=7, first_row=2 + b)
        a3, c3 = ops.nmf(dev(V), K, n_iter=2, seed=7, first_row=2)
        assert torch.equal(a1[0], a3[b]) and torch.equal(c1[0], c3[b])
    # only the missing factor is drawn
    A2, C2 = ops.nmf(dev(V), A0=A, n_iter=0, seed=7, first_row=2)
    assert torch.equal(A2, A) and torch.equal(C2, C)


@pytest.mark.parametrize("shape", [(5, 33, 3), (65, 129, 17), (9, 257, 64), (8, 256, 4), (3, 2049, 5)], ids=str)
def test_masks(ops, shape):
    T, F, K = shape
    g = np.random.default_rng(5)
    V = np.abs(g.standard_normal((T, F))).astype(np.float32)
    A0, C0 = R.init_factors(V, K, g.standard_normal(K * F + T * K))
    A, C = R.nmf(V, A0, C0, 2, "frobenius", dtype=np.float32)
    A[0, :] = 0.0                                                    # a frame whose model is 0: the eps branch
    D = (g.standard_normal((T, F)) + 1j * g.standard_normal((T, F))).astype(np.complex64)
    Dd = torch.view_as_real(torch.from_numpy(D)).contiguous().cuda()
    split = np.zeros((2, K), np.float32)
    split[0, :(K + 1) // 2] = 1
    split[1, (K + 1) // 2:] = 1
    peak = float(np.abs(D).max())
    for G in (None, np.ones((1, K), np.float32), split):
        out = ops.nmf_masks(Dd[None], dev(A)[None], dev(C)[None], None if G is None else dev(G))
        got = torch.view_as_complex(out[0]).cpu().numpy()
        want = R.masks(D, A, C, np.eye(K) if G is None else G)
        assert got.shape == want.shape
        e = float(np.abs(got - want).max()) / peak
        print(f"masks {shape} groups {got.shape[0]}: {e:.2e} of |D|'s peak")
        assert e <= 1e-5
        ok = (A.astype(np.float64) @ C.astype(np.float64)) >= R.EPS      # a partition adds up to D where AC >= eps
        assert ok.any() and not ok[0].any()
        s = float(np.abs(got.astype(np.complex128).sum(axis=0) - D)[ok].max()) / peak
        print(f"masks {shape} groups {got.shape[0]}: partition sums to D within {s:.2e}")
        assert s <= 1e-6


def test_decompose_and_separation(ops):
    from sygnals_amd.core import decompose as DC
    g = np.random.default_rng(3)
    t = np.arange(8192) / 22050.0
    y = np.stack([np.sin(2 * np.pi * 440 * t) + 0.5 * np.sin(2 * np.pi * 1500 * t) * (t > 0.2) + 0.05 * g.standard_normal(8192),
                  g.standard_normal(8192) * np.exp(-8 * t)]).astype(np.float32)
    yd = dev(y)
    out, A, C = DC.separate_components_batch(yd, 4, n_iter=10, return_factors=True)
    assert out.shape == (2, 4, 8192) and A.shape == (2, 17, 4) and C.shape == (2, 4, 1025)
    rt = ops.istft2048(ops.stft2048_c2c(yd), length=8192)
    e = float((out.sum(dim=1) - rt).abs().max() / rt.abs().max())
    print(f"separation: components sum to the STFT round trip within {e:.2e} of the peak")
    assert e <= 1e-5
    one = DC.separate_components(y[0], 22050, 4, n_iter=10)
    assert one.shape == (4, 8192) and np.array_equal(one, out[0].cpu().numpy())
    # decompose: librosa's orientation, the same factors as the batch form; sort orders by the peak bin
    S = ops.cabs_pow(ops.stft2048_c2c(yd), 1)
    comps, acts = DC.decompose(S[0].T.cpu().numpy(), 4, n_iter=10)
    assert comps.shape == (1025, 4) and acts.shape == (4, 17)
    assert np.array_equal(comps.T, C[0].cpu().numpy()) and np.array_equal(acts.T, A[0].cpu().numpy())
    cs, as_ = DC.decompose(S[0].T.cpu().numpy(), 4, n_iter=10, sort=True)
    order = np.argsort(np.argmax(comps, axis=0), kind="stable")
    assert np.array_equal(cs, comps[:, order]) and np.array_equal(as_, acts[order])
    # fit=False: the dictionary stays, the activations are those of ops.nmf with update_C=False
    c2, a2 = DC.decompose(S[1].T.cpu().numpy(), n_iter=5, fit=False, components=comps, seed=4)
    wa, wc = ops.nmf(S[1:2], A0=None, C0=dev(comps.T)[None], n_iter=5, update_C=False, seed=4)
    assert np.array_equal(c2, comps) and np.array_equal(a2.T, wa[0].cpu().numpy())
