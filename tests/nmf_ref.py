"""The contract of the device NMF: scikit-learn's multiplicative-update solver (`_fit_multiplicative_update` at tol = 0, no
regularisation, gamma = 1) restated in NumPy, in this project's frame-major orientation.

    V [T, F] = A [T, K] C [K, F];    A is sklearn's W (activations), C its H (components), V its X (= S.T of librosa).

Every function takes `dtype`: float64 is the contract, float32 the same code in the device's number format, which is the
rounding floor the GPU tests are conditioned on.  tests/test_nmf_ref.py pins this file to sklearn where sklearn exists.
Under Kullback-Leibler sklearn zeroes the entries of H below float64's epsilon (2.2e-16) after each update of H ("necessary
for stability with beta_loss < 1", applied at beta_loss <= 1); without that step the factors drift from sklearn's by
4e-12 of the peak within 50 iterations, so it is part of the contract: C_FLUSH."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)            # sklearn.decomposition._nmf.EPSILON
LOSSES = ("frobenius", "kullback-leibler")
C_FLUSH = float(np.finfo(np.float64).eps)        # KL: entries of C below this become 0 after the C-step


def _kl_ratio(V, A, C):
    WH = A @ C
    WH[WH < EPS] = EPS
    return V / WH


def step_A(V, A, C, loss):
    """The A-step (sklearn's _multiplicative_update_w): a new A."""
    if loss == "frobenius":
        num = V @ C.T
        den = A @ (C @ C.T)
    else:
        num = _kl_ratio(V, A, C) @ C.T
        den = np.repeat(C.sum(axis=1)[None, :], A.shape[0], axis=0)
    den = np.where(den == 0, np.asarray(EPS, den.dtype), den)
    return A * (num / den)


def step_C(V, A, C, loss):
    """The C-step (sklearn's _multiplicative_update_h): a new C."""
    if loss == "frobenius":
        num = A.T @ V
        den = (A.T @ A) @ C
    else:
        num = A.T @ _kl_ratio(V, A, C)
        den = np.repeat(A.sum(axis=0)[:, None], C.shape[1], axis=1)
    den = np.where(den == 0, np.asarray(EPS, den.dtype), den)
    C = C * (num / den)
    if loss != "frobenius":
        C[C < C_FLUSH] = 0.0
    return C


def nmf(V, A, C, n_iter, loss="frobenius", update_A=True, update_C=True, dtype=np.float64):
    """n_iter iterations (A-step, then C-step with the new A) from the given factors: (A, C) in `dtype`."""
    assert loss in LOSSES
    V, A, C = (np.array(x, dtype=dtype) for x in (V, A, C))
    for _ in range(int(n_iter)):
        if update_A:
            A = step_A(V, A, C, loss)
        if update_C:
            C = step_C(V, A, C, loss)
    return A, C


def divergence(V, A, C, loss="frobenius"):
    """sklearn's _beta_divergence (not its square root) in float64."""
    V, A, C = (np.asarray(x, dtype=np.float64) for x in (V, A, C))
    WH = A @ C
    if loss == "frobenius":
        return 0.5 * float(np.sum((V - WH) ** 2))
    keep = V > EPS
    wh = np.maximum(WH[keep], EPS)
    v = V[keep]
    return float(np.dot(v, np.log(v / wh)) + WH.sum() - v.sum())


def masks(D, A, C, G):
    """D [T, F] complex times each group's soft mask: [n_groups, T, F] complex128."""
    D = np.asarray(D, dtype=np.complex128)
    A, C, G = (np.asarray(x, dtype=np.float64) for x in (A, C, G))
    tot = np.maximum(A @ C, EPS)
    return np.stack([D * (((A * g[None, :]) @ C) / tot) for g in G])


def init_scale(V, K):
    """sklearn's init="random" scale sqrt(mean(V) / K) as a float32, the mean in float64."""
    return np.float32(np.sqrt(np.mean(np.asarray(V, dtype=np.float64)) / K))


def init_factors(V, K, normals):
    """(A0 [T, K], C0 [K, F]) float32 from one row of standard normals of length K F + T K: the components first, as
    sklearn draws H before W."""
    T, F = V.shape
    s = init_scale(V, K)
    z = np.abs(np.asarray(normals, dtype=np.float32))
    return (s * z[K * F:K * F + T * K].reshape(T, K)).astype(np.float32), (s * z[:K * F].reshape(K, F)).astype(np.float32)


def rel_peak(x, ref):
    """max |x - ref| over the peak of ref (0 where both are all zero)."""
    ref = np.asarray(ref, dtype=np.float64)
    d = float(np.max(np.abs(np.asarray(x, dtype=np.float64) - ref))) if ref.size else 0.0
    p = float(np.max(np.abs(ref))) if ref.size else 0.0
    return d / p if p > 0 else d
