"""Spectrogram decomposition on the device: `librosa.decompose.decompose` with scikit-learn's multiplicative-update NMF
as its transformer, and the separation of a clip into its components, over the kernels of csrc/nmf.hip.  The reference
package has no such functions, so there is nothing to mirror: the float64 restatement tests/nmf_ref.py, pinned to
scikit-learn's solver="mu" at tol=0, is the contract.

`decompose` takes one non-negative matrix in librosa's orientation, S [F, T], and returns (components [F, K],
activations [K, T]) as NumPy; `decompose_batch` works on float32 device tensors in the device layout (V [B, T, F] ->
activations A [B, T, K], components C [B, K, F]) and stays on the device.  Served: beta_loss "frobenius" or
"kullback-leibler", 1 to 64 components, 1 to 2049 bins, random or given starting factors; exactly n_iter iterations
run.  Itakura-Saito, the coordinate-descent solver (librosa's default transformer) and the nndsvd initialisations raise
ValueError.

`separate_components` goes clip -> STFT (n_fft 2048, hann, hop 512, centred) -> magnitudes -> NMF -> soft masks -> inverse
STFT: one signal per component, which together add up to the clip's own STFT round trip."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import ops

__all__ = ["decompose", "decompose_batch", "separate_components", "separate_components_batch"]

torch = ops.torch


def _sort_by_peak(A, C):
    """Components ordered by the bin of their peak (librosa's sort=True), the activations with them."""
    order = torch.argsort(torch.argmax(C, dim=2), dim=1, stable=True)                      # [B, K]
    C = torch.gather(C, 1, order[:, :, None].expand_as(C))
    A = torch.gather(A, 2, order[:, None, :].expand_as(A))
    return A, C, order


def decompose_batch(V, n_components: Optional[int] = None, *, n_iter: int = 200, beta_loss="frobenius", fit: bool = True,
                    components=None, activations=None, sort: bool = False, seed: int = 0, first_row: int = 0,
                    return_trace: bool = False):
    """V [B, T, F] float32 on the device -> (activations A [B, T, K], components C [B, K, F]) (ops.nmf).  fit=False keeps
    `components` ([B, K, F], or [1, K, F] for every clip) and finds the activations alone."""
    who = "decompose_batch"
    if not fit and components is None:
        raise ValueError(f"{who}: fit=False needs components")
    if sort and not fit:
        raise ValueError(f"{who}: sort=True reorders learned components; with fit=False they are the caller's")
    res = ops.nmf(V, n_components, A0=activations, C0=components, n_iter=n_iter, beta_loss=beta_loss, update_C=bool(fit),
                  seed=seed, first_row=first_row, return_trace=return_trace)
    A, C = res[0], res[1]
    if sort:
        A, C, _ = _sort_by_peak(A, C)
    return (A, C, res[2]) if return_trace else (A, C)


def decompose(S, n_components: Optional[int] = None, *, n_iter: int = 200, beta_loss="frobenius", fit: bool = True,
              components=None, sort: bool = False, seed: int = 0):
    """librosa.decompose.decompose(S, n_components, transformer=NMF(solver="mu", init="random", tol=0, max_iter=n_iter),
    fit=fit, sort=sort) of one non-negative matrix S [F, T]: (components [F, K], activations [K, T]), float32 NumPy.
    `components` [F, K] start the components, and stay as given with fit=False; `seed` takes the place of random_state."""
    who = "decompose"
    a = S.detach().cpu().numpy() if hasattr(S, "detach") else np.asarray(S)
    if a.ndim != 2 or a.dtype.kind not in "fiu" or a.size == 0:
        raise ValueError(f"{who}: S must be a real non-negative matrix [F, T] (got shape {list(a.shape)}); "
                         f"decompose_batch takes batches")
    if not np.all(np.isfinite(a)) or np.min(a) < 0:
        raise ValueError(f"{who}: S must be non-negative and finite")
    F, Tn = a.shape
    C0 = None
    if components is not None:
        c = np.asarray(components)
        if c.ndim != 2 or c.shape[0] != F or c.dtype.kind not in "fiu" or (n_components is not None and c.shape[1] != n_components):
            raise ValueError(f"{who}: components must be a real matrix [{F}, K] (got shape {list(c.shape)})")
        if not np.all(np.isfinite(c)) or np.min(c) < 0:
            raise ValueError(f"{who}: components must be non-negative and finite")
        C0 = torch.from_numpy(np.array(c.T[None], dtype=np.float32, order="C"))
    elif not fit:
        raise ValueError(f"{who}: fit=False needs components")
    if sort and not fit:
        raise ValueError(f"{who}: sort=True reorders learned components; with fit=False they are the caller's")
    V = torch.from_numpy(np.array(a.T[None], dtype=np.float32, order="C"))
    ops._nmf_loss(who, beta_loss)
    ops._nmf_factors(who, V, None, C0, n_components if C0 is None else None)
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
        raise ValueError(f"{who}: n_iter must be a non-negative integer (got {n_iter!r})")
    dev = ops.require_gpu()
    A, C = decompose_batch(V.to(dev), n_components, n_iter=n_iter, beta_loss=beta_loss, fit=fit,
                           components=C0.to(dev) if C0 is not None else None, sort=sort, seed=seed)
    return C[0].T.contiguous().cpu().numpy(), A[0].T.contiguous().cpu().numpy()


def separate_components_batch(y, n_components: int, *, n_iter: int = 200, beta_loss="frobenius", groups=None,
                              components=None, fit: bool = True, seed: int = 0, first_row: int = 0,
                              return_factors: bool = False):
    """Clips y [B, L] float32 on the device -> [B, n_groups, L]: stft2048_c2c -> magnitudes -> ops.nmf -> ops.nmf_masks ->
    istft2048(length=L).  groups [n_groups, K] weights the components of each output (default: one output a component);
    the outputs of a partition add up to istft2048(stft2048_c2c(y))."""
    who = "separate_components_batch"
    ops._f32(y, f"{who}: y", 2, (), "[B, L]")
    B, L = int(y.shape[0]), int(y.shape[1])
    if B < 1 or L < 1:
        raise ValueError(f"{who}: empty input (y has shape {list(y.shape)})")
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or not 1 <= n_components <= 64:
        raise ValueError(f"{who}: n_components={n_components!r} must be an integer in [1, 64]")
    ops._nmf_loss(who, beta_loss)
    D = ops.stft2048_c2c(y)
    S = ops.cabs_pow(D, 1)
    A, C = decompose_batch(S, int(n_components), n_iter=n_iter, beta_loss=beta_loss, fit=fit, components=components,
                           seed=seed, first_row=first_row)
    M = ops.nmf_masks(D, A, C, groups)                                                    # [B, G, T, 1025, 2]
    G, Tn = int(M.shape[1]), int(M.shape[2])
    out = ops.istft2048(M.view(B * G, Tn, 1025, 2), length=L).reshape(B, G, L)
    return (out, A, C) if return_factors else out


def separate_components(y, sr=None, n_components: int = 2, *, n_iter: int = 200, beta_loss="frobenius", seed: int = 0):
    """One clip y [L] -> its components [K, L] as float32 NumPy (sr is accepted for symmetry with the other clip functions;
    the STFT geometry is fixed)."""
    a = np.asarray(y.detach().cpu().numpy() if hasattr(y, "detach") else y)
    if a.ndim != 1 or a.dtype.kind not in "fiu" or a.size == 0:
        raise ValueError(f"separate_components: y must be one real clip [L] (got shape {list(a.shape)}); "
                         f"separate_components_batch takes batches")
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or not 1 <= n_components <= 64:
        raise ValueError(f"separate_components: n_components={n_components!r} must be an integer in [1, 64]")
    ops._nmf_loss("separate_components", beta_loss)
    yd = ops.to_device_f32(np.asarray(a, dtype=np.float32)[None])
    return separate_components_batch(yd, int(n_components), n_iter=n_iter, beta_loss=beta_loss, seed=seed)[0].cpu().numpy()
