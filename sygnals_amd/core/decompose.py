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
STFT: one signal per component, which together add up to the clip's own STFT round trip.

`nn_filter` (librosa.decompose.nn_filter) and `separate_repeating` (foreground / background by similarity, REPET-SIM)
stand at the end of the file, over the kernels of csrc/similarity.hip; tests/similarity_ref.py is their contract."""
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


# ------------------------------------------------------------------ nn_filter and separation by similarity (REPET-SIM)
# Over the kernels of csrc/similarity.hip; tests/similarity_ref.py is their contract.  (Not in __all__, which lists the
# factorisation functions; the plugin registers nn_filter and separate_repeating by name.)

def _lists_of_rec(who, rec, T):
    """A dense librosa-style matrix rec [T, T] (rec[i, j] != 0: frame i is a neighbour of frame j) as lists on the host:
    (idx [1, T, k] int32, weights [1, T, k] float32, count [1, T] int32)."""
    r = np.asarray(rec.detach().cpu().numpy() if hasattr(rec, "detach") else rec)
    if r.ndim != 2 or r.shape != (T, T) or r.dtype.kind not in "fiub":
        raise ValueError(f"{who}: rec must be a real matrix [{T}, {T}] (got shape {list(r.shape)})")
    nz = r.T != 0                                                                   # row j: the neighbours of frame j
    count = nz.sum(axis=1).astype(np.int32)
    k = max(1, int(count.max()))
    if k > ops.K_MAX:
        raise ValueError(f"{who}: a frame of rec has {k} neighbours; at most {ops.K_MAX} are served")
    idx = np.full((T, k), -1, dtype=np.int32)
    w = np.zeros((T, k), dtype=np.float32)
    for j in range(T):
        js = np.nonzero(nz[j])[0]
        idx[j, :len(js)] = js
        w[j, :len(js)] = r[js, j]
    return torch.from_numpy(idx[None]), torch.from_numpy(w[None]), torch.from_numpy(count[None])


def nn_filter_batch(S, *, aggregate: str = "mean", lists=None, features=None, k: Optional[int] = None, width: int = 1,
                    metric: str = "euclidean", bandwidth=None, return_lists: bool = False):
    """S [B, T, F] float32 on the device -> [B, T, F]: every frame replaced by the aggregate of its nearest neighbours
    (ops.sim_knn on `features` [B, T, D], by default S itself, then ops.nn_filter).  lists: (idx, count) or
    (idx, count, weights) of the caller's instead of the search.  aggregate "average" weights the neighbours by the
    caller's weights, or by the lists' affinities exp(-distance / bandwidth) (bandwidth=None: ops.sim_bandwidth of the
    rows' largest distances)."""
    who = "nn_filter_batch"
    ops._sim_name(who, "aggregate", aggregate, ops.NN_AGGREGATES)
    weights = bw = None
    if lists is not None:
        if not isinstance(lists, (tuple, list)) or len(lists) not in (2, 3):
            raise ValueError(f"{who}: lists must be (idx, count) or (idx, count, weights)")
        idx, count = lists[0], lists[1]
        if aggregate == "average":
            if len(lists) != 3:
                raise ValueError(f"{who}: aggregate='average' over the caller's lists needs their weights: (idx, count, weights)")
            weights = lists[2]
    else:
        idx, dist, count = ops.sim_knn(S if features is None else features, None, k, width, metric)
        if aggregate == "average":
            weights = dist
            if bandwidth is None:
                bw = ops.sim_bandwidth(dist.masked_fill(torch.isinf(dist), -1.0).amax(dim=2), who)    # the padding is +inf
            else:
                bw = bandwidth
    out = ops.nn_filter(S, idx, count, weights, aggregate, bandwidth=bw)
    return (out, idx, count) if return_lists else out


def nn_filter(S, rec=None, aggregate="mean", **recurrence_kwargs):
    """librosa.decompose.nn_filter(S [F, T], rec, aggregate) -> [F, T] float32 NumPy.  aggregate: "mean", "average" or
    "median" (or numpy's mean / average / median).  rec: a dense recurrence matrix [T, T], rec[i, j] != 0 where frame i
    is a neighbour of frame j, its values the weights of "average"; without it the neighbours are found on S with
    recurrence_kwargs (k, width, metric, bandwidth)."""
    who = "nn_filter"
    aggregate = {np.mean: "mean", np.average: "average", np.median: "median"}.get(aggregate, aggregate) \
        if callable(aggregate) else aggregate
    ops._sim_name(who, "aggregate", aggregate, ops.NN_AGGREGATES)
    a = S.detach().cpu().numpy() if hasattr(S, "detach") else np.asarray(S)
    if a.ndim != 2 or a.dtype.kind not in "fiu" or a.size == 0:
        raise ValueError(f"{who}: S must be a real matrix [F, T] (got shape {list(a.shape)}); nn_filter_batch takes batches")
    unknown = set(recurrence_kwargs) - {"k", "width", "metric", "bandwidth"}
    if unknown:
        raise ValueError(f"{who}: recurrence arguments served are k, width, metric and bandwidth (got {sorted(unknown)})")
    if rec is not None and recurrence_kwargs:
        raise ValueError(f"{who}: recurrence arguments apply where rec is not given")
    if "metric" in recurrence_kwargs:
        ops._sim_metric(who, recurrence_kwargs["metric"])
    lists = _lists_of_rec(who, rec, a.shape[1]) if rec is not None else None
    dev = ops.require_gpu()
    Sd = torch.from_numpy(np.array(a.T[None], dtype=np.float32, order="C")).to(dev)
    if lists is not None:
        lists = tuple(t.to(dev) for t in (lists[0], lists[2], lists[1]))
    return nn_filter_batch(Sd, aggregate=aggregate, lists=lists, **recurrence_kwargs)[0].T.contiguous().cpu().numpy()


def _repeating_args(who, width, margin_b, margin_f, power, metric):
    ops._sim_int(who, "width", width, 1, 1 << 30)
    for name, v in (("margin_background", margin_b), ("margin_foreground", margin_f), ("power", power)):
        ops._repet_number(who, name, v)
    ops._sim_metric(who, metric)


def separate_repeating_batch(y, *, width: int = 86, k: Optional[int] = None, metric: str = "cosine", margin_b: float = 2.0,
                             margin_f: float = 10.0, power: float = 2.0, return_parts: bool = False):
    """Clips y [B, L] float32 on the device -> [B, 2, L], foreground then background, by REPET-SIM (the vocal separation
    recipe of librosa's gallery): stft2048_c2c -> magnitudes -> ops.sim_knn (frames at least `width` apart) -> median
    ops.nn_filter -> ops.repet_masks -> istft2048 with both masks (length=L).  width is in frames of 512 samples
    (the default is two seconds at 22050 Hz)."""
    who = "separate_repeating_batch"
    ops._f32(y, f"{who}: y", 2, (), "[B, L]")
    B, L = int(y.shape[0]), int(y.shape[1])
    if B < 1 or L < 1:
        raise ValueError(f"{who}: empty input (y has shape {list(y.shape)})")
    _repeating_args(who, width, margin_b, margin_f, power, metric)
    D = ops.stft2048_c2c(y)
    S = ops.cabs_pow(D, 1)
    idx, dist, count = ops.sim_knn(S, None, k, int(width), metric)
    Sf = ops.nn_filter(S, idx, count, None, "median")
    Mf, Mb = ops.repet_masks(S, Sf, margin_b, margin_f, power)
    fg, bg = ops.istft2048(D, length=L, mask=(Mf, Mb))
    out = torch.stack((fg, bg), dim=1)
    return (out, D, idx, count) if return_parts else out


def separate_repeating(y, sr=22050, *, width_seconds: float = 2.0, k: Optional[int] = None, metric: str = "cosine",
                       margin_background: float = 2.0, margin_foreground: float = 10.0, power: float = 2.0):
    """One clip y [L] -> (foreground, background) [L] float32 NumPy: frames are compared with those at least
    width_seconds away (max(1, round(width_seconds sr / 512)) frames)."""
    who = "separate_repeating"
    a = np.asarray(y.detach().cpu().numpy() if hasattr(y, "detach") else y)
    if a.ndim != 1 or a.dtype.kind not in "fiu" or a.size == 0:
        raise ValueError(f"{who}: y must be one real clip [L] (got shape {list(a.shape)}); separate_repeating_batch takes batches")
    for name, v in (("sr", sr), ("width_seconds", width_seconds)):
        ops._repet_number(who, name, v)
    width = max(1, int(round(float(width_seconds) * float(sr) / 512)))
    _repeating_args(who, width, margin_background, margin_foreground, power, metric)
    yd = ops.to_device_f32(np.asarray(a, dtype=np.float32)[None])
    out = separate_repeating_batch(yd, width=width, k=k, metric=metric, margin_b=margin_background, margin_f=margin_foreground,
                                   power=power)[0].cpu().numpy()
    return out[0], out[1]
