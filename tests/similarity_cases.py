"""The gated k-NN cases of tests/test_gpu_similarity.py and the inputs they run on, shared with
tests/test_similarity_ref.py, which asserts on the CPU that each case leaves out at most 10 % of its rows from the
neighbour-set comparison (rows whose float64 gap between the k-th and the (k + 1)-th candidate is under 2e-5 of the
clip's largest kept distance: below that gap two distances within the 1e-5 gate may swap)."""
from __future__ import annotations

import numpy as np

DIST_GATE = 1e-5            # sorted kept distances, relative to the clip's largest kept distance
GAP_MIN = 2e-5              # rows with a smaller boundary gap are left out of the set comparison
LEFT_OUT_MAX = 0.10         # of a case's rows


def frames(kind, T, D, seed):
    """[T, D] float32.  normal: N(0, 1); magnitudes: |N(0, 1)|; neardup: the second half repeats the first plus 1e-3 of
    noise (the cancellation case of the dot-product form)."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((T, D)).astype(np.float32)
    if kind == "magnitudes":
        return np.abs(rng.standard_normal((T, D))).astype(np.float32)
    if kind == "neardup":
        x = rng.standard_normal((T, D))
        h = T // 2
        x[T - h:] = x[:h] + 1e-3 * rng.standard_normal((h, D))
        return x.astype(np.float32)
    raise ValueError(kind)


# (T, D, k, width, metric, kind, seed): the sizes cross the row block (16), the column tile (64), the MFMA's depth (4), the
# staged chunk of D (64) and the list's lane groups (64, 256); width = T leaves no candidate; k above the candidates.
KNN_CASES = [
    (1, 3, 1, 1, "euclidean", "normal", 1),
    (2, 1, 1, 1, "sqeuclidean", "normal", 2),
    (3, 4, 2, 1, "cosine", "normal", 3),
    (15, 5, 7, 3, "euclidean", "magnitudes", 4),
    (16, 12, 7, 1, "cosine", "magnitudes", 5),
    (16, 1, 256, 1, "cosine", "normal", 6),
    (17, 65, 64, 1, "sqeuclidean", "normal", 7),
    (63, 3, 2, 3, "euclidean", "normal", 8),
    (64, 1025, 7, 1, "cosine", "magnitudes", 9),
    (64, 12, 7, 64, "euclidean", "normal", 10),
    (65, 65, 64, 1, "euclidean", "normal", 11),
    (65, 12, 65, 1, "sqeuclidean", "normal", 12),
    (257, 12, 33, 3, "euclidean", "normal", 13),
    (257, 1025, 256, 1, "sqeuclidean", "magnitudes", 14),
    (257, 5, 65, 1, "cosine", "normal", 15),
    (257, 4, 64, 1, "euclidean", "magnitudes", 16),
    (64, 12, 1, 1, "euclidean", "neardup", 17),
    (65, 65, 2, 1, "sqeuclidean", "neardup", 18),
    (64, 1025, 1, 1, "cosine", "neardup", 19),        # k = 1: the boundary lies between the duplicate and the rest, never inside a pair
    (257, 12, 7, 1, "euclidean", "neardup", 20),
]


def case_id(c):
    return "T{}-D{}-k{}-w{}-{}-{}".format(*c[:6])
