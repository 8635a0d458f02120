"""Device dynamic time warping against the float64 restatement tests/dtw_ref.py.

Gates (the first two are derived, not measured):
  G1  cost kernel: |C_dev - C_ref64| <= 1e-5 max C_ref64 per pair.
  G2  recurrence and backtrack fed a float32 C, the restatement fed the same C: with the default weights D (bit for bit),
      the step codes and the path are identical, in both forms; with other weights D is within 1e-12 relative, the path
      is valid and its float64 cost over C equals D_ref[end] within 1e-12 relative.
  G3  end to end from X and Y: |D_dev[n, m] - D_ref[n, m]| <= 1e-5 (n + m + 1) max|w_mul| max C_ref (every path into
      (n, m) has at most n + m + 1 cells and min is 1-Lipschitz); the device path is valid and its cost over the float64
      C_ref is within the same bound of D_ref[end].  On integer-valued features with cityblock / sqeuclidean float32 is
      exact and D, steps and path are identical end to end, ties included.
"""
import numpy as np
import pytest
import torch

from tests import dtw_ref as R

pytestmark = pytest.mark.gpu

W2 = ((1.5, 0.75, 2.0), (0.0, 0.25, 0.5))
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 257)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tied_cost(rng, N, M):
    """float32 costs full of ties: small integers, with a sprinkling of fractions"""
    C = rng.integers(0, 4, size=(N, M)).astype(np.float32)
    frac = rng.random((N, M)) < 0.25
    C[frac] += rng.random(int(frac.sum())).astype(np.float32)
    return C


def _run(C, **kw):
    from sygnals_amd import ops
    C = np.asarray(C, dtype=np.float32)
    r = ops.dtw(_dev(C[None] if C.ndim == 2 else C), **kw)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in r.items()}


def _check_identical(C, subseq=False, forms=(("resident", 0),), what=""):
    """G2 with the default weights: D bit for bit, steps, end column, cost and path, in every form asked for"""
    D, steps, wp, start = R.dtw(C, subseq=subseq)
    N, M = C.shape
    for form, tile in forms:
        r = _run(C, subseq=subseq, want_D=True, want_steps=True, form=form, tile=tile)
        tag = f"{what} {N}x{M} subseq={subseq} {form}/{tile}"
        assert np.array_equal(r["D"][0], D), tag
        assert np.array_equal(r["steps"][0], steps), tag
        assert r["end_col"][0] == start and r["cost"][0] == D[-1, start], tag
        n = int(r["path_len"][0])
        assert n == len(wp) and np.array_equal(r["path"][0, :n], wp), tag
        assert (r["path"][0, n:] == -1).all(), tag


def test_g1_cost_kernel():
    from sygnals_amd import ops
    rng = np.random.default_rng(11)
    worst = 0.0
    for K in (1, 2, 13, 40, 128, 129):
        N, M = (65, 129) if K != 13 else (257, 63)
        X = rng.standard_normal((3, K, N)).astype(np.float32)
        Y = rng.standard_normal((3, K, M)).astype(np.float32)
        for metric in ("euclidean", "sqeuclidean", "cityblock", "cosine"):
            Cd = ops.dtw_cost(_dev(X), _dev(Y), metric).cpu().numpy()
            for b in range(3):
                ref = R.cost_matrix(X[b], Y[b], metric)
                frac = np.max(np.abs(Cd[b] - ref)) / (1e-5 * np.max(ref))
                worst = max(worst, frac)
                assert frac <= 1.0, (K, metric, frac)
    print(f"G1 worst fraction of the gate: {worst:.3f}")


def test_cost_strided_ragged_and_shared():
    """ld > length, NaN in the padding of a ragged batch, a batch stride of 0, and a batch equal to its pairs"""
    from sygnals_amd import ops
    rng = np.random.default_rng(12)
    B, K, N, M = 3, 13, 70, 130
    Xf = rng.standard_normal((B, K, N + 9)).astype(np.float32)
    Yf = rng.standard_normal((B, K, M + 5)).astype(np.float32)
    xl, yl = np.array([70, 1, 33]), np.array([64, 130, 1])
    for b in range(B):
        Xf[b, :, xl[b]:] = np.nan
        Yf[b, :, yl[b]:] = np.nan
    Xd, Yd = _dev(Xf)[:, :, :N], _dev(Yf)[:, :, :M]                   # row stride above the length
    Cd = ops.dtw_cost(Xd, Yd, "euclidean", xl, yl).cpu().numpy()
    assert np.isfinite(Cd).all()
    for b in range(B):
        ref = R.cost_matrix(Xf[b, :, :xl[b]], Yf[b, :, :yl[b]])
        assert np.max(np.abs(Cd[b, :xl[b], :yl[b]] - ref)) <= 1e-5 * np.max(ref)
        assert (Cd[b, xl[b]:, :] == 0).all() and (Cd[b, :, yl[b]:] == 0).all()
        one = ops.dtw_cost(Xd[b:b + 1], Yd[b:b + 1], "euclidean", xl[b:b + 1], yl[b:b + 1]).cpu().numpy()
        assert np.array_equal(one[0], Cd[b])                          # a batch equals its pairs
    X1 = _dev(Xf[:1, :, :N][:, :, :60].copy())
    shared = ops.dtw_cost(X1.expand(B, K, 60), Yd, "cityblock", None, yl).cpu().numpy()
    for b in range(B):
        ref = R.cost_matrix(Xf[0, :, :60], Yf[b, :, :yl[b]], "cityblock")
        assert np.max(np.abs(shared[b, :, :yl[b]] - ref)) <= 1e-5 * np.max(ref)


def test_g2_sizes_both_forms():
    rng = np.random.default_rng(13)
    for i, (N, M) in enumerate((n, m) for n in SIZES for m in SIZES):
        _check_identical(_tied_cost(rng, N, M), subseq=(i % 3 == 0), forms=(("resident", 0), ("tiled", 64)))


def test_g2_run_and_wave_boundaries():
    """the widths at which a lane's column run doubles, the last lane fills, and the resident form ends"""
    from sygnals_amd import ops
    k = ops.dtw_constants()
    rng = np.random.default_rng(14)
    top = k["resident_max_cols"]
    widths = sorted({w + d for w in (64, 128, 256, 512, top) for d in (-1, 0, 1)} | {3 * 63, 4 * 63 + 1, 16 * 63})
    for M in widths:
        for N in (3, 70):
            form = "resident" if M <= top else None                   # one past the widest: the rule takes the tiled form
            _check_identical(_tied_cost(rng, N, M), subseq=(M % 2 == 0), forms=((form, 0),))
    assert ops.dtw_plan(1, 3, top + 1)["form"] == "tiled" and ops.dtw_plan(1, 3, top)["form"] == "resident"
    for N, M in ((1, 300), (300, 1), (5, 1000), (1000, 5)):
        _check_identical(_tied_cost(rng, N, M), forms=(("resident", 0), ("tiled", 0)))


def test_g2_vector_form_and_its_fallbacks():
    """widths that are multiples of four move a lane's run in 16-byte pieces (runs of 4, 8 and 16 columns, both forms,
    batches); a view whose rows start off 16 bytes, and a ragged width, take the element form: all give the same bits"""
    from sygnals_amd import ops
    rng = np.random.default_rng(25)
    for N, M, tiles in ((130, 256, (64, 128, 256)), (67, 512, (256, 512)), (70, 1000, (256, 500, 1000)), (9, 1024, (1024,)),
                        (300, 260, (132,))):
        for subseq in (False, True):
            _check_identical(_tied_cost(rng, N, M), subseq=subseq, forms=(("resident", 0),) + tuple(("tiled", t) for t in tiles))
    B, N, M = 3, 37, 256
    C = np.stack([_tied_cost(rng, N, M + 8) for _ in range(B)])
    Cd = _dev(C)
    refs = [R.dtw(C[b, :, 1:M + 1]) for b in range(B)]
    aligned = [R.dtw(C[b, :, 4:M + 4]) for b in range(B)]
    for form, tile in (("resident", 0), ("tiled", 64), ("tiled", 128)):
        for view, want in ((Cd[:, :, 1:M + 1], refs), (Cd[:, :, 4:M + 4], aligned)):     # rows 4 bytes / 16 bytes off the start
            r = ops.dtw(view, want_D=True, want_steps=True, form=form, tile=tile)
            for b in range(B):
                D, steps, wp, _ = want[b]
                assert np.array_equal(r["D"][b].cpu().numpy(), D) and np.array_equal(r["steps"][b].cpu().numpy(), steps)
                assert np.array_equal(r["path"][b, :int(r["path_len"][b])].cpu().numpy(), wp)
        yl = np.array([256, 255, 4])
        r = ops.dtw(Cd[:, :, 4:M + 4], y_len=yl, want_D=True, form=form, tile=tile)
        for b in range(B):
            D = R.dtw(C[b, :, 4:4 + yl[b]])[0]
            assert np.array_equal(r["D"][b, :, :yl[b]].cpu().numpy(), D)


def test_g2_tiled_seams_small_tile():
    rng = np.random.default_rng(15)
    shapes = [(8, 8), (5, 7), (15, 15), (16, 16), (17, 17), (15, 17), (17, 16), (16, 9), (3, 20), (20, 3), (1, 1), (1, 9), (9, 1),
              (25, 40)]
    for N, M in shapes:
        for subseq in (False, True):
            _check_identical(_tied_cost(rng, N, M), subseq=subseq, forms=(("tiled", 8), ("tiled", 3), ("tiled", 1)))


def test_g2_tiled_large_pair_product_tile():
    """one pair of 4097 x 3001 at the product tile, compared in full with the vectorised restatement"""
    rng = np.random.default_rng(16)
    C = _tied_cost(rng, 4097, 3001)
    _check_identical(C, forms=((None, 0),))


def test_g2_weights():
    rng = np.random.default_rng(17)
    worst = 0.0
    for N, M in ((1, 1), (2, 65), (64, 64), (129, 63), (70, 300)):
        for subseq in (False, True):
            C = (rng.random((N, M)) + 0.01).astype(np.float32)
            D, steps, wp, start = R.dtw(C, W2[0], W2[1], subseq=subseq)
            for form, tile in (("resident", 0), ("tiled", 32)):
                r = _run(C, weights_mul=W2[0], weights_add=W2[1], subseq=subseq, want_D=True, form=form, tile=tile)
                rel = np.max(np.abs(r["D"][0] - D) / np.abs(D))
                worst = max(worst, rel)
                assert rel <= 1e-12
                p = r["path"][0, :int(r["path_len"][0])]
                R.check_path(p, N, M, subseq=subseq, start=int(r["end_col"][0]))
                pc = R.path_cost(C.astype(np.float64), p, *W2)
                assert abs(pc - D[-1, start]) <= 1e-12 * abs(D[-1, start])
    print(f"G2 (weights) worst relative difference of D: {worst:.3e}")


@pytest.mark.parametrize("B", [1, 3, 33])
def test_ragged_batches_equal_their_pairs(B):
    """per-pair lengths (length 1 included), NaN in every padding cell; a batch equals its pairs; the same call twice"""
    rng = np.random.default_rng(18 + B)
    N, M = 70, 131
    xl = rng.integers(1, N + 1, size=B); yl = rng.integers(1, M + 1, size=B)
    xl[0], yl[0] = N, M
    if B > 1:
        xl[1], yl[1] = 1, 1
    if B > 2:
        xl[2], yl[2] = 1, M
    C = np.stack([_tied_cost(rng, N, M) for _ in range(B)])
    for b in range(B):
        C[b, xl[b]:, :] = np.nan
        C[b, :, yl[b]:] = np.nan
    for subseq in (False, True):
        refs = [R.dtw(C[b, :xl[b], :yl[b]], subseq=subseq) for b in range(B)]
        for form, tile in (("resident", 0), ("tiled", 32)):
            kw = dict(subseq=subseq, want_D=True, want_steps=True, form=form, tile=tile)
            r = _run(C, x_len=xl, y_len=yl, **kw)
            r2 = _run(C, x_len=xl, y_len=yl, **kw)
            for k in r:
                assert np.array_equal(r[k], r2[k], equal_nan=True), k     # the same call twice gives the same bits
            assert np.isfinite(r["D"]).all() and np.isfinite(r["cost"]).all()
            for b in range(B):
                D, steps, wp, start = refs[b]
                assert np.array_equal(r["D"][b, :xl[b], :yl[b]], D) and np.array_equal(r["steps"][b, :xl[b], :yl[b]], steps)
                assert r["cost"][b] == D[-1, start] and r["end_col"][b] == start
                n = int(r["path_len"][b])
                assert np.array_equal(r["path"][b, :n], wp) and (r["path"][b, n:] == -1).all()
            for b in sorted({0, 1, 2, B - 1} & set(range(B))):            # a batch equals its pairs
                one = _run(C[b:b + 1], x_len=xl[b:b + 1], y_len=yl[b:b + 1], **kw)
                for k in r:
                    assert np.array_equal(one[k][0], r[k][b], equal_nan=True), (k, b)


def test_subseq_orientations_and_tied_minima():
    rng = np.random.default_rng(19)
    for N, M in ((7, 400), (64, 64), (129, 129), (5, 1030)):
        C = rng.integers(0, 3, size=(N, M)).astype(np.float32)           # integers: the last row is full of tied minima
        D, _, _, start = R.dtw(C, subseq=True)
        assert (D[-1] == D[-1].min()).sum() >= 2 and start == int(np.argmin(D[-1]))
        forms = (("resident", 0), ("tiled", 16)) if M <= 1024 else ((None, 0), ("tiled", 100))
        _check_identical(C, subseq=True, forms=forms)


def test_distance_only_equals_the_full_path():
    rng = np.random.default_rng(20)
    B, N, M = 5, 94, 101
    C = rng.random((B, N, M)).astype(np.float32)
    for subseq in (False, True):
        for form, tile in (("resident", 0), ("tiled", 40)):
            full = _run(C, subseq=subseq, want_D=True, form=form, tile=tile)
            dist = _run(C, subseq=subseq, want_path=False, form=form, tile=tile)
            assert dist["D"] is None and dist["steps"] is None and dist["path"] is None
            assert np.array_equal(dist["cost"], full["cost"]) and np.array_equal(dist["end_col"], full["end_col"])
            for b in range(B):
                assert full["cost"][b] == full["D"][b, -1, full["end_col"][b]]


def test_g3_end_to_end():
    import sygnals_amd.core.alignment as A
    rng = np.random.default_rng(21)
    worst = 0.0
    for K, N, M, metric in ((1, 129, 65, "euclidean"), (13, 94, 94, "euclidean"), (40, 64, 257, "cityblock"),
                            (128, 63, 127, "sqeuclidean"), (129, 65, 64, "cosine"), (13, 130, 128, "cosine")):
        X = rng.standard_normal((K, N)).astype(np.float32)
        Y = rng.standard_normal((K, M)).astype(np.float32)
        if metric == "cosine":
            X += 0.5; Y += 0.5                                           # K = 1 aside, keep the norms away from zero
        for wm, wa in ((None, None), W2):
            Cref = R.cost_matrix(X, Y, metric)
            Dref, _, _, _ = R.dtw(Cref, wm, wa)
            D, wp = A.dtw(X, Y, metric=metric, weights_mul=wm, weights_add=wa)
            scale = 1e-5 * (1.0 if wm is None else max(np.abs(wm))) * np.max(Cref)
            n, m = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
            frac = np.max(np.abs(D - Dref) / (scale * (n + m + 1)))
            worst = max(worst, frac)
            assert frac <= 1.0, (K, metric, frac)
            R.check_path(wp, N, M)
            assert abs(R.path_cost(Cref, wp, wm, wa) - Dref[-1, -1]) <= scale * (N + M - 1)
    print(f"G3 worst fraction of the gate: {worst:.3e}")


@pytest.mark.parametrize("metric", ["cityblock", "sqeuclidean"])
def test_g3_integer_features_identical_end_to_end(metric):
    import sygnals_amd.core.alignment as A
    rng = np.random.default_rng(22)
    for K, N, M in ((1, 65, 130), (4, 129, 94), (13, 64, 64)):
        X = rng.integers(-3, 4, size=(K, N)).astype(np.float32)
        Y = rng.integers(-3, 4, size=(K, M)).astype(np.float32)
        for subseq in (False, True):
            Dref, sref, wpref, _ = R.dtw(R.cost_matrix(X, Y, metric), subseq=subseq)
            D, wp, steps = A.dtw(_dev(X), Y, metric=metric, subseq=subseq, return_steps=True)
            assert np.array_equal(D, Dref) and np.array_equal(steps, sref) and np.array_equal(wp, wpref)


@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "cityblock"])
def test_identical_sequences(metric):
    import sygnals_amd.core.alignment as A
    X = np.random.default_rng(23).standard_normal((13, 150)).astype(np.float32)
    D, wp = A.dtw(X, X, metric=metric)
    assert D[-1, -1] == 0.0 and np.array_equal(wp[::-1], np.stack([np.arange(150)] * 2, axis=1))
    Xd = _dev(np.stack([X, 2 * X]))
    cost, path, plen = A.dtw_batch(Xd, Xd.clone(), metric=metric)
    assert (cost.cpu().numpy() == 0.0).all() and (plen.cpu().numpy() == 150).all()
    assert (A.dtw_distance_batch(Xd, Xd, metric=metric).cpu().numpy() == 0.0).all()


def test_mirror_options():
    """(K, N) and (N,) inputs, tensors and arrays, a caller's C, backtrack=False, return_steps, dtypes"""
    import sygnals_amd.core.alignment as A
    rng = np.random.default_rng(24)
    x, y = rng.integers(0, 5, size=40).astype(np.float64), rng.integers(0, 5, size=55).astype(np.float64)
    Dref, sref, wpref, _ = R.dtw(R.cost_matrix(x, y, "cityblock"))
    D, wp = A.dtw(x, y, metric="cityblock")
    assert D.dtype == np.float64 and D.shape == (40, 55) and np.issubdtype(wp.dtype, np.integer)
    assert np.array_equal(D, Dref) and np.array_equal(wp, wpref)
    D2 = A.dtw(x, y, metric="cityblock", backtrack=False)
    assert isinstance(D2, np.ndarray) and np.array_equal(D2, Dref)
    D3, steps = A.dtw(x, y, metric="cityblock", backtrack=False, return_steps=True)
    assert np.array_equal(D3, Dref) and np.array_equal(steps, sref) and np.issubdtype(steps.dtype, np.integer)
    Cm = _tied_cost(rng, 33, 70)
    for subseq in (False, True):
        Dr, sr, wr, _ = R.dtw(Cm, subseq=subseq)
        for Cin in (Cm, _dev(Cm)):
            D, wp, steps = A.dtw(C=Cin, subseq=subseq, return_steps=True)
            assert np.array_equal(D, Dr) and np.array_equal(wp, wr) and np.array_equal(steps, sr)
    Dr, _, wr, _ = R.dtw(Cm, *W2)
    D, wp = A.dtw(C=Cm, weights_mul=W2[0], weights_add=W2[1], step_sizes_sigma=np.array([[1, 1], [0, 1], [1, 0]]))
    assert np.max(np.abs(D - Dr) / np.abs(Dr)) <= 1e-12
    R.check_path(wp, 33, 70)
    assert abs(R.path_cost(Cm.astype(np.float64), wp, *W2) - Dr[-1, -1]) <= 1e-12 * Dr[-1, -1]
    # the batch mirror on a caller's C and on (X, Y), D when asked for
    Cb = _dev(np.stack([Cm, Cm[::-1].copy()]))
    cost, path, plen, Db = A.dtw_batch(C=Cb, return_D=True)
    assert cost.dtype == torch.float64 and path.shape == (2, 33 + 70 - 1, 2) and path.dtype == torch.int32 and Db.is_cuda
    assert np.array_equal(Db[0].cpu().numpy(), R.dtw(Cm)[0]) and np.array_equal(Db[1].cpu().numpy(), R.dtw(Cm[::-1])[0])
    assert np.array_equal(A.dtw_distance_batch(C=Cb).cpu().numpy(), cost.cpu().numpy())


def test_cli_dtw(tmp_path):
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli.main import cli
    import pandas as pd
    sr = 16000
    t = np.arange(sr) / sr
    a = np.sin(2 * np.pi * (300 + 500 * t) * t)
    b = np.concatenate([np.zeros(2048), a])[:sr]                          # the same sweep, four hops late
    for name, v in (("a.wav", a), ("b.wav", b)):
        wavfile.write(tmp_path / name, sr, (v * 20000).astype(np.int16))
    r = CliRunner().invoke(cli, ["dsp", "dtw", str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), "-o", str(tmp_path / "p.npz")])
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "p.npz")
    T = 1 + sr // 512
    assert int(z["hop_length"]) == 512 and str(z["metric"]) == "euclidean" and float(z["cost"]) >= 0
    R.check_path(z["path"], T, T)
    x = np.round(np.sin(np.arange(60) * 0.3) * 4)
    pd.DataFrame({"value": x}).to_csv(tmp_path / "x.csv", index=False)
    pd.DataFrame({"value": np.repeat(x, 2)}).to_csv(tmp_path / "y.csv", index=False)
    r = CliRunner().invoke(cli, ["dsp", "dtw", str(tmp_path / "x.csv"), str(tmp_path / "y.csv"), "-o", str(tmp_path / "q.csv"),
                                 "--metric", "cityblock"])
    assert r.exit_code == 0, r.output
    tab = pd.read_csv(tmp_path / "q.csv")
    assert list(tab.columns) == ["index_x", "index_y", "time_x", "time_y"]
    wp = tab[["index_x", "index_y"]].to_numpy()[::-1]
    R.check_path(wp, 60, 120)
    assert R.path_cost(R.cost_matrix(x, np.repeat(x, 2), "cityblock"), wp) == 0.0
