"""The noise generator's restatement (tests/rng_ref.py) against the Random123 known answers, the host-side Philox of
sygnals_amd/_rng.py against the restatement bit for bit, and the statistics of the restatement itself.  No GPU."""
import numpy as np
import pytest

from tests import rng_ref as R

SEEDS = [0, 1, 1234, (1 << 40) + 7]
ROWS = [0, 1, 32]
LENGTHS = [4096, 65536]
LAGS = [1, 2, 3, 4, 5, 7, 8]


def test_known_answers():
    from sygnals_amd import _rng
    for ctr, key, want in R.KNOWN_ANSWERS:
        assert tuple(int(v) for v in R.philox([ctr], key)[0]) == want
        assert tuple(int(v) for v in _rng.philox([ctr], key)[0]) == want


def test_host_philox_equals_the_restatement_bit_for_bit():
    from sygnals_amd import _rng
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 1 << 32, size=(4096, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(4096, 2), dtype=np.uint64)
    ctr[:8] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0xFFFFFFFF, 0, 0, 0], [0, 0xFFFFFFFF, 0, 0], [0, 0, 0xFFFFFFFF, 0],
               [0, 0, 0, 0xFFFFFFFF], [1, 0, 0, 0], [0, 0, 1, 0]]
    a, b = _rng.philox(ctr, key), R.philox(ctr, key)
    assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape == (4096, 4) and np.array_equal(a, b)
    assert np.array_equal(_rng.philox(ctr, key[0]), R.philox(ctr, key[0]))          # one key for every counter


def test_stream_layout_of_the_host_side():
    from sygnals_amd import _rng
    seed = (0xDEADBEEF << 32) | 0x12345678
    assert [int(v) for v in _rng.key_of(seed)] == [0x12345678, 0xDEADBEEF]
    q = np.array([0, 5, (1 << 32) - 1, 1 << 32, (1 << 34) + 3], dtype=np.uint64)
    c = _rng.counters(q, 7, _rng.STREAM_NOISE)
    assert c.tolist() == [[0, 0, 7, 0], [5, 0, 7, 0], [0xFFFFFFFF, 0, 7, 0], [0, 1, 7, 0], [3, 4, 7, 0]]
    assert np.array_equal(_rng.philox(c, _rng.key_of(seed)), R.words(seed, 7, q))
    assert np.array_equal(_rng.row_words(seed, 5, 3), np.concatenate([R.words(seed, 5 + b, [0], stream=1) for b in range(3)]))


def test_seed_and_row_checks():
    from sygnals_amd import _rng
    assert _rng.check_seed(0) == 0 and _rng.check_seed((1 << 64) - 1) == (1 << 64) - 1 and _rng.check_seed(np.int64(9)) == 9
    for bad in (-1, 1 << 64, 1.5, "3", True):
        with pytest.raises(ValueError, match="seed must be an integer"):
            _rng.check_seed(bad)
    a, b = _rng.check_seed(None), _rng.check_seed(None)
    assert 0 <= a < (1 << 64) and 0 <= b < (1 << 64) and a != b                     # (equal once in 2^64 runs)
    assert _rng.check_rows(0, 1 << 31) == 0 and _rng.check_rows((1 << 31) - 1, 1) == (1 << 31) - 1
    for first_row, B in ((-1, 1), (1 << 31, 1), ((1 << 31) - 1, 2), (0, 0)):
        with pytest.raises(ValueError, match="must lie in"):
            _rng.check_rows(first_row, B)


@pytest.fixture(scope="module")
def samples():
    return {(s, r): R.normals(s, r, max(LENGTHS)) for s in SEEDS for r in ROWS}


def test_statistics_of_the_restatement(samples):
    """Every moment and lag autocorrelation within 5 standard errors (264 figures: the chance that one of a true normal
    sample exceeds 5 is 2e-4 over all of them).  Worst measured: 4.10, a lag autocorrelation at L = 4096."""
    worst = 0.0
    for (seed, row), zz in samples.items():
        for L in LENGTHS:
            z = zz[:L]
            dev = np.concatenate([R.moments(z), [R.autocorr(z, lag) for lag in LAGS]])
            worst = max(worst, float(np.max(np.abs(dev))))
            assert np.all(np.abs(dev) <= 5.0), (seed, row, L, dev)
        assert np.max(np.abs(zz)) <= 5.77
    print(f"worst deviation {worst:.2f} standard errors")


def test_slicing_and_offsets_of_the_restatement(samples):
    z = samples[(1234, 1)]
    assert np.array_equal(R.normals(1234, 1, 63, start=37), z[37:100])
    assert np.array_equal(R.normals(1234, 1, 1, start=4095), z[4095:4096])
    assert R.normals(3, 0, 5, start=(1 << 34) - 3).shape == (5,)


def test_rows_and_seeds_do_not_correlate(samples):
    for L in LENGTHS:
        a, b = samples[(1234, 0)][:L], samples[(1234, 1)][:L]
        c, d = R.normals(5, 0, L), R.normals(6, 0, L)
        for x, y in ((a, b), (c, d)):
            assert abs(np.mean(x * y)) * np.sqrt(L) <= 5.0
            assert not np.array_equal(x, y)


@pytest.mark.parametrize("alpha,name", [(1.0, "pink"), (2.0, "brown")])
def test_coloured_slope_and_mean(alpha, name):
    x = R.colored(9, 0, 65536, alpha)
    slope = R.octave_slope(x)
    print(f"{name}: {slope:.3f} dB per octave")
    assert abs(slope - (-3.01 * alpha)) <= 0.2
    assert abs(np.mean(x)) <= 1e-12 * np.max(np.abs(x))
    assert R.colored(9, 0, 1, alpha).tolist() == [0.0]


def test_coloured_exponent_zero_is_the_white_row():
    z = R.normals(9, 3, 1024)
    assert np.max(np.abs(R.colored(9, 3, 1000, 0.0) - z[:1000])) <= 1e-12


def test_snr_draws():
    from sygnals_amd import _rng
    lo, hi = 5.0, 30.0
    d = R.snr_draws(77, 3, 64, lo, hi)
    assert np.all(d >= lo) and np.all(d < hi) and len(np.unique(d)) == 64
    assert np.array_equal(_rng.uniform_rows(77, 3, 64, lo, hi), d)
    assert np.array_equal(R.snr_draws(77, 10, 4, lo, hi), d[7:11])                 # a row's draw is its own
    assert np.array_equal(_rng.uniform_rows(77, 0, 2, 12.0, 12.0), [12.0, 12.0])
    for bad in ((3.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="lo <= hi"):
            _rng.uniform_rows(77, 0, 2, *bad)
