"""The inputs the rhythm tests share, their float64 references (computed once) and the two conditions under which a
decision of the device may be compared with the restatement's."""
import functools

import numpy as np

from tests import beat_ref as R

SR, HOP = 22050, 512
WIN = int(np.floor(8.0 * SR / HOP))            # 344
EPS = 1e-5                                     # the tempogram's gate

# click envelopes for the end-to-end tests: name -> (T, period, phase, seed)
ENV_CASES = {
    "p20": (300, 20, 3, 1),
    "p24": (517, 24, 0, 2),
    "p31": (400, 31, 7, 3),
}


def envelope(name):
    T, period, phase, seed = ENV_CASES[name]
    return R.click_envelope(T, period, phase, 1.0, 0.1, seed)


def condition_a(a, logprior):
    """The winning lag's score at a - EPS exceeds every other lag's score at a + EPS."""
    a = np.asarray(a, dtype=np.float64)
    k = R.tempo_pick(a, logprior)
    with np.errstate(invalid="ignore", divide="ignore"):
        lo = np.log1p(1e6 * (a[k] - EPS)) + logprior[k]
        hi = np.log1p(1e6 * (a + EPS)) + logprior
    hi[k] = -np.inf
    return bool(lo > np.max(hi))


def condition_b(env, period, tightness=100.0, trim=True):
    """The beats do not move when ls is rounded to float32 or perturbed by +-EPS max|ls| (three seeds)."""
    ls = R.local_score(env, period)
    want = R.beats_from(ls, period, tightness, trim)[0]
    if not np.array_equal(R.beats_from(ls.astype(np.float32), period, tightness, trim)[0], want):
        return False
    for seed in range(3):
        d = np.random.default_rng(seed).uniform(-1.0, 1.0, len(ls)) * EPS * np.max(np.abs(ls))
        if not np.array_equal(R.beats_from((ls + d).astype(np.float32), period, tightness, trim)[0], want):
            return False
    return True


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 chain of an envelope case: tempo, lag, beats, and the aggregate and prior behind the lag."""
    env = envelope(name)
    bpms, lp = R.prior(WIN, SR, HOP)
    a = R.aggregate(R.tempogram(env, WIN))
    k = R.tempo_pick(a, lp)
    return dict(env=env, a=a, logprior=lp, bpms=bpms, k=k, tempo=float(bpms[k]), beats=R.beat_track(env, k))
