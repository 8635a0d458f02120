"""A model of the clip hand-over of the free-running STFT-2048 MFCC kernel whose waves never meet (stft_meet = 0,
sygnals_amd/csrc/stft_mel.hip, LOAD 4), in plain Python: sixteen actors walk the tile loop's events of one workgroup, a
seeded random scheduler picks the interleaving.  The counters are the kernel's: filled[p] (+1 per wave that is through with a
clip on matrix p), drained[p] (+1 per wave that ran the clip epilogue on p), bad (a writer's wait ran out).  Checked on
every schedule: an epilogue reads a matrix only with all sixteen increments of its clip in, no store hits a matrix (or its
maxima) that an unfinished epilogue still needs, every wait is satisfied and every schedule ends."""
import random

import pytest

WAVES = 16
UNBOUNDED = 1 << 60


class Workgroup:
    def __init__(self, T, clips, n_mfcc, bound, rng):
        self.T, self.clips, self.bound, self.rng = T, clips, bound, rng
        self.tiles = (T + WAVES - 1) // WAVES
        tp = self.tiles * WAVES
        self.ndct = ((n_mfcc + 15) // 16) * (tp // 16)          # output tiles of a clip epilogue
        self.idle = tp - T                                      # waves without a frame in a clip's last tile
        self.defer = self.idle > 0 and -(-self.ndct // self.idle) <= 3
        self.nepi = self.idle if self.defer else min(self.ndct, WAVES)
        self.filled, self.drained, self.bad = [0, 0], [0, 0], 0
        # ground truth, kept beside the counters
        self.through = [0] * clips          # waves that are through with clip k
        self.reading = [0, 0]               # epilogues in progress per matrix
        self.epi_done = [0] * clips         # waves that finished the epilogue of clip k
        self.epi_waves = [0] * clips        # waves that run the epilogue of clip k
        self.marked = set()                 # clips whose output is NaN
        self.expired = 0
        self.checked_reads = self.checked_stores = 0

    # a poll: ("wait", counter list, index, target) -> resumes with True (satisfied) or False (the bound ran out)
    def epilogue(self, k):
        p = k & 1
        ok = yield ("wait", self.filled, p, WAVES * ((k >> 1) + 1))
        if not ok or self.bad:
            self.marked.add(k)
        else:
            assert self.through[k] == WAVES, f"epilogue of clip {k} reads with {self.through[k]} of 16 waves through"
            self.checked_reads += 1
        self.reading[p] += 1
        yield ("step",)                     # the reads of the matrix and of red[p][]
        self.reading[p] -= 1
        self.epi_done[k] += 1
        self.drained[p] += 1

    def store(self, k, what):
        p = k & 1
        if self.expired == 0:
            assert self.reading[p] == 0, f"{what} of clip {k} hits matrix {p} while an epilogue reads it"
            if k >= 2:
                assert self.epi_done[k - 2] == self.nepi, f"{what} of clip {k}: epilogue of clip {k - 2} unfinished"
            self.checked_stores += 1

    def wave(self, w):
        pend = -1
        for k in range(self.clips):
            cur = k & 1
            for tile in range(self.tiles):
                t0 = tile * WAVES
                mine, clip_done = t0 + w < self.T, t0 + WAVES >= self.T
                yield ("step",)             # transform (own row only)
                if t0 == 0 and k >= 2:
                    ok = yield ("wait", self.drained, cur, self.nepi * (k >> 1))
                    if not ok:
                        self.bad = 1
                if mine:
                    self.store(k, "column store")
                    yield ("step",)
                elif self.defer and pend >= 0:
                    yield from self.epilogue(pend)
                if clip_done:
                    self.store(k, "publish_max")
                    yield ("step",)
                    self.through[k] += 1
                    self.filled[cur] += 1
                    if self.defer:
                        pend = k
                    elif w < self.ndct:
                        yield from self.epilogue(k)
        if pend >= 0 and w < self.ndct:
            yield from self.epilogue(pend)

    def run(self):
        actors = {w: self.wave(w) for w in range(WAVES)}
        state = {w: next(g) for w, g in actors.items()}
        rounds = {w: 0 for w in actors}
        while actors:
            ready = []
            for w, ev in state.items():
                if ev[0] == "step" or ev[1][ev[2]] >= ev[3] or rounds[w] >= self.bound:
                    ready.append(w)
                else:
                    rounds[w] += 0 if self.bound == UNBOUNDED else 1
            if not ready:
                assert self.bound != UNBOUNDED, f"deadlock: {state}"
                continue                     # (a bounded poll: the rounds go on counting)
            w = self.rng.choice(ready)
            ev = state[w]
            arg = None
            if ev[0] == "wait":
                arg = ev[1][ev[2]] >= ev[3]
                if not arg:
                    self.expired += 1
                rounds[w] = 0
            try:
                state[w] = actors[w].send(arg)
            except StopIteration:
                del actors[w], state[w]
        return self


# (T, clips of the workgroup, n_mfcc): T = 94 deferred on two idle waves | T = 32 no idle wave | T = 6 one-tile clips,
# ten idle waves | T = 17 fifteen idle waves | n_mfcc = 20, T = 44: two rows of output tiles on four idle waves | T = 36 |
# T = 1 | one and two clips: nothing to hand back | T = 16: full one-tile clips | T = 250, n_mfcc = 40: all sixteen waves
# run the epilogue
CASES = [(94, 4, 13), (94, 5, 13), (32, 6, 13), (6, 5, 13), (6, 4, 13), (17, 4, 13), (44, 4, 20), (36, 5, 13), (1, 6, 13),
         (94, 1, 13), (17, 2, 13), (32, 1, 13), (16, 7, 13), (250, 3, 40)]


@pytest.mark.parametrize("T,clips,n_mfcc", CASES)
def test_handover_is_safe_and_ends_on_every_schedule(T, clips, n_mfcc):
    for seed in range(300):
        wg = Workgroup(T, clips, n_mfcc, UNBOUNDED, random.Random(seed * 7919 + T)).run()
        assert wg.expired == 0 and not wg.marked and wg.bad == 0
        assert wg.through == [WAVES] * clips and wg.filled[0] + wg.filled[1] == WAVES * clips
        ran = [wg.nepi] * (clips - 1) + [wg.nepi if not wg.defer else min(wg.ndct, WAVES)]
        assert wg.epi_done == ran
        assert wg.checked_reads == sum(ran) and wg.checked_stores > 0


def test_model_takes_both_epilogue_placements():
    assert Workgroup(94, 4, 13, UNBOUNDED, random.Random(0)).defer
    assert Workgroup(6, 4, 13, UNBOUNDED, random.Random(0)).defer
    assert not Workgroup(32, 4, 13, UNBOUNDED, random.Random(0)).defer
    assert Workgroup(32, 4, 13, UNBOUNDED, random.Random(0)).nepi == 2


@pytest.mark.parametrize("T,clips,n_mfcc", [(94, 5, 13), (32, 6, 13), (6, 5, 13)])
def test_a_bound_that_runs_out_marks_the_clip_and_the_schedule_still_ends(T, clips, n_mfcc):
    """Bound 0: a wait that is not satisfied at its first look runs out.  Every epilogue that ran out, or that started
    behind a writer's mark, turns its clip into NaN; nothing hangs."""
    marked = 0
    for seed in range(200):
        wg = Workgroup(T, clips, n_mfcc, 0, random.Random(seed)).run()
        assert wg.through == [WAVES] * clips                  # every wave went on to the end
        assert (wg.expired > 0) == bool(wg.marked or wg.bad)
        if wg.bad:
            assert wg.marked, "a writer's mark must reach a later epilogue"
        marked += bool(wg.marked)
    assert marked > 0, "no schedule made a wait run out: the expiry path was not exercised"
