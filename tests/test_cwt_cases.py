"""tests/cwt_cases.py checked on the host: every direct case reaches the inner forms of csrc/cwt.hip it names (through
cwt_cases.route, with the library's constants), every spectral case the transform length and engine it names, the pairing
cases pair as stated, and the plan's filters of every scale list the device tests use are the restatement's, bit for bit
(so the device gate measures the device alone).  No device."""
import os

import numpy as np
import pytest

from sygnals_amd import _cwt as CW
from tests import cwt_cases as K
from tests import cwt_ref as R


@pytest.fixture(scope="module")
def k():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return K.constants()


def test_route_restates_the_launch_rules_on_known_answers(k):
    tile, spg = k["tile"], k["scales_per_group"]
    # one short real filter over one tile and one column more: vec, delta 0 (it alone sets the earliest sample: base = taps - 1)
    r = K.route(tile + 1, 1, (1,), "morl", k=k)
    assert [(x.group, x.tile, x.scale, x.form, x.taps, x.cnt) for x in r] == [(0, 0, 0, "vec", 18, tile), (0, 1, 0, "vec", 18, 1)]
    assert [x.delta for x in r] == [(4 - (17 & 3)) & 3] * 2
    # any other stride: never vec; the span of a full tile decides staged or not
    assert {x.form for x in K.route(4 * tile, 2, (1,), "morl", k=k)} == {"staged"}
    big = k["span_max"] // (tile - 1) + 1
    assert [x.form for x in K.route(big * tile + 1, big, (1,), "morl", k=k)] == ["global", "staged"]
    # spg + 1 scales: two groups, the tap-count sort decides who shares a span; idx names the subset that runs direct
    scales = tuple(range(spg + 1, 0, -1))
    r = K.route(10, 1, scales, "morl", k=k)
    assert [x.scale for x in r] == list(range(spg, -1, -1)) and [x.group for x in r] == [0] * spg + [1]
    assert [x.scale for x in K.route(10, 1, scales, "morl", idx=[0, 3], k=k)] == [3, 0]
    assert K.sorted_order(scales, "morl") == list(range(spg, -1, -1))


@pytest.mark.parametrize("c", K.direct_cases(), ids=K.case_id)
def test_direct_cases_reach_the_forms_they_name(k, c):
    r = K.route(c.L, c.stride, c.scales, c.wavelet, k=k)
    assert len({x.group for x in r}) == c.groups and len({x.tile for x in r}) == c.tiles
    assert frozenset((x.tile, x.form) for x in r) == c.must
    for i, forms in c.per_scale.items():
        assert {x.form for x in r if x.scale == i} == forms
    assert sum(x.cnt for x in r if x.group == 0 and x.scale == r[0].scale) == -(-c.L // c.stride)


def test_direct_cases_by_name(k):
    cases = {c.name: c for c in K.direct_cases()}
    assert len(cases) == len(K.direct_cases())
    tile = k["tile"]
    # the bound of the staged taps sits between scales 512 and 513 of a complex wavelet
    p = CW.cwt_plan((512, 513), K.CMOR)
    assert 2 * (int(p.taps[0]) + 6) <= k["taps_lds_max"] < 2 * (int(p.taps[1]) + 6)
    # a stride with a remainder: the last column is a tile of its own
    c = cases["stride-17"]
    assert c.L % c.stride == 5 and -(-c.L // c.stride) == tile + 1
    r = K.route(c.L, c.stride, c.scales, c.wavelet, k=k)
    assert {x.cnt for x in r if x.tile == 1} == {1}
    assert {x.cnt for x in K.route(20000, 16, K.SIX, "morl", k=k) if x.tile == 1} == {226}
    # the shuffled list: the launch's order is not the caller's, and not a reversal of it either; one scale twice
    for w in ("morl", K.CMOR):
        order = K.sorted_order(K.SHUFFLED, w)
        assert order != sorted(order) and order != sorted(order, reverse=True) and len(set(K.SHUFFLED)) == len(K.SHUFFLED) - 1
        assert order[:k["scales_per_group"]] != sorted(order[:k["scales_per_group"]])
    # the smallest filters: 3 ... 7 taps and about 1000; at stride 1 every delta of cw_scale_vec, at stride 2 every length
    # of the scalar form's tail loop
    for w in K.WAVELETS:
        plan = CW.cwt_plan(K.small_scales(w), w)
        assert tuple(int(t) for t in plan.taps[:5]) == K.SMALL_TAPS and 900 <= int(plan.taps[5]) <= k["direct_taps_max"]
        for t, s in zip(K.SMALL_TAPS, K.small_scales(w)):
            with_less = round(s - 0.005, 3)
            assert with_less <= 0 or _taps_or_none(w, with_less) != t
        for L in K.SMALL_L:
            r = K.route(L, 1, K.small_scales(w), w, k=k)
            assert {x.form for x in r} == {"vec"} and {x.delta for x in r} == {0, 1, 2, 3}
            assert {x.taps % 4 for x in K.route(L, 2, K.small_scales(w), w, k=k) if x.form == "staged"} == {0, 1, 2, 3}


def _taps_or_none(w, s):
    try:
        return CW.scale_filter(CW.parse_wavelet(w), s)[0].size
    except ValueError:
        return None


@pytest.mark.parametrize("c", K.SPECTRAL_CASES, ids=lambda c: c.name)
def test_spectral_cases_reach_the_lengths_they_name(k, c):
    from sygnals_amd import ops
    for w in ("morl", "mexh", K.CMOR):
        plan = CW.cwt_plan(K.spectral_scales(c), w)
        assert int(plan.taps.max()) == int(plan.taps[1]) == c.taps
        M = ops.cwt_fft_len(c.L, c.taps)
        assert M == c.M and ops.fft_plan(M) == c.plan
        assert (M == c.L + c.taps - 1) == (c.name in K.TIGHT)
        # a real wavelet's two scales share a filter row; both are spectral under the rule as well
        assert CW.spectral_rows(plan, [0, 1]) == ([(0, -1), (1, -1)] if plan.wavelet.complex else [(0, 1)])
        assert list(CW.split_forms(plan, k["direct_taps_max"], None)[0]) == []


def test_pairing_cases():
    s = float(K.PAIR_S)
    assert CW.spectral_rows(CW.cwt_plan((s, CW.PAIR_RATIO * s), "morl"), [0, 1]) == [(0, 1)]
    assert CW.spectral_rows(CW.cwt_plan((CW.PAIR_RATIO * s, s), "morl"), [0, 1]) == [(1, 0)]
    assert CW.spectral_rows(CW.cwt_plan((s, 4.0001 * s), "morl"), [0, 1]) == [(0, -1), (1, -1)]
    assert K.PAIR_S * 4 == CW.PAIR_RATIO * K.PAIR_S
    # five spectral scales leave one alone
    plan = CW.cwt_plan((100, 150, 200, 300, 400), "morl")
    assert CW.spectral_rows(plan, range(5)) == [(0, 1), (2, 3), (4, -1)]
    # the interleaved list: four direct scales, six spectral ones in three rows; with every scale spectral the two equal
    # scales share a row
    plan = CW.cwt_plan(K.MIXED_ORDER, "morl")
    d, sp = CW.split_forms(plan, 1024, None)
    assert list(d) == [1, 3, 7, 9] and list(sp) == [0, 2, 4, 5, 6, 8]
    assert CW.spectral_rows(plan, sp) == [(5, 6), (4, 8), (0, 2)]
    assert CW.spectral_rows(plan, range(10)) == [(3, 1), (9, 7), (5, 6), (4, 8), (0, 2)]
    assert K.MIXED_ORDER[1] == K.MIXED_ORDER[9]
    for perm in (K.MIXED_ORDER, tuple(sorted(K.MIXED_ORDER)), tuple(sorted(K.MIXED_ORDER, reverse=True))):
        assert sorted(perm) == sorted(K.MIXED_ORDER)


@pytest.mark.parametrize("w,scales", K.every_scale_list(), ids=lambda v: v if isinstance(v, str) else f"{len(v)}-from-{v[0]:g}")
def test_plan_tables_are_the_restatement_rounded_once(w, scales):
    plan = CW.cwt_plan(scales, w)
    for i, s in enumerate(scales):
        hs, off = R.h_filter(w, s)
        assert np.array_equal(plan.table64[i], hs) and plan.table64[i].dtype == hs.dtype and plan.offset[i] == off
        got = plan.filter32(i)
        if plan.wavelet.complex:
            assert np.array_equal(got.real, hs.real.astype(np.float32)) and np.array_equal(got.imag, hs.imag.astype(np.float32))
        else:
            assert np.array_equal(got, hs.astype(np.float32))
        assert plan.l1[i] == np.abs(hs).sum() and plan.l1[i] > 0
