"""The feature fuzz (tests/feature_fuzz.py), no GPU: what makes its inputs worth running on the device,
checked from the references alone before any device run.

* the selections: case counts, every memory grid, every node count of the fuzz, an empty stream;
* every shape is accepted by ``qs_shape_table`` and tabulates as tests/strategy_ref.py does;
* per arm, the floors of tests/feature_fuzz.py: streams placed differently from the configuration the
  arm departs from, over-committed winners, pods placed, the spread filter biting and holding, and the
  number of cases on the wide layout.

The references are computed once per arm and process (``functools.lru_cache`` in tests/feature_fuzz.py).
"""
import collections

import numpy as np
import pytest

import qsched

import antiaffinity_ref as AA
import feature_fuzz as F
import spread_ref as S
import strategy_ref as R

# selection: (cases, {grid: cases}, cases with the config-4 features)
SELECTION_FACTS = {
    "strategy": (52, dict(binary=18, ki=17, decimal=17), 20),
    "qos": (51, dict(binary=17, ki=17, decimal=17), 17),
    "lists": (49, dict(binary=19, ki=16, decimal=14), 49),
    "tracked": (54, dict(binary=15, ki=15, decimal=24), 0),
    "tracked-norm": (49, dict(binary=19, ki=16, decimal=14), 49),
}


@pytest.mark.parametrize("name", list(F.SELECTIONS))
def test_selection(name):
    sel = F.SELECTIONS[name]
    cases = [F.CASES[i] for i in sel]
    count, grids, feat = SELECTION_FACTS[name]
    assert len(sel) == count and sel == sorted(set(sel))
    assert dict(collections.Counter(c["grid"] for c in cases)) == grids
    assert set(grids) == set(F.GRIDS)
    assert {c["n"] for c in cases} == F.NODE_COUNTS
    assert any(c["p"] == 0 for c in cases)
    assert sum(bool(c["features"]) for c in cases) == feat
    assert max(c["n"] for c in cases) == 300 and max(c["p"] for c in cases) <= 3000


def test_every_arm_has_a_selection_and_each_grid_its_cases():
    assert len(F.CASES) == 360
    for arm in F.ARMS:
        per_grid = [F.selection(arm, g) for g in F.GRIDS]
        assert sorted(sum(per_grid, [])) == F.selection(arm)
        assert all(14 <= len(s) <= 24 for s in per_grid), arm


@pytest.mark.parametrize("name", list(F.SHAPES))
def test_shapes_are_accepted_and_tabulated_alike(name):
    shape = F.SHAPES[name]
    assert len(shape) <= qsched.QS_MAX_SHAPE
    got = qsched.shape_table(shape)
    assert np.array_equal(got, R.shape_table(shape))
    if name == "zero":
        assert not got.any()
    if name == "sixteen":
        assert len(shape) == qsched.QS_MAX_SHAPE == 16 and (got == 0).sum() >= 2
    if name == "steep":  # a negative slope whose product is no multiple of the span: truncation, not floor
        assert any((b[1] - a[1]) * 10 * (p - a[0]) % (b[0] - a[0]) and b[1] < a[1]
                   for a, b in zip(shape, shape[1:]) for p in range(a[0] + 1, b[0]))


def test_arm_inputs():
    """The arms are what the module says: weights, lists, kinds, ids and zones."""
    seen = set()
    for pos, i in enumerate(F.selection("maxw")):
        x = F.inputs("maxw", i)
        assert (x["gcfg"]["fit_weight_cpu"], x["gcfg"]["fit_weight_mem"]) == (x["ocfg"]["wc"], x["ocfg"]["wm"]) \
            == F.MAXW[pos % 3]
        seen.add(F.MAXW[pos % 3])
        assert x["ocfg"].get("w_fit") == F.inputs("three", i)["ocfg"].get("w_fit")  # plugin weights: the case's
    assert seen == set(F.MAXW) and max(max(w) for w in F.MAXW) == 65535
    # 2 num + den of the rounding division, both resources at raw = 100: beyond 2^24, below 2^25
    assert 1 << 24 < 2 * 100 * (65535 + 65535) + 2 * 65535 == 26_345_070 < 1 << 25
    strategies = collections.Counter()
    for i in F.selection("lists"):
        x = F.inputs("lists", i)
        assert not {"wc", "wm"} & set(x["ocfg"]) and not {"fit_weight_cpu", "fit_weight_mem"} & set(x["gcfg"])
        assert x["gcfg"]["fit_resources"] == x["ocfg"]["fit_resources"]
        assert x["gcfg"]["enable_taint"] == x["gcfg"]["enable_affinity"] == 1
        strategies[x["ocfg"]["scoring_strategy"]] += 1
    assert sorted(strategies.values()) == [16, 16, 17]
    for arm in F.TRACKED_ARMS:
        kinds = set()
        for i in F.selection(arm):
            x = F.inputs(arm, i)
            app, kind = x["pods"]["app"], x["pods"]["anti_affinity"]
            a = (app.astype(np.int64) - 5) // 137
            assert ((0 <= a) & (a < 8) & (app == F.app_id(a))).all() and int(app.max(initial=0)) < AA.MAX_APPS
            assert np.array_equal(kind, np.array(F.APP_KINDS)[a])
            assert set(np.unique(x["nodes"]["zone"])) <= set(F.ZONE_IDS.tolist())
            assert bool(x["case"]["features"]) == (arm == "tracked-norm")
            kinds |= set(np.unique(kind).tolist())
        assert kinds == set(F.APP_KINDS)
        assert max(int(F.inputs(arm, i)["pods"]["app"].max(initial=0)) for i in F.selection(arm)) == F.app_id(7) == 964
        # tables with fewer nodes than zones, and the 64 / 65 node block edge, all with SPREAD pods
        for n in (1, 2, 3, 64, 65):
            assert any(F.CASES[i]["n"] == n and (S.kind_of(F.inputs(arm, i)["pods"]["anti_affinity"]) == S.SPREAD).any()
                       for i in F.selection(arm)), (arm, n)


@pytest.mark.parametrize("arm", F.ARMS)
def test_wide_cases(arm):
    wide = F.wide_cases(arm)
    print(f"{arm}: {wide} of {len(F.selection(arm))} cases on the wide layout")
    assert wide >= F.WIDE_FLOOR
    assert all(F.inputs(arm, i)["compact"] for i in F.selection(arm, "binary"))


@pytest.mark.parametrize("arm", list(F.STRATEGY_ARMS))
def test_strategy_arm(arm):
    got = F.strategy_figures(arm)
    print(f"{arm}: {got[0]} cases placed differently from LeastAllocated, {got[1]} over-committed winners, "
          f"{got[2]} pods placed")
    assert all(g >= f for g, f in zip(got, F.STRATEGY_FLOORS[arm])), (got, F.STRATEGY_FLOORS[arm])
    if arm == "zero":  # every fit score is 0: the winner's total holds no fit term
        for i in F.selection(arm)[:10]:
            x = F.inputs(arm, i)
            for j in range(min(3, x["case"]["p"])):
                assert not F.score_reference(arm, i, j)[1][:, 0].any()


def test_steep_tells_truncation_from_floor(monkeypatch):
    """With floor division in place of Go's truncating one the reference gives other keys on the `steep`
    streams: a device table built with the wrong division would not pass."""
    sel = F.selection("steep")
    refs = [F.reference("steep", i) for i in sel]  # (before the reference is bent)
    monkeypatch.setattr(R, "trunc_div", lambda a, b: a // b)
    assert not np.array_equal(R.shape_table(F.STEEP), qsched.shape_table(F.STEEP))
    keys = places = 0
    for i, r in zip(sel, refs):
        x = F.inputs("steep", i)
        pl, k, _, _ = R.run(x["nodes"], x["pods"], x["ocfg"])
        keys += int(not np.array_equal(k, r["keys"]))
        places += int(not np.array_equal(pl, r["pl"]))
    print(f"steep with floor division: {keys} cases with other keys, {places} with other placements")
    assert keys >= 18 and places >= 6  # 36, 13


def test_maxw_passes_2_24_on_the_score_path():
    """Weights (65535, 65535), both resources counted, fit score >= 65: num / den >= 64.5, so 2 num + den
    of the rounding division is at least 130 * 131070 > 2^24 (the streams reach it far more often)."""
    assert 130 * 131070 > 1 << 24 > 128 * 131070
    big = 0
    for pos, i in enumerate(F.selection("maxw")):
        x = F.inputs("maxw", i)
        both = (x["nodes"]["alloc_cpu"] != 0) & (x["nodes"]["alloc_mem"] != 0)
        for j in range(min(3, x["case"]["p"]) if F.MAXW[pos % 3] == (65535, 65535) else 0):
            feas, sc, _, _ = F.score_reference("maxw", i, j)
            big += int((feas & both & (sc[:, 0] >= 65)).sum())
    print(f"maxw: {big} node evaluations past 2^24 among the scored pods")
    assert big >= 85  # 170


@pytest.mark.parametrize("arm", list(F.QOS_ARMS))
def test_qos_arm(arm):
    got = F.qos_figures(arm)
    print(f"{arm}: {got[0]} cases placed differently from LeastAllocated, {got[1]} from all three uniform runs")
    assert all(g >= f for g, f in zip(got, F.QOS_FLOORS[arm])), (got, F.QOS_FLOORS[arm])


def test_list_arm():
    got = F.list_figures()
    print(f"lists: {got[0]} cases placed differently from the default lists, {got[1]} lists with three or more "
          "balanced entries")
    assert all(g >= f for g, f in zip(got, F.LIST_FLOORS)), (got, F.LIST_FLOORS)


@pytest.mark.parametrize("arm", list(F.TRACKED_ARMS))
def test_tracked_arm(arm):
    differ, lost, apps, held, broken = F.tracked_figures(arm)
    print(f"{arm}: {differ} cases placed differently from every kind NONE, {lost} SPREAD pods unplaced here and "
          f"placed there, {held} of {apps} pure spread apps within max_skew, {broken} beyond it without the filter")
    assert all(g >= f for g, f in zip((differ, lost, broken), F.TRACKED_FLOORS[arm])), (differ, lost, broken)
    assert held == apps == F.PURE_SPREAD_APPS[arm]


def test_tracked_score_reference_is_the_s12_reference():
    """score_reference masks as antiaffinity_ref.pod_keys does: the same feasible set, totals and winner."""
    for arm in F.TRACKED_ARMS:
        for i in F.selection(arm)[:12]:
            x, r = F.inputs(arm, i), F.reference(arm, i)
            for j in range(min(3, x["case"]["p"])):
                k = AA.pod_keys(r["final"], x["pods"], j, r["state"], x["ocfg"], F.scorer(arm, x["ocfg"]))
                feas, _, total, best = F.score_reference(arm, i, j, r["final"], r["state"])
                assert np.array_equal(feas, k != 0)
                assert np.array_equal(total[feas], (k[feas] >> np.uint64(32)).astype(np.int64) - 1)
                assert best == (int(0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)) if feas.any() else -1)
