"""Arms, case selections and cached references of the feature fuzz (tests/test_feature_fuzz_cpu.py,
tests/test_gpu_feature_fuzz.py).  CPU only; test infrastructure.

The adversarial clusters of tests/adversarial.py (the committed seeds of tests/golden/fuzz_cases.json:
arbitrary cpu denominators, allocatable 0, odd-Ki / decimal memory, max_pods 1..110, pre-used and
over-committed nodes, missing vs zero requests, tie blocks, tables of 1..300 nodes) run under the
features that were added after that fuzz was written.  A case is chosen by its index ``i`` in the
committed list; nothing is skipped inside a selection.

  * strategy arms (``i % 7 == 0``): MostAllocated and six RequestedToCapacityRatio shapes, the case's own
    weights kept; ``maxw`` is ``three`` under the legacy weights 65535 (qs_open accepts them as they
    are, so no smaller pair stands in), where ``2 num + den`` of the device's rounding division passes
    2^24.  Reference: strategy_ref.run.
  * per-QoS arms (``i % 7 == 3``): two class mixes.  Reference: qos_strategy_ref.run.
  * list arm (every third config-4 case): a random scoring-resource list per case, the strategy cycling
    over LeastAllocated / MostAllocated / ``three``.  Reference: strategy_ref.run.
  * tracked arms (every fourth case without config-4 features; ``norm``: every third with them): the
    builder's eight apps get the kinds NONE, HOSTNAME, ZONE and SPREAD(1 / 2 / 31 / 1 / 3), ids 137 a + 5
    (up to 964), its four zones the ids 0, 5, 63, 31.  Reference: spread_ref.run with the sub-arm's scorer.

Each floor below is a condition on the references alone (tests/test_feature_fuzz_cpu.py asserts them);
the value measured when the arm was written stands beside it.
"""
import functools

import numpy as np

import adversarial as A
import antiaffinity_cases as AC
import antiaffinity_ref as AA
import qos_strategy_ref as Q
import spread_ref as S
import strategy_ref as R
from rescfg import random_resource_cfg

CASES = A.load_cases()
GRIDS = ["binary", "ki", "decimal"]
NODE_COUNTS = {1, 2, 3, 7, 24, 64, 65, 130, 300}


def rtcr(shape):
    return dict(scoring_strategy="RequestedToCapacityRatio", shape=shape)


# ---- shapes ---------------------------------------------------------------------------------------
THREE = [(0, 2), (40, 10), (70, 3), (100, 8)]
# adjacent utilisations, and negative slopes (Go's division truncates toward zero there)
STEEP = [(0, 10), (3, 0), (4, 9), (99, 1), (100, 10)]
ZERO = [(0, 0), (100, 0)]  # every resource scores 0: weight sum 0, fit score 0
SINGLE = [(50, 7)]
SIXTEEN = list(zip([0, 1, 2, 3, 10, 20, 30, 40, 50, 60, 70, 80, 90, 98, 99, 100],
                   [0, 10, 1, 9, 2, 8, 3, 7, 4, 6, 5, 5, 6, 4, 10, 0]))  # the largest shape, zeros inside
SHAPES = dict(three=THREE, steep=STEEP, zero=ZERO, single=SINGLE, sixteen=SIXTEEN, fall30=AC.FALL30)
MOST = dict(scoring_strategy="MostAllocated")
LEAST = dict(scoring_strategy="LeastAllocated")

STRATEGY_ARMS = {"most": MOST, "three": rtcr(THREE), "steep": rtcr(STEEP), "zero": rtcr(ZERO),
                 "single": rtcr(SINGLE), "sixteen": rtcr(SIXTEEN), "maxw": rtcr(THREE)}
MAXW = [(65535, 65535), (65535, 1), (1, 65535)]  # (fit_weight_cpu, fit_weight_mem), cycling by case

QOS_ARMS = {
    "mix-a": AC.QOS_MIX,
    "mix-b": dict(qos_strategies={"BestEffort": rtcr(THREE), "Burstable": LEAST, "Guaranteed": MOST}),
}
LIST_STRATEGIES = [LEAST, MOST, rtcr(THREE)]  # cycling by position in the selection
LIST_ARMS = ["lists"]

# tracked arms: name -> (scorer kind of antiaffinity_cases.scorer_of, configuration on top of the case's)
TRACKED_ARMS = {"tracked": (None, {}), "tracked-most": ("strategy", MOST), "tracked-mix-a": ("qos", AC.QOS_MIX),
                "tracked-norm": (None, {})}
APP_KINDS = [AA.NONE, AA.HOSTNAME, AA.ZONE, S.spread(1), S.spread(2), S.spread(31), S.spread(1), S.spread(3)]
ZONE_IDS = np.array([0, 5, 63, 31])

STREAM_ARMS = list(STRATEGY_ARMS) + list(QOS_ARMS) + LIST_ARMS
ARMS = STREAM_ARMS + list(TRACKED_ARMS)


def app_id(a):
    return 137 * a + 5


# ---- selections -----------------------------------------------------------------------------------
_FEAT = [i for i, c in enumerate(CASES) if c["features"]]
_PLAIN = [i for i, c in enumerate(CASES) if not c["features"]]
SELECTIONS = {
    "strategy": [i for i in range(len(CASES)) if i % 7 == 0],
    "qos": [i for i in range(len(CASES)) if i % 7 == 3],
    "lists": _FEAT[::3],
    "tracked": _PLAIN[::4],
    "tracked-norm": _FEAT[::3],
}


def selection_name(arm):
    if arm in STRATEGY_ARMS:
        return "strategy"
    if arm in QOS_ARMS:
        return "qos"
    if arm in ("lists", "tracked-norm"):
        return arm
    assert arm in TRACKED_ARMS, arm
    return "tracked"


def selection(arm, grid=None):
    """The case indices of an arm, in list order (those of one memory grid when `grid` is given)."""
    sel = SELECTIONS[selection_name(arm)]
    return sel if grid is None else [i for i in sel if CASES[i]["grid"] == grid]


# ---- inputs ---------------------------------------------------------------------------------------
def _without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


@functools.lru_cache(maxsize=None)
def built(i):
    return A.build(CASES[i])


@functools.lru_cache(maxsize=None)
def inputs(arm, i):
    """dict(case, nodes, pods (dict form), gcfg (device), ocfg (reference), compact) of case i under `arm`.
    Shared between the tests: nobody writes into it."""
    case = CASES[i]
    nodes, pods, gcfg, ocfg = built(i)
    pos = selection(arm).index(i)
    if arm in STRATEGY_ARMS:
        extra = STRATEGY_ARMS[arm]
        if arm == "maxw":
            wc, wm = MAXW[pos % 3]
            gcfg = dict(gcfg, fit_weight_cpu=wc, fit_weight_mem=wm)
            ocfg = dict(ocfg, wc=wc, wm=wm)
        gcfg, ocfg = dict(gcfg, **extra), dict(ocfg, **extra)
    elif arm in QOS_ARMS:
        gcfg, ocfg = dict(gcfg, **QOS_ARMS[arm]), dict(ocfg, **QOS_ARMS[arm])
    elif arm == "lists":
        extra = dict(random_resource_cfg(np.random.default_rng(case["seed"] ^ 0x11575)),
                     **LIST_STRATEGIES[pos % 3])
        gcfg = dict(_without(gcfg, "fit_weight_cpu", "fit_weight_mem"), **extra)  # the list carries the weights
        ocfg = dict(_without(ocfg, "wc", "wm"), **extra)
    else:
        extra = TRACKED_ARMS[arm][1]
        nodes, pods = dict(nodes), dict(pods)
        zone, app = nodes["zone"], pods["app"]
        if arm == "tracked-norm":  # the builder draws neither for a config-4 case
            rng = np.random.default_rng(case["seed"] ^ 0x5A0E)
            zone = rng.integers(0, 4, case["n"])
            app = rng.integers(0, 8, case["p"])
        nodes["zone"] = ZONE_IDS[zone].astype(np.int32)
        pods["anti_affinity"] = np.array(APP_KINDS, np.int32)[app]
        pods["app"] = app_id(np.asarray(app)).astype(np.int32)
        gcfg, ocfg = dict(gcfg, **extra), dict(ocfg, **extra)
    return dict(case=case, index=i, nodes=nodes, pods=pods, gcfg=gcfg, ocfg=ocfg,
                compact=A.memory_is_compact(nodes, pods))


def scorer(arm, ocfg):
    return AC.scorer_of(TRACKED_ARMS[arm][0], ocfg)


# ---- references -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(arm, i):
    """dict(pl, keys, final) of case i under `arm`, plus info (strategy and list arms) or state (tracked)."""
    x = inputs(arm, i)
    if arm in QOS_ARMS:
        pl, keys, final = Q.run(x["nodes"], x["pods"], x["ocfg"])
        return dict(pl=pl, keys=keys, final=final)
    if arm in TRACKED_ARMS:
        pl, keys, final, state = S.run(x["nodes"], x["pods"], x["ocfg"], scorer(arm, x["ocfg"]))
        return dict(pl=pl, keys=keys, final=final, state=state)
    pl, keys, final, info = R.run(x["nodes"], x["pods"], x["ocfg"])
    return dict(pl=pl, keys=keys, final=final, info=info)


@functools.lru_cache(maxsize=None)
def least_allocated(i):
    """Placements of case i as built (LeastAllocated, default lists, the case's weights)."""
    nodes, pods, _, ocfg = built(i)
    return R.run(nodes, pods, ocfg)[0]


def score_reference(arm, i, j, nodes=None, state=None):
    """(feasible, scores[n, 4], total, best) of pod j of case i under `arm` against `nodes` (default: the
    table as built).  Tracked arms: under `state`, the nodes the pod's kind excludes masked as
    antiaffinity_ref does it (max_pods 0 in a scratch column, so Fit drops them from the maxima too)."""
    x = inputs(arm, i)
    nodes = x["nodes"] if nodes is None else nodes
    if arm in TRACKED_ARMS:
        nodes = AA.masked(nodes, state, int(x["pods"]["app"][j]), int(x["pods"]["anti_affinity"][j]))
    if "qos_strategies" in x["ocfg"]:
        return Q.score_pod(nodes, x["pods"], j, x["ocfg"])
    return R.score_pod(nodes, x["pods"], j, x["ocfg"])


# ---- conditions (from the references alone) ---------------------------------------------------------
def wide_cases(arm):
    return sum(not inputs(arm, i)["compact"] for i in selection(arm))


def strategy_figures(arm):
    """(cases placed differently from LeastAllocated, winners with an over-committed counted entry, pods
    placed) of a strategy arm."""
    differ = over = placed = 0
    for i in selection(arm):
        r = reference(arm, i)
        differ += int(not np.array_equal(r["pl"], least_allocated(i)))
        over += r["info"]["overcommitted"]
        placed += int((r["pl"] >= 0).sum())
    return differ, over, placed


def qos_figures(arm):
    """(cases placed differently from LeastAllocated, cases placed differently from each of the three
    one-strategy configurations the mix is made of)."""
    differ = mixed = 0
    for i in selection(arm):
        r = reference(arm, i)
        differ += int(not np.array_equal(r["pl"], least_allocated(i)))
        mixed += int(all(not np.array_equal(r["pl"], uniform(arm, i, q)) for q in range(3)))
    return differ, mixed


def uniform(arm, i, q):
    """Placements of qos_strategy_ref.uniform: every class scoring as class q of the mix does."""
    u = Q.uniform(inputs(arm, i)["ocfg"], q)
    return _one_strategy(i, u["scoring_strategy"], tuple(u["shape"] or ()))


@functools.lru_cache(maxsize=None)
def _one_strategy(i, strategy, shape):  # (the two mixes share their MostAllocated / LeastAllocated runs)
    nodes, pods, _, ocfg = built(i)
    if strategy == "LeastAllocated":
        return least_allocated(i)
    return R.run(nodes, pods, dict(ocfg, scoring_strategy=strategy, shape=list(shape) or None))[0]


def list_figures():
    """(cases placed differently from the same strategy over the default lists, lists with three or more
    balanced entries)."""
    differ = three = 0
    for i in selection("lists"):
        x, r = inputs("lists", i), reference("lists", i)
        plain = R.run(x["nodes"], x["pods"], _without(x["ocfg"], "fit_resources", "balanced_resources"))[0]
        differ += int(not np.array_equal(r["pl"], plain))
        three += int(len(x["ocfg"]["balanced_resources"]) >= 3)
    return differ, three


def pure_spread_apps(pods):
    """{app: max_skew} of the apps whose pods are all SPREAD with one max_skew."""
    out = {}
    for app in np.unique(pods["app"]):
        v = np.unique(pods["anti_affinity"][pods["app"] == app])
        if len(v) == 1 and int(S.kind_of(v[0])) == S.SPREAD:
            out[int(app)] = int(S.skew_of(v[0]))
    return out


def tracked_figures(arm):
    """(cases placed differently from the same stream with every kind NONE, SPREAD pods unplaced here and
    placed there, pure spread apps, those that end within their max_skew, those that exceed it without
    the filter)."""
    differ = lost = apps = held = broken = 0
    for i in selection(arm):
        x, r = inputs(arm, i), reference(arm, i)
        plain = dict(x["pods"], anti_affinity=np.zeros_like(x["pods"]["anti_affinity"]))
        ppl, _, _, pstate = S.run(x["nodes"], plain, x["ocfg"], scorer(arm, x["ocfg"]))
        differ += int(not np.array_equal(r["pl"], ppl))
        spread = S.kind_of(x["pods"]["anti_affinity"]) == S.SPREAD
        lost += int((spread & (r["pl"] < 0) & (ppl >= 0)).sum())
        for app, skew in pure_spread_apps(x["pods"]).items():
            apps += 1
            held += int(S.skew_of_app(r["state"], app) <= skew)
            broken += int(S.skew_of_app(pstate, app) > skew)
    return differ, lost, apps, held, broken


# ---- floors: the least each figure may be, the measured value in the comment beside it ---------------
WIDE_FLOOR = 10  # selected cases on the wide layout, per arm (measured: strategy arms 30, per-QoS 33, lists 27,
#                  tracked 38, tracked-norm 27)
# strategy_figures: (cases placed differently from LeastAllocated, over-committed winners, pods placed)
STRATEGY_FLOORS = {
    "most": (20, 1000, 4000),     # 30, 2224, 4570
    "three": (20, 1000, 4000),    # 28, 2092, 4598
    "steep": (20, 1000, 4000),    # 26, 2222, 4614
    "zero": (20, 1000, 4000),     # 30, 2019, 4661
    "maxw": (20, 1000, 4000),     # 29, 2054, 4600
    "single": (14, 1000, 2300),   # 29, 2016, 4642 (floors at about half)
    "sixteen": (14, 1000, 2300),  # 28, 2059, 4706 (floors at about half)
}
# qos_figures: (cases placed differently from LeastAllocated, ... from all three one-strategy runs)
QOS_FLOORS = {
    "mix-a": (15, 12),  # 21, 19
    "mix-b": (15, 12),  # 27, 18
}
# list_figures: (cases placed differently from the default lists, lists with >= 3 balanced entries)
LIST_FLOORS = (17, 14)  # 23, 21
# tracked_figures: (cases placed differently from every kind NONE, SPREAD pods unplaced here and placed
# there, pure spread apps that exceed their max_skew without the filter); every pure spread app must end
# within its max_skew with it (173 of 173; tracked-norm 164 of 164)
TRACKED_FLOORS = {
    "tracked": (20, 500, 50),        # 28, 1073, 101
    "tracked-most": (20, 500, 45),   # 28, 1046, 93
    "tracked-mix-a": (20, 500, 45),  # 28, 1064, 95
    "tracked-norm": (11, 250, 30),   # 22, 518, 63 (floors at about half)
}
PURE_SPREAD_APPS = {"tracked": 173, "tracked-most": 173, "tracked-mix-a": 173, "tracked-norm": 164}
