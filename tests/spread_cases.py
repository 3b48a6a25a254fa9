"""Inputs shared by tests/test_spread_cpu.py and tests/test_gpu_spread.py (spec S13): the known answers
K32-K36 of spec/kat.md as clusters, and the parity inputs with their references (tests/spread_ref.py),
each computed once per process.  CPU only.
"""
import functools

import numpy as np

import qsched

import antiaffinity_cases as C
import antiaffinity_ref as A
import spread_ref as S
from rescfg import GPU_CFG

ARRIVAL = dict(qos_sort=0)  # arrival order: the runs of same-app pods below stay consecutive
SPARSE_ZONES = np.array([0, 5, 63])


# ---- known answers (spec/kat.md K32-K36) ---------------------------------------------------------
# (node, sign, feasible set of the SPREAD(1) pod) of K36
K36_STEPS = [(0, +1, [1]), (1, +1, [0, 1]), (1, +1, [0]), (1, -1, [0, 1]), (1, -1, [1]), (0, -1, [0, 1])]


def kat(name):
    """(nodes, pods, cfg, placements, winners' totals) of one known answer, computed by hand."""
    s1, s2 = S.spread(1), S.spread(2)
    if name == "K32":
        return C._nodes([1, 1, 1], [0, 0, 1]), C._pods([(1, 3, s1)] * 3), {}, [0, 2, 1], [274, 274, 274]
    if name == "K33":
        return C._nodes([1, 1, 1], [0, 0, 1]), C._pods([(1, 3, s2)] * 4), {}, [0, 1, 2, 0], [274, 274, 274, 250]
    if name == "K34":
        return C._nodes([1, 1, 1], [0, 5, 63]), C._pods([(1, 3, s1)] * 4), {}, [0, 1, 2, 0], [274, 274, 274, 250]
    if name == "K35":
        pods = C._pods([(1, 3, A.NONE), (1, 3, s1), (1, 3, s1)])
        return C._nodes([1, 1, 1], [0, 0, 1]), pods, {}, [0, 2, 1], [274, 274, 274]
    if name == "K36":
        return C._nodes([1, 1], [0, 1]), C._pods([(2, 4, s1), (2, 4, A.HOSTNAME)]), {}, None, None
    raise KeyError(name)


# ---- parity inputs -------------------------------------------------------------------------------
def redraw(nodes, pods, apps, zones=None):
    """Kinds redrawn per app of a folded cluster (antiaffinity_ref.fold: app id = 25 x + 24): by x % 6
    SPREAD(1), SPREAD(2), ZONE, HOSTNAME, NONE, and SPREAD(1) with every third pod of the app NONE.
    The pods are then grouped by app inside blocks of 64 arrivals, which makes runs of consecutive
    same-app SPREAD pods (with qos_sort = 0 the stream keeps them)."""
    pods = pods.copy()
    x = (pods["app"].astype(np.int64) - 24) // 25
    assert int(x.max()) < apps
    table = np.array([S.spread(1), S.spread(2), A.ZONE, A.HOSTNAME, A.NONE, S.spread(1)])
    kind = table[x % 6]
    seen = {}
    for j in np.flatnonzero(x % 6 == 5):
        k = seen.get(int(x[j]), 0)
        seen[int(x[j])] = k + 1
        if k % 3 == 2:
            kind[j] = A.NONE
    pods["anti_affinity"] = kind
    order = np.lexsort((pods["app"], np.arange(len(pods)) // 64))
    pods = np.ascontiguousarray(pods[order])
    if zones is not None:
        nodes = dict(nodes)
        nodes["zone"] = np.asarray(zones)[nodes["zone"]].astype(nodes["zone"].dtype)
    return nodes, pods


def c5(n, p, apps=40, zones=4, zone_ids=None):
    return redraw(*C.c5(n, p, apps, zones), apps, zone_ids)


def c4(n, p, apps=40, zones=4):
    return redraw(*C.c4(n, p, apps, zones), apps)


def wide(n, p):
    return redraw(*C.wide(n, p), 40)


def many_apps(n, p, apps):
    """`apps` distinct apps, all SPREAD (max_skew 1 and 2 alternating): the spread-app cap of PERSISTENT.
    App ids 14 x + 20 (up to 986 for 70 apps)."""
    nodes, pods = qsched.synth_generate(5, n, p)
    pods = pods.copy()
    x = pods["app"].astype(np.int64) % apps
    x[:apps] = np.arange(apps)  # every app occurs
    pods["app"] = x * 14 + 20
    assert int(pods["app"].max()) < A.MAX_APPS
    pods["anti_affinity"] = np.where(x % 2 == 0, S.spread(1), S.spread(2))
    nodes = dict(nodes)
    nodes["zone"] = nodes["zone"] % 4
    return nodes, pods


def _cfg(**kw):
    return dict(ARRIVAL, **kw)


# name: (cluster builder, configuration, engine asked for, engine that must run, scorer, flags)
PARITY = {
    # PERSISTENT, default class: one 64-thread block (3 zones, tight); one, two (ragged) and three nodes per lane
    "persistent-24": (lambda: c5(24, 600, 20, 3), _cfg(), "auto", "persistent", None, {"tight"}),
    "persistent-300": (lambda: c5(300, 1500), _cfg(), "auto", "persistent", None, set()),
    "persistent-1100": (lambda: c5(1100, 2000), _cfg(), "auto", "persistent", None, set()),
    "persistent-2049": (lambda: c5(2049, 3000), _cfg(), "auto", "persistent", None, set()),
    # SCAN over rows, over the column-major copy, and where AUTO picks it
    "scan-700": (lambda: c5(700, 1200), _cfg(), "scan", "scan", None, set()),
    "scan-soa-300": (lambda: c5(300, 1000), _cfg(scan_soa_min_nodes=1), "scan", "scan", None, set()),
    "scan-3073": (lambda: c5(3073, 1000), _cfg(), "auto", "scan", None, set()),
    # general class
    "norm-persistent": (lambda: c4(600, 1500), _cfg(**C.CFG4), "auto", "persistent", None, set()),
    "norm-scan": (lambda: c4(600, 1500), _cfg(**C.CFG4), "scan", "scan", None, set()),
    "most-persistent": (lambda: c5(300, 1200), _cfg(**C.MOST), "auto", "persistent", "strategy", set()),
    "qos-mix": (lambda: c5(300, 1200), _cfg(**C.QOS_MIX), "auto", "persistent", "qos", set()),
    "gpu-list": (lambda: c4(600, 1500), _cfg(**GPU_CFG), "auto", "persistent", None, set()),
    # wide layout
    "wide-persistent": (lambda: wide(1100, 1500), _cfg(), "auto", "persistent", None, {"wide"}),
    "wide-scan": (lambda: wide(300, 1000), _cfg(), "scan", "scan", None, {"wide"}),
    # zone ids {0, 5, 63}: the 61 absent zones must not pull the minimum to 0
    "sparse-persistent": (lambda: c5(300, 1200, 40, 3, SPARSE_ZONES), _cfg(), "auto", "persistent", None, {"sparse"}),
    "sparse-scan": (lambda: c5(300, 1200, 40, 3, SPARSE_ZONES), _cfg(), "scan", "scan", None, {"sparse"}),
}


@functools.lru_cache(maxsize=None)
def parity_case(name):
    build, cfg, engine, runs, kind, flags = PARITY[name]
    nodes, pods = build()
    ocfg = {k: v for k, v in cfg.items() if k != "scan_soa_min_nodes"}
    pl, keys, final, state = S.run(nodes, pods, ocfg, C.scorer_of(kind, ocfg))
    return dict(name=name, nodes=nodes, pods=pods, cfg=cfg, ocfg=ocfg, engine=engine, runs=runs, kind=kind,
                flags=flags, pl=pl, keys=keys, final=final, state=state)


def plain_run(case):
    """The same stream without any filter, its pods still recorded: (placements, state)."""
    p = case["pods"].copy()
    p["anti_affinity"] = 0
    pl, _, _, st = S.run(case["nodes"], p, case["ocfg"], C.scorer_of(case["kind"], case["ocfg"]))
    return pl, st


def pure_spread_apps(pods):
    """{app: max_skew} of the apps whose pods are all SPREAD with one max_skew."""
    out = {}
    for app in np.unique(pods["app"]):
        v = np.unique(pods["anti_affinity"][pods["app"] == app])
        if len(v) == 1 and int(S.kind_of(v[0])) == S.SPREAD:
            out[int(app)] = int(S.skew_of(v[0]))
    return out


def check_conditions(case):
    """From the reference alone, before any GPU run (see the issue's list)."""
    pods, pl = case["pods"], case["pl"]
    kind = S.kind_of(pods["anti_affinity"])
    plain_pl, plain_st = plain_run(case)
    differ = int((pl != plain_pl).sum())
    pure = pure_spread_apps(pods)
    assert pure
    held = [S.skew_of_app(case["state"], a) <= s for a, s in pure.items()]
    broken = [S.skew_of_app(plain_st, a) > s for a, s in pure.items()]
    unsched = int(((pl < 0) & (kind == S.SPREAD)).sum())
    app = pods["app"]
    runs = int(((kind[1:] == S.SPREAD) & (kind[:-1] == S.SPREAD) & (app[1:] == app[:-1])).sum())
    print(f"{case['name']}: {differ} placed differently, {len(pure)} pure spread apps ({sum(broken)} violated "
          f"without the filter), {unsched} SPREAD pods unschedulable, {runs} same-app SPREAD successors")
    assert differ >= 1, case["name"]
    assert all(held), case["name"]
    assert any(broken), case["name"]
    assert runs >= 1, case["name"]
    assert set(np.unique(kind)) == {A.NONE, A.HOSTNAME, A.ZONE, S.SPREAD}
    if "tight" in case["flags"]:
        assert unsched >= 1, case["name"]
    if "sparse" in case["flags"]:
        assert set(np.unique(case["nodes"]["zone"])) == {0, 5, 63}
        wrong = S.run(case["nodes"], pods, case["ocfg"], C.scorer_of(case["kind"], case["ocfg"]), all_zones=True)[0]
        assert not np.array_equal(wrong, pl), case["name"]
    assert int(app.max()) >= 480  # ids beyond the first presence words
