"""Inputs shared by tests/test_hostspread_cpu.py and tests/test_gpu_hostspread.py (spec S15): the known
answers K42-K47 of spec/kat.md as clusters, and the parity inputs with their references
(tests/hostspread_ref.py), each computed once per process.  CPU only.
"""
import functools

import numpy as np

import qsched

import antiaffinity_cases as C
import antiaffinity_ref as A
import hostspread_ref as H
import spread_ref as S
from rescfg import GPU_CFG

ARRIVAL = dict(qos_sort=0)  # arrival order: the runs of same-app pods below stay consecutive
HS1, HS2 = H.spread_hostname(1), H.spread_hostname(2)


# ---- known answers (spec/kat.md K42-K47) ---------------------------------------------------------
# (node, sign, feasible set of the HOSTSPREAD(1) pod) of K46
K46_STEPS = [(0, +1, [1]), (1, +1, [0, 1]), (1, -1, [1]), (1, +1, [0, 1]), (1, +1, [0]), (0, -1, [0])]


def kat(name):
    """(nodes, pods, cfg, placements) of one known answer, computed by hand."""
    if name == "K42":  # the preferred (big) node closed by the skew: the small node wins
        return C._nodes([1, 0]), C._pods([(1, 3, HS1)] * 2), {}, [0, 1]
    if name == "K43":  # m rises to 1 and reopens every node
        return C._nodes([1, 1]), C._pods([(1, 3, HS1)] * 3), {}, [0, 1, 0]
    if name == "K44":  # a full node holds m at 0 until a pod is unschedulable
        nodes = C._nodes([1, 1, 1])
        nodes["max_pods"][2] = 0
        return nodes, C._pods([(1, 3, HS1)] * 3), {}, [0, 1, -1]
    if name == "K45":  # a NONE and a HOSTNAME pod of the app are counted
        pods = C._pods([(1, 3, A.NONE), (1, 3, A.HOSTNAME), (1, 3, HS1), (1, 3, HS1), (1, 3, HS1)])
        return C._nodes([1, 1]), pods, {}, [0, 1, 0, 1, 0]
    if name == "K46":  # qs_reserve / qs_unreserve (K46_STEPS)
        return C._nodes([1, 1]), C._pods([(2, 4, HS1), (2, 4, A.HOSTNAME)]), {}, None
    if name == "K47":  # K42's input with max_skew 2 and a third pod: the big node takes two
        return C._nodes([1, 0]), C._pods([(1, 3, HS2)] * 3), {}, [0, 0, 1]
    raise KeyError(name)


# ---- parity inputs -------------------------------------------------------------------------------
def redraw(nodes, pods, apps):
    """Kinds redrawn per app of a folded cluster (antiaffinity_ref.fold: app id = 25 x + 24): by x % 7
    HOSTSPREAD(1), HOSTSPREAD(2), SPREAD(1), ZONE, HOSTNAME, NONE, and HOSTSPREAD(1) with every third pod
    of the app NONE.  The pods are then grouped by app inside blocks of 64 arrivals, which makes runs of
    consecutive same-app pods (with qos_sort = 0 the stream keeps them)."""
    pods = pods.copy()
    x = ((pods["app"].astype(np.int64) - 24) // 25) % apps  # (35 apps: 15 of them hostname-spread, within the
    pods["app"] = x * 25 + 24                                 # 16 slots of PERSISTENT)
    table = np.array([HS1, HS2, S.spread(1), A.ZONE, A.HOSTNAME, A.NONE, HS1])
    kind = table[x % 7]
    seen = {}
    for j in np.flatnonzero(x % 7 == 6):
        k = seen.get(int(x[j]), 0)
        seen[int(x[j])] = k + 1
        if k % 3 == 2:
            kind[j] = A.NONE
    pods["anti_affinity"] = kind
    order = np.lexsort((pods["app"], np.arange(len(pods)) // 64))
    return nodes, np.ascontiguousarray(pods[order])


def c5(n, p, apps=35, zones=4):
    return redraw(*C.c5(n, p, apps, zones), apps)


def c4(n, p, apps=35, zones=4):
    return redraw(*C.c4(n, p, apps, zones), apps)


def wide(n, p):
    return redraw(*C.wide(n, p), 35)


def blocked_c5(n, p, apps=35):
    """One node no pod can take: max_pods already reached (it keeps every app's minimum at 0)."""
    nodes, pods = c5(n, p, apps)
    nodes = {k: v.copy() for k, v in nodes.items()}
    nodes["max_pods"][n // 2] = nodes["pods"][n // 2]
    return nodes, pods


def blocked_c4(n, p, apps=35):
    """One node with a hard taint that no pod tolerates."""
    nodes, pods = c4(n, p, apps)
    nodes = {k: v.copy() for k, v in nodes.items()}
    bit = np.uint64(1 << 62)
    nodes["taint_hard"][n // 2] |= bit
    pods["tol_hard"] &= ~bit
    return nodes, pods


def many_apps(n, p, apps):
    """`apps` distinct apps, all HOSTSPREAD (max_skew 1 and 2 alternating).  App ids 14 x + 20."""
    nodes, pods = qsched.synth_generate(5, n, p)
    pods = pods.copy()
    x = pods["app"].astype(np.int64) % apps
    x[:apps] = np.arange(apps)  # every app occurs
    pods["app"] = x * 14 + 20
    assert int(pods["app"].max()) < A.MAX_APPS
    pods["anti_affinity"] = np.where(x % 2 == 0, HS1, HS2)
    return dict(nodes), pods


def _cfg(**kw):
    return dict(ARRIVAL, **kw)


# name: (cluster builder, configuration, engine asked for, engine that must run, scorer, flags)
# flags: "min1" / "min2": some hostname-spread app's minimum reaches 1 / 2 (and the min_zero variant places
# differently); "blocked": a node no pod can take (and the feasible_only variant places differently);
# "wide": the wide layout
PARITY = {
    # PERSISTENT, default class: one 64-thread block (idle lanes must not feed the minimum; the minimum rises
    # to 1), three nodes with 12 pods per app (counts well beyond a bit), one, two (ragged) and three nodes per lane
    "persistent-24": (lambda: c5(24, 600, 20, 3), _cfg(), "auto", "persistent", None, {"min1"}),
    "persistent-3": (lambda: c5(3, 84, 7, 3), _cfg(), "auto", "persistent", None, {"min2"}),
    "persistent-300": (lambda: c5(300, 1500), _cfg(), "auto", "persistent", None, set()),
    "persistent-1100": (lambda: c5(1100, 2000), _cfg(), "auto", "persistent", None, set()),
    "persistent-2049": (lambda: c5(2049, 2500), _cfg(), "auto", "persistent", None, set()),
    # SCAN over rows (one 64-lane wave of real nodes in a 256-thread block at 24), where AUTO picks it, and
    # the column-major copy (columns padded to 128 and 320): padding rows must not feed the minimum
    "scan-24": (lambda: c5(24, 600, 20, 3), _cfg(), "scan", "scan", None, {"min1"}),
    "scan-3": (lambda: c5(3, 84, 7, 3), _cfg(), "scan", "scan", None, {"min2"}),
    "scan-700": (lambda: c5(700, 1200), _cfg(), "scan", "scan", None, set()),
    "scan-soa-65": (lambda: c5(65, 900, 10), _cfg(scan_soa_min_nodes=1), "scan", "scan", None, {"min1"}),
    "scan-soa-300": (lambda: c5(300, 1000), _cfg(scan_soa_min_nodes=1), "scan", "scan", None, set()),
    "scan-3073": (lambda: c5(3073, 1000), _cfg(), "auto", "scan", None, set()),
    # general class, both engines; the compact normalizing class runs PERSISTENT up to 1,024 nodes
    "norm-persistent": (lambda: c4(600, 1500), _cfg(**C.CFG4), "auto", "persistent", None, set()),
    "norm-scan": (lambda: c4(600, 1500), _cfg(**C.CFG4), "scan", "scan", None, set()),
    "norm-scan-1025": (lambda: c4(1025, 1200), _cfg(**C.CFG4), "auto", "scan", None, set()),
    # (config 4's own hard taints keep the minimum of most apps at 0: a naturally blocked table)
    "norm-65": (lambda: c4(65, 900, 10), _cfg(**C.CFG4), "auto", "persistent", None, set()),
    "most-65": (lambda: c5(65, 900, 10), _cfg(**C.MOST), "auto", "persistent", "strategy", {"min1"}),
    "most-65-scan": (lambda: c5(65, 900, 10), _cfg(**C.MOST), "scan", "scan", "strategy", {"min1"}),
    "most-persistent": (lambda: c5(300, 1200), _cfg(**C.MOST), "auto", "persistent", "strategy", set()),
    "qos-mix": (lambda: c5(300, 1200), _cfg(**C.QOS_MIX), "auto", "persistent", "qos", set()),
    "qos-mix-scan": (lambda: c5(300, 1200), _cfg(**C.QOS_MIX), "scan", "scan", "qos", set()),
    "gpu-list": (lambda: c4(600, 1500), _cfg(**GPU_CFG), "auto", "persistent", None, set()),
    "gpu-list-scan": (lambda: c4(600, 1500), _cfg(**GPU_CFG), "scan", "scan", None, set()),
    # wide layout
    "wide-persistent": (lambda: wide(1100, 1500), _cfg(), "auto", "persistent", None, {"wide"}),
    "wide-scan": (lambda: wide(300, 1000), _cfg(), "scan", "scan", None, {"wide"}),
    # a node that no pod can take keeps m at 0: hostname-spread pods are left unschedulable
    "blocked-c5": (lambda: blocked_c5(24, 600, 20), _cfg(), "auto", "persistent", None, {"blocked"}),
    "blocked-c5-scan": (lambda: blocked_c5(24, 600, 20), _cfg(), "scan", "scan", None, {"blocked"}),
    "blocked-c4": (lambda: blocked_c4(40, 900, 20), _cfg(**C.CFG4), "auto", "persistent", None, {"blocked"}),
    "blocked-c4-scan": (lambda: blocked_c4(40, 900, 20), _cfg(**C.CFG4), "scan", "scan", None, {"blocked"}),
}


@functools.lru_cache(maxsize=None)
def parity_case(name):
    build, cfg, engine, runs, kind, flags = PARITY[name]
    nodes, pods = build()
    ocfg = {k: v for k, v in cfg.items() if k != "scan_soa_min_nodes"}
    pl, keys, final, state = H.run(nodes, pods, ocfg, C.scorer_of(kind, ocfg))
    return dict(name=name, nodes=nodes, pods=pods, cfg=cfg, ocfg=ocfg, engine=engine, runs=runs, kind=kind,
                flags=flags, pl=pl, keys=keys, final=final, state=state)


def variant_run(case, variant=None, filter_off=False):
    """The same stream under a wrong variant, or without any filter (its pods still recorded)."""
    p = case["pods"].copy()
    if filter_off:
        p["anti_affinity"] = 0
    pl, _, _, st = H.run(case["nodes"], p, case["ocfg"], C.scorer_of(case["kind"], case["ocfg"]), variant=variant)
    return pl, st


def pure_apps(pods):
    """{app: max_skew} of the apps whose pods are all HOSTSPREAD with one max_skew."""
    out = {}
    for app in np.unique(pods["app"]):
        v = np.unique(pods["anti_affinity"][pods["app"] == app])
        if len(v) == 1 and int(H.is_hostkey(v[0])):
            out[int(app)] = int(S.skew_of(v[0]))
    return out


def check_conditions(case):
    """From the reference alone, before any GPU run."""
    pods, pl, name = case["pods"], case["pl"], case["name"]
    host = H.is_hostkey(pods["anti_affinity"]) == 1
    plain_pl, plain_st = variant_run(case, filter_off=True)
    differ = int((pl != plain_pl).sum())
    pure = pure_apps(pods)
    assert pure
    held = [H.skew_of_app(case["state"], a) <= s for a, s in pure.items()]
    broken = [H.skew_of_app(plain_st, a) > s for a, s in pure.items()]
    unsched = int(((pl < 0) & host).sum())
    app = pods["app"]
    runs = int((host[1:] & host[:-1] & (app[1:] == app[:-1])).sum())
    hs_apps = np.unique(app[host])
    top = max(int(case["state"].node[a].min()) for a in hs_apps)
    print(f"{name}: {differ} placed differently, {len(pure)} pure apps ({sum(broken)} violated without the "
          f"filter), {unsched} HOSTSPREAD pods unschedulable, {runs} same-app successors, largest minimum {top}")
    assert differ >= 1, name
    assert all(held), name
    assert any(broken), name
    assert runs >= 1, name
    if len(np.unique(app)) >= 20:
        assert int(app.max()) >= 480, name  # ids beyond the first presence words
    if "min1" in case["flags"] or "min2" in case["flags"]:
        assert top >= (2 if "min2" in case["flags"] else 1), name
        assert not np.array_equal(variant_run(case, "min_zero")[0], pl), name
    if "blocked" in case["flags"]:
        assert unsched >= 1, name
        assert top == 0, name
        assert not np.array_equal(variant_run(case, "feasible_only")[0], pl), name
