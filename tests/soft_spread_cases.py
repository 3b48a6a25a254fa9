"""Inputs shared by tests/test_soft_spread_cpu.py and tests/test_gpu_soft_spread.py (spec S14): the known
answers K37-K41 of spec/kat.md as clusters, and the parity inputs with their references
(tests/soft_spread_ref.py), each computed once per process.  CPU only.
"""
import functools

import numpy as np

import qsched

import antiaffinity_cases as C
import antiaffinity_ref as A
import soft_spread_ref as R
import spread_cases as SC
import spread_ref as S
from rescfg import GPU_CFG

ARRIVAL = SC.ARRIVAL


# ---- known answers (spec/kat.md K37-K41) ---------------------------------------------------------
# K41: (node, sign, [PTS zone 0, PTS zone 1] of the soft probe pod afterwards)
K41_STEPS = [(0, +1, [0, 100]), (1, +1, [100, 100]), (1, +1, [100, 33]), (0, +1, [100, 100]), (1, -1, [33, 100]),
             (1, -1, [0, 100]), (0, -1, [0, 100]), (0, -1, [100, 100])]


def kat(name):
    """(nodes, pods, cfg, placements, winners' totals, per-node totals of the last pod) of one known
    answer, computed by hand (Wpts = 2; an empty big node totals 274 for these pods, one that holds one
    of them 250: K32, K33)."""
    s1, s3 = R.spread_soft(1), R.spread_soft(3)
    if name == "K37":  # mx = 0, then (0, 100), then a tie at raw 1
        return C._nodes([1, 1, 1], [0, 0, 1]), C._pods([(1, 3, s1)] * 3), {}, [0, 2, 1], [474, 474, 474], [450, 474, 450]
    if name == "K38":  # c = (1, 2), D = 2: raw (1, 3) rounded, (1, 2) truncated; 100 / 3 truncates to 33
        pods = C._pods([(1, 3, A.NONE)] * 3 + [(1, 3, s1)])
        return C._nodes([1, 1, 1, 1], [0, 1, 1, 1]), pods, {}, [0, 1, 2, 0], [274, 274, 274, 450], [450, 316, 316, 340]
    if name == "K39":  # zone 2 holds no feasible node: D = 2 and mn = 1 (over every domain: D = 3, mn = 0)
        nodes = C._nodes([1, 1, 1, 1], [0, 0, 1, 2])
        nodes["max_pods"][3] = 0
        pods = C._pods([(1, 3, A.NONE)] * 3 + [(1, 3, s1)])
        return nodes, pods, {}, [0, 1, 2, 2], [274, 274, 274, 450], [316, 316, 450, -1]
    if name == "K40":  # K38 with max_skew 3: raw (3, 5), PTS (100, 60)
        pods = C._pods([(1, 3, A.NONE)] * 3 + [(1, 3, s3)])
        return C._nodes([1, 1, 1, 1], [0, 1, 1, 1]), pods, {}, [0, 1, 2, 0], [274, 274, 274, 450], [450, 370, 370, 394]
    if name == "K41":  # Reserve / Unreserve on the score path (K41_STEPS)
        return C._nodes([1, 1], [0, 1]), C._pods([(2, 4, s1), (2, 4, A.HOSTNAME)]), {}, None, None, None
    raise KeyError(name)


# ---- parity inputs -------------------------------------------------------------------------------
SKEWS = (1, 3, 31)


def mix(nodes, pods, small_zone=True):
    """Every pod's kind redrawn by its arrival index, so that soft (max_skew 1, 3, 31), SPREAD, ZONE,
    HOSTNAME and plain pods of shared apps alternate at every pod: of 8 consecutive pods 4 are soft.  The
    highest zone takes one pod on each of its first p / 16 nodes and none on the others (`small_zone`):
    once those are full that zone holds no feasible node, so D drops below the table's domain count."""
    pods = pods.copy()
    j = np.arange(len(pods))
    table = np.array([R.spread_soft(1), A.NONE, R.spread_soft(3), S.spread(2), R.spread_soft(31), A.HOSTNAME,
                      R.spread_soft(1), A.ZONE])
    pods["anti_affinity"] = table[j % 8]
    nodes = {k: v.copy() for k, v in nodes.items()}
    if small_zone:
        last = np.flatnonzero(nodes["zone"] == nodes["zone"].max())
        keep = max(1, len(pods) // 16)
        nodes["max_pods"][last[:keep]] = 1
        nodes["max_pods"][last[keep:]] = 0
    return nodes, pods


def c5(n, p, apps=6, zones=4, zone_ids=None, small_zone=True):
    nodes, pods = C.c5(n, p, apps, zones)
    if zone_ids is not None:
        nodes["zone"] = np.asarray(zone_ids)[nodes["zone"]].astype(nodes["zone"].dtype)
    return mix(nodes, pods, small_zone)


def c4(n, p, apps=6, zones=4):
    return mix(*C.c4(n, p, apps, zones))


def wide(n, p):
    nodes, pods = C.wide(n, p)
    pods["app"] = (pods["app"].astype(np.int64) // 25 % 6) * 25 + 24
    return mix(nodes, pods)


def wide_norm(n, p):
    """Config-4 nodes and pods (taints, labels, preferred terms, amd.com/gpu) in the wide layout."""
    nodes, pods = C.wide_norm(n, p)
    pods["app"] = (pods["app"].astype(np.int64) // 25 % 6) * 25 + 24
    return mix(nodes, pods)


def tiny(n, p=40):
    """1-3 nodes (fewer nodes than lanes hold a zone), zones {0, 5, 63}, one pod per node of zone 63."""
    nodes, pods = C.c5(3, p, 3, 3)
    nodes = {k: v[:n].copy() for k, v in nodes.items()}
    nodes["zone"][:] = SC.SPARSE_ZONES[:n]
    return mix(nodes, pods, small_zone=n == 3)


def one_pod_per_node(n, p):
    nodes, pods = c5(n, p, small_zone=False)
    nodes["max_pods"][:] = 1
    return nodes, pods


def many_apps(n, p, apps):
    """`apps` distinct apps of soft and SPREAD pods alternating: the spread-app cap of PERSISTENT, shared."""
    nodes, pods = SC.many_apps(n, p, apps)
    pods = pods.copy()
    j = np.arange(len(pods))
    pods["anti_affinity"] = np.where(j % 2 == 0, R.spread_soft(1), pods["anti_affinity"])
    return nodes, pods


def _cfg(**kw):
    return dict(ARRIVAL, **kw)


# name: (cluster builder, configuration, engine asked for, engine that must run, scorer, Wpts, flags)
PARITY = {
    # the six classes on PERSISTENT: default, general (MostAllocated; a resource list), general + normalizing
    "persistent-24": (lambda: c5(24, 600, 6, 3), _cfg(), "auto", "persistent", None, 2, set()),
    "persistent-65": (lambda: c5(65, 800), _cfg(), "auto", "persistent", None, 2, set()),
    "persistent-1100": (lambda: c5(1100, 2000), _cfg(), "auto", "persistent", None, 2, set()),
    "most-persistent": (lambda: c5(300, 1200), _cfg(**C.MOST), "auto", "persistent", "strategy", 2, set()),
    "gpu-list": (lambda: c4(600, 1500), _cfg(**GPU_CFG), "auto", "persistent", None, 2, set()),
    "norm-persistent": (lambda: c4(600, 1500), _cfg(**C.CFG4), "auto", "persistent", None, 2, set()),
    "wide-persistent": (lambda: wide(1100, 1500), _cfg(), "auto", "persistent", None, 2, {"wide"}),
    "wide-most-persistent": (lambda: wide(300, 1200), _cfg(**C.MOST), "auto", "persistent", "strategy", 2, {"wide"}),
    "wide-gpu-list": (lambda: wide_norm(600, 1500), _cfg(**GPU_CFG), "auto", "persistent", None, 2, {"wide"}),
    "wide-norm-persistent": (lambda: wide_norm(300, 1000), _cfg(**C.CFG4), "auto", "persistent", None, 2, {"wide"}),
    # ... and on SCAN: rows, the column-major copy (a soft pod goes through the row kernels), AUTO above the cap
    "scan-64": (lambda: c5(64, 800), _cfg(), "scan", "scan", None, 2, set()),
    "scan-700": (lambda: c5(700, 1200), _cfg(), "scan", "scan", None, 2, set()),
    "scan-soa-300": (lambda: c5(300, 1000), _cfg(scan_soa_min_nodes=1), "scan", "scan", None, 2, set()),
    "norm-scan": (lambda: c4(600, 1500), _cfg(**C.CFG4), "scan", "scan", None, 2, set()),
    "norm-auto-scan-1100": (lambda: c4(1100, 1200), _cfg(**C.CFG4), "auto", "scan", None, 2, set()),
    "most-scan": (lambda: c5(300, 1200), _cfg(**C.MOST), "scan", "scan", "strategy", 2, set()),
    "wide-scan": (lambda: wide(300, 1000), _cfg(), "scan", "scan", None, 2, {"wide"}),
    "wide-most-scan": (lambda: wide(300, 1200), _cfg(**C.MOST), "scan", "scan", "strategy", 2, {"wide"}),
    "wide-gpu-list-scan": (lambda: wide_norm(600, 1500), _cfg(**GPU_CFG), "scan", "scan", None, 2, {"wide"}),
    "wide-norm-scan": (lambda: wide_norm(300, 1000), _cfg(**C.CFG4), "scan", "scan", None, 2, {"wide"}),
    # zone ids {0, 5, 63}
    "sparse-persistent": (lambda: c5(300, 1200, 6, 3, SC.SPARSE_ZONES), _cfg(), "auto", "persistent", None, 2, set()),
    "sparse-scan": (lambda: c5(300, 1200, 6, 3, SC.SPARSE_ZONES), _cfg(), "scan", "scan", None, 2, set()),
    # three nodes in three zones
    "tiny-3": (lambda: tiny(3), _cfg(), "auto", "persistent", None, 2, set()),
}


# Wpts = 0 and 100 run on inputs of PARITY (whose conditions hold at Wpts = 2): at 100 the zone with the
# smallest raw count wins nearly every pod under either wrong variant too, so placements alone cannot
# tell the variants apart there; the keys are compared bit for bit all the same.
WEIGHTS = [("persistent-24", 0), ("persistent-24", 100), ("scan-64", 0), ("scan-64", 100), ("norm-persistent", 100)]


def reference(nodes, pods, ocfg, kind, **kw):
    return R.run(nodes, pods, ocfg, C.scorer_of(kind, ocfg), **kw)


@functools.lru_cache(maxsize=None)
def parity_case(name):
    build, cfg, engine, runs, kind, wpts, flags = PARITY[name]
    nodes, pods = build()
    ocfg = {k: v for k, v in cfg.items() if k != "scan_soa_min_nodes"}
    log = []
    pl, keys, final, state = reference(nodes, pods, ocfg, kind, wpts=wpts, log=log)
    return dict(name=name, nodes=nodes, pods=pods, cfg=cfg, ocfg=ocfg, engine=engine, runs=runs, kind=kind,
                wpts=wpts, flags=flags, pl=pl, keys=keys, final=final, state=state, log=log)


def check_conditions(case):
    """From the reference alone, before any GPU run (see the issue's list)."""
    nodes, pods, ocfg, kind, pl = case["nodes"], case["pods"], case["ocfg"], case["kind"], case["pl"]
    off = reference(nodes, pods, ocfg, kind, wpts=0)[0]
    dom = reference(nodes, pods, ocfg, kind, wpts=case["wpts"], all_domains=True)[0]
    trunc = reference(nodes, pods, ocfg, kind, wpts=case["wpts"], truncate=True)[0]
    log = case["log"]
    few = sum(1 for D, nd, mn, mx in log if D < nd)
    mx0 = sum(1 for D, nd, mn, mx in log if mx == 0)
    mnp = sum(1 for D, nd, mn, mx in log if mn > 0)
    print(f"{case['name']}: {len(log)} soft pods scored; placed differently from Wpts = 0: {int((pl != off).sum())}, "
          f"from all-domains: {int((pl != dom).sum())}, from truncation: {int((pl != trunc).sum())}; "
          f"D below the domain count: {few}, mx = 0: {mx0}, mn > 0: {mnp}")
    assert not np.array_equal(pl, off), case["name"]
    assert not np.array_equal(pl, dom), case["name"]
    assert not np.array_equal(pl, trunc), case["name"]
    assert few >= 1 and mx0 >= 1 and mnp >= 1, case["name"]
    k = pods["anti_affinity"]
    assert set(np.unique(S.kind_of(k))) == {A.NONE, A.HOSTNAME, A.ZONE, S.SPREAD}
    assert set(np.unique(S.skew_of(k[R.is_soft(k)]))) == set(SKEWS)
    assert len(pods) <= 2000
