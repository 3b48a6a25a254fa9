"""Inputs shared by tests/test_antiaffinity_cpu.py and tests/test_gpu_antiaffinity.py (spec S12): the
known answers K27-K31 of spec/kat.md as clusters, and the parity inputs with their references
(tests/antiaffinity_ref.py), each computed once per process.  CPU only.
"""
import functools

import numpy as np

import qsched
from oracle import oracle as O

import antiaffinity_ref as A
from rescfg import GPU_CFG

GIB, MIB, KI = 1 << 30, 1 << 20, 1 << 10
CFG4 = dict(enable_taint=1, enable_affinity=1)
FALL30 = [(0, 10), (30, 0)]
MOST = dict(scoring_strategy="MostAllocated")
QOS_MIX = dict(qos_strategies={"BestEffort": dict(scoring_strategy="MostAllocated"),
                               "Burstable": dict(scoring_strategy="RequestedToCapacityRatio", shape=FALL30),
                               "Guaranteed": dict(scoring_strategy="LeastAllocated")})


# ---- known answers (spec/kat.md K27-K31) ---------------------------------------------------------
def _nodes(sizes, zones=None):
    nodes, _ = O.empty_cluster(len(sizes), 0)
    for i, big in enumerate(sizes):
        nodes["alloc_cpu"][i], nodes["alloc_mem"][i] = (8000, 16 * GIB) if big else (2000, 4 * GIB)
    nodes["max_pods"][:] = 110
    if zones is not None:
        nodes["zone"][:] = zones
    return nodes


def _pods(specs):
    """specs: (qos, app, kind) of pods requesting 1000 m / 2 GiB."""
    _, pods = O.empty_cluster(0, len(specs))
    for j, (qos, app, kind) in enumerate(specs):
        pods["qos"][j], pods["app"][j], pods["anti_affinity"][j] = qos, app, kind
    pods["req_cpu"][:] = pods["nz_cpu"][:] = 1000
    pods["req_mem"][:] = pods["nz_mem"][:] = 2 * GIB
    return pods


K31_STEPS = [(0, +1, [1]), (1, +1, []), (1, -1, [1]), (0, -1, [0, 1])]  # (node, sign, feasible set of H and of Z)


def kat(name):
    """(nodes, pods, cfg, placements, winners' totals) of one known answer, computed by hand."""
    if name == "K27":
        return _nodes([1, 0]), _pods([(2, 7, A.HOSTNAME)] * 2), {}, [0, 1], [361, 250]
    if name == "K28":
        return _nodes([1, 1, 1], [0, 0, 1]), _pods([(1, 3, A.ZONE)] * 3), {}, [0, 2, -1], [274, 274, 0]
    if name == "K29":
        pods = _pods([(2, 5, A.NONE), (2, 5, A.HOSTNAME), (2, 6, A.HOSTNAME)])
        return _nodes([1, 0]), pods, {}, [0, 1, 0], [361, 250, 325]
    if name == "K30":
        nodes = _nodes([1, 1, 1])
        nodes["label_bits"][:, 0] = [3, 1, 2]
        nodes["req_cpu"][1] = nodes["nz_cpu"][1] = 2720
        nodes["req_mem"][1] = nodes["nz_mem"][1] = 5570 * MIB
        nodes["pods"][1] = 1
        pods = _pods([(2, 9, A.NONE), (2, 9, A.HOSTNAME)])
        pods["n_pref_terms"][1] = 2
        pods["pref_terms"][1, 0, 0], pods["pref_weight"][1, 0] = 1, 50
        pods["pref_terms"][1, 1, 0], pods["pref_weight"][1, 1] = 2, 20
        return nodes, pods, dict(enable_affinity=1), [0, 1], [361, 458]
    if name == "K31":
        return _nodes([1, 1], [0, 1]), _pods([(2, 4, A.HOSTNAME), (2, 4, A.ZONE)]), {}, None, None
    raise KeyError(name)


# ---- parity inputs -------------------------------------------------------------------------------
def c5(n, p, apps=40, zones=4, seed=None):
    """Config-5 cluster, apps folded to `apps` groups whose ids spread over the presence words up to the
    last one ((app % apps) * 25 + 24: 999 for 40 apps), zones folded to `zones`."""
    nodes, pods = qsched.synth_generate(5, n, p, seed=seed)
    return A.fold(nodes, pods, apps, zones)


def c4(n, p, apps=40, zones=4):
    """Config-4 cluster (taints, labels, amd.com/gpu, zones) with config 5's app / anti_affinity draws."""
    nodes, pods = qsched.synth_generate(4, n, p)
    _, p5 = qsched.synth_generate(5, n, p)
    pods["app"], pods["anti_affinity"] = p5["app"], p5["anti_affinity"]
    return A.fold(nodes, pods, apps, zones)


def wide(n, p):
    """Odd-Ki node memory and decimal (100M ...) pod requests: the wide device layout."""
    nodes, pods = c5(n, p)
    rng = np.random.default_rng(7)
    nodes["alloc_mem"][:] = (rng.integers(64 << 20, 768 << 20, n) | 1) * KI
    dec = rng.choice([100 * 10**6, 512 * 10**6, 10**9, 3 * 10**9], p)
    has = pods["req_mem"] > 0
    pods["req_mem"] = np.where(has, dec, 0)
    pods["nz_mem"] = np.where(has, dec, O.DEF_MEM)
    return nodes, pods


# name: (cluster builder, configuration, engine asked for, engine that must run, scorer, flags)
PARITY = {
    # PERSISTENT, default class: one 64-thread block and hostname apps with more pods than nodes;
    # one, two (ragged tail) and three nodes per lane
    "persistent-24": (lambda: c5(24, 600, 20, 3), {}, "auto", "persistent", None, {"tight"}),
    "persistent-300": (lambda: c5(300, 1500), {}, "auto", "persistent", None, set()),
    "persistent-1100": (lambda: c5(1100, 2000), {}, "auto", "persistent", None, set()),
    "persistent-2049": (lambda: c5(2049, 3000), {}, "auto", "persistent", None, set()),
    # SCAN over rows, over the column-major copy (columns padded to 320), and where AUTO picks it
    "scan-700": (lambda: c5(700, 1200), {}, "scan", "scan", None, set()),
    "scan-soa-300": (lambda: c5(300, 1000), dict(scan_soa_min_nodes=1), "scan", "scan", None, set()),
    "scan-3073": (lambda: c5(3073, 1000), {}, "auto", "scan", None, set()),
    # general class
    "norm-persistent": (lambda: c4(600, 1500), CFG4, "auto", "persistent", None, set()),
    "norm-scan": (lambda: c4(600, 1500), CFG4, "scan", "scan", None, set()),
    "most-persistent": (lambda: c5(300, 1200), MOST, "auto", "persistent", "strategy", set()),
    "most-scan-2049": (lambda: c5(2049, 1000), MOST, "auto", "scan", "strategy", set()),  # just above the general cap
    "most-scan-soa": (lambda: c5(300, 1000), dict(MOST, scan_soa_min_nodes=1), "scan", "scan", "strategy", set()),
    "qos-mix": (lambda: c5(300, 1200), QOS_MIX, "auto", "persistent", "qos", set()),
    "gpu-list": (lambda: c4(600, 1500), GPU_CFG, "auto", "persistent", None, set()),
    "gpu-list-norm-scan": (lambda: c4(600, 1200), dict(GPU_CFG, **CFG4), "scan", "scan", None, set()),
    # wide layout
    "wide-persistent": (lambda: wide(1100, 1500), {}, "auto", "persistent", None, {"wide"}),
    "wide-scan": (lambda: wide(300, 1000), {}, "scan", "scan", None, {"wide"}),
    "wide-norm-scan-1025": (lambda: wide_norm(1025, 1000), CFG4, "auto", "scan", None, {"wide"}),
}


def wide_norm(n, p):
    nodes, pods = c4(n, p)
    w, wp = wide(n, p)
    nodes["alloc_mem"] = w["alloc_mem"]
    has = pods["req_mem"] > 0
    pods["req_mem"] = np.where(has, wp["nz_mem"], 0)
    pods["nz_mem"] = np.where(has, wp["nz_mem"], O.DEF_MEM)
    return nodes, pods


def scorer_of(kind, cfg):
    if kind == "strategy":
        return A.strategy_scorer(cfg)
    if kind == "qos":
        return A.qos_scorer(cfg)
    return A.oracle_scorer(cfg)


@functools.lru_cache(maxsize=None)
def parity_case(name):
    build, cfg, engine, runs, kind, flags = PARITY[name]
    nodes, pods = build()
    ocfg = {k: v for k, v in cfg.items() if k != "scan_soa_min_nodes"}
    pl, keys, final, state = A.run(nodes, pods, ocfg, scorer_of(kind, ocfg))
    return dict(name=name, nodes=nodes, pods=pods, cfg=cfg, ocfg=ocfg, engine=engine, runs=runs, kind=kind,
                flags=flags, pl=pl, keys=keys, final=final, state=state)


def plain_placements(case):
    """The same stream without the filter (oracle.schedule's semantics, the case's scorer)."""
    nodes = {k: v.copy() for k, v in case["nodes"].items()}
    pods = A.pods_dict(case["pods"])
    if case["kind"] is None:
        return O.schedule(nodes, pods, case["ocfg"])[0]
    p = pods.copy() if isinstance(pods, np.ndarray) else {k: v.copy() for k, v in pods.items()}
    p["anti_affinity"] = np.zeros_like(p["anti_affinity"])
    return A.schedule(nodes, p, case["ocfg"], scorer_of(case["kind"], case["ocfg"]))[0]


def check_conditions(case):
    """From the reference alone, before any GPU run: a pod placed differently than without the filter,
    an unschedulable ZONE pod, and in the tight case an unschedulable HOSTNAME pod."""
    pl, kind = case["pl"], np.asarray(case["pods"]["anti_affinity"])
    differ = int((pl != plain_placements(case)).sum())
    zone = int(((pl < 0) & (kind == A.ZONE)).sum())
    host = int(((pl < 0) & (kind == A.HOSTNAME)).sum())
    print(f"{case['name']}: {differ} placed differently, {zone} ZONE / {host} HOSTNAME pods unschedulable")
    assert differ >= 1, case["name"]
    assert zone >= 1, case["name"]
    if "tight" in case["flags"]:
        assert host >= 1, case["name"]
    assert int(np.asarray(case["pods"]["app"]).max()) >= 480  # ids beyond the first presence words
