"""Inputs shared by tests/test_honor_spread_cpu.py and tests/test_gpu_honor_spread.py (spec S16): the known
answers K48-K52 of spec/kat.md as clusters, and the parity inputs with their references
(tests/honor_spread_ref.py), each computed once per process.  CPU only.
"""
import functools

import numpy as np

import qsched
from oracle import oracle as O

import antiaffinity_cases as C
import antiaffinity_ref as A
import honor_spread_ref as HR
import hostspread_ref as H
import soft_spread_ref as R
import spread_ref as S

AFF = dict(enable_affinity=1)  # the default scoring class with the NodeAffinity filter on (Honor needs it)
NORM = dict(enable_taint=1, enable_affinity=1)
SP1, SO1, HS1 = S.spread(1), R.spread_soft(1), H.spread_hostname(1)


# ---- known answers (spec/kat.md K48-K52) ---------------------------------------------------------
def _labelled(sizes, zones, labels):
    nodes = C._nodes(sizes, zones)
    nodes["label_bits"][:, 0] = labels
    return nodes


def _sel(pods, which, bits):
    for j in which:
        pods["sel"][j, 0] = bits
    return pods


def kat(name):
    """(nodes, pods, cfg, placements under HONOR, placements under IGNORE), worked by hand in spec/kat.md."""
    if name == "K48":  # zone 2 holds no node of M: under Ignore it pins the minimum at 0
        nodes = _labelled([1, 1, 1], [0, 1, 2], [1, 1, 0])
        return nodes, _sel(C._pods([(1, 3, SP1)] * 3), range(3), 1), AFF, [0, 1, 0], [0, 1, -1]
    if name == "K49":  # a pod of the app recorded on node 1, outside M = {0, 2}: not counted
        nodes = _labelled([1, 1, 1], [0, 0, 1], [1, 2, 1])
        pods = _sel(C._pods([(1, 3, A.NONE), (1, 3, SP1), (1, 3, SP1)]), [1, 2], 1)
        return nodes, _sel(pods, [0], 2), AFF, [1, 0, 2], [1, 2, 0]
    if name == "K50":  # soft: two pods of the app on node 2 (zone 0, outside M) change mn / mx under Ignore
        nodes = _labelled([1, 1, 1], [0, 1, 0], [1, 1, 2])
        pods = _sel(C._pods([(1, 3, A.NONE)] * 2 + [(1, 3, SO1)] * 2), [2, 3], 1)
        return nodes, _sel(pods, [0, 1], 2), AFF, [2, 2, 0, 1], [2, 2, 1, 1]
    if name == "K51":  # hostname: node 2 (count 0, outside M) pins the minimum at 0 under Ignore
        nodes = _labelled([1, 1, 1], [0, 0, 0], [1, 1, 2])
        return nodes, _sel(C._pods([(1, 3, HS1)] * 3), range(3), 1), AFF, [0, 1, 0], [0, 1, -1]
    if name == "K52":  # pods that do not restrict: S13 to the letter under either policy
        nodes = _labelled([1, 1, 1], [0, 0, 1], [1, 2, 1])
        return nodes, C._pods([(1, 3, SP1)] * 3), AFF, [0, 2, 1], [0, 2, 1]
    raise KeyError(name)


# K50's zone scores of its two soft pods (zones 0 and 1), under HONOR and under IGNORE
K50_ZONE_SCORES = {HR.HONOR: [(100, 100), (0, 100)], HR.IGNORE: [(0, 100), (33, 100)]}


# ---- parity inputs -------------------------------------------------------------------------------
ZONES = np.array([0, 5, 63])
# label bits: 0 ssd (preferred terms), 1 / 2 / 3 the node's zone (0 / 5 / 63), 4 pool A (three nodes in five),
# 70 pool B (every seventh of the first 70 nodes: ten nodes, those of zone 0 closed), 71 pool C (nodes 1-6)
L_SSD, L_Z0, L_Z5, L_Z63, L_A, L_B, L_C = 0, 1, 2, 3, 4, 70, 71


def _bit(b):
    return np.array([1 << b if b < 64 else 0, 1 << (b - 64) if b >= 64 else 0], np.uint64)


def cluster(n, p, kind, norm=False, wide=False, seed=None):
    """Config-5 resources on `n` nodes in the zones {0, 5, 63} with the labels above; `p` pods of eight
    apps.  Apps by x % 4: `kind`(1), `kind`(2), `kind`(1) with every third pod NONE, and a second kind
    (SPREAD(1); HOSTNAME spread(1) when `kind` is SPREAD).  Per pod one of six restrictions: none (2 in 7),
    pool A, zone 0 or zone 5 (two required terms), pool B, pool C, pool A and zone 5 or 63.  `norm`: soft
    taints, tolerations and preferred terms (the normalizing plugins have work).  `wide`: odd-Ki node memory and
    decimal pod requests (the wide layout)."""
    nodes, pods = qsched.synth_generate(5, n, p, seed=seed)
    nodes = {k: v.copy() for k, v in nodes.items()}
    pods = pods.copy()
    rng = np.random.default_rng(1000 * n + p + (seed or 0))
    i = np.arange(n)
    nodes["zone"][:] = ZONES[i % 3]
    lab = np.zeros((n, 2), np.uint64)
    lab[i % 2 == 0] |= _bit(L_SSD)
    for z, b in ((0, L_Z0), (5, L_Z5), (63, L_Z63)):
        lab[nodes["zone"] == z] |= _bit(b)
    lab[i % 5 < 3] |= _bit(L_A)
    pool_b = (i % 7 == 0) & (i < 70)
    lab[pool_b] |= _bit(L_B)
    lab[(i >= 1) & (i <= 6)] |= _bit(L_C)
    nodes["label_bits"][:] = lab
    nodes["max_pods"][pool_b & (nodes["zone"] == 0)] = 0  # zone 0 of pool B takes no pod: its count stays 0
    x = rng.integers(0, 8, p)
    pods["app"] = x * 123 + 7
    spread = {"spread": S.spread, "soft": R.spread_soft, "host": H.spread_hostname}[kind]
    second = H.spread_hostname(1) if kind == "spread" else S.spread(1)
    table = np.array([spread(1), spread(2), spread(1), second])
    aa = table[x % 4]
    seen = {}
    for j in np.flatnonzero(x % 4 == 2):
        k = seen.get(int(x[j]), 0)
        seen[int(x[j])] = k + 1
        if k % 3 == 2:
            aa[j] = A.NONE
    pods["anti_affinity"] = aa
    pods["sel"][:] = 0
    pods["n_req_terms"][:] = 0
    pods["req_terms"][:] = 0
    pods["n_pref_terms"][:] = 0
    pods["pref_terms"][:] = 0
    pods["pref_weight"][:] = 0
    r = rng.integers(0, 7, p)
    for j in range(p):
        if r[j] == 2:
            pods["sel"][j] = _bit(L_A)
        elif r[j] == 3:
            pods["n_req_terms"][j] = 2
            pods["req_terms"][j, 0], pods["req_terms"][j, 1] = _bit(L_Z0), _bit(L_Z5)
        elif r[j] == 4:
            pods["sel"][j] = _bit(L_B)
        elif r[j] == 5:
            pods["sel"][j] = _bit(L_C)
        elif r[j] == 6:
            pods["sel"][j] = _bit(L_A)
            pods["n_req_terms"][j] = 2
            pods["req_terms"][j, 0], pods["req_terms"][j, 1] = _bit(L_Z5), _bit(L_Z63)
    if norm:
        nodes["taint_soft"][:] = np.where(i % 4 == 1, 2, 0).astype(np.uint64)
        pods["tol_soft"] = np.where(rng.integers(0, 3, p) == 0, 2, 0).astype(np.uint64)
        pods["tol_hard"] = np.uint64(0)
        pref = rng.integers(0, 3, p)
        for j in np.flatnonzero(pref > 0):
            pods["n_pref_terms"][j] = pref[j]
            pods["pref_terms"][j, 0], pods["pref_weight"][j, 0] = _bit(L_SSD), 50
            if pref[j] == 2:
                pods["pref_terms"][j, 1], pods["pref_weight"][j, 1] = _bit(L_Z5), 20
    if wide:
        nodes["alloc_mem"][:] = (rng.integers(64 << 20, 768 << 20, n) | 1) * C.KI
        dec = rng.choice([100 * 10**6, 512 * 10**6, 10**9, 3 * 10**9], p)
        has = pods["req_mem"] > 0
        pods["req_mem"] = np.where(has, dec, 0)
        pods["nz_mem"] = np.where(has, dec, O.DEF_MEM)
    return nodes, pods


KINDS, SHAPES = ("spread", "soft", "host"), (70, 300)
# name: (kind, nodes, normalizing class, wide layout)
PARITY = {f"{k}-{n}-{'norm' if nm else 'default'}-{'wide' if w else 'compact'}": (k, n, nm, w)
          for k in KINDS for n in SHAPES for nm in (False, True) for w in (False, True)}
PODS = 400


def restricting(pods):
    """bool[p]: spread pods of any of the three kinds with a selector or required terms."""
    sp = (np.asarray(pods["anti_affinity"]) & 0xFF) == S.SPREAD
    return sp & (np.asarray(pods["sel"]).any(axis=1) | (np.asarray(pods["n_req_terms"]) > 0))


@functools.lru_cache(maxsize=None)
def parity_case(name):
    kind, n, norm, wide = PARITY[name]
    nodes, pods = cluster(n, PODS, kind, norm, wide)
    cfg = dict(NORM if norm else AFF)
    facts = []
    pl, keys, final, state = HR.run(nodes, pods, cfg, facts=facts)
    return dict(name=name, kind=kind, nodes=nodes, pods=pods, cfg=cfg, ocfg=cfg, wide=wide, pl=pl, keys=keys,
                final=final, state=state, facts=facts)


def old_reference(case):
    """The case under the reference of its kind as it stood before S16 (Ignore): placements and keys."""
    nodes, pods, cfg = case["nodes"], case["pods"], case["cfg"]
    if case["kind"] == "soft":
        return R.run(nodes, pods, cfg)[:2]
    if case["kind"] == "host":
        return H.run(nodes, pods, cfg)[:2]
    st = H.HostSpreadState(nodes["zone"])  # (the SPREAD cases' second kind is the hostname spread)
    return H.run(nodes, pods, cfg, state=st)[:2]


def check_conditions(case):
    """Conditions of the inputs, from the reference alone, before any GPU run."""
    name, pods, pl, facts = case["name"], case["pods"], case["pl"], case["facts"]
    rs = restricting(pods)
    share = float(rs.mean())
    no_node = sum(1 for f in facts if (f["zones_table"] & ~f["zones_m"]).any())
    outside = sum(1 for f in facts if f["outside"] > 0)
    by_rule = sum(1 for f in facts if f["fits_plain"] and not f["fits"])
    diff = {}
    for v in ("ignore", "domains_only", "counts_only"):
        diff[v] = int((HR.run(case["nodes"], pods, case["cfg"], variant=v)[0] != pl).sum())
    ign = HR.run(case["nodes"], pods, case["cfg"], policy=HR.IGNORE)
    old = old_reference(case)
    print(f"{name}: {share:.0%} restricting spread pods, {no_node} decided with a zone outside M, {outside} with "
          f"app pods outside M, {by_rule} unschedulable by the rule, placed differently under {diff}")
    assert len(facts) == int(rs.sum()), name
    assert share >= 0.20, name
    assert no_node >= 1 and outside >= 1 and by_rule >= 1, name
    assert all(d >= 1 for d in diff.values()), (name, diff)
    assert np.array_equal(ign[0], old[0]) and np.array_equal(ign[1], old[1]), name
