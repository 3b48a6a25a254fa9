"""Inputs shared by tests/test_taint_spread_cpu.py and tests/test_gpu_taint_spread.py (spec S17): the known
answers K53-K58 of spec/kat.md as clusters, and the parity inputs with their references
(tests/taint_spread_ref.py), each computed once per process.  CPU only.
"""
import functools

import numpy as np

import qsched
from oracle import oracle as O

import antiaffinity_cases as C
import antiaffinity_ref as A
import hostspread_ref as H
import soft_spread_ref as R
import spread_ref as S
import taint_spread_ref as TR

TAINT = dict(enable_taint=1)  # the normalizing class with the TaintToleration filter on (Honor needs it)
NORM = dict(enable_taint=1, enable_affinity=1)
SP1, SO1, HS1 = S.spread(1), R.spread_soft(1), H.spread_hostname(1)
IGNORE, HONOR = TR.IGNORE, TR.HONOR
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- known answers (spec/kat.md K53-K58) ---------------------------------------------------------
def _table(zones, taints, labels=None):
    nodes = C._nodes([1] * len(zones), zones)
    nodes["taint_hard"][:] = np.array(taints, np.uint64)
    if labels is not None:
        nodes["label_bits"][:, 0] = labels
    return nodes


def _set(pods, field, which, value):
    for j in which:
        if field == "sel":
            pods["sel"][j, 0] = value
        else:
            pods[field][j] = value
    return pods


def kat(name):
    """(nodes, pods, cfg, nodeAffinityPolicy, placements under nodeTaintsPolicy HONOR, under IGNORE), worked by
    hand in spec/kat.md.  Taint bit 0 is "T"; B pods of app 3 on big nodes."""
    if name == "K53":  # hostname: the tainted node (count 0, never usable) pins the minimum at 0 under Ignore
        nodes = _table([0, 0, 0, 0], [0, 0, 0, 1])
        return nodes, C._pods([(1, 3, HS1)] * 4), TAINT, IGNORE, [0, 1, 2, 0], [0, 1, 2, -1]
    if name == "K54":  # zone 2 holds untolerated nodes only: not a domain
        nodes = _table([0, 1, 2, 2], [0, 0, 1, 1])
        return nodes, C._pods([(1, 3, SP1)] * 3), TAINT, IGNORE, [0, 1, 0], [0, 1, -1]
    if name == "K55":  # a pod of the app recorded on node 1, untolerated by the others: not counted
        nodes = _table([0, 0, 1], [0, 1, 0], [1, 2, 1])
        pods = C._pods([(1, 3, A.NONE), (1, 3, SP1), (1, 3, SP1)])
        _set(pods, "sel", [0], 2)
        return nodes, _set(pods, "tol_hard", [0], 1), NORM, IGNORE, [1, 0, 2], [1, 2, 0]
    if name == "K56":  # soft: two pods of the app on node 2 (zone 0, untolerated) change mn / mx under Ignore
        nodes = _table([0, 1, 0], [0, 0, 1], [1, 1, 2])
        pods = C._pods([(1, 3, A.NONE)] * 2 + [(1, 3, SO1)] * 2)
        _set(pods, "sel", [0, 1], 2)
        return nodes, _set(pods, "tol_hard", [0, 1], 1), NORM, IGNORE, [2, 2, 0, 1], [2, 2, 1, 1]
    if name == "K57":  # both policies: M_A = {0, 1, 2}, M_T = {0, 1, 3}, M = {0, 1}
        nodes = _table([0] * 5, [0, 0, 1, 0, 1], [1, 1, 1, 0, 0])
        pods = _set(C._pods([(1, 3, HS1)] * 3), "sel", range(3), 1)
        return nodes, pods, NORM, HONOR, [0, 1, 0], [0, 1, -1]
    if name == "K58":  # pods that tolerate every bit: S13 to the letter under either policy
        nodes = _table([0, 1, 2, 2], [0, 0, 1, 1])
        pods = _set(C._pods([(1, 3, SP1)] * 3), "tol_hard", range(3), ALL)
        return nodes, pods, TAINT, IGNORE, [0, 1, 2], [0, 1, 2]
    raise KeyError(name)


KATS = ("K53", "K54", "K55", "K56", "K57", "K58")
# K56's zone scores of its two soft pods (zones 0 and 1), under HONOR and under IGNORE
K56_ZONE_SCORES = {HONOR: [(100, 100), (0, 100)], IGNORE: [(0, 100), (33, 100)]}


# ---- parity inputs -------------------------------------------------------------------------------
ZONES = np.array([0, 0, 5, 5, 63])
T1, T2 = np.uint64(1 << 2), np.uint64(1 << 40)  # the pool's two hard taints
L_SSD, L_A = 0, 70  # label bits: ssd (preferred terms), pool A (two nodes in three; the both-policies cases)


def _bit(b):
    return np.array([1 << b if b < 64 else 0, 1 << (b - 64) if b >= 64 else 0], np.uint64)


def cluster(n, p, both=False, norm=False, wide=False, seed=None):
    """Config-5 resources on `n` nodes, node i in zone (0, 0, 5, 5, 63)[i % 5].  The tainted pool: every node of
    zone 63 (a fifth of the table, T1 and T2 alternating, so the zone holds tainted nodes only) and every tenth
    node (zone 0, T1): 30 % of the nodes.  `p` pods of six apps: SPREAD(1), SPREAD_SOFT(2), SPREAD_HOSTNAME(1),
    SPREAD(3), SPREAD_SOFT(1), SPREAD_HOSTNAME(2), every fifth pod of an app NONE or HOSTNAME instead, with
    tol_hard 0 (one in two), T1 (one in four) or all ones (one in four).  `both`: pool A labelled, a third of
    the pods select it (for nodeAffinityPolicy Honor on top).  `norm`: soft taints, tolerations and preferred
    terms.  `wide`: odd-Ki node memory and decimal pod requests (the wide layout)."""
    nodes, pods = qsched.synth_generate(5, n, p, seed=seed)
    nodes = {k: v.copy() for k, v in nodes.items()}
    pods = pods.copy()
    rng = np.random.default_rng(2000 * n + p + (seed or 0))
    i = np.arange(n)
    nodes["zone"][:] = ZONES[i % 5]
    th = np.zeros(n, np.uint64)
    th[i % 5 == 4] = np.where((i[i % 5 == 4] // 5) % 2 == 0, T1, T2)
    th[i % 10 == 0] = T1
    nodes["taint_hard"][:] = th
    nodes["taint_soft"][:] = 0
    lab = np.zeros((n, 2), np.uint64)
    lab[i % 2 == 0] |= _bit(L_SSD)
    if both:
        lab[i % 3 != 0] |= _bit(L_A)
    nodes["label_bits"][:] = lab
    x = rng.integers(0, 6, p)
    pods["app"] = x * 123 + 7
    table = np.array([S.spread(1), R.spread_soft(2), H.spread_hostname(1), S.spread(3), R.spread_soft(1),
                      H.spread_hostname(2)])
    aa = table[x]
    seen = {}
    for j in range(p):
        k = seen.get(int(x[j]), 0)
        seen[int(x[j])] = k + 1
        if k % 5 == 4:
            aa[j] = A.NONE if (k // 5) % 2 == 0 else A.HOSTNAME
    pods["anti_affinity"] = aa
    for f in ("sel", "n_req_terms", "req_terms", "n_pref_terms", "pref_terms", "pref_weight", "tol_soft"):
        pods[f][:] = 0
    r = rng.integers(0, 4, p)
    pods["tol_hard"] = np.where(r < 2, np.uint64(0), np.where(r == 2, T1, ALL)).astype(np.uint64)
    if both:
        for j in np.flatnonzero(rng.integers(0, 3, p) == 0):
            pods["sel"][j] = _bit(L_A)
    if norm:
        nodes["taint_soft"][:] = np.where(i % 4 == 1, 2, 0).astype(np.uint64)
        pods["tol_soft"] = np.where(rng.integers(0, 3, p) == 0, 2, 0).astype(np.uint64)
        pref = rng.integers(0, 3, p)
        for j in np.flatnonzero(pref > 0):
            pods["n_pref_terms"][j] = pref[j]
            pods["pref_terms"][j, 0], pods["pref_weight"][j, 0] = _bit(L_SSD), 50
    if wide:
        nodes["alloc_mem"][:] = (rng.integers(64 << 20, 768 << 20, n) | 1) * C.KI
        dec = rng.choice([100 * 10**6, 512 * 10**6, 10**9, 3 * 10**9], p)
        has = pods["req_mem"] > 0
        pods["req_mem"] = np.where(has, dec, 0)
        pods["nz_mem"] = np.where(has, dec, O.DEF_MEM)
    return nodes, pods


# name: (nodes, pods, both policies, the plugins' scores at work, wide layout).  24 nodes: one partial wave of
# the count pass; 64 / 65: the last full wave and one node more; 300: two workgroups, the second partial.
PARITY = {
    "pool-24": (24, 300, False, False, False),
    "pool-64": (64, 400, False, False, False),
    "pool-65-wide": (65, 400, False, False, True),
    "pool-300-norm": (300, 600, False, True, False),
    "both-130-norm": (130, 500, True, True, False),
    "both-300-wide": (300, 600, True, False, True),
}


def spreads(pods):
    return (np.asarray(pods["anti_affinity"]) & 0xFF) == S.SPREAD


def restricting(pods, both=False):
    """bool[p]: spread pods of any of the three kinds that restrict by taints (some bit untolerated) or, with
    `both`, by a selector or required terms."""
    r = np.asarray(pods["tol_hard"]) != ALL
    if both:
        r = r | np.asarray(pods["sel"]).any(axis=1) | (np.asarray(pods["n_req_terms"]) > 0)
    return spreads(pods) & r


@functools.lru_cache(maxsize=None)
def parity_case(name):
    n, p, both, norm, wide = PARITY[name]
    nodes, pods = cluster(n, p, both, norm, wide)
    cfg = dict(NORM if (both or norm) else TAINT)
    policy = HONOR if both else IGNORE
    facts = []
    pl, keys, final, state = TR.run(nodes, pods, cfg, policy=policy, facts=facts)
    return dict(name=name, nodes=nodes, pods=pods, cfg=cfg, policy=policy, both=both, wide=wide, pl=pl, keys=keys,
                final=final, state=state, facts=facts)


def check_conditions(case):
    """Conditions of the inputs, from the reference alone, before any GPU run."""
    name, nodes, pods, cfg, pl, facts = (case[k] for k in ("name", "nodes", "pods", "cfg", "pl", "facts"))
    policy = case["policy"]
    n = len(nodes["zone"])
    tainted = float((nodes["taint_hard"] != 0).mean())
    kinds = {int(k) for k in np.unique(pods["anti_affinity"])}
    diff = {}
    for v in ("ignore", "domains_only", "counts_only", "affinity_only"):
        diff[v] = int((TR.run(nodes, pods, cfg, policy=policy, variant=v)[0] != pl).sum())
    ign = TR.run(nodes, pods, cfg, policy=policy, taints_policy=IGNORE)[0]
    rescued = int(((ign < 0) & (pl >= 0)).sum())
    no_node = sum(1 for f in facts if (f["zones_table"] & ~f["zones_m"]).any())
    outside = sum(1 for f in facts if f["outside"] > 0)
    checked = TR.skew_holds(nodes, pods, pl, policy, HONOR, cfg)
    tol = np.asarray(pods["tol_hard"])
    print(f"{name}: {tainted:.0%} of {n} nodes tainted, {len(facts)} pods decided over a smaller M, {no_node} with a "
          f"zone outside M, {outside} with app pods outside M, {rescued} unschedulable under Ignore and placed under "
          f"Honor, placed differently under {diff}, differently from policy Ignore {int((ign != pl).sum())}; skew "
          f"invariant over M at {checked} placements")
    assert 24 <= n <= 300 and len(pods) <= 600, name
    assert 0.20 <= tainted <= 0.40 and len(np.unique(nodes["taint_hard"])) == 3, name
    assert set(np.unique(nodes["zone"])) == {0, 5, 63} and (nodes["taint_hard"][nodes["zone"] == 63] != 0).all(), name
    assert (tol == 0).any() and (tol == T1).any() and (tol == ALL).any(), name
    skews = {(k >> 8) & 0x1F for k in kinds if (k & 0xFF) == S.SPREAD}
    assert skews == {1, 2, 3} and A.NONE in kinds and A.HOSTNAME in kinds, name
    assert any(R.is_soft(k) for k in kinds) and any(k & H.HOSTKEY for k in kinds), name
    assert no_node >= 1 and outside >= 1, name
    assert all(d >= 1 for d in diff.values()), (name, diff)
    assert (ign != pl).any() and rescued >= 1, name
    assert checked >= 20, name
    if case["both"]:  # M_A ∩ M_T strictly smaller than either factor, for some pod at its turn
        import honor_spread_ref as HR

        op = A.pods_dict(pods)
        small = 0
        for j in np.flatnonzero(restricting(pods, True)):
            if not HR.restricts(op, j):
                continue
            ma, mt = HR.matches(nodes["label_bits"], op, j), TR.tolerated(nodes["taint_hard"], op, j)
            small += int((ma & mt).sum() < min(ma.sum(), mt.sum()))
        assert small >= 20, name
