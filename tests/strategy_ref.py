"""Reference for the NodeResourcesFit scoring strategies (spec/semantics.md S5 "Scoring strategies").

A sequential scheduler (spec S7 keys and Reserve, S8 order) vectorised over the nodes in numpy
int64 / float64, with the three fit scorers — LeastAllocated, MostAllocated,
RequestedToCapacityRatio — written from the spec's pseudocode, BalancedAllocation and the filters
from S4 / S5 (numpy float64 is IEEE binary64, so Balanced is bit-identical to Go's float64), and
the normalizing plugins of S5.  Python's ``//`` floors where Go's integer division truncates, so
``raw`` truncates explicitly.

Also the scalar scorers ``py_most_allocated`` / ``py_rtcr`` with the signature of
``oracle.py_least_allocated``, so that the pure-Python oracle (``py_keys`` looks the scorer up at
call time) can be run with another strategy.

Configuration: the oracle's dict (``fit_resources``, ``balanced_resources``, ``enable_taint``, ...)
plus ``scoring_strategy`` ("LeastAllocated" | "MostAllocated" | "RequestedToCapacityRatio") and
``shape`` ([(utilization, score), ...]).
"""
import numpy as np

DEFAULTS = dict(wc=1, wm=1, w_fit=(1, 2, 3), w_bal=(1, 1, 1), w_tt=3, w_na=2, enable_taint=0, enable_affinity=0,
                balanced_skip_besteffort=0, qos_sort=1, fit_resources=None, balanced_resources=None,
                scoring_strategy="LeastAllocated", shape=None)
RES_IDS = {"cpu": 1, "memory": 2, "ext0": 3, "ext1": 4}
BIN_PACK = [(0, 0), (100, 10)]
U64 = np.uint64


def trunc_div(a, b):
    """Go's integer division: toward zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def raw(shape, p):
    """UP helper/shape_score.go#BuildBrokenLinearFunction over the scores scaled by 10."""
    U = [u for u, _ in shape]
    S = [s * 10 for _, s in shape]
    for i in range(len(shape)):
        if p <= U[i]:
            if i == 0:
                return S[0]
            return S[i - 1] + trunc_div((S[i] - S[i - 1]) * (p - U[i - 1]), U[i] - U[i - 1])
    return S[-1]


def shape_table(shape):
    return np.array([raw(shape, p) for p in range(101)], np.int64)


def round_half_away(num, den):
    """Go's math.Round(float64(num) / float64(den)) for num >= 0, den > 0."""
    return int(np.floor(np.float64(num) / np.float64(den) + 0.5))


# ---- scalar scorers (signature of oracle.py_least_allocated) ------------------------------------
def py_most_allocated(alloc, reqd, weights=(1, 1)):
    num = den = 0
    for a, r, w in zip(alloc, reqd, weights):
        if a == 0:
            continue
        num += ((min(r, a) * 100) // a) * w
        den += w
    return 0 if den == 0 else num // den


def py_rtcr(shape):
    def score(alloc, reqd, weights=(1, 1)):
        num = den = 0
        for a, r, w in zip(alloc, reqd, weights):
            if a == 0:
                continue
            s = raw(shape, 100) if r > a else raw(shape, (r * 100) // a)
            if s > 0:
                num += s * w
                den += w
        return 0 if den == 0 else round_half_away(num, den)
    return score


def py_scorer(cfg):
    """The scalar fit scorer of a configuration, or None for LeastAllocated."""
    st = (cfg or {}).get("scoring_strategy", "LeastAllocated")
    if st == "MostAllocated":
        return py_most_allocated
    if st == "RequestedToCapacityRatio":
        return py_rtcr(cfg["shape"])
    return None


# ---- vectorised evaluation of one pod on every node ---------------------------------------------
def _cfg(cfg):
    c = dict(DEFAULTS)
    c.update(cfg or {})
    return c


def _pods_dict(pods):
    if isinstance(pods, np.ndarray):
        return {f: np.ascontiguousarray(pods[f]) for f in pods.dtype.names}
    return pods


def _entry(nodes, pods, j, rid, use_requested):
    """(alloc[n], reqd[n]) of one scoring resource (UP resource_allocation.go#
    calculateResourceAllocatableRequest)."""
    if rid == 1:
        k = "req_cpu" if use_requested else "nz_cpu"
        return nodes["alloc_cpu"], nodes[k] + int(pods[k][j])
    if rid == 2:
        k = "req_mem" if use_requested else "nz_mem"
        return nodes["alloc_mem"], nodes[k] + int(pods[k][j])
    e = rid - 3
    q = int(pods["req_ext"][j][e])
    if q == 0:
        z = np.zeros(len(nodes["alloc_cpu"]), np.int64)
        return z, z
    return nodes["alloc_ext"][:, e], nodes["req_ext"][:, e] + q


def fit_score(c, entries, weights, over=None):
    """The configured strategy over the list entries [(alloc[n], reqd[n])]; `over` (optional, bool
    [n]) is or-ed with the nodes on which a counted entry has reqd > alloc."""
    n = len(entries[0][0])
    num = np.zeros(n, np.int64)
    den = np.zeros(n, np.int64)
    st = c["scoring_strategy"]
    tab = shape_table(c["shape"]) if st == "RequestedToCapacityRatio" else None
    for (a, r), w in zip(entries, weights):
        has = a != 0
        a1 = np.where(has, a, 1)
        if over is not None:
            over |= has & (r > a)
        if st == "LeastAllocated":
            s = np.where(r > a, 0, ((a - r) * 100) // a1)
            inc = has
        elif st == "MostAllocated":
            s = (np.minimum(r, a) * 100) // a1
            inc = has
        else:
            p = np.where(r > a, 100, (np.minimum(r, a) * 100) // a1)
            s = tab[p]
            inc = has & (s > 0)
        num += np.where(inc, s * w, 0)
        den += np.where(inc, w, 0)
    d1 = np.where(den == 0, 1, den)
    if st == "RequestedToCapacityRatio":
        out = np.floor(num.astype(np.float64) / d1.astype(np.float64) + 0.5).astype(np.int64)
    else:
        out = num // d1
    return np.where(den == 0, 0, out)


def balanced_score(entries):
    """UP balanced_allocation.go#balancedResourceScorer, float64 in the list's order."""
    n = len(entries[0][0])
    cnt = np.zeros(n, np.int64)
    tot = np.zeros(n, np.float64)
    fa = np.zeros(n, np.float64)
    fb = np.zeros(n, np.float64)
    fs, incs = [], []
    for a, r in entries:
        inc = a != 0
        f = r.astype(np.float64) / np.where(inc, a, 1).astype(np.float64)
        f = np.where(f > 1, 1.0, f)
        fa = np.where(inc & (cnt == 0), f, fa)
        fb = np.where(inc & (cnt == 1), f, fb)
        tot = tot + np.where(inc, f, 0.0)
        cnt = cnt + inc
        fs.append(f)
        incs.append(inc)
    std = np.where(cnt == 2, np.abs((fa - fb) / 2), 0.0)
    c1 = np.where(cnt == 0, 1, cnt).astype(np.float64)
    mean = tot / c1
    s = np.zeros(n, np.float64)
    for f, inc in zip(fs, incs):
        d = f - mean
        s = s + np.where(inc, d * d, 0.0)
    std = np.where(cnt > 2, np.sqrt(s / c1), std)
    return ((1 - std) * 100.0).astype(np.int64)


def _subset(m0, m1, lb):
    return ((U64(m0) & ~lb[:, 0]) | (U64(m1) & ~lb[:, 1])) == 0


def feasible(c, nodes, pods, j):
    ok = nodes["pods"] + 1 <= nodes["max_pods"]
    rc, rm = int(pods["req_cpu"][j]), int(pods["req_mem"][j])
    if rc > 0:
        ok &= rc <= nodes["alloc_cpu"] - nodes["req_cpu"]
    if rm > 0:
        ok &= rm <= nodes["alloc_mem"] - nodes["req_mem"]
    for e in range(2):
        q = int(pods["req_ext"][j][e])
        if q != 0:
            ok &= q <= nodes["alloc_ext"][:, e] - nodes["req_ext"][:, e]
    if c["enable_taint"]:
        ok &= (nodes["taint_hard"] & ~U64(pods["tol_hard"][j])) == 0
    if c["enable_affinity"]:
        lb = nodes["label_bits"]
        ok &= _subset(pods["sel"][j][0], pods["sel"][j][1], lb)
        nt = int(pods["n_req_terms"][j])
        if nt:
            any_ = np.zeros(len(ok), bool)
            for t in range(nt):
                any_ |= _subset(pods["req_terms"][j][t][0], pods["req_terms"][j][t][1], lb)
            ok &= any_
    return ok


def _popcount(x):
    bits = np.unpackbits(np.ascontiguousarray(x, dtype=np.uint64).view(np.uint8).reshape(-1, 8), axis=1)
    return bits.sum(axis=1).astype(np.int64)


def evaluate(c, nodes, pods, j, over=None):
    """(feasible[n], scores[n, 4], total[n]) of pod j; scores / total are 0 / -1 where infeasible."""
    n = len(nodes["alloc_cpu"])
    ok = feasible(c, nodes, pods, j)
    q = int(pods["qos"][j])
    fit = c["fit_resources"] or [("cpu", c["wc"]), ("memory", c["wm"])]
    la = fit_score(c, [_entry(nodes, pods, j, RES_IDS.get(r, r), False) for r, _ in fit], [w for _, w in fit], over)
    bal = c["balanced_resources"] or ["cpu", "memory"]
    ba = balanced_score([_entry(nodes, pods, j, RES_IDS.get(r, r), True) for r in bal])
    if c["balanced_skip_besteffort"] and q == 0:
        ba = np.zeros(n, np.int64)
    sc = np.zeros((n, 4), np.int64)
    sc[:, 0], sc[:, 1] = la, ba
    total = c["w_fit"][q] * la + c["w_bal"][q] * ba
    if c["enable_taint"]:
        rt = _popcount(nodes["taint_soft"] & ~U64(pods["tol_soft"][j]))
        mt = int(rt[ok].max()) if ok.any() else 0
        sc[:, 2] = 100 if mt == 0 else 100 - (100 * rt) // mt
        total = total + c["w_tt"] * sc[:, 2]
    if c["enable_affinity"]:
        ra = np.zeros(n, np.int64)
        for t in range(int(pods["n_pref_terms"][j])):
            hit = _subset(pods["pref_terms"][j][t][0], pods["pref_terms"][j][t][1], nodes["label_bits"])
            ra += np.where(hit, int(pods["pref_weight"][j][t]), 0)
        ma = int(ra[ok].max()) if ok.any() else 0
        sc[:, 3] = ra if ma == 0 else (100 * ra) // ma
        total = total + c["w_na"] * sc[:, 3]
    sc[~ok] = 0
    return ok, sc, np.where(ok, total, -1)


def reserve(nodes, pods, j, n):
    for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem"):
        nodes[f][n] += int(pods[f][j])
    nodes["req_ext"][n] += pods["req_ext"][j]
    nodes["pods"][n] += 1


def score_pod(nodes, pods, j, cfg=None):
    """(feasible, scores[n, 4], total, best) of pod j against `nodes` (no state change)."""
    c, pods = _cfg(cfg), _pods_dict(pods)
    ok, sc, total = evaluate(c, nodes, pods, j)
    best = -1
    if ok.any():
        best = int(np.flatnonzero(total == total.max())[0])  # highest total, lowest index (spec S7)
    return ok, sc, total, best


def schedule(nodes, pods, cfg=None):
    """The exact stream.  Mutates `nodes` (Reserve).  Returns (placement[p] int32, key[p] uint64,
    info) with info["overcommitted"] = the pods whose winning node held a counted fit entry with
    reqd > alloc (MostAllocated's clip / RequestedToCapacityRatio's raw(100))."""
    c, pods = _cfg(cfg), _pods_dict(pods)
    p = len(pods["qos"])
    order = list(range(p))
    if c["qos_sort"]:
        order.sort(key=lambda j: (-int(pods["qos"][j]), -int(pods["priority"][j]), j))
    placement = np.full(p, -1, np.int32)
    keys = np.zeros(p, np.uint64)
    n = len(nodes["alloc_cpu"])
    overc = 0
    for j in order:
        over = np.zeros(n, bool)
        ok, _, total = evaluate(c, nodes, pods, j, over)
        if not ok.any():
            continue
        b = int(np.flatnonzero(total == total.max())[0])
        placement[j] = b
        keys[j] = ((int(total[b]) + 1) << 32) | (0xFFFFFFFF - b)
        overc += int(over[b])
        reserve(nodes, pods, j, b)
    return placement, keys, dict(overcommitted=overc)


def run(nodes, pods, cfg=None):
    """schedule() on a copy of the table: (placement, keys, final nodes, info)."""
    on = {k: v.copy() for k, v in nodes.items()}
    pl, keys, info = schedule(on, pods, cfg)
    return pl, keys, on, info
