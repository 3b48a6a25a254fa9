"""Inputs shared by tests/test_preempt_cpu.py and tests/test_gpu_preempt.py (spec S18): the known answers
K59-K67 of spec/kat.md as small clusters with hand-computed results, and the parity cases.  CPU only.

A case is a table, a list of (node, pod) reservations that fill the registry, a policy and preemptor
pods.  `check_conditions(case)` states, from the reference alone, what the case is there to show: which
edge it contains and that its answers differ from each wrong variant of tests/preempt_ref.py that
applies to it (in the chosen node, the victim set or the victims per node).
"""
import functools

import numpy as np

import qsched
from qsched import POD_DTYPE

import preempt_ref as R

GI = 1 << 30
MI = 1 << 20
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def mk_pod(cpu, mem, prio, qos, app=0, ext=(0, 0), tol_hard=ALL, sel=(0, 0)):
    p = np.zeros(1, POD_DTYPE)[0]
    p["req_cpu"], p["req_mem"] = cpu, mem
    p["req_ext"] = ext
    p["nz_cpu"], p["nz_mem"] = cpu or 100, mem or 200 * MI
    p["priority"], p["qos"], p["app"] = prio, qos, app
    p["tol_hard"], p["tol_soft"] = tol_hard, ALL
    p["sel"] = sel
    return p


def mk_nodes(cpus, mem=64 * GI, max_pods=110):
    n = len(cpus)
    d = qsched.empty_nodes(n)
    d["alloc_cpu"][:] = cpus
    d["alloc_mem"][:] = mem
    d["max_pods"][:] = max_pods
    return d


# ---- known answers (spec/kat.md K59-K67) ---------------------------------------------------------
def kat(name):
    """dict(nodes, fill=[(node, pod)], policy, pod, node, victims=[seq], nvict_n): computed by hand."""
    P = mk_pod
    if name == "K59":  # the reprieve walk: C (priority 5) and B come back, A is the victim
        fill = [(0, P(2000, GI, 0, 1)), (0, P(1000, GI, 0, 1)), (0, P(1000, GI, 5, 1))]
        return dict(nodes=mk_nodes([4000]), fill=fill, policy=0, pod=P(2000, GI, 10, 2), node=0, victims=[1],
                    nvict_n=[1])
    if name == "K60":  # criterion 2 before 4: two victims of priority 3 beat one of priority 5
        fill = [(0, P(2000, GI, 5, 1)), (1, P(1000, GI, 3, 1)), (1, P(1000, GI, 3, 1))]
        return dict(nodes=mk_nodes([2000, 2000]), fill=fill, policy=0, pod=P(2000, GI, 10, 2), node=1,
                    victims=[2, 3], nvict_n=[1, 2])
    if name == "K61":  # criterion 3: equal top victims, the smaller sum (every victim adds priority + 2^31)
        fill = [(0, P(1000, GI, 5, 1)), (0, P(1000, GI, 4, 1)),
                (1, P(1000, GI, 5, 1)), (1, P(500, GI, 1, 1)), (1, P(500, GI, 1, 1))]
        return dict(nodes=mk_nodes([2000, 2000]), fill=fill, policy=0, pod=P(2000, GI, 10, 2), node=0,
                    victims=[1, 2], nvict_n=[2, 3])
    if name == "K62":  # criterion 5: all equal, the node whose top victim started last (seq 2)
        fill = [(0, P(2000, GI, 5, 1)), (1, P(2000, GI, 5, 1))]
        return dict(nodes=mk_nodes([2000, 2000]), fill=fill, policy=0, pod=P(2000, GI, 10, 2), node=1,
                    victims=[2], nvict_n=[1, 1])
    if name == "K63":  # node 1 holds a lower pod and room: a candidate without victims wins at once;
        # node 2 has room and no lower pod: no candidate
        fill = [(0, P(2000, GI, 1, 1)), (1, P(1000, GI, 1, 1)), (2, P(1000, GI, 50, 1))]
        return dict(nodes=mk_nodes([2000, 4000, 4000]), fill=fill, policy=0, pod=P(2000, GI, 10, 2), node=1,
                    victims=[], nvict_n=[1, 0, -1])
    if name in ("K64a", "K64b"):  # one table, two policies: priority alone against class first
        fill = [(0, P(2000, GI, 100, 0)), (1, P(2000, GI, -5, 2))]
        by_qos = name == "K64b"
        return dict(nodes=mk_nodes([2000, 2000]), fill=fill, policy=1 if by_qos else 0, pod=P(2000, GI, 0, 1),
                    node=0 if by_qos else 1, victims=[1] if by_qos else [2],
                    nvict_n=[1, -1] if by_qos else [-1, 1])
    if name == "K65":  # the only node with victims to give is tainted: unresolvable, no candidate
        nodes = mk_nodes([2000])
        nodes["taint_hard"][0] = 4
        return dict(nodes=nodes, fill=[(0, P(2000, GI, 1, 1))], policy=0, pod=P(2000, GI, 10, 2, tol_hard=3),
                    node=-1, victims=[], nvict_n=[-1])
    if name == "K66":  # priorities at the ends of int32; equal importance walks by seq: seq 2 is reprieved
        # first and stays, seq 3 does not fit beside it
        fill = [(0, P(1000, GI, I32_MAX, 1)), (0, P(1000, GI, I32_MIN, 1)), (0, P(1000, GI, I32_MIN, 1))]
        return dict(nodes=mk_nodes([3000]), fill=fill, policy=0, pod=P(1000, GI, I32_MIN + 1, 2), node=0,
                    victims=[3], nvict_n=[1])
    raise KeyError(name)


KATS = ("K59", "K60", "K61", "K62", "K63", "K64a", "K64b", "K65", "K66")


ON = dict(enable_taint=1, enable_affinity=1)


def new_ref(c):
    """A reference for the case's (or known answer's) table, flags and policy."""
    cfg = c.get("cfg", ON)
    return R.Ref(c["nodes"], bool(cfg.get("enable_taint", 0)), bool(cfg.get("enable_affinity", 0)), c["policy"])


def kat_ref(k):
    ref = new_ref(k)
    for node, pod in k["fill"]:
        ref.reserve(node, pod)
    return ref


# ---- parity cases --------------------------------------------------------------------------------
PRIOS = np.array([I32_MIN, -7, 0, 0, 3, 3, 10, 1000, I32_MAX], np.int64)


def _cluster(n, seed, wide=False, ext=False, masks=False, preload=False, long_node=None, long_len=0,
             max_pods=(4, 10), kshift=0):
    """A table of n nodes and the reservations that fill most of it.  Node kinds cycle so that every
    table holds nodes short in cpu, in memory, in the pod count alone and (ext) in an extended resource
    alone, empty lists, lists of 1, 8 and 9, and (long_node) one list of long_len entries."""
    rng = np.random.default_rng(seed)
    nodes = mk_nodes(rng.choice([4000, 8000, 16000], n), max_pods=110)
    unit = MI * 64
    nodes["alloc_mem"][:] = rng.choice([16, 32, 64], n) * GI + (1001 if wide else 0)
    nodes["max_pods"][:] = rng.integers(max_pods[0], max_pods[1] + 1, n)
    if ext:
        nodes["alloc_ext"][:, 0] = rng.choice([0, 4, 8], n)
        nodes["alloc_ext"][:, 1] = rng.choice([0, 2], n)
    if masks:
        nodes["taint_hard"][:] = np.where(rng.random(n) < 0.2, 4, 0).astype(np.uint64)
        nodes["label_bits"][:, 0] = np.where(rng.random(n) < 0.7, 3, 1).astype(np.uint64)
    if preload:  # load that belongs to no entry
        nodes["req_cpu"][:] = rng.choice([0, 500, 1000], n)
        nodes["nz_cpu"][:] = nodes["req_cpu"]
        nodes["req_mem"][:] = rng.choice([0, 1, 2], n) * GI
        nodes["nz_mem"][:] = nodes["req_mem"]
        nodes["pods"][:] = (nodes["req_cpu"] > 0).astype(np.int64)
    fill = []
    free_c = nodes["alloc_cpu"] - nodes["req_cpu"]
    free_m = nodes["alloc_mem"] - nodes["req_mem"]
    free_e = nodes["alloc_ext"].copy()
    trap = (4, 12) if n >= 16 else ()
    for i in trap:  # the two nodes of the label-256 preemptor (see _preemptors): kept out of the random fill
        nodes["alloc_cpu"][i], nodes["max_pods"][i] = 4000, 110
        for f in ("req_cpu", "nz_cpu", "req_mem", "nz_mem", "pods", "taint_hard"):
            nodes[f][i] = 0
        nodes["label_bits"][i, 0] |= np.uint64(256)
    if trap:  # node 4 gives up two pods of priority 3, node 12 one of priority 10: criterion 2 before 4
        fill += [(4, mk_pod(1900, GI, 3, 1)), (4, mk_pod(1900, GI, 3, 1)), (12, mk_pod(3800, GI, 10, 1))]
    for i in range(n):
        if i in trap:
            continue
        kind = (i + kshift) % 8
        cap = int(nodes["max_pods"][i] - nodes["pods"][i])
        if i == long_node:
            nodes["max_pods"][i] = cap = long_len
            nodes["alloc_cpu"][i] = 100 * long_len + 50
            free_c[i] = nodes["alloc_cpu"][i] - nodes["req_cpu"][i]
            want = long_len - int(nodes["pods"][i])
        else:
            want = {0: 0, 1: 1, 2: 8, 3: 9}.get(kind, int(rng.integers(2, 10)))
            if kind in (2, 3):
                nodes["max_pods"][i] = max(int(nodes["max_pods"][i]), want + int(nodes["pods"][i]) + (kind == 2))
                cap = int(nodes["max_pods"][i] - nodes["pods"][i])
        cnt = min(want, cap)
        if cnt == 0:
            continue
        # the node ends up nearly full in what its kind is short of: cpu (most kinds), the pod count alone
        # (kind 5 and the long list: tiny pods, max_pods = the count), memory (kind 6), ext 0 (kind 7, ext)
        tiny = i == long_node or kind == 5
        if tiny:
            nodes["max_pods"][i] = int(nodes["pods"][i]) + cnt
        w = rng.random(cnt) + 0.3
        w /= w.sum()
        for k in range(cnt):
            e = (0, 0)
            if tiny:
                cpu, mem = 100, unit
            elif ext and kind == 7 and nodes["alloc_ext"][i, 0] > 0:
                cpu = max(100, int((nodes["alloc_cpu"][i] - nodes["req_cpu"][i]) * 0.97 * w[k]) // 100 * 100)
                mem = unit
                e = (int(free_e[i, 0]) if k == cnt - 1 else int(min(free_e[i, 0], 1)), 0)
            elif kind == 6:
                cpu = 100
                mem = max(unit, int((nodes["alloc_mem"][i] - nodes["req_mem"][i]) * 0.97 * w[k]) // unit * unit)
            else:
                cpu = max(100, int((nodes["alloc_cpu"][i] - nodes["req_cpu"][i]) * 0.97 * w[k]) // 100 * 100)
                mem = int(rng.integers(1, 16)) * unit
            if cpu > free_c[i] or mem > free_m[i]:
                continue
            free_c[i] -= cpu
            free_m[i] -= mem
            free_e[i, 0] -= e[0]
            qos = int(rng.integers(0, 3))
            fill.append((i, mk_pod(cpu, mem, int(rng.choice(PRIOS)), qos, app=int(rng.integers(0, 50)), ext=e)))
    order = rng.permutation(len(fill))  # sequence numbers interleave across nodes
    return nodes, [fill[k] for k in order]


def _preemptors(ext=False, masks=False):
    tol = np.uint64(3) if masks else ALL
    sel = (2, 0) if masks else (0, 0)
    pods = [mk_pod(7000, 8 * GI, 2000, 2, tol_hard=tol, sel=sel),      # above all but INT32_MAX, several victims
            mk_pod(3000, 8 * GI, 11, 2, tol_hard=tol),
            mk_pod(2500, GI, -6, 1, tol_hard=tol),                     # only -7 and INT32_MIN lie below
            mk_pod(1500, 40 * GI, 5, 1, tol_hard=tol),                 # mid priority, memory-heavy
            mk_pod(100, 64 * MI, I32_MAX, 2, tol_hard=tol),            # tiny: pod-count shortages
            mk_pod(6000, 2 * GI, 1, 0, tol_hard=tol, sel=sel),         # BestEffort: the policies part here
            mk_pod(100, 64 * MI, I32_MIN, 0)]                          # nothing is less important
    pods.append(mk_pod(3000, GI, 2000, 1, tol_hard=tol, sel=(256, 0)))  # the two labelled nodes alone
    if ext:
        pods.append(mk_pod(100, 64 * MI, 2000, 2, ext=(3, 0), tol_hard=tol))  # short in ext 0 alone
    return pods


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(nodes, fill, policy, pods, cfg, differs): differs = the wrong variants the case must tell apart."""
    base = ("no_reprieve", "reprieve_low_first", "count_first")
    spec = {
        # n at the wave and workgroup edges; 257 and 1000: more than one workgroup record
        "n1": dict(n=1, seed=11, kshift=4, differs=("no_reprieve",)),  # (one node: nothing to choose)
        "n63": dict(n=63, seed=2), "n64": dict(n=64, seed=3), "n65": dict(n=65, seed=4, long_node=5, long_len=110),
        "n257": dict(n=257, seed=5, preload=True), "n1000": dict(n=1000, seed=6),
        "wide": dict(n=130, seed=7, wide=True, ext=True), "ext": dict(n=96, seed=8, ext=True),
        "masks": dict(n=200, seed=9, masks=True),
        # the same table on a context with both filters off: tainted and unlabelled nodes are candidates
        # (with the selector unread the labelled pair is not alone, so count_first has nothing to get wrong here)
        "masks_off": dict(n=200, seed=9, masks=True, cfg=dict(enable_taint=0, enable_affinity=0),
                          differs=("no_reprieve", "reprieve_low_first")),
        "qos": dict(n=150, seed=10, policy=1, differs=base + ("priority_only",)),
        "wide_qos": dict(n=70, seed=12, wide=True, policy=1, masks=True, differs=base + ("priority_only",)),
    }[name]
    kw = {k: v for k, v in spec.items() if k not in ("n", "seed", "policy", "differs", "cfg")}
    nodes, fill = _cluster(spec["n"], spec["seed"], **kw)
    return dict(name=name, nodes=nodes, fill=fill, policy=spec.get("policy", 0),
                pods=_preemptors(kw.get("ext", False), kw.get("masks", False)), cfg=dict(spec.get("cfg", ON)),
                differs=spec.get("differs", base), long_node=kw.get("long_node"))


CASES = ("n1", "n63", "n64", "n65", "n257", "n1000", "wide", "ext", "masks", "masks_off", "qos", "wide_qos")


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(reference after the fill, [(node, victims, nvict_n) per preemptor]): computed once, never changed."""
    c = case(name)
    ref = new_ref(c)
    for node, pod in c["fill"]:
        ref.reserve(node, pod)
    return ref, [ref.preempt(p) for p in c["pods"]]


def answers_differ(a, b):
    return a[0] != b[0] or sorted(e["seq"] for e in a[1]) != sorted(e["seq"] for e in b[1]) or \
        not np.array_equal(a[2], b[2])


def check_conditions(name):
    """What the case is for, from the reference alone."""
    c = case(name)
    ref, ans = case_ref(name)
    n = ref.n
    lens = {len(l) for l in ref.reg}
    if n >= 63:
        assert {0, 1, 8, 9} <= lens, (name, sorted(lens))
        assert any(a[0] >= 0 and len(a[1]) > 0 for a in ans), name
        assert any(a[0] == -1 for a in ans), name                       # INT32_MIN preemptor: no candidate
        assert any((a[2] == -1).any() and (a[2] > 0).any() for a in ans), name
        prios = {e["priority"] for l in ref.reg for e in l}
        assert {I32_MIN, I32_MAX, -7} <= prios, name
        # equal-importance entries on one node (seq decides the walk)
        assert any(len({ref.imp(e) for e in l}) < len(l) for l in ref.reg if len(l) > 1), name
    if c["long_node"] is not None:
        assert len(ref.reg[c["long_node"]]) == 110, name
        assert any(a[2][c["long_node"]] > 0 for a in ans), name
    for v in c["differs"]:
        wrong = [ref.preempt(p, v) for p in c["pods"]]
        assert any(answers_differ(a, w) for a, w in zip(ans, wrong)), (name, v)
    if name in ("wide", "wide_qos"):  # memory that no power-of-two unit below 2^24 units holds
        assert int(c["nodes"]["alloc_mem"][0]) % 8 != 0
    if name == "n257":                # load that belongs to no entry
        assert (c["nodes"]["req_cpu"] > 0).any()
    if name in ("ext", "wide"):       # a node short only in the extended resource for the ext preemptor
        t = ref.t
        p = c["pods"][-1]
        short = [i for i in range(n) if t["alloc_ext"][i, 0] - t["req_ext"][i, 0] < p["req_ext"][0] <= t["alloc_ext"][i, 0]
                 and t["pods"][i] < t["max_pods"][i] and t["alloc_cpu"][i] - t["req_cpu"][i] >= p["req_cpu"]
                 and t["alloc_mem"][i] - t["req_mem"][i] >= p["req_mem"]]
        assert short and any(ans[-1][2][i] > 0 for i in short), name
    if n >= 63:                       # a node whose only shortage is the pod count, for the tiny preemptor
        t = ref.t
        full = [i for i in range(n) if t["pods"][i] >= t["max_pods"][i] and t["alloc_cpu"][i] - t["req_cpu"][i] >= 100
                and t["alloc_mem"][i] - t["req_mem"][i] >= 64 * MI]
        assert full and any(ans[4][2][i] == 1 for i in full), name
    if name in ("masks", "masks_off", "wide_qos"):  # nodes excluded by taint and by selector, when the filters are on
        t = ref.t
        tainted = np.flatnonzero(t["taint_hard"] != 0)
        assert len(tainted) and (t["label_bits"][:, 0] == 1).any()
        hit = any((a[2][tainted] >= 0).any() for a in ans)
        assert hit == (name == "masks_off"), name
