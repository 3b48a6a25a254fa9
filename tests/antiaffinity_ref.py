"""Reference for required pod anti-affinity on the exact stream and the score path
(spec/semantics.md S12; qs_set_pod_anti_affinity), CPU only.

The sequential loop over the committed oracle.  Per pod, in S8 order:

1. the aa-infeasible node mask from the recorded state (a HOSTNAME pod: nodes that hold a pod of its
   app; a ZONE pod: every node of a zone that holds one);
2. ``max_pods`` of those nodes set to 0 in a scratch copy of that column: Fit then rejects them, so
   ``or_score_pod`` leaves them out of the normalize maxima and scores no other node differently;
3. ``oracle.score_pod`` keys and their maximum (spec S7);
4. Reserve with numpy adds;
5. the pod recorded under its app, whatever its kind.

No scorer is restated here.  ``scorer(nodes, pods, j) -> keys[n]`` replaces step 3 for the other
scoring strategies: ``strategy_scorer(cfg)`` evaluates with tests/strategy_ref.py, ``qos_scorer(cfg)``
with the strategy of the pod's QoS class (tests/qos_strategy_ref.py), under the same masking.
"""
import numpy as np

from oracle import oracle as O

MAX_APPS, MAX_ZONES = 1024, 64
NONE, HOSTNAME, ZONE = 0, 1, 2


def pods_dict(pods):
    if isinstance(pods, np.ndarray) and pods.dtype.names:
        return {f: np.ascontiguousarray(pods[f]) for f in pods.dtype.names}
    return pods


class State:
    """Spec S11 / S12 state: pods per (app, node) (presence = count > 0) and per (app, zone)."""

    def __init__(self, zone):
        self.zone = np.asarray(zone).astype(np.int64)
        self.node = np.zeros((MAX_APPS, len(self.zone)), np.int32)
        self.zcount = np.zeros((MAX_APPS, MAX_ZONES), np.int32)

    def copy(self):
        s = State(self.zone)
        s.node, s.zcount = self.node.copy(), self.zcount.copy()
        return s

    def infeasible(self, app, kind):
        """bool[n]: the nodes a pod of `app` with anti-affinity `kind` may not take."""
        if kind == HOSTNAME:
            return self.node[app] > 0
        if kind == ZONE:
            return self.zcount[app][self.zone] > 0
        return np.zeros(len(self.zone), bool)

    def record(self, app, node, sign=+1):
        """One pod of `app` more or fewer on `node`; False (and no change) if none is there to remove."""
        if sign < 0 and self.node[app, node] == 0:
            return False
        self.node[app, node] += sign
        self.zcount[app, self.zone[node]] += sign
        return True

    def presence(self):
        return self.node > 0


def oracle_scorer(cfg=None):
    return lambda nodes, pods, j: O.score_pod(nodes, pods, j, cfg)[0]


def _keys(ok, total):
    n = len(ok)
    idx = np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64)
    k = ((np.where(ok, total, 0).astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | idx
    return np.where(ok, k, np.uint64(0))


def strategy_scorer(cfg=None):
    import strategy_ref as R
    c = R._cfg(cfg)
    return lambda nodes, pods, j: _keys(*[R.evaluate(c, nodes, pods, j)[i] for i in (0, 2)])


def qos_scorer(cfg=None):
    import qos_strategy_ref as Q
    import strategy_ref as R
    cs = Q.class_cfgs(cfg)
    return lambda nodes, pods, j: _keys(*[R.evaluate(cs[int(pods["qos"][j])], nodes, pods, j)[i] for i in (0, 2)])


def order_of(pods, cfg=None):
    c = dict(O.DEFAULT_CONFIG)
    c.update(cfg or {})
    return O.py_order(pods, c)


def masked(nodes, state, app, kind):
    """`nodes` with max_pods 0 on the aa-infeasible nodes (a scratch copy of that one column)."""
    bad = state.infeasible(app, kind)
    if not bad.any():
        return nodes
    m = dict(nodes)
    m["max_pods"] = np.where(bad, 0, nodes["max_pods"]).astype(nodes["max_pods"].dtype)
    return m


def pod_keys(nodes, pods, j, state, cfg=None, scorer=None):
    """Keys of pod j on every node under the recorded state (0 = infeasible); no state change."""
    pods = pods_dict(pods)
    scorer = scorer or oracle_scorer(cfg)
    return scorer(masked(nodes, state, int(pods["app"][j]), int(pods["anti_affinity"][j])), pods, j)


def reserve(nodes, pods, j, n, sign=+1):
    for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem"):
        nodes[f][n] += sign * int(pods[f][j])
    nodes["req_ext"][n] += sign * pods["req_ext"][j]
    nodes["pods"][n] += sign


def schedule(nodes, pods, cfg=None, scorer=None, state=None):
    """The S12 stream.  Mutates `nodes` (Reserve) and `state` (a fresh one when None).
    Returns (placement[p] int32, key[p] uint64, state)."""
    pods = pods_dict(pods)
    scorer = scorer or oracle_scorer(cfg)
    state = State(nodes["zone"]) if state is None else state
    p = len(pods["qos"])
    placement = np.full(p, -1, np.int32)
    keys = np.zeros(p, np.uint64)
    for j in order_of(pods, cfg):
        app, kind = int(pods["app"][j]), int(pods["anti_affinity"][j])
        k = scorer(masked(nodes, state, app, kind), pods, j)
        best = int(k.max()) if len(k) else 0
        if best == 0:
            continue
        n = 0xFFFFFFFF - (best & 0xFFFFFFFF)
        placement[j], keys[j] = n, best
        reserve(nodes, pods, j, n)
        state.record(app, n)
    return placement, keys, state


def run(nodes, pods, cfg=None, scorer=None, state=None):
    """schedule() on a copy of the table (and of `state`): (placement, keys, final nodes, state)."""
    on = {k: v.copy() for k, v in nodes.items()}
    st = None if state is None else state.copy()
    pl, keys, st = schedule(on, pods, cfg, scorer, st)
    return pl, keys, on, st


def fold(nodes, pods, apps, zones, seed_mul=25, seed_add=24):
    """The folded config-5 inputs of the tests: `apps` app groups whose ids spread over the presence
    words ((app % apps) * 25 + 24, so the largest is 24 + 25 (apps - 1): beyond 992 for 40 apps),
    `anti_affinity` kept per app (config 5 draws the kind per app), zones folded to `zones`."""
    pods = pods.copy() if isinstance(pods, np.ndarray) else {k: v.copy() for k, v in pods.items()}
    nodes = {k: v.copy() for k, v in nodes.items()}
    a = pods["app"].astype(np.int64) % apps
    kind = np.zeros(apps, np.int64)
    first = {}
    for j, x in enumerate(a):
        first.setdefault(int(x), j)
    for x, j in first.items():
        kind[x] = int(pods["anti_affinity"][j])
    pods["anti_affinity"][:] = kind[a]
    pods["app"][:] = a * seed_mul + seed_add
    assert int(pods["app"].max()) < MAX_APPS
    nodes["zone"][:] = nodes["zone"] % zones
    return nodes, pods
