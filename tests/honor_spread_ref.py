"""Reference for ``nodeAffinityPolicy: Honor`` of the topology spread constraints on the exact stream and
the score path (spec/semantics.md S16; qs_set_topology_spread_node_affinity_policy), CPU only.

One state class for the three spread kinds: the state of tests/soft_spread_ref.py (S13 + S14) with the
S15 filter of tests/hostspread_ref.py, given the table's ``label_bits`` and, before each pod, that pod's
``sel`` / ``req_terms``.  No scorer is restated: the stream masks ``max_pods`` and asks the oracle, as
tests/antiaffinity_ref.py does, and the S14 term is soft_spread_ref's.

``M(pod)`` = the nodes that pass the pod's nodeSelector and required node-affinity terms (the NodeAffinity
filter's predicate).  A pod *restricts* when it has a selector bit or a required term.  Under ``honor``,
for a restricting pod: the zone counts are ``cH[z]`` = the app's recorded pods on the nodes of ``M`` in
zone ``z``; the domains are the zones of ``M``; a hostname-spread pod's minimum runs over ``M``.  A pod
that does not restrict, and every pod under ``ignore``, follows S13 / S14 / S15 to the letter.

Three deliberately wrong variants serve the conditions on the test inputs:

* ``ignore``: today's rule whatever the policy;
* ``domains_only``: Honor's domains (and the hostname minimum over ``M``), the counts over all nodes;
* ``counts_only``: Honor's counts, all zones of the table as domains (and the hostname minimum over all nodes).
"""
import numpy as np

import antiaffinity_ref as A
import hostspread_ref as H
import soft_spread_ref as R
import spread_ref as S

IGNORE, HONOR = 0, 1
VARIANTS = (None, "ignore", "domains_only", "counts_only")


def _subset(mask, lb):
    """bool[n]: every bit of the 128-bit `mask` is set in the rows of `lb` (uint64[n, 2])."""
    m0, m1 = np.uint64(mask[0]), np.uint64(mask[1])
    return ((m0 & ~lb[:, 0]) | (m1 & ~lb[:, 1])) == 0


def restricts(pods, j):
    return bool(np.asarray(pods["sel"][j]).any()) or int(pods["n_req_terms"][j]) > 0


def matches(label_bits, pods, j):
    """M(pod j) as bool[n]: nodeSelector (all bits) and required terms (any term), spec S5."""
    lb = np.asarray(label_bits).astype(np.uint64)
    ok = _subset(pods["sel"][j], lb)
    nt = int(pods["n_req_terms"][j])
    if nt:
        hit = np.zeros(len(lb), bool)
        for t in range(nt):
            hit |= _subset(pods["req_terms"][j][t], lb)
        ok &= hit
    return ok


class HonorState(R.SoftSpreadState):
    """S13 / S14 / S15 state with the S16 rule.  ``set_pod`` tells it the pod at turn; ``M`` is then that
    pod's node set when the rule applies to it, else None."""

    def __init__(self, zone, label_bits, policy=HONOR, variant=None, wpts=2):
        super().__init__(zone, wpts)
        assert variant in VARIANTS and policy in (IGNORE, HONOR)
        self.label_bits = np.asarray(label_bits).astype(np.uint64).copy()
        self.policy, self.variant = policy, variant
        self.M = None

    def copy(self):
        s = HonorState(self.zone, self.label_bits, self.policy, self.variant, self.wpts)
        s.node, s.zcount, s.log = self.node.copy(), self.zcount.copy(), self.log
        return s

    def set_pod(self, pods, j):
        on = self.policy == HONOR and self.variant != "ignore" and restricts(pods, j)
        self.M = matches(self.label_bits, pods, j) if on else None

    def _honor_counts(self):
        return self.M is not None and self.variant in (None, "counts_only")

    def _honor_domains(self):
        return self.M is not None and self.variant in (None, "domains_only")

    def counts(self, app):
        """int64[64]: c[z], or cH[z] over the nodes of M."""
        if not self._honor_counts():
            return self.zcount[app].astype(np.int64)
        m = self.M
        return np.bincount(self.zone[m], weights=self.node[app][m], minlength=A.MAX_ZONES).astype(np.int64)

    def pod_domains(self):
        if not self._honor_domains():
            return self.domains()
        d = np.zeros(A.MAX_ZONES, bool)
        d[self.zone[self.M]] = True
        return d

    def infeasible(self, app, kind):
        kind = int(kind)
        n = len(self.zone)
        if (kind & 0xFF) != S.SPREAD:
            return A.State.infeasible(self, app, kind & 0xFF)
        if R.is_soft(kind):
            return np.zeros(n, bool)
        skew = (kind >> 8) & 0x1F
        if kind & H.HOSTKEY:
            cnt = self.node[app].astype(np.int64)
            over = cnt[self.M] if self._honor_domains() else cnt
            m = int(over.min()) if len(over) else 0
            return cnt + 1 - m > skew
        c, dom = self.counts(app), self.pod_domains()
        if not dom.any():
            return np.zeros(n, bool)
        return c[self.zone] + 1 - int(c[dom].min()) > skew

    def pod_zone_scores(self, app, kind, feas):
        none = np.full(A.MAX_ZONES, -1, np.int64)
        if not R.is_soft(kind) or not feas.any():
            return none
        zones = np.unique(self.zone[feas])
        pts, D, mn, mx = R.zone_scores(self.counts(app), zones, int(S.skew_of(kind)))
        if self.log is not None:
            self.log.append((D, int(self.domains().sum()), mn, mx))
        return pts

    def set_table(self, zone, label_bits):
        """The table's zone and label columns after a qs_node_upsert (appended nodes)."""
        self.set_zones(zone)
        self.label_bits = np.asarray(label_bits).astype(np.uint64).copy()


def pod_keys(nodes, pods, j, state, cfg=None, scorer=None):
    """Keys of pod j on every node under `state` (0 = infeasible), the S14 term included; no state change."""
    pods = A.pods_dict(pods)
    state.set_pod(pods, j)
    return A.pod_keys(nodes, pods, j, state, cfg, state.scorer(scorer, cfg))


def pod_zone_scores(nodes, pods, j, state, cfg=None, scorer=None):
    """What qs_score_pod_zone_scores returns for pod j under `state`: int64[64]."""
    pods = A.pods_dict(pods)
    state.set_pod(pods, j)
    return R.pod_zone_scores(nodes, pods, j, state, cfg, scorer)


def schedule(nodes, pods, cfg=None, scorer=None, state=None, facts=None):
    """antiaffinity_ref.schedule with the pod announced to the state before its turn.  `facts` (a list,
    optional) receives, per restricting spread pod under Honor, a dict: j, the zones of M, the table's
    domains, the app's pods recorded outside M, and whether some node fits the pod without / with the
    spread rule."""
    pods = A.pods_dict(pods)
    state = HonorState(nodes["zone"], nodes["label_bits"]) if state is None else state
    keys_of = state.scorer(scorer, cfg)
    p = len(pods["qos"])
    placement = np.full(p, -1, np.int32)
    keys = np.zeros(p, np.uint64)
    for j in A.order_of(pods, cfg):
        app, kind = int(pods["app"][j]), int(pods["anti_affinity"][j])
        state.set_pod(pods, j)
        k = keys_of(A.masked(nodes, state, app, kind), pods, j)
        if facts is not None and state.M is not None and (kind & 0xFF) == S.SPREAD:
            dom = np.zeros(A.MAX_ZONES, bool)
            dom[state.zone[state.M]] = True
            facts.append(dict(j=j, kind=kind, zones_m=dom, zones_table=state.domains(),
                              outside=int(state.node[app][~state.M].sum()),
                              fits_plain=bool((keys_of(nodes, pods, j) != 0).any()), fits=bool((k != 0).any())))
        best = int(k.max()) if len(k) else 0
        if best == 0:
            continue
        n = 0xFFFFFFFF - (best & 0xFFFFFFFF)
        placement[j], keys[j] = n, best
        A.reserve(nodes, pods, j, n)
        state.record(app, n)
    return placement, keys, state


def run(nodes, pods, cfg=None, scorer=None, state=None, policy=HONOR, variant=None, wpts=2, facts=None):
    """schedule() on a copy of the table (and of `state`): (placement, keys, final nodes, state)."""
    on = {k: v.copy() for k, v in nodes.items()}
    st = HonorState(nodes["zone"], nodes["label_bits"], policy, variant, wpts) if state is None else state.copy()
    pl, keys, st = schedule(on, pods, cfg, scorer, st, facts)
    return pl, keys, on, st
