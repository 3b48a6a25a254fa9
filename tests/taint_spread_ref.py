"""Reference for ``nodeTaintsPolicy: Honor`` of the topology spread constraints on the exact stream and the
score path (spec/semantics.md S17; qs_set_topology_spread_node_taints_policy), CPU only.

The state of tests/honor_spread_ref.py (S13 - S16) with a second inclusion predicate: besides the table's
``label_bits`` it is given the table's ``taint_hard`` and, before each pod, that pod's ``tol_hard``.

``M_T(pod)`` = the nodes with ``taint_hard & ~tol_hard == 0`` (the TaintToleration filter's predicate);
``M_A(pod)`` is S16's ``M``; ``M(pod) = M_A ∩ M_T``, each factor replaced by "all nodes" when its policy is
``ignore`` (and ``M_A`` for a pod without a selector or required terms).  Every rule of S16 then holds with
this ``M``.  A pod for which ``M`` is every node follows S13 / S14 / S15 to the letter.

Four deliberately wrong variants serve the conditions on the test inputs:

* ``ignore``: both policies ``ignore`` whatever the context says;
* ``domains_only``: the domains of ``M`` (and the hostname minimum over ``M``), the counts over all nodes;
* ``counts_only``: the counts over ``M``, all zones of the table as domains (and the hostname minimum over all
  nodes);
* ``affinity_only``: ``M_T`` dropped, ``M = M_A`` (with both policies on: S16 alone).
"""
import numpy as np

import honor_spread_ref as HR

IGNORE, HONOR = HR.IGNORE, HR.HONOR
VARIANTS = (None, "ignore", "domains_only", "counts_only", "affinity_only")


def tolerated(taint_hard, pods, j):
    """M_T(pod j) as bool[n]: no hard taint of the node that the pod does not tolerate (spec S5)."""
    th = np.asarray(taint_hard).astype(np.uint64)
    return (th & ~np.uint64(pods["tol_hard"][j])) == 0


class TaintState(HR.HonorState):
    """S13 - S16 state with the S17 rule.  ``policy`` is the nodeAffinityPolicy, ``taints_policy`` the
    nodeTaintsPolicy; ``set_pod`` tells it the pod at turn, and ``M`` is then that pod's node set when
    either predicate leaves a node out, else None."""

    def __init__(self, zone, label_bits, taint_hard, policy=IGNORE, taints_policy=HONOR, variant=None, wpts=2):
        assert variant in VARIANTS and taints_policy in (IGNORE, HONOR)
        base = variant if variant in HR.VARIANTS else None
        super().__init__(zone, label_bits, policy, base, wpts)
        self.variant = variant
        self.taint_hard = np.asarray(taint_hard).astype(np.uint64).copy()
        self.taints_policy = taints_policy

    def copy(self):
        s = TaintState(self.zone, self.label_bits, self.taint_hard, self.policy, self.taints_policy, self.variant,
                       self.wpts)
        s.node, s.zcount, s.log = self.node.copy(), self.zcount.copy(), self.log
        return s

    def set_pod(self, pods, j):
        m = None
        if self.variant != "ignore":
            if self.policy == HONOR and HR.restricts(pods, j):
                m = HR.matches(self.label_bits, pods, j)
            if self.taints_policy == HONOR and self.variant != "affinity_only":
                mt = tolerated(self.taint_hard, pods, j)
                if not mt.all():
                    m = mt if m is None else m & mt
        self.M = m

    # (domains_only / counts_only are HonorState's; affinity_only differs in M alone)
    def _honor_counts(self):
        return self.M is not None and self.variant in (None, "counts_only", "affinity_only")

    def _honor_domains(self):
        return self.M is not None and self.variant in (None, "domains_only", "affinity_only")

    def set_table(self, zone, label_bits, taint_hard=None):
        """The table's zone, label and hard-taint columns after a qs_node_upsert."""
        super().set_table(zone, label_bits)
        if taint_hard is not None:
            self.taint_hard = np.asarray(taint_hard).astype(np.uint64).copy()


pod_keys = HR.pod_keys
pod_zone_scores = HR.pod_zone_scores


def state_of(nodes, policy=IGNORE, taints_policy=HONOR, variant=None, wpts=2):
    return TaintState(nodes["zone"], nodes["label_bits"], nodes["taint_hard"], policy, taints_policy, variant, wpts)


def schedule(nodes, pods, cfg=None, scorer=None, state=None, facts=None):
    """honor_spread_ref.schedule under a TaintState; `facts` as there, per pod whose M leaves a node out."""
    state = state_of(nodes) if state is None else state
    return HR.schedule(nodes, pods, cfg, scorer, state, facts)


def run(nodes, pods, cfg=None, scorer=None, state=None, policy=IGNORE, taints_policy=HONOR, variant=None, wpts=2,
        facts=None):
    """schedule() on a copy of the table (and of `state`): (placement, keys, final nodes, state)."""
    on = {k: v.copy() for k, v in nodes.items()}
    st = state_of(nodes, policy, taints_policy, variant, wpts) if state is None else state.copy()
    pl, keys, st = schedule(on, pods, cfg, scorer, st, facts)
    return pl, keys, on, st


def skew_holds(nodes, pods, placement, policy=IGNORE, taints_policy=HONOR, cfg=None):
    """The invariant of the two DoNotSchedule kinds over M, replayed in stream order: right after a SPREAD /
    SPREAD_HOSTNAME pod is placed, its domain's count over M is at most max_skew above the minimum over the
    domains of M (spec S13 / S15 with S17's M).  Returns the number of placements checked."""
    import antiaffinity_ref as A
    import hostspread_ref as H
    import soft_spread_ref as R
    import spread_ref as S

    pods = A.pods_dict(pods)
    st = state_of(nodes, policy, taints_policy)
    seen = 0
    for j in A.order_of(pods, cfg):
        n = int(placement[j])
        if n < 0:
            continue
        app, kind = int(pods["app"][j]), int(pods["anti_affinity"][j])
        st.set_pod(pods, j)
        m = np.ones(len(st.zone), bool) if st.M is None else st.M
        st.record(app, n)
        if (kind & 0xFF) != S.SPREAD or R.is_soft(kind):
            continue
        skew = (kind >> 8) & 0x1F
        assert m[n], (j, n)
        cnt = st.node[app].astype(np.int64)
        if kind & H.HOSTKEY:
            assert cnt[n] - int(cnt[m].min()) <= skew, (j, n)
        else:
            c = np.bincount(st.zone[m], weights=cnt[m], minlength=A.MAX_ZONES).astype(np.int64)
            dom = np.zeros(A.MAX_ZONES, bool)
            dom[st.zone[m]] = True
            assert c[st.zone[n]] - int(c[dom].min()) <= skew, (j, n)
        seen += 1
    return seen
