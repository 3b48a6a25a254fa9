"""Reference for zone topology spread scoring on the exact stream and the score path
(spec/semantics.md S14; ``anti_affinity = QS_AA_SPREAD_SOFT(max_skew)``), CPU only.

The S13 reference state (tests/spread_ref.py) with one more term on the keys of
``antiaffinity_ref.pod_keys`` / ``schedule``: a soft pod is filtered by nothing of spread, and every
feasible node's total gains ``Wpts * PTS(zone of the node)``.  The scorers are those the S12 reference
takes (oracle, strategy, per-QoS) and are wrapped, not restated: the term is added to the score half of
the keys they return.  LOGTAB comes from tests/golden/soft_spread_logtab.json.

Two wrong variants for the bite checks of the tests: ``all_domains=True`` takes ``D`` and the minimum /
maximum over every domain of the table instead of the zones that hold a feasible node; ``truncate=True``
takes ``int(x)`` instead of ``floor(x + 0.5)``.
"""
import json
import math
import os

import numpy as np

import antiaffinity_ref as A
import spread_ref as S

SOFT = 1 << 16
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_spread_logtab.json")) as _f:
    LOGTAB = [None] + [float.fromhex(v) for v in json.load(_f)["logtab"]]  # LOGTAB[D], D = 1..64
assert len(LOGTAB) == 65


def spread_soft(max_skew):
    """QS_AA_SPREAD_SOFT(max_skew)."""
    return S.spread(max_skew) | SOFT


def is_soft(v):
    return ((np.asarray(v) >> 16) & 1) == 1


def zone_scores(c, zones, max_skew, truncate=False):
    """(PTS per zone as int64[64] with -1 outside `zones`, D, mn, mx): spec S14 for the counts c[64] and
    the zones of Z (non-empty).  Python floats round each operation once: c * w, then + t."""
    zones = sorted(int(z) for z in zones)
    D = len(zones)
    w, t = LOGTAB[D], max_skew - 1
    raw = {}
    for z in zones:
        x = float(int(c[z])) * w + float(t)
        raw[z] = int(x) if truncate else math.floor(x + 0.5)
    mn, mx = min(raw.values()), max(raw.values())
    pts = np.full(A.MAX_ZONES, -1, np.int64)
    for z in zones:
        pts[z] = 100 if mx == 0 else (100 * (mx + mn - raw[z])) // mx
    return pts, D, mn, mx


class SoftSpreadState(S.SpreadState):
    """S13's state; a soft pod is filtered by nothing, and `scorer(base)` adds its S14 term.  `log`
    (a list, optional) receives (D, domains of the table, mn, mx) of every soft pod scored."""

    def __init__(self, zone, wpts=2, all_domains=False, truncate=False, all_zones=False):
        super().__init__(zone, all_zones)
        self.wpts, self.all_domains, self.truncate = wpts, all_domains, truncate
        self.log = None

    def copy(self):
        s = SoftSpreadState(self.zone, self.wpts, self.all_domains, self.truncate, self.all_zones)
        s.node, s.zcount, s.log = self.node.copy(), self.zcount.copy(), self.log
        return s

    def infeasible(self, app, kind):
        if is_soft(kind):
            return np.zeros(len(self.zone), bool)
        return super().infeasible(app, kind)

    def pod_zone_scores(self, app, kind, feas):
        """PTS per zone (-1 outside Z) of a soft pod of `app` with the feasible-node mask `feas`; all -1
        for every other pod or when nothing is feasible."""
        none = np.full(A.MAX_ZONES, -1, np.int64)
        if not is_soft(kind) or not feas.any():
            return none
        zones = np.flatnonzero(self.domains()) if self.all_domains else np.unique(self.zone[feas])
        pts, D, mn, mx = zone_scores(self.zcount[app], zones, int(S.skew_of(kind)), self.truncate)
        if self.log is not None:
            self.log.append((D, int(self.domains().sum()), mn, mx))
        return pts

    def scorer(self, base, cfg=None):
        """`base` (a scorer of antiaffinity_ref, None = the oracle's) with the S14 term on its keys."""
        base = base or A.oracle_scorer(cfg)

        def keys(nodes, pods, j):
            k = base(nodes, pods, j)
            kind = int(pods["anti_affinity"][j])
            if not is_soft(kind):
                return k
            feas = k != 0
            pts = self.pod_zone_scores(int(pods["app"][j]), kind, feas)
            add = np.where(feas, self.wpts * np.maximum(pts[self.zone], 0), 0).astype(np.uint64)
            return np.where(feas, k + (add << np.uint64(32)), np.uint64(0))

        return keys


def pod_keys(nodes, pods, j, state, cfg=None, scorer=None):
    """antiaffinity_ref.pod_keys with the S14 term (no state change)."""
    return A.pod_keys(nodes, pods, j, state, cfg, state.scorer(scorer, cfg))


def pod_zone_scores(nodes, pods, j, state, cfg=None, scorer=None):
    """What qs_score_pod_zone_scores returns for pod j under `state`: int64[64]."""
    pods = A.pods_dict(pods)
    kind = int(pods["anti_affinity"][j])
    k = A.pod_keys(nodes, pods, j, state, cfg, scorer)
    log, state.log = state.log, None
    try:
        return state.pod_zone_scores(int(pods["app"][j]), kind, k != 0)
    finally:
        state.log = log


def run(nodes, pods, cfg=None, scorer=None, state=None, wpts=2, all_domains=False, truncate=False, log=None):
    """The S14 stream on a copy of the table (and of `state`): (placement, keys, final nodes, state)."""
    st = SoftSpreadState(nodes["zone"], wpts, all_domains, truncate) if state is None else state.copy()
    st.log = log
    on = {k: v.copy() for k, v in nodes.items()}
    pl, keys, st = A.schedule(on, pods, cfg, st.scorer(scorer, cfg), st)
    st.log = None
    return pl, keys, on, st
