"""Reference for zone topology spread on the exact stream and the score path (spec/semantics.md S13;
``anti_affinity = QS_AA_SPREAD(max_skew)``), CPU only.

The S12 reference (tests/antiaffinity_ref.py) with one more kind of infeasible-node mask: the stream is
``antiaffinity_ref.schedule(..., state=SpreadState(zone))`` with every scorer that reference takes
(oracle, strategy, per-QoS).  No scorer is restated here, and recording / Unreserve / order are S12's.

``anti_affinity`` carries the kind in its low byte and, for kind 3, ``max_skew`` in bits 8-12.  With
``c[z]`` the recorded pods of the pod's app in zone ``z`` and ``m`` the minimum of ``c`` over the domains
(the zones that hold a node of the table), node ``i`` is infeasible when ``c[zone(i)] + 1 - m > max_skew``.
"""
import numpy as np

import antiaffinity_ref as A

SPREAD = 3
MAX_SKEW = 31


def spread(max_skew):
    """QS_AA_SPREAD(max_skew)."""
    assert 1 <= max_skew <= MAX_SKEW
    return SPREAD | (max_skew << 8)


def kind_of(v):
    return np.asarray(v) & 0xFF


def skew_of(v):
    return (np.asarray(v) >> 8) & 0x1F


class SpreadState(A.State):
    """S12's state plus the S13 filter.  ``all_zones=True`` is the wrong variant that takes the minimum
    over all 64 zone ids (the tests show that the sparse-zone input tells the two apart)."""

    def __init__(self, zone, all_zones=False):
        super().__init__(zone)
        self.all_zones = all_zones

    def copy(self):
        s = SpreadState(self.zone, self.all_zones)
        s.node, s.zcount = self.node.copy(), self.zcount.copy()
        return s

    def domains(self):
        """bool[MAX_ZONES]: the zones that hold at least one node of the table."""
        d = np.zeros(A.MAX_ZONES, bool)
        d[self.zone] = True
        return d

    def infeasible(self, app, kind):
        k = int(kind) & 0xFF
        if k != SPREAD:
            return super().infeasible(app, k)
        skew = (int(kind) >> 8) & 0x1F
        c = self.zcount[app].astype(np.int64)
        dom = np.ones(A.MAX_ZONES, bool) if self.all_zones else self.domains()
        if not dom.any():
            return np.zeros(len(self.zone), bool)
        return c[self.zone] + 1 - int(c[dom].min()) > skew

    def set_zones(self, zone):
        """The table's zone column after a qs_node_upsert (a changed zone of a node that holds no
        recorded pod, or appended nodes): the per-node counts grow with the table."""
        zone = np.asarray(zone).astype(np.int64)
        grow = len(zone) - self.node.shape[1]
        if grow > 0:
            self.node = np.concatenate([self.node, np.zeros((A.MAX_APPS, grow), np.int32)], axis=1)
        self.zone = zone


def run(nodes, pods, cfg=None, scorer=None, state=None, all_zones=False):
    """The S13 stream on a copy of the table: (placement, keys, final nodes, state)."""
    st = SpreadState(nodes["zone"], all_zones) if state is None else state
    return A.run(nodes, pods, cfg, scorer, st)


def skew_of_app(state, app):
    """max c - min c of `app` over the domains."""
    c = state.zcount[app][state.domains()]
    return int(c.max() - c.min()) if len(c) else 0
