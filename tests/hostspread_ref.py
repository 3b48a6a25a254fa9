"""Reference for hostname topology spread on the exact stream and the score path (spec/semantics.md S15;
``anti_affinity = QS_AA_SPREAD_HOSTNAME(max_skew)``), CPU only.

The S13 reference (tests/spread_ref.py) with one more kind of infeasible-node mask; the stream, the
scorers, recording, Unreserve and order are S12's.  No scorer is restated here.

``anti_affinity`` carries kind 3 in its low byte, ``max_skew`` in bits 8-12 and the flag ``HOSTKEY``
(bit 18).  With ``cnt[i]`` the recorded pods of the pod's app on node ``i`` (``State.node[app]``) and
``m`` the minimum of ``cnt`` over EVERY node of the table, node ``i`` is infeasible when
``cnt[i] + 1 - m > max_skew``.

Two deliberately wrong variants serve the conditions on the test inputs:

* ``feasible_only``: the minimum over the nodes the pod could otherwise take (``fits(i)`` true);
* ``min_zero``: the minimum always 0.
"""
import numpy as np

import antiaffinity_ref as A
import spread_ref as S

HOSTKEY = 1 << 18


def spread_hostname(max_skew):
    """QS_AA_SPREAD_HOSTNAME(max_skew)."""
    return S.spread(max_skew) | HOSTKEY


def is_hostkey(v):
    return (np.asarray(v) >> 18) & 1


class HostSpreadState(S.SpreadState):
    """S13's state plus the S15 filter.  ``variant``: None (the specification), "feasible_only" or
    "min_zero".  ``fits`` (feasible_only alone) is set by the stream before each pod: bool[n], the nodes
    the pod could take were it not for the tracked filters."""

    def __init__(self, zone, variant=None):
        super().__init__(zone)
        assert variant in (None, "feasible_only", "min_zero")
        self.variant = variant
        self.fits = None

    def copy(self):
        s = HostSpreadState(self.zone, self.variant)
        s.node, s.zcount = self.node.copy(), self.zcount.copy()
        return s

    def minimum(self, app):
        cnt = self.node[app].astype(np.int64)
        if self.variant == "min_zero" or len(cnt) == 0:
            return 0
        if self.variant == "feasible_only":
            return int(cnt[self.fits].min()) if self.fits is not None and self.fits.any() else 0
        return int(cnt.min())

    def infeasible(self, app, kind):
        kind = int(kind)
        if (kind & 0xFF) != S.SPREAD or not (kind & HOSTKEY):
            return super().infeasible(app, kind)
        skew = (kind >> 8) & 0x1F
        cnt = self.node[app].astype(np.int64)
        return cnt + 1 - self.minimum(app) > skew


def schedule(nodes, pods, cfg=None, scorer=None, state=None, variant=None):
    """The S15 stream: antiaffinity_ref.schedule with a HostSpreadState.  For ``feasible_only`` the
    state learns, before each pod, the nodes that pod could take on the unmasked table."""
    pods = A.pods_dict(pods)
    state = HostSpreadState(nodes["zone"], variant) if state is None else state
    if state.variant != "feasible_only":
        return A.schedule(nodes, pods, cfg, scorer, state)
    base = scorer or A.oracle_scorer(cfg)
    # feasible_only needs fits per pod: A.schedule's loop with that one step added
    p = len(pods["qos"])
    placement = np.full(p, -1, np.int32)
    keys = np.zeros(p, np.uint64)
    for j in A.order_of(pods, cfg):
        app, kind = int(pods["app"][j]), int(pods["anti_affinity"][j])
        state.fits = base(nodes, pods, j) != 0
        k = base(A.masked(nodes, state, app, kind), pods, j)
        best = int(k.max()) if len(k) else 0
        if best == 0:
            continue
        n = 0xFFFFFFFF - (best & 0xFFFFFFFF)
        placement[j], keys[j] = n, best
        A.reserve(nodes, pods, j, n)
        state.record(app, n)
    return placement, keys, state


def run(nodes, pods, cfg=None, scorer=None, state=None, variant=None):
    """schedule() on a copy of the table (and of `state`): (placement, keys, final nodes, state)."""
    on = {k: v.copy() for k, v in nodes.items()}
    st = None if state is None else state.copy()
    pl, keys, st = schedule(on, pods, cfg, scorer, st, variant)
    return pl, keys, on, st


def skew_of_app(state, app):
    """max cnt - min cnt of `app` over every node of the table."""
    c = state.node[app]
    return int(c.max() - c.min()) if len(c) else 0
