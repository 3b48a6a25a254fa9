"""Reference for one NodeResourcesFit scoring strategy per QoS class (spec/semantics.md S9 "Strategy
per QoS class"; qs_set_scoring_strategy_qos).

The sequential loop of ``strategy_ref.schedule`` — spec S7 keys and Reserve, S8 order — in which pod j
is evaluated with the configuration of class ``qos[j]``: ``strategy_ref.evaluate`` and
``strategy_ref.reserve`` do the work, no scorer is restated here.

Configuration: strategy_ref's dict plus ``qos_strategies`` = {class: dict(scoring_strategy=...,
shape=...)} with the class given by name or id; a class that is not listed keeps the dict's own
``scoring_strategy`` / ``shape`` (LeastAllocated by default), as a context-wide strategy set before
the per-class ones.
"""
import numpy as np

import strategy_ref as R

QOS = {"BestEffort": 0, "Burstable": 1, "Guaranteed": 2}


def class_cfgs(cfg):
    """The three configurations [BestEffort, Burstable, Guaranteed] of strategy_ref."""
    base = dict(cfg or {})
    per = base.pop("qos_strategies", None) or {}
    out = [R._cfg(base) for _ in range(3)]
    for q, sc in per.items():
        q = QOS[q] if isinstance(q, str) else int(q)
        out[q] = R._cfg(dict(base, scoring_strategy=sc.get("scoring_strategy") or "LeastAllocated",
                             shape=sc.get("shape")))
    return out


def uniform(cfg, q):
    """The one-strategy configuration in which every class scores as class q of `cfg` does."""
    c = class_cfgs(cfg)[QOS[q] if isinstance(q, str) else int(q)]
    base = dict(cfg or {})
    base.pop("qos_strategies", None)
    return dict(base, scoring_strategy=c["scoring_strategy"], shape=c["shape"])


def score_pod(nodes, pods, j, cfg=None):
    """(feasible, scores[n, 4], total, best) of pod j with its class's strategy (no state change)."""
    pods = R._pods_dict(pods)
    return R.score_pod(nodes, pods, j, class_cfgs(cfg)[int(pods["qos"][j])])


def schedule(nodes, pods, cfg=None):
    """The exact stream.  Mutates `nodes` (Reserve).  Returns (placement[p] int32, key[p] uint64)."""
    cs, pods = class_cfgs(cfg), R._pods_dict(pods)
    p = len(pods["qos"])
    order = list(range(p))
    if cs[0]["qos_sort"]:
        order.sort(key=lambda j: (-int(pods["qos"][j]), -int(pods["priority"][j]), j))
    placement = np.full(p, -1, np.int32)
    keys = np.zeros(p, np.uint64)
    for j in order:
        ok, _, total = R.evaluate(cs[int(pods["qos"][j])], nodes, pods, j)
        if not ok.any():
            continue
        b = int(np.flatnonzero(total == total.max())[0])
        placement[j] = b
        keys[j] = ((int(total[b]) + 1) << 32) | (0xFFFFFFFF - b)
        R.reserve(nodes, pods, j, b)
    return placement, keys


def run(nodes, pods, cfg=None):
    """schedule() on a copy of the table: (placement, keys, final nodes)."""
    on = {k: v.copy() for k, v in nodes.items()}
    pl, keys = schedule(on, pods, cfg)
    return pl, keys, on
