"""Inputs and references shared by tests/test_qos_strategy_cpu.py and tests/test_gpu_qos_strategy.py
(spec/semantics.md S9 "Strategy per QoS class"): each reference is computed once per session
(tests/qos_strategy_ref.py) and never changed.

The pod classes are assigned here, qos[j] = (j * 7) % 3 with qos_sort = 0, so that every 32-pod
lookahead window holds the three classes interleaved (the strategy switches from pod to pod), except
in the `sorted` case (qos_sort = 1: three runs, two switches).
"""
import functools

import numpy as np

import qos_strategy_ref as QR
import strategy_ref as R
from rescfg import GPU_CFG, NAMED

GIB = 1 << 30
CFG4 = dict(enable_taint=1, enable_affinity=1)  # (= test_gpu_parity.CFG4)
FALL30 = [(0, 10), (30, 0)]
THREE = [(0, 2), (40, 10), (70, 3), (100, 8)]  # (= test_gpu_strategy.THREE)
LEAST = dict(scoring_strategy="LeastAllocated")
MOST = dict(scoring_strategy="MostAllocated")


def rtcr(shape):
    return dict(scoring_strategy="RequestedToCapacityRatio", shape=shape)


MIX = {"BestEffort": MOST, "Burstable": rtcr(THREE), "Guaranteed": LEAST}
TWO_TABLES = {"BestEffort": rtcr(R.BIN_PACK), "Burstable": rtcr(FALL30), "Guaranteed": MOST}
TIES = {"Guaranteed": LEAST, "BestEffort": MOST}
PROFILES = {"fit-balanced": {}, "norm": CFG4}
LISTS = {"gpu5": NAMED["gpu5"], "default": {}}


def interleaved(pods):
    """A copy of the stream with qos[j] = (j * 7) % 3."""
    pods = pods.copy()
    pods["qos"] = (np.arange(len(pods)) * 7) % 3
    return pods


def windows_hold_every_class(qos, K=32):
    """Every full window of K consecutive pods holds the three classes, and no two neighbours share
    one (the strategy changes at every pod)."""
    qos = np.asarray(qos)
    full = all(set(qos[s:s + K].tolist()) == {0, 1, 2} for s in range(0, len(qos) - K + 1, K))
    return full and bool((qos[1:] != qos[:-1]).all())


def _cluster(n, p, **kw):
    from test_gpu_resources import cluster
    return cluster(n, p, **kw)


@functools.lru_cache(maxsize=None)
def engines_case(prof, lst, qos_sort=0):
    """test_gpu_resources.cluster(1800, 3000) under MIX: (nodes, pods, cfg, reference)."""
    nodes, pods = _cluster(1800, 3000)
    pods = interleaved(pods)
    cfg = dict(LISTS[lst], **PROFILES[prof], qos_strategies=MIX, qos_sort=qos_sort)
    return nodes, pods, cfg, QR.run(nodes, pods, cfg)


@functools.lru_cache(maxsize=None)
def two_tables_case():
    nodes, pods = _cluster(1800, 3000)
    pods = interleaved(pods)
    cfg = dict(NAMED["gpu5"], qos_strategies=TWO_TABLES, qos_sort=0)
    return nodes, pods, cfg, QR.run(nodes, pods, cfg)


@functools.lru_cache(maxsize=None)
def ties_case():
    """test_gpu_strategy.identical_cluster(): 300 identical empty nodes x 2,500 equal pods, the classes
    alternating Guaranteed / BestEffort."""
    from test_gpu_strategy import identical_cluster
    nodes, pods = identical_cluster()
    pods = pods.copy()
    pods["qos"] = np.where(np.arange(len(pods)) % 2 == 0, 2, 0)
    cfg = dict(qos_strategies=TIES, qos_sort=0)
    return nodes, pods, cfg, QR.run(nodes, pods, cfg)


@functools.lru_cache(maxsize=None)
def wide_case():
    from test_gpu_wide import ki_cluster
    nodes, pods = ki_cluster(3000, 4000, features=True)
    pods = interleaved(pods)
    cfg = dict(CFG4, **GPU_CFG, qos_strategies=MIX, qos_sort=0)
    return nodes, pods, cfg, QR.run(nodes, pods, cfg)


def uniform_cfgs(cfg):
    """The distinct one-strategy configurations a per-class configuration is built from."""
    out = []
    for q in range(3):
        u = QR.uniform(cfg, q)
        if u not in out:
            out.append(u)
    return out
