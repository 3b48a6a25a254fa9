"""The resident ring resolver's 32-bit keys and the zero-allocatable fast path.

Every case runs the resident lookahead stream three times — as shipped, with QS_RES_K32=0 (64-bit
resolver keys) and with QS_FAST_ALLOC=0 (generic scorers) — and each run must be resident and equal
the CPU oracle bit for bit: placements, per-pod 64-bit keys, final node table.  The shapes are the
places the 32-bit path can go wrong: empty list entries (fewer nodes than lanes), unschedulable pods
(winner key 0), one-pod / partial / full windows, high node bits with the boundary fallback on
nearly every window, ties (the node half of the key decides), the key-width boundary
100 * wmax + 1 < 1024, zero-allocatable nodes (flag off), the same tables without them (flag on),
extended resources and the configurable-resource class.  stats["resident_path"] says which path ran
(bit 0: 32-bit resolver keys, bit 1: key waves without the zero-allocatable terms); every variant
asserts the bits it names.  The key helpers themselves are swept on the CPU by tests/test_key32.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import pods_from_struct, pods_to_struct, synth_generate  # noqa: E402

import adversarial as A  # noqa: E402
from oracle import oracle as O  # noqa: E402
from rescfg import GPU_CFG  # noqa: E402
from test_gpu_parity import assert_same, run_gpu  # noqa: E402

GIB, KI = 1 << 30, 1 << 10
VARIANTS = [{}, {"QS_RES_K32": "0"}, {"QS_FAST_ALLOC": "0"}]


K32_BIT, FAST_BIT = 1, 2


def check(monkeypatch, nodes, pods, cfg=None, ocfg=None, K=0, k32=True, fast=True):
    """pods: the struct array.  k32 / fast: what the run as shipped must report in
    stats["resident_path"]; QS_RES_K32=0 / QS_FAST_ALLOC=0 must clear their bit and leave the other.
    Returns the oracle's placements."""
    cfg = cfg or {}
    on = {k: v.copy() for k, v in nodes.items()}
    pl, keys, _ = O.schedule(on, pods_from_struct(pods), cfg if ocfg is None else ocfg, nthreads=16)
    for env in VARIANTS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            g = run_gpu(nodes, pods, cfg, "lookahead", lookahead=K)
        assert g[3]["resident"] == 1, env
        want = (K32_BIT if k32 and "QS_RES_K32" not in env else 0) | \
               (FAST_BIT if fast and "QS_FAST_ALLOC" not in env else 0)
        assert g[3]["resident_path"] == want, (env, g[3]["resident_path"], want)
        assert_same(g[:2], (pl, keys), g[2], on)
    return pl


def test_empty_entries(monkeypatch):
    """Fewer nodes than lanes: most list entries are empty (key 0)."""
    nodes, pods = synth_generate(2, 40, 1500)
    check(monkeypatch, nodes, pods)


def test_unschedulable_pods(monkeypatch):
    """The cluster fills: winner key 0, placement -1."""
    nodes, pods = synth_generate(2, 60, 4000)
    pl = check(monkeypatch, nodes, pods)
    assert (pl == -1).any()


@pytest.mark.parametrize("K", [1, 7, 32])
def test_window_shapes(monkeypatch, K):
    """One-pod windows, partial last windows (5000 = 714 * 7 + 2 = 156 * 32 + 8), full windows."""
    nodes, pods = synth_generate(2, 700, 5000)
    check(monkeypatch, nodes, pods, K=K)


def test_boundary_fallback_high_node_bits(monkeypatch):
    """50,000 nodes: node indices up to 16 bits in the key's low half, and a selection long enough
    that the next window's lists miss the prefetch check on nearly every window."""
    nodes, pods = synth_generate(2, 50000, 1500)
    check(monkeypatch, nodes, pods, K=32)


def test_ties_lowest_index_wins(monkeypatch):
    """Identical empty nodes, identical pods: every pod's best total is shared by many nodes and the
    node half of the key decides (spec S7: the lowest index)."""
    nodes, pods = O.empty_cluster(2000, 3000)
    nodes["alloc_cpu"][:] = 4000
    nodes["alloc_mem"][:] = 8 * GIB
    nodes["max_pods"][:] = 110
    pods["req_cpu"][:] = pods["nz_cpu"][:] = 100
    pods["req_mem"][:] = pods["nz_mem"][:] = 128 << 20
    pods["qos"][:] = 1
    pl = check(monkeypatch, nodes, pods_to_struct(pods))
    assert pl[0] == 0 and (pl >= 0).all()


@pytest.mark.parametrize("w_fit,k32", [((5, 5, 5), True), ((6, 6, 6), False)], ids=["1001-k32", "1101-k64"])
def test_key_width_boundary(monkeypatch, w_fit, k32):
    """100 * wmax + 1 < 1024: w_fit = w_bal = 5 gives 1001 (32-bit keys, all ten score bits in use),
    w_fit = 6 gives 1101 (the 64-bit path)."""
    cfg = dict(w_fit=w_fit, w_bal=(5, 5, 5))
    assert (100 * (w_fit[0] + 5) + 1 < 1024) == k32
    nodes, pods = synth_generate(2, 1500, 6000)
    check(monkeypatch, nodes, pods, cfg, k32=k32)


def zero_alloc(nodes):
    return (nodes["alloc_cpu"] == 0) | (nodes["alloc_mem"] == 0)


@pytest.mark.parametrize("weights", [0, 2])
@pytest.mark.parametrize("grid", ["binary", "ki"])
def test_zero_allocatable_nodes(monkeypatch, grid, weights):
    """Adversarial tables (tests/adversarial.py; the ki grid takes the wide layout) with
    zero-allocatable nodes: the flag is off and the generic scorers run.  The same cluster with
    those nodes given non-zero allocatable runs the flag-on path; one zero-allocatable node in that
    table switches it off again."""
    case = dict(seed=7100 + weights, n=300, p=3000, grid=grid, init_usage=1, weights=weights, qos_sort=0,
                features=0)
    nodes, pods, gcfg, ocfg = A.build(case)
    sp = pods_to_struct(pods)
    assert zero_alloc(nodes).any()
    check(monkeypatch, nodes, sp, gcfg, ocfg, fast=False)
    fixed = {k: v.copy() for k, v in nodes.items()}
    fixed["alloc_cpu"][nodes["alloc_cpu"] == 0] = 3000
    fixed["alloc_mem"][nodes["alloc_mem"] == 0] = 4 * GIB if grid == "binary" else ((5 << 20) | 1) * KI
    assert not zero_alloc(fixed).any()
    check(monkeypatch, fixed, sp, gcfg, ocfg)
    one = {k: v.copy() for k, v in fixed.items()}
    one["alloc_cpu"][len(one["alloc_cpu"]) // 2] = 0
    assert int(zero_alloc(one).sum()) == 1
    check(monkeypatch, one, sp, gcfg, ocfg, fast=False)


def test_ext_resources(monkeypatch):
    """Config-4 generator with the Fit + Balanced profile (amd.com/gpu in Filter, no taints / affinity)."""
    nodes, pods = synth_generate(4, 1800, 5000)
    check(monkeypatch, nodes, pods)


def test_configurable_resources(monkeypatch):
    """The configurable-resource class: LeastAllocated {cpu:1, memory:1, ext0:5}, Balanced over
    [cpu, memory, ext0]."""
    nodes, pods = synth_generate(4, 1500, 4000)
    assert not zero_alloc(nodes).any()
    check(monkeypatch, nodes, pods, dict(GPU_CFG), fast=False)  # (the flag is for the two-resource scorers)
