"""GPU parity of the MostAllocated / RequestedToCapacityRatio scoring strategies (spec/semantics.md S5
"Scoring strategies", qs_set_scoring_strategy): every exact engine and the framework path against
tests/strategy_ref.py bit for bit — placements, per-pod keys and the final table.  The reference is
pinned by spec/kat.md K16-K23 and cross-checked against the pure-Python oracle and the C++ CPU
plugins in tests/test_strategy_cpu.py.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import QschedError, Scheduler, _abi, pods_from_struct, synth_generate  # noqa: E402

import strategy_ref as R  # noqa: E402
from rescfg import GPU_CFG, NAMED  # noqa: E402
from test_gpu_parity import CFG4, assert_same, run_gpu, run_oracle  # noqa: E402
from test_gpu_resources import cluster  # noqa: E402
from test_gpu_wide import ki_cluster  # noqa: E402

GIB, MIB = 1 << 30, 1 << 20
FALL30 = [(0, 10), (30, 0)]
THREE = [(0, 2), (40, 10), (70, 3), (100, 8)]
STRATEGIES = {
    "most": dict(scoring_strategy="MostAllocated"),
    "binpack": dict(scoring_strategy="RequestedToCapacityRatio", shape=R.BIN_PACK),
    "fall30": dict(scoring_strategy="RequestedToCapacityRatio", shape=FALL30),
    "three": dict(scoring_strategy="RequestedToCapacityRatio", shape=THREE),
}
PROFILES = {"fit-balanced": {}, "norm": CFG4}
LISTS = {"gpu5": NAMED["gpu5"], "default": {}}
ENGINES = [("lookahead", "1"), ("lookahead", "0"), ("scan", "1"), ("persistent", "1")]


def check(g, ref):
    """g = run_gpu's (placement, keys, final, stats); ref = strategy_ref.run's."""
    assert_same(g[:2], ref[:2], g[2], ref[2])


@functools.lru_cache(maxsize=None)
def engines_case(strat, prof, lst):
    nodes, pods = cluster(1800, 3000)
    cfg = dict(LISTS[lst], **PROFILES[prof], **STRATEGIES[strat])
    return nodes, pods, cfg, R.run(nodes, pods, cfg)


@pytest.mark.parametrize("lst", list(LISTS))
@pytest.mark.parametrize("prof", list(PROFILES))
@pytest.mark.parametrize("engine,resident", ENGINES, ids=["resident", "per-window", "scan", "persistent"])
@pytest.mark.parametrize("strat", list(STRATEGIES))
def test_strategy_engines(monkeypatch, strat, engine, resident, prof, lst):
    monkeypatch.setenv("QS_RESIDENT", resident)
    nodes, pods, cfg, ref = engines_case(strat, prof, lst)
    g = run_gpu(nodes, pods, cfg, engine)
    check(g, ref)
    if engine == "lookahead":
        assert g[3]["resident"] == int(resident)


@pytest.mark.parametrize("strat", ["most", "three"])
def test_strategy_scan_soa(strat):
    """The SCAN engine over the column-major copy (Fit + Balanced, compact rows)."""
    nodes, pods, cfg, ref = engines_case(strat, "fit-balanced", "gpu5")
    check(run_gpu(nodes, pods, dict(cfg, scan_soa_min_nodes=1), "scan"), ref)


def identical_cluster(n=300, p=2500):
    nodes, _ = synth_generate(2, n, 1)
    for k in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "pods"):
        nodes[k][:] = 0
    nodes["alloc_cpu"][:], nodes["alloc_mem"][:], nodes["max_pods"][:] = 4000, 16 * GIB, 110
    _, pods = synth_generate(2, 1, p)
    pods["req_cpu"] = pods["nz_cpu"] = 500
    pods["req_mem"] = pods["nz_mem"] = GIB
    pods["qos"] = 2
    return nodes, pods


@functools.lru_cache(maxsize=None)
def ties_case(strat):
    nodes, pods = identical_cluster()
    return nodes, pods, R.run(nodes, pods, STRATEGIES[strat])


@pytest.mark.parametrize("variant", [{}, {"lookahead_serial": 1}, {"virtual_shards": 2}],
                         ids=["overlapped", "serial", "shards2"])
@pytest.mark.parametrize("strat", ["most", "binpack"])
def test_ties_and_filling(strat, variant):
    """300 identical empty nodes: every list boundary is a tie broken by node index, nodes fill up and
    turn infeasible inside windows (8 pods of 500 m fill 4000 m), and the last 100 pods find no node."""
    nodes, pods, ref = ties_case(strat)
    assert (ref[0][:2400] >= 0).all() and (ref[0][2400:] == -1).all() and (ref[1][2400:] == 0).all()
    assert np.array_equal(ref[0][:2400], np.arange(2400) // 8)  # bin-packed in index order
    check(run_gpu(nodes, pods, dict(STRATEGIES[strat], **variant), "lookahead"), ref)


@pytest.mark.parametrize("engine", ["lookahead", "scan"])
@pytest.mark.parametrize("strat", ["most", "binpack", "fall30"])
def test_overcommitted_nonzero_requested(strat, engine):
    """BestEffort pods (request 0, non-zero 100 m / 200 MiB) on small nodes: they fit until max_pods,
    so NonZeroRequested passes the allocatable on feasible nodes — MostAllocated's clip to 100, and
    raw(100) for RequestedToCapacityRatio."""
    nodes, pods = synth_generate(2, 40, 1500, seed=9)
    for k in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "pods"):
        nodes[k][:] = 0
    nodes["alloc_cpu"][:] = np.where(np.arange(40) % 3 == 0, 2000, 1000)
    nodes["alloc_mem"][:] = np.where(np.arange(40) % 2 == 0, 2 * GIB, GIB)
    nodes["max_pods"][:] = 60
    be = np.arange(1500) % 4 != 0
    pods["req_cpu"] = np.where(be, 0, 100)
    pods["nz_cpu"] = 100
    pods["req_mem"] = np.where(be, 0, 64 * MIB)
    pods["nz_mem"] = np.where(be, 200 * MIB, 64 * MIB)
    pods["qos"] = np.where(be, 0, 1)
    ref = R.run(nodes, pods, STRATEGIES[strat])
    assert ref[3]["overcommitted"] >= 100, ref[3]
    check(run_gpu(nodes, pods, STRATEGIES[strat], engine), ref)


@pytest.mark.parametrize("prof", list(PROFILES))
@pytest.mark.parametrize("strat", ["most", "three"])
def test_zero_allocatables(strat, prof):
    """3 % of the nodes with allocatable cpu 0 (the cpu entry is skipped there)."""
    nodes, pods = cluster(1500, 2000, seed=5)
    rng = np.random.default_rng(5)
    nodes["alloc_cpu"][rng.random(1500) < 0.03] = 0
    cfg = dict(NAMED["four-res"], **PROFILES[prof], **STRATEGIES[strat])
    ref = R.run(nodes, pods, cfg)
    for engine in ("lookahead", "scan"):
        check(run_gpu(nodes, pods, cfg, engine), ref)


@pytest.mark.parametrize("strat", ["most", "fall30"])
def test_wide_layout(strat):
    """The wide row layout (odd-Ki memory, decimal requests): f64 memory utilisation."""
    nodes, pods = ki_cluster(3000, 4000, features=True)
    cfg = dict(CFG4, **GPU_CFG, **STRATEGIES[strat])
    g = run_gpu(nodes, pods, cfg, "lookahead")
    assert g[3]["table_layout"] == "wide"
    check(g, R.run(nodes, pods, cfg))
    cfg = dict(GPU_CFG, **STRATEGIES[strat])
    s = run_gpu(nodes, pods, cfg, "scan")
    assert s[3]["table_layout"] == "wide"
    check(s, R.run(nodes, pods, cfg))


@pytest.mark.parametrize("layout", [{}, {"scan_soa_min_nodes": 1}], ids=["rows", "soa"])
@pytest.mark.parametrize("prof", list(PROFILES))
@pytest.mark.parametrize("strat", ["most", "three"])
def test_score_pod(strat, prof, layout):
    """The framework path (qs_score_pod) across 20 Reserves: feasible, the four scores, total, best."""
    nodes, pods = cluster(2500, 60)
    cfg = dict(GPU_CFG, **PROFILES[prof], **STRATEGIES[strat])
    on = {k: v.copy() for k, v in nodes.items()}
    op = pods_from_struct(pods)
    with Scheduler(dict(cfg, **layout)) as s:
        s.load_nodes(nodes)
        for j in range(0, 60, 3):
            got = s.score_pod(pods[j])
            feas, sc, total, best = R.score_pod(on, op, j, cfg)
            assert np.array_equal(got["feasible"], feas)
            assert np.array_equal(got["total"], total)
            np.testing.assert_array_equal(got["scores"], sc)
            assert got["best"] == best
            bp, packed = s.score_pod_packed(pods[j])
            assert bp == best and np.array_equal(packed != 0xFFFFFFFF, feas)
            assert np.array_equal((packed & 255)[feas], sc[feas, 0])
            if best >= 0:
                s.reserve(best, pods[j])
                R.reserve(on, op, j, best)


def test_interface(oracle):
    nodes, pods = synth_generate(2, 700, 2000)
    with Scheduler({"engine": "lookahead"}) as s:
        s.load_nodes(nodes)
        for bad in ([], [(0, 0), (0, 10)], [(0, 11)], [(101, 1)], [(i, 1) for i in range(17)][:16] + [(3, 1)]):
            with pytest.raises((QschedError, ValueError)) as e:
                s.set_scoring_strategy("RequestedToCapacityRatio", bad)
            if isinstance(e.value, QschedError):
                assert e.value.status == _abi.QS_EINVAL and "shape" in str(e.value)
        with pytest.raises(QschedError) as e:
            s.set_scoring_strategy("MostAllocated", R.BIN_PACK)  # a shape for a type that takes none
        assert e.value.status == _abi.QS_EINVAL and "shape" in str(e.value)
        with pytest.raises(QschedError) as e:
            s.set_scoring_strategy(7)
        assert e.value.status == _abi.QS_EINVAL and "strategy" in str(e.value)
        # a prepared stream pins the strategy
        st = s.prepare(pods)
        with pytest.raises(QschedError) as e:
            s.set_scoring_strategy("MostAllocated")
        assert e.value.status == _abi.QS_ESTATE and "prepared" in str(e.value)
        st.free()
        s.set_scoring_strategy("MostAllocated")
        s.save_table()
        st = s.prepare(pods)
        st.run()
        pl, keys = st.results()
        ref = R.run(nodes, pods, STRATEGIES["most"])
        assert np.array_equal(pl, ref[0]) and np.array_equal(keys, ref[1])
        # batched mode scores LeastAllocated only
        s.restore_table()
        with pytest.raises(QschedError) as e:
            st.run(mode="batched")
        assert e.value.status == _abi.QS_EINVAL and "LeastAllocated" in str(e.value)
        st.free()
        # LeastAllocated again: the C oracle's placements on the same context
        s.restore_table()
        s.set_scoring_strategy("LeastAllocated")
        st = s.prepare(pods)
        st.run()
        pl, keys = st.results()
        st.free()
        o = run_oracle(oracle, nodes, pods, {})
        assert np.array_equal(pl, o[0]) and np.array_equal(keys, o[1])
        assert not np.array_equal(pl, ref[0])


def test_stream_freed_after_close():
    """A prepared stream outlives its context: qs_close detaches it, qs_stream_free then frees it."""
    nodes, pods = synth_generate(2, 100, 50)
    s = Scheduler({})
    s.load_nodes(nodes)
    a, b = s.prepare(pods), s.prepare(pods)
    a.free()
    with pytest.raises(QschedError) as e:
        s.set_scoring_strategy("MostAllocated")  # b still pins the strategy
    assert e.value.status == _abi.QS_ESTATE
    s.close()
    b.free()
    assert b.h is None
