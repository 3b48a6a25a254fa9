"""GPU parity of one NodeResourcesFit scoring strategy per QoS class (spec/semantics.md S9 "Strategy
per QoS class", qs_set_scoring_strategy_qos): every exact engine and the framework path against
tests/qos_strategy_ref.py bit for bit — placements, per-pod keys and the final table.  The reference
is pinned by spec/kat.md K24-K26 and cross-checked against the C++ CPU plugins in
tests/test_qos_strategy_cpu.py, which also shows that each configuration here places differently from
the one-strategy configurations it is built from.  The inputs and references are shared
(tests/qos_strategy_cases.py).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import QschedError, Scheduler, _abi, pods_from_struct, synth_generate  # noqa: E402

import qos_strategy_cases as C  # noqa: E402
import qos_strategy_ref as QR  # noqa: E402
import strategy_ref as R  # noqa: E402
from rescfg import GPU_CFG  # noqa: E402
from test_gpu_parity import assert_same, run_gpu  # noqa: E402
from test_gpu_resources import cluster  # noqa: E402

ENGINES = [("lookahead", "1"), ("lookahead", "0"), ("scan", "1"), ("persistent", "1")]
ENGINE_IDS = ["resident", "per-window", "scan", "persistent"]


def check(g, ref):
    """g = run_gpu's (placement, keys, final, stats); ref = qos_strategy_ref.run's."""
    assert_same(g[:2], ref[:2], g[2], ref[2])


@pytest.mark.parametrize("lst", list(C.LISTS))
@pytest.mark.parametrize("prof", list(C.PROFILES))
@pytest.mark.parametrize("engine,resident", ENGINES, ids=ENGINE_IDS)
def test_mix_engines(monkeypatch, engine, resident, prof, lst):
    """MIX = {BestEffort: MostAllocated, Burstable: RequestedToCapacityRatio THREE, Guaranteed:
    LeastAllocated}, the strategy changing at every pod of every window."""
    monkeypatch.setenv("QS_RESIDENT", resident)
    nodes, pods, cfg, ref = C.engines_case(prof, lst)
    assert C.windows_hold_every_class(pods["qos"])
    g = run_gpu(nodes, pods, cfg, engine)
    check(g, ref)
    if engine == "lookahead":
        assert g[3]["resident"] == int(resident)


def test_mix_qos_sorted(monkeypatch):
    """qos_sort = 1: the stream is three runs (Guaranteed, Burstable, BestEffort), two switches."""
    monkeypatch.setenv("QS_RESIDENT", "1")
    nodes, pods, cfg, ref = C.engines_case("fit-balanced", "gpu5", 1)
    g = run_gpu(nodes, pods, cfg, "lookahead")
    check(g, ref)
    assert g[3]["resident"] == 1


@pytest.mark.parametrize("engine", ["lookahead", "scan"])
def test_two_tables(monkeypatch, engine):
    """{BestEffort: RTCR bin-pack, Burstable: RTCR FALL30, Guaranteed: MostAllocated}: two different
    shape tables read in one stream."""
    monkeypatch.setenv("QS_RESIDENT", "1")
    nodes, pods, cfg, ref = C.two_tables_case()
    g = run_gpu(nodes, pods, cfg, engine)
    check(g, ref)
    if engine == "lookahead":
        assert g[3]["resident"] == 1


@pytest.mark.parametrize("variant", [{}, {"lookahead_serial": 1}, {"virtual_shards": 2}],
                         ids=["overlapped", "serial", "shards2"])
def test_ties_and_filling(variant):
    """300 identical empty nodes, Guaranteed (LeastAllocated: spreads) and BestEffort (MostAllocated:
    packs) pods alternating: every list boundary is a tie broken by node index, and nodes fill up and
    turn infeasible inside windows."""
    nodes, pods, cfg, ref = C.ties_case()
    assert (ref[0][:2400] >= 0).all() and (ref[0][2400:] == -1).all() and (ref[1][2400:] == 0).all()
    check(run_gpu(nodes, pods, dict(cfg, **variant), "lookahead"), ref)


def test_wide_layout():
    """The wide row layout (odd-Ki memory, decimal requests) under MIX."""
    nodes, pods, cfg, ref = C.wide_case()
    g = run_gpu(nodes, pods, cfg, "lookahead")
    assert g[3]["table_layout"] == "wide"
    check(g, ref)
    s = run_gpu(nodes, pods, cfg, "scan")
    assert s[3]["table_layout"] == "wide"
    check(s, ref)


@pytest.mark.parametrize("layout", [{}, {"scan_soa_min_nodes": 1}], ids=["rows", "soa"])
@pytest.mark.parametrize("prof", list(C.PROFILES))
def test_score_pod(prof, layout):
    """The framework path (qs_score_pod) across 21 Reserves, a pod of each class in turn: feasible, the
    four scores, total, best against strategy_ref.score_pod with the class's configuration."""
    nodes, pods = cluster(2500, 63)
    pods = C.interleaved(pods)
    cfg = dict(GPU_CFG, **C.PROFILES[prof], qos_strategies=C.MIX)
    classes = QR.class_cfgs(cfg)
    on = {k: v.copy() for k, v in nodes.items()}
    op = pods_from_struct(pods)
    seen = set()
    with Scheduler(dict(cfg, **layout)) as s:
        s.load_nodes(nodes)
        for j in range(0, 63, 3):
            j += (j // 3) % 3  # pods 0, 4, 8, 9, 13, 17, ...: classes 0, 1, 2 in turn
            q = int(pods["qos"][j])
            seen.add(q)
            got = s.score_pod(pods[j])
            feas, sc, total, best = R.score_pod(on, op, j, classes[q])
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
    assert seen == {0, 1, 2}


def test_guaranteed_stream_reduces_to_the_default_kernels(monkeypatch):
    """A stream whose pods all belong to a LeastAllocated class runs what a default context runs: the
    same resident path (the strategy kernels would clear bit 1), placements and keys."""
    monkeypatch.setenv("QS_RESIDENT", "1")
    monkeypatch.delenv("QS_FAST_ALLOC", raising=False)
    nodes, pods = synth_generate(2, 700, 2000)
    pods = pods.copy()
    pods["qos"] = 2
    d = run_gpu(nodes, pods, {}, "lookahead")
    g = run_gpu(nodes, pods, dict(qos_strategies=C.MIX), "lookahead")
    assert d[3]["resident"] == 1 and g[3]["resident"] == 1 and d[3]["resident_path"] & 2
    assert g[3]["resident_path"] == d[3]["resident_path"]
    check(g, d[:3])
    # a stream with one BestEffort pod (MostAllocated) does not reduce, and scores as the reference
    pods["qos"][1000] = 0
    cfg = dict(qos_strategies=C.MIX, qos_sort=0)
    m = run_gpu(nodes, pods, cfg, "lookahead")
    assert m[3]["resident"] == 1 and not m[3]["resident_path"] & 2
    check(m, QR.run(nodes, pods, cfg))


def test_interface():
    nodes, pods = synth_generate(2, 700, 2000)
    pods = C.interleaved(pods)
    with Scheduler({"engine": "lookahead"}) as s:
        s.load_nodes(nodes)
        # get returns what set stored; a new context scores LeastAllocated in every class
        for q in ("BestEffort", "Burstable", "Guaranteed", 0, 1, 2):
            assert s.get_scoring_strategy(q) == ("LeastAllocated", [])
        s.set_scoring_strategy("RequestedToCapacityRatio", C.THREE, qos="Burstable")
        s.set_scoring_strategy("MostAllocated", qos=0)
        assert s.get_scoring_strategy(0) == ("MostAllocated", [])
        assert s.get_scoring_strategy(1) == ("RequestedToCapacityRatio", C.THREE)
        assert s.get_scoring_strategy("Guaranteed") == ("LeastAllocated", [])
        # qs_set_scoring_strategy overwrites all three classes
        s.set_scoring_strategy("RequestedToCapacityRatio", C.FALL30)
        assert [s.get_scoring_strategy(q) for q in range(3)] == [("RequestedToCapacityRatio", C.FALL30)] * 3
        # bad qos, a bad shape, a null pointer: QS_EINVAL with a message, and nothing stored
        for q in (-1, 3):
            with pytest.raises(QschedError) as e:
                s.set_scoring_strategy("MostAllocated", qos=q)
            assert e.value.status == _abi.QS_EINVAL and "qos" in str(e.value)
            with pytest.raises(QschedError) as e:
                s.get_scoring_strategy(q)
            assert e.value.status == _abi.QS_EINVAL and "qos" in str(e.value)
        for bad in ([], [(0, 0), (0, 10)], [(0, 11)], [(101, 1)]):
            with pytest.raises(QschedError) as e:
                s.set_scoring_strategy("RequestedToCapacityRatio", bad, qos=1)
            assert e.value.status == _abi.QS_EINVAL and "shape" in str(e.value)
        with pytest.raises(QschedError) as e:
            s.set_scoring_strategy("MostAllocated", R.BIN_PACK, qos=1)  # a shape for a type that takes none
        assert e.value.status == _abi.QS_EINVAL and "shape" in str(e.value)
        with pytest.raises(QschedError) as e:
            s.set_scoring_strategy(7, qos=1)
        assert e.value.status == _abi.QS_EINVAL and "strategy" in str(e.value)
        with pytest.raises(QschedError) as e:
            s._chk(s.lib.qs_set_scoring_strategy_qos(s.ctx, 1, None))
        assert e.value.status == _abi.QS_EINVAL and "null" in str(e.value)
        with pytest.raises(QschedError) as e:
            s._chk(s.lib.qs_get_scoring_strategy_qos(s.ctx, 1, None))
        assert e.value.status == _abi.QS_EINVAL and "null" in str(e.value)
        assert [s.get_scoring_strategy(q) for q in range(3)] == [("RequestedToCapacityRatio", C.FALL30)] * 3
        # a prepared stream pins every class's strategy
        for q, sc in C.MIX.items():
            s.set_scoring_strategy(sc["scoring_strategy"], sc.get("shape"), qos=q)
        st = s.prepare(pods)
        with pytest.raises(QschedError) as e:
            s.set_scoring_strategy("MostAllocated", qos="Guaranteed")
        assert e.value.status == _abi.QS_ESTATE and "prepared" in str(e.value)
        assert s.get_scoring_strategy("Guaranteed") == ("LeastAllocated", [])
        # batched mode scores LeastAllocated only
        s.save_table()
        with pytest.raises(QschedError) as e:
            st.run(mode="batched")
        assert e.value.status == _abi.QS_EINVAL and "LeastAllocated" in str(e.value)
        s.restore_table()
        st.run()
        pl, keys = st.results()
        st.free()
        cfg = dict(qos_strategies=C.MIX)
        ref = QR.run(nodes, pods, cfg)
        assert np.array_equal(pl, ref[0]) and np.array_equal(keys, ref[1])
    # the config key, applied after a context-wide strategy
    with Scheduler({"scoring_strategy": "MostAllocated",
                    "qos_strategies": {"Guaranteed": dict(scoring_strategy="RequestedToCapacityRatio",
                                                          shape=C.FALL30)}}) as s:
        assert s.get_scoring_strategy(0) == s.get_scoring_strategy(1) == ("MostAllocated", [])
        assert s.get_scoring_strategy(2) == ("RequestedToCapacityRatio", C.FALL30)
        assert ctypes.sizeof(_abi.QsScoringStrategy) == s.lib.qs_struct_size(6)
