"""GPU parity of required pod anti-affinity on the exact engines and the score path (spec/semantics.md
S12, qs_set_pod_anti_affinity): PERSISTENT and SCAN, every feature class and both row layouts,
qs_score_pod / qs_reserve / qs_unreserve, and the state across streams, save / restore and batched
mode, against tests/antiaffinity_ref.py bit for bit (placements, per-pod keys, the final table) plus
the anti-affinity invariant of qsched.checks.  The reference is pinned by spec/kat.md K27-K31 and
equals the batched oracle with batch = 1 (tests/test_antiaffinity_cpu.py).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import QschedError, Scheduler, _abi, checks, pods_from_struct, pods_to_struct  # noqa: E402

import antiaffinity_cases as C  # noqa: E402
import antiaffinity_ref as A  # noqa: E402
from test_gpu_parity import assert_same, run_oracle  # noqa: E402


def run_tracked(nodes, pods, cfg, engine, track=True):
    with Scheduler(dict(cfg, engine=engine)) as s:
        if track:
            s.set_pod_anti_affinity(True)
            assert s.get_pod_anti_affinity() is True
        s.load_nodes(nodes)
        st = s.prepare(pods)
        stats = st.run()
        pl, keys = st.results()
        st.free()
        final = s.read_nodes()
    return pl, keys, final, stats


def check_case(case, g):
    assert_same(g[:2], (case["pl"], case["keys"]), g[2], case["final"])
    inv = checks.batched_invariants(case["nodes"], A.pods_dict(case["pods"]), g[0], g[2])
    assert inv["anti_affinity"], inv


@pytest.mark.parametrize("name", list(C.PARITY))
def test_parity(name):
    case = C.parity_case(name)
    C.check_conditions(case)  # from the reference alone, before the GPU runs
    g = run_tracked(case["nodes"], case["pods"], case["cfg"], case["engine"])
    check_case(case, g)
    assert g[3]["engine_used"] == case["runs"], g[3]["engine_used"]
    assert g[3]["table_layout"] == ("wide" if "wide" in case["flags"] else "compact")


@pytest.mark.parametrize("name", ["persistent-24", "persistent-1100", "norm-persistent", "most-persistent"])
def test_scan_agrees_on_persistent_inputs(name):
    """The same inputs on the other engine (PERSISTENT inputs through SCAN)."""
    case = C.parity_case(name)
    g = run_tracked(case["nodes"], case["pods"], case["cfg"], "scan")
    check_case(case, g)
    assert g[3]["engine_used"] == "scan"


# ---- known answers -------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["persistent", "scan"])
@pytest.mark.parametrize("name", ["K27", "K28", "K29", "K30"])
def test_kat_streams(name, engine):
    nodes, pods, cfg, want_pl, want_tot = C.kat(name)
    pl, keys, final, _ = run_tracked(nodes, pods_to_struct(pods), cfg, engine)
    assert list(pl) == want_pl
    assert [int(k) for k in keys] == [((t + 1) << 32) | (0xFFFFFFFF - n) if n >= 0 else 0
                                      for t, n in zip(want_tot, want_pl)]


@pytest.mark.parametrize("name", ["K27", "K28", "K29", "K30"])
def test_kat_score_path(name):
    """The same cases pod by pod through qs_score_pod + qs_reserve."""
    nodes, pods, cfg, want_pl, want_tot = C.kat(name)
    sp = pods_to_struct(pods)
    with Scheduler(cfg) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        for j, (n, t) in enumerate(zip(want_pl, want_tot)):
            got = s.score_pod(sp[j])
            assert got["best"] == n
            if n >= 0:
                assert got["total"][n] == t
                s.reserve(n, sp[j])
            else:
                assert not got["feasible"].any() and (got["total"] == -1).all()


def _score_matches(s, nodes, pods, sp, j, state, cfg):
    """qs_score_pod / qs_score_pod_packed of pod j against the reference under `state`."""
    k = A.pod_keys(nodes, pods, j, state, cfg)
    feas = k != 0
    best = int(0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)) if feas.any() else -1
    got = s.score_pod(sp[j])
    assert np.array_equal(got["feasible"], feas)
    assert got["best"] == best
    assert np.array_equal(got["total"], np.where(feas, (k >> np.uint64(32)).astype(np.int64) - 1, -1))
    assert (got["scores"][~feas] == 0).all()
    bp, packed = s.score_pod_packed(sp[j])
    assert bp == best and np.array_equal(packed != 0xFFFFFFFF, feas)
    return best


def test_kat_k31_unreserve_reopens():
    nodes, pods, cfg, _, _ = C.kat("K31")
    sp = pods_to_struct(pods)
    st = A.State(nodes["zone"])
    with Scheduler(cfg) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        for node, sign, want in C.K31_STEPS:
            (s.reserve if sign > 0 else s.unreserve)(node, sp[0])
            assert st.record(4, node, sign)
            A.reserve(nodes, pods, 0, node, sign)
            for j in (0, 1):
                assert _score_matches(s, nodes, pods, sp, j, st, cfg) == (want[0] if want else -1)
                assert list(np.flatnonzero(s.score_pod(sp[j])["feasible"])) == want
        with pytest.raises(QschedError) as e:
            s.unreserve(0, sp[0])
        assert e.value.status == _abi.QS_EINVAL and "recorded" in str(e.value)
        assert _score_matches(s, nodes, pods, sp, 0, st, cfg) == 0  # ... and nothing changed
        final = s.read_nodes()
        for k in nodes:
            assert np.array_equal(final[k], nodes[k]), k


# ---- state ---------------------------------------------------------------------------------------
def test_two_streams_equal_one_run_over_the_concatenation():
    case = C.parity_case("persistent-300")
    nodes, pods = case["nodes"], case["pods"]
    cfg = dict(qos_sort=0)  # arrival order: the concatenation's order is the two streams' orders
    ref = A.run(nodes, pods, cfg)
    half = len(pods) // 2
    for engine in ("persistent", "scan"):
        pls, keys = [], []
        with Scheduler(dict(cfg, engine=engine)) as s:
            s.set_pod_anti_affinity(True)
            s.load_nodes(nodes)
            for part in (pods[:half], pods[half:]):
                st = s.prepare(part)
                st.run()
                a, b = st.results()
                st.free()
                pls.append(a)
                keys.append(b)
            final = s.read_nodes()
        assert_same((np.concatenate(pls), np.concatenate(keys)), ref[:2], final, ref[2])


def test_save_run_restore_run():
    case = C.parity_case("scan-700")
    nodes, pods = case["nodes"], case["pods"]
    first, rest = pods[:400], pods[400:]
    ref1 = A.run(nodes, first, {})
    ref2 = A.run(ref1[2], rest, {}, state=ref1[3])
    for engine in ("persistent", "scan"):
        with Scheduler(dict(engine=engine)) as s:
            s.set_pod_anti_affinity(True)
            s.load_nodes(nodes)
            a = s.prepare(first)
            a.run()
            assert np.array_equal(a.results()[0], ref1[0])
            s.save_table()
            b = s.prepare(rest)
            outs = []
            for _ in range(2):
                b.run()
                outs.append(b.results() + (s.read_nodes(),))
                s.restore_table()
            a.free()
            b.free()
            # the restored table and state take a Reserve / score as the reference after `first` does
            sp = pods_to_struct(rest)
            _score_matches(s, ref1[2], pods_from_struct(sp), sp, 0, ref1[3], {})
        for pl, keys, final in outs:
            assert_same((pl, keys), ref2[:2], final, ref2[2])


@pytest.mark.parametrize("engine", ["persistent", "scan"])
def test_relayout_rebuilds_the_state_from_the_mirror(engine):
    """A second stream with decimal memory requests re-lays the table out (compact -> wide): the device
    table is uploaded again from the host mirror, the recorded anti-affinity state with it (the path a
    recovery after a device fault takes too), so the second stream still sees the first one's pods."""
    case = C.parity_case("persistent-300")
    nodes, pods = case["nodes"], case["pods"]
    first, rest = pods[:600], pods[600:].copy()
    has = rest["req_mem"] > 0
    rest["req_mem"] = np.where(has, 100 * 10**6, 0)
    rest["nz_mem"] = np.where(has, 100 * 10**6, rest["nz_mem"])
    ref1 = A.run(nodes, first, {})
    ref2 = A.run(ref1[2], rest, {}, state=ref1[3])
    blind = A.run(ref1[2], rest, {})
    assert not np.array_equal(blind[0], ref2[0])  # an emptied state would place differently
    with Scheduler(dict(engine=engine)) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        a = s.prepare(first)
        sa = a.run()
        assert np.array_equal(a.results()[0], ref1[0]) and sa["table_layout"] == "compact"
        a.free()
        b = s.prepare(rest)
        sb = b.run()
        pl, keys = b.results()
        b.free()
        final = s.read_nodes()
    assert sb["table_layout"] == "wide"
    assert_same((pl, keys), ref2[:2], final, ref2[2])


def test_batched_then_tracked_exact_stream():
    """A batched stream records into the same state: the exact stream after it sees its placements."""
    case = C.parity_case("persistent-300")
    nodes, pods = case["nodes"], case["pods"]
    first, rest = pods[:500], pods[500:]
    with Scheduler(dict(batch_pods=1)) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        a = s.prepare(first)
        a.run(mode="batched")
        bpl, bkeys = a.results()
        a.free()
        mid = s.read_nodes()
        b = s.prepare(rest)
        stats = b.run()
        pl, keys = b.results()
        b.free()
        final = s.read_nodes()
    ref1 = A.run(nodes, first, {})  # (batches of one: the S12 stream)
    assert_same((bpl, bkeys), ref1[:2], mid, ref1[2])
    ref2 = A.run(ref1[2], rest, {}, state=ref1[3])
    assert_same((pl, keys), ref2[:2], final, ref2[2])
    assert stats["engine_used"] == "persistent"
    blind = A.run(ref1[2], rest, {})  # the exact stream with an empty state places differently
    assert not np.array_equal(blind[0], ref2[0])


@pytest.mark.parametrize("cfg", [{}, C.CFG4, C.MOST], ids=["default", "norm", "most"])
def test_score_reserve_unreserve_interleaved(cfg):
    """qs_score_pod, qs_reserve and qs_unreserve interleaved, checked against the reference state after
    each call; two pods of one app share a node, so the bit must survive the first Unreserve."""
    nodes, pods = C.c4(300, 90, apps=6, zones=3)
    op = pods_from_struct(pods)
    scorer = A.strategy_scorer(cfg) if "scoring_strategy" in cfg else None
    ocfg = {k: v for k, v in cfg.items()}
    on = {k: v.copy() for k, v in nodes.items()}
    st = A.State(nodes["zone"])
    held = []
    with Scheduler(cfg) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)

        def score(j):
            k = A.pod_keys(on, op, j, st, ocfg, scorer)
            feas = k != 0
            best = int(0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)) if feas.any() else -1
            got = s.score_pod(pods[j])
            assert np.array_equal(got["feasible"], feas), j
            assert got["best"] == best
            assert np.array_equal(got["total"], np.where(feas, (k >> np.uint64(32)).astype(np.int64) - 1, -1))
            return best

        # two pods of one app on node 5, whatever their kind asks (Reserve does not filter)
        j0, j1 = [j for j in range(90) if op["app"][j] == op["app"][0]][:2]
        for j in (j0, j1):
            s.reserve(5, pods[j])
            A.reserve(on, op, j, 5)
            st.record(int(op["app"][j]), 5)
        score(j0)
        s.unreserve(5, pods[j0])
        A.reserve(on, op, j0, 5, -1)
        st.record(int(op["app"][j0]), 5, -1)
        assert st.presence()[int(op["app"][j0]), 5]
        for j in range(90):
            if op["app"][j] == op["app"][j0]:
                score(j)  # HOSTNAME pods of the app still see node 5 taken, ZONE pods its zone
        for j in range(2, 90):
            b = score(j)
            if b >= 0:
                s.reserve(b, pods[j])
                A.reserve(on, op, j, b)
                st.record(int(op["app"][j]), b)
                held.append((j, b))
            if j % 7 == 0 and held:
                u, node = held.pop(len(held) // 2)
                s.unreserve(node, pods[u])
                A.reserve(on, op, u, node, -1)
                assert st.record(int(op["app"][u]), node, -1)
                score(u)
        final = s.read_nodes()
    for k in on:
        assert np.array_equal(final[k], on[k]), k


# ---- interface -----------------------------------------------------------------------------------
def test_tracking_off_changes_nothing(oracle):
    case = C.parity_case("persistent-300")
    nodes, pods = case["nodes"], case["pods"]
    o = run_oracle(oracle, nodes, pods, {})
    for engine in ("persistent", "scan", "lookahead"):
        never = run_tracked(nodes, pods, {}, engine, track=False)
        with Scheduler(dict(engine=engine)) as s:
            s.set_pod_anti_affinity(True)
            s.set_pod_anti_affinity(False)
            assert s.get_pod_anti_affinity() is False
            s.load_nodes(nodes)
            st = s.prepare(pods)
            stats = st.run()
            off = st.results() + (s.read_nodes(),)
            idx, counts = st.fit_errors()  # FitError works with tracking off
            assert len(idx) == int((off[0] < 0).sum())
            st.free()
        assert_same(off[:2], never[:2], off[2], never[2])
        assert_same(off[:2], o[:2], off[2], o[2])
        assert stats["engine_used"] == engine
    assert not np.array_equal(o[0], case["pl"])


def _raises(status, word, fn, *a, **k):
    with pytest.raises(QschedError) as e:
        fn(*a, **k)
    assert e.value.status == status, e.value
    assert word in str(e.value), str(e.value)


def test_interface_errors():
    case = C.parity_case("persistent-300")
    nodes, pods = case["nodes"], case["pods"]
    with Scheduler({}) as s:
        lib = s.lib
        s.load_nodes(nodes)
        st = s.prepare(pods)
        _raises(_abi.QS_ESTATE, "prepared", s.set_pod_anti_affinity, True)  # a prepared stream pins it
        st.free()
        assert lib.qs_get_pod_anti_affinity(s.ctx, None) == _abi.QS_EINVAL
        assert lib.qs_last_error(s.ctx)
        s.set_pod_anti_affinity(True)
        st = s.prepare(pods)
        st.run()
        _raises(_abi.QS_EINVAL, "anti-affinity", st.fit_errors, np.array([0], np.uint32))
        _raises(_abi.QS_EINVAL, "anti-affinity", st.fit_errors, np.array([0], np.uint32), by_taint=True)
        pl, _ = st.results()
        st.free()
        # a node that holds recorded pods keeps its zone; any other change of the row is fine
        node = int(pl[pl >= 0][0])
        final = s.read_nodes()
        row = {f: final[f][node] for f in final}
        s.upsert(node, dict(row, max_pods=int(row["max_pods"]) + 1))
        _raises(_abi.QS_EINVAL, "zone", s.upsert, node, dict(row, zone=(int(row["zone"]) + 1) % 4))
    for engine in ("lookahead", "allreduce"):
        with Scheduler(dict(engine=engine)) as s:
            s.set_pod_anti_affinity(True)
            s.load_nodes(nodes)
            st = s.prepare(pods)
            _raises(_abi.QS_EINVAL, "anti-affinity", st.run)
            st.free()
    with Scheduler(dict(virtual_shards=2)) as s:
        _raises(_abi.QS_EINVAL, "unsharded", s.set_pod_anti_affinity, True)
    with Scheduler({}, shard=(0, 2, None)) as s:
        _raises(_abi.QS_EINVAL, "unsharded", s.set_pod_anti_affinity, True)


def test_table_that_keeps_no_anti_affinity_state(oracle):
    """More than 2^20 nodes: the table allocation carries no presence bits and no zone counts.  Switching
    tracking on after the load is refused at the setter; switched on before the load (no table to ask
    yet), every call that would filter or record is refused instead.  Each refusal leaves a message and
    changes nothing: the rows stay as loaded, and with tracking off again the context schedules as one
    that never heard of the call."""
    n = (1 << 20) + 1
    nodes, _ = oracle.empty_cluster(n, 0)
    nodes["alloc_cpu"][:], nodes["alloc_mem"][:], nodes["max_pods"][:] = 8000, 16 * C.GIB, 110
    nodes["zone"][:] = np.arange(n) % 4
    pods = pods_to_struct(C._pods([(2, 7, A.HOSTNAME), (2, 7, A.ZONE), (2, 7, A.HOSTNAME)]))
    with Scheduler({}) as s:
        s.load_nodes(nodes)
        _raises(_abi.QS_EINVAL, "2^20", s.set_pod_anti_affinity, True)
        assert s.get_pod_anti_affinity() is False
        assert s.score_pod(pods[0], outputs=False)["best"] == 0  # untracked calls are unaffected
    with Scheduler({}) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        assert s.get_pod_anti_affinity() is True
        st = s.prepare(pods)
        _raises(_abi.QS_EINVAL, "2^20", st.run)
        _raises(_abi.QS_EINVAL, "2^20", st.run, mode="batched")
        st.free()
        _raises(_abi.QS_EINVAL, "2^20", s.reserve, 0, pods[0])
        _raises(_abi.QS_EINVAL, "2^20", s.unreserve, 0, pods[0])
        _raises(_abi.QS_EINVAL, "2^20", s.score_pod, pods[0], outputs=False)
        final = s.read_nodes()
        for k in nodes:
            assert np.array_equal(final[k], nodes[k]), k
        s.set_pod_anti_affinity(False)
        s.reserve(0, pods[0])      # plain Reserve / Unreserve: no app bookkeeping is asked for
        s.unreserve(0, pods[0])
        pl = s.schedule(pods)
    o = run_oracle(oracle, nodes, pods, {})
    assert np.array_equal(pl, o[0])
