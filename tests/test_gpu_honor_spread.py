"""GPU parity of ``nodeAffinityPolicy: Honor`` of the topology spread constraints (spec/semantics.md S16,
qs_set_topology_spread_node_affinity_policy) on the SCAN engine and the score path, against
tests/honor_spread_ref.py bit for bit: placements, per-pod keys and the final table of streams of the three
spread kinds in both layouts and both scoring classes; qs_score_pod / qs_score_pod_zone_scores across
qs_reserve / qs_unreserve; streams without restricting pods; a policy switched between streams; an
appended node in a new zone, save / restore; and the refusals.  The reference is pinned by spec/kat.md
K48-K52 (tests/test_honor_spread_cpu.py), which also checks the conditions on the inputs used here.

Shapes: 70 nodes are one 256-thread workgroup of the count pass whose last wave is partial; 300 nodes two
workgroups, the second partial, so the cross-workgroup atomics and the reset are exercised; zone ids 0, 5
and 63.  The score path's workgroups hold 1,024 nodes: 1,100 nodes make two of them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import QschedError, Scheduler, _abi, pods_from_struct, pods_to_struct  # noqa: E402

import antiaffinity_ref as A  # noqa: E402
import honor_spread_cases as HC  # noqa: E402
import honor_spread_ref as HR  # noqa: E402
from test_gpu_parity import assert_same, run_oracle  # noqa: E402


def _open(cfg, engine, policy="honor"):
    s = Scheduler(dict(cfg, engine=engine))
    s.set_pod_anti_affinity(True)
    s.set_topology_spread_node_affinity_policy(policy)
    return s


def _stream(s, pods):
    st = s.prepare(pods)
    stats = st.run()
    pl, keys = st.results()
    st.free()
    return pl, keys, stats


def _raises(status, word, fn, *a, **k):
    with pytest.raises(QschedError) as e:
        fn(*a, **k)
    assert e.value.status == status, e.value
    assert word in str(e.value), str(e.value)


# ---- parity --------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["scan", "auto"])
@pytest.mark.parametrize("name", list(HC.PARITY))
def test_parity(name, engine):
    case = HC.parity_case(name)
    with _open(case["cfg"], engine) as s:
        assert s.get_topology_spread_node_affinity_policy() == _abi.QS_POLICY_HONOR
        s.load_nodes(case["nodes"])
        pl, keys, stats = _stream(s, case["pods"])
        final = s.read_nodes()
    assert_same((pl, keys), (case["pl"], case["keys"]), final, case["final"])
    assert stats["engine_used"] == "scan", stats["engine_used"]
    assert stats["table_layout"] == ("wide" if case["wide"] else "compact")


@pytest.mark.parametrize("name", ["K48", "K49", "K50", "K51", "K52"])
def test_kat_streams(name):
    nodes, pods, cfg, honor, ignore = HC.kat(name)
    for policy, want in (("honor", honor), ("ignore", ignore)):
        ref = HR.run(nodes, pods, cfg, policy=HR.HONOR if policy == "honor" else HR.IGNORE)
        assert list(ref[0]) == want
        with _open(cfg, "scan", policy) as s:
            s.load_nodes(nodes)
            pl, keys, _ = _stream(s, pods_to_struct(pods))
        assert list(pl) == want, policy
        assert np.array_equal(keys, ref[1]), policy


# ---- the score path ------------------------------------------------------------------------------
def _score_matches(s, nodes, pods, sp, j, state, cfg):
    """qs_score_pod / qs_score_pod_packed / qs_score_pod_zone_scores of pod j against the reference."""
    k = HR.pod_keys(nodes, pods, j, state, cfg)
    feas = k != 0
    best = int(0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)) if feas.any() else -1
    zs = HR.pod_zone_scores(nodes, pods, j, state, cfg)
    got = s.score_pod(sp[j])
    assert np.array_equal(got["feasible"], feas), j
    assert got["best"] == best, j
    assert np.array_equal(got["total"], np.where(feas, (k >> np.uint64(32)).astype(np.int64) - 1, -1)), j
    assert (got["scores"][~feas] == 0).all()
    assert np.array_equal(got["zone_scores"], zs), (j, got["zone_scores"], zs)
    bp, packed = s.score_pod_packed(sp[j])
    assert bp == best and np.array_equal(packed != 0xFFFFFFFF, feas)
    assert np.array_equal(s.score_pod_zone_scores(), zs)
    return best


@pytest.mark.parametrize("kind,n,norm,wide", [("spread", 70, False, False), ("soft", 70, True, False),
                                              ("host", 70, False, True), ("spread", 300, True, True),
                                              ("soft", 300, False, False), ("host", 300, True, False),
                                              ("spread", 1100, False, False), ("soft", 1100, True, False),
                                              ("host", 1100, True, True)])
def test_score_reserve_unreserve_interleaved_then_a_stream(kind, n, norm, wide):
    """qs_score_pod of every pod across qs_reserve / qs_unreserve steps, each call against the reference
    state; then a stream on the same context: a word of the count pass left behind by the score path (or
    the other way round) would show in either."""
    P = 90
    nodes, pods = HC.cluster(n, P + 60, kind, norm, wide)
    cfg = dict(HC.NORM if norm else HC.AFF)
    op = pods_from_struct(pods)
    on = {k: v.copy() for k, v in nodes.items()}
    st = HR.HonorState(nodes["zone"], nodes["label_bits"])
    rs = np.flatnonzero(HC.restricting(pods)[:P])
    assert len(rs) >= 30
    held = []
    with _open(cfg, "auto") as s:
        s.load_nodes(nodes)
        for step, j in enumerate(range(P)):
            b = _score_matches(s, on, op, pods, j, st, cfg)
            if b >= 0:
                s.reserve(b, pods[j])
                A.reserve(on, op, j, b)
                st.record(int(op["app"][j]), b)
                held.append((j, b))
            if step % 5 == 4 and held:
                u, node = held.pop(len(held) // 2)
                s.unreserve(node, pods[u])
                A.reserve(on, op, u, node, -1)
                assert st.record(int(op["app"][u]), node, -1)
                _score_matches(s, on, op, pods, int(rs[step % len(rs)]), st, cfg)
        mid = s.read_nodes()
        for k in on:
            assert np.array_equal(mid[k], on[k]), k
        ref = HR.run(on, pods[P:], cfg, state=st)
        pl, keys, stats = _stream(s, pods[P:])
        assert_same((pl, keys), ref[:2], s.read_nodes(), ref[2])
        assert stats["engine_used"] == "scan"
        # ... and the score path again behind the stream
        tail = pods_from_struct(pods[P:])
        for j in range(0, 60, 7):
            _score_matches(s, ref[2], tail, pods[P:], j, ref[3], cfg)


# ---- streams without restricting pods ------------------------------------------------------------
@pytest.mark.parametrize("kind", HC.KINDS)
def test_a_stream_without_restricting_pods_runs_as_under_ignore(kind):
    nodes, pods = HC.cluster(300, 300, kind)
    pods = pods.copy()
    pods["sel"][:] = 0
    pods["n_req_terms"][:] = 0
    got = {}
    for policy in ("honor", "ignore"):
        with _open(HC.AFF, "auto", policy) as s:
            s.load_nodes(nodes)
            pl, keys, stats = _stream(s, pods)
            got[policy] = (pl, keys, s.read_nodes())
            assert stats["engine_used"] == "persistent", (policy, stats["engine_used"])
    assert_same(got["honor"][:2], got["ignore"][:2], got["honor"][2], got["ignore"][2])
    ref = HR.run(nodes, pods, HC.AFF)
    assert_same(got["honor"][:2], ref[:2], got["honor"][2], ref[2])


def test_tracking_off_ignores_the_policy(oracle):
    """The policy is read on a context that tracks only: with tracking off the stream is the plain oracle's,
    on whatever engine AUTO picks, as it was before the policy existed."""
    case = HC.parity_case("spread-300-default-compact")
    o = run_oracle(oracle, case["nodes"], case["pods"], case["cfg"])
    for engine in ("auto", "persistent", "scan"):
        with Scheduler(dict(case["cfg"], engine=engine)) as s:
            s.set_topology_spread_node_affinity_policy("honor")
            s.load_nodes(case["nodes"])
            pl, keys, stats = _stream(s, case["pods"])
            assert_same((pl, keys), o[:2], s.read_nodes(), o[2])
            assert engine == "auto" or stats["engine_used"] == engine
    assert not np.array_equal(o[0], case["pl"])


# ---- the policy switched between two streams -----------------------------------------------------
@pytest.mark.parametrize("first", ["honor", "ignore"])
def test_policy_switched_between_streams(first):
    case = HC.parity_case("spread-300-default-compact")
    nodes, pods, cfg = case["nodes"], case["pods"], case["cfg"]
    a, b = pods[:200], pods[200:]
    pol = {"honor": HR.HONOR, "ignore": HR.IGNORE}
    second = "ignore" if first == "honor" else "honor"
    ref_a = HR.run(nodes, a, cfg, policy=pol[first])
    st = ref_a[3].copy()
    st.policy = pol[second]
    ref_b = HR.run(ref_a[2], b, cfg, state=st)
    st.policy = pol[first]
    assert not np.array_equal(ref_b[0], HR.run(ref_a[2], b, cfg, state=st)[0])  # the switch shows
    with _open(cfg, "auto", first) as s:
        s.load_nodes(nodes)
        sa = s.prepare(a)
        _raises(_abi.QS_ESTATE, "prepared streams", s.set_topology_spread_node_affinity_policy, second)
        sa.run()
        assert_same(sa.results(), ref_a[:2], s.read_nodes(), ref_a[2])
        sa.free()
        s.set_topology_spread_node_affinity_policy(second)
        assert s.get_topology_spread_node_affinity_policy() == pol[second]
        pl, keys, _ = _stream(s, b)
        assert_same((pl, keys), ref_b[:2], s.read_nodes(), ref_b[2])


# ---- table changes -------------------------------------------------------------------------------
def test_appended_node_in_a_new_zone_and_save_restore():
    """K48's table after its stream: cH = (2, 1) over the domains {0, 1}, m = 1.  A qs_node_upsert appends a
    node that matches the selector in a new zone: the domain appears and the minimum drops to 0.  Then the
    parity input around qs_table_save / qs_table_restore."""
    nodes, pods, cfg, honor, _ = HC.kat("K48")
    sp = pods_to_struct(pods)
    ref = HR.run(nodes, pods, cfg)
    with _open(cfg, "scan") as s:
        s.load_nodes(nodes)
        pl, _, _ = _stream(s, sp)
        assert list(pl) == honor
        assert list(np.flatnonzero(s.score_pod(sp[0])["feasible"])) == [1]
        grown = {k: np.concatenate([v, v[:1]]) for k, v in ref[2].items()}
        for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "pods"):
            grown[f][3] = 0
        grown["req_ext"][3] = 0
        grown["zone"][3] = 7
        st = ref[3].copy()
        st.set_table(grown["zone"], grown["label_bits"])
        s.upsert(3, {f: grown[f][3] for f in grown})
        assert list(np.flatnonzero(s.score_pod(sp[0])["feasible"])) == [3]
        _score_matches(s, grown, pods, sp, 0, st, cfg)
        ref_g = HR.run(grown, pods, cfg, state=st)
        assert list(ref_g[0]) == [3, 1, 3]  # cH = (2, 1, 0) -> (2, 1, 1) -> (2, 2, 1): zone 7 stays open
        pl, keys, _ = _stream(s, sp)
        assert_same((pl, keys), ref_g[:2], s.read_nodes(), ref_g[2])
    case = HC.parity_case("soft-300-norm-compact")
    nodes, pods, cfg = case["nodes"], case["pods"], case["cfg"]
    a, b = pods[:150], pods[150:]
    ref_a = HR.run(nodes, a, cfg)
    ref_b = HR.run(ref_a[2], b, cfg, state=ref_a[3])
    with _open(cfg, "auto") as s:
        s.load_nodes(nodes)
        pl, keys, _ = _stream(s, a)
        assert_same((pl, keys), ref_a[:2], s.read_nodes(), ref_a[2])
        s.save_table()
        sb = s.prepare(b)
        for _ in range(2):  # the same pods again from the restored state
            sb.run()
            assert_same(sb.results(), ref_b[:2], s.read_nodes(), ref_b[2])
            s.restore_table()
        ob = pods_from_struct(b)
        for j in range(0, 40, 3):
            _score_matches(s, ref_a[2], ob, b, j, ref_a[3], cfg)
        sb.free()


# ---- refusals ------------------------------------------------------------------------------------
def test_refusals():
    case = HC.parity_case("spread-70-default-compact")
    nodes, pods, cfg = case["nodes"], case["pods"], case["cfg"]
    with _open(cfg, "persistent") as s:
        s.load_nodes(nodes)
        st = s.prepare(pods)
        _raises(_abi.QS_EINVAL, "nodeAffinityPolicy Honor", st.run)
        assert all(np.array_equal(s.read_nodes()[k], nodes[k]) for k in nodes)
        _raises(_abi.QS_ESTATE, "prepared streams", s.set_topology_spread_node_affinity_policy, "ignore")
        st.free()
        for bad in (2, -1, 7):
            _raises(_abi.QS_EINVAL, "QS_POLICY", s.set_topology_spread_node_affinity_policy, bad)
        assert s.get_topology_spread_node_affinity_policy() == _abi.QS_POLICY_HONOR
        # an explicit PERSISTENT serves the stream once none of its spread pods restricts
        plain = pods.copy()
        plain["sel"][:] = 0
        plain["n_req_terms"][:] = 0
        assert _stream(s, plain)[2]["engine_used"] == "persistent"
    with Scheduler(dict(enable_affinity=0)) as s:
        assert s.get_topology_spread_node_affinity_policy() == _abi.QS_POLICY_IGNORE
        _raises(_abi.QS_EINVAL, "enable_affinity", s.set_topology_spread_node_affinity_policy, "honor")
        s.set_topology_spread_node_affinity_policy("ignore")
        assert s.get_topology_spread_node_affinity_policy() == _abi.QS_POLICY_IGNORE
    # 16-bit counts: once the context keeps them a node with max_pods 70,000 is refused, and a table that
    # holds one refuses the restricting pod
    with _open(cfg, "auto") as s:
        s.load_nodes(nodes)
        rs = pods[HC.restricting(pods) & ((pods["anti_affinity"] & 0xFF) == 3)]
        s.score_pod(rs[0])
        row = {f: nodes[f][1] for f in nodes}
        row["max_pods"] = 70000
        _raises(_abi.QS_EINVAL, "65535", s.upsert, 1, row)
    with _open(cfg, "auto") as s:
        big = {k: v.copy() for k, v in nodes.items()}
        big["max_pods"][5] = 70000
        s.load_nodes(big)
        _raises(_abi.QS_EINVAL, "65535", s.score_pod, rs[0])
        st = s.prepare(pods)
        _raises(_abi.QS_EINVAL, "65535", st.run)
        st.free()
        free = rs[:1].copy()  # ... and a pod that does not restrict is served
        free["sel"][:] = 0
        free["n_req_terms"][:] = 0
        free["anti_affinity"] = HC.SP1
        assert s.score_pod(free[0])["best"] >= 0
