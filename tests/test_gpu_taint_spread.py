"""GPU parity of ``nodeTaintsPolicy: Honor`` of the topology spread constraints (spec/semantics.md S17,
qs_set_topology_spread_node_taints_policy) on the SCAN engine and the score path, against
tests/taint_spread_ref.py bit for bit: placements, per-pod keys and the final table of streams that mix the
three spread kinds, in both layouts, with the plugins' scores idle and at work, alone and together with
nodeAffinityPolicy Honor; qs_score_pod / qs_score_pod_packed / qs_score_pod_zone_scores across qs_reserve /
qs_unreserve; streams whose pods tolerate everything; save / restore; a taint upserted between prepare and
run; and the refusals.  The reference is pinned by spec/kat.md K53-K58 (tests/test_taint_spread_cpu.py), which
also checks the conditions on the inputs used here.

Shapes: 24 nodes are one partial wave of the count pass, 64 / 65 nodes the last full wave and one node more,
130 nodes a partial third wave, 300 nodes two workgroups (the second partial), so the cross-workgroup atomics
and the reset are exercised; zone ids 0, 5 and 63; taint bits 2 and 40.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import QschedError, Scheduler, _abi, pods_from_struct, pods_to_struct  # noqa: E402

import antiaffinity_ref as A  # noqa: E402
import taint_spread_cases as TC  # noqa: E402
import taint_spread_ref as TR  # noqa: E402
from test_gpu_parity import assert_same  # noqa: E402

NAMES = {TR.IGNORE: "ignore", TR.HONOR: "honor"}


def _open(cfg, engine, taints="honor", affinity=TR.IGNORE):
    s = Scheduler(dict(cfg, engine=engine))
    s.set_pod_anti_affinity(True)
    s.set_topology_spread_node_affinity_policy(NAMES.get(affinity, affinity))
    s.set_topology_spread_node_taints_policy(NAMES.get(taints, taints))
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
@pytest.mark.parametrize("engine", ["scan", "auto", "scan-soa"])
@pytest.mark.parametrize("name", list(TC.PARITY))
def test_parity(name, engine):
    """SCAN, AUTO (which must pick SCAN: the stream holds restricting pods) and SCAN on a context that keeps
    the column-major copy."""
    case = TC.parity_case(name)
    cfg = dict(case["cfg"], scan_soa_min_nodes=1) if engine == "scan-soa" else case["cfg"]
    with _open(cfg, engine.split("-")[0], affinity=case["policy"]) as s:
        assert s.get_topology_spread_node_taints_policy() == _abi.QS_POLICY_HONOR
        assert s.get_topology_spread_node_affinity_policy() == case["policy"]
        s.load_nodes(case["nodes"])
        pl, keys, stats = _stream(s, case["pods"])
        final = s.read_nodes()
    assert_same((pl, keys), (case["pl"], case["keys"]), final, case["final"])
    assert stats["engine_used"] == "scan", stats["engine_used"]
    assert stats["table_layout"] == ("wide" if case["wide"] else "compact")


@pytest.mark.parametrize("name", TC.KATS)
def test_kat_streams(name):
    nodes, pods, cfg, policy, honor, ignore = TC.kat(name)
    for taints, want in ((TR.HONOR, honor), (TR.IGNORE, ignore)):
        ref = TR.run(nodes, pods, cfg, policy=policy, taints_policy=taints)
        assert list(ref[0]) == want
        with _open(cfg, "scan", taints, policy) as s:
            s.load_nodes(nodes)
            pl, keys, _ = _stream(s, pods_to_struct(pods))
        assert list(pl) == want, taints
        assert np.array_equal(keys, ref[1]), taints


# ---- the score path ------------------------------------------------------------------------------
def _score_matches(s, nodes, pods, sp, j, state, cfg):
    """qs_score_pod / qs_score_pod_packed / qs_score_pod_zone_scores of pod j against the reference."""
    k = TR.pod_keys(nodes, pods, j, state, cfg)
    feas = k != 0
    best = int(0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)) if feas.any() else -1
    zs = TR.pod_zone_scores(nodes, pods, j, state, cfg)
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


@pytest.mark.parametrize("n,both,norm,wide", [(24, False, False, False), (65, False, True, True),
                                              (130, True, True, False), (300, False, False, False),
                                              (300, True, False, True)])
def test_score_reserve_unreserve_interleaved_then_a_stream(n, both, norm, wide):
    """qs_score_pod of every pod (the three spread kinds alternate in the input) across qs_reserve /
    qs_unreserve steps, each call against the reference state; then a stream on the same context: a word of
    the count pass left behind by the score path (or the other way round) would show in either."""
    P = 90
    nodes, pods = TC.cluster(n, P + 60, both, norm, wide)
    cfg = dict(TC.NORM if (both or norm) else TC.TAINT)
    policy = TR.HONOR if both else TR.IGNORE
    op = pods_from_struct(pods)
    on = {k: v.copy() for k, v in nodes.items()}
    st = TR.state_of(nodes, policy)
    rs = np.flatnonzero(TC.restricting(pods, both)[:P])
    kinds = {int(k) & ~0x1F00 for k in pods["anti_affinity"][rs]}
    assert len(rs) >= 30 and len(kinds) == 3  # SPREAD, SPREAD_SOFT and SPREAD_HOSTNAME among them
    held = []
    with _open(cfg, "auto", affinity=policy) as s:
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
        ref = TR.run(on, pods[P:], cfg, state=st)
        pl, keys, stats = _stream(s, pods[P:])
        assert_same((pl, keys), ref[:2], s.read_nodes(), ref[2])
        assert stats["engine_used"] == "scan"
        # ... and the score path again behind the stream
        tail = pods_from_struct(pods[P:])
        for j in range(0, 60, 7):
            _score_matches(s, ref[2], tail, pods[P:], j, ref[3], cfg)


# ---- streams whose spread pods tolerate everything -----------------------------------------------
def test_a_stream_whose_spread_pods_tolerate_everything_runs_persistent():
    """No spread pod restricts: the stream is dispatched as before the policy existed (PERSISTENT under AUTO),
    under either policy, and equals the reference under Ignore."""
    nodes, pods = TC.cluster(300, 300)
    pods = pods.copy()
    pods["tol_hard"][TC.spreads(pods)] = TC.ALL
    # (soft and hostname pods in one stream run SCAN whatever the policy, spec S15: keep the soft apps plain)
    pods["anti_affinity"][(pods["anti_affinity"] & (1 << 16)) != 0] = A.NONE
    got = {}
    for taints in ("honor", "ignore"):
        with _open(TC.TAINT, "auto", taints) as s:
            s.load_nodes(nodes)
            pl, keys, stats = _stream(s, pods)
            got[taints] = (pl, keys, s.read_nodes())
            assert stats["engine_used"] == "persistent", (taints, stats["engine_used"])
    assert_same(got["honor"][:2], got["ignore"][:2], got["honor"][2], got["ignore"][2])
    ref = TR.run(nodes, pods, TC.TAINT, taints_policy=TR.IGNORE)
    assert_same(got["honor"][:2], ref[:2], got["honor"][2], ref[2])
    assert (nodes["taint_hard"][ref[0][ref[0] >= 0]] != 0).any()  # the tainted pool is in use


# ---- save / restore between two streams ----------------------------------------------------------
def test_save_restore_between_two_streams():
    case = TC.parity_case("both-130-norm")
    nodes, pods, cfg, policy = case["nodes"], case["pods"], case["cfg"], case["policy"]
    a, b = pods[:200], pods[200:]
    ref_a = TR.run(nodes, a, cfg, policy=policy)
    ref_b = TR.run(ref_a[2], b, cfg, state=ref_a[3])
    with _open(cfg, "auto", affinity=policy) as s:
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


# ---- a taint upserted between prepare and run ----------------------------------------------------
def test_a_taint_upserted_between_prepare_and_run():
    """K54's table without its taints: no node carries a hard taint when the stream is prepared, so M_T is every
    node for every pod.  Then nodes 2 and 3 (all of zone 2) get a taint the pods do not tolerate.  The run
    must see the table as it stands: zone 2 is no domain and the third pod is placed; a record resolved
    against the table at prepare would strand it."""
    nodes, pods, cfg, policy, honor, stranded = TC.kat("K54")
    clean = {k: v.copy() for k, v in nodes.items()}
    clean["taint_hard"][:] = 0
    sp = pods_to_struct(pods)
    with _open(cfg, "auto") as s:
        s.load_nodes(clean)
        st = s.prepare(sp)
        for i in (2, 3):
            s.upsert(i, {f: nodes[f][i] for f in nodes})
        try:
            stats = st.run()
        except QschedError as e:  # a refusal must say why
            assert e.status in (_abi.QS_ESTATE, _abi.QS_EINVAL) and "taint" in str(e)
            return
        pl, keys = st.results()
        ref = TR.run(nodes, pods, cfg)
        assert list(ref[0]) == honor and honor != stranded
        assert_same((pl, keys), ref[:2], s.read_nodes(), ref[2])
        assert stats["engine_used"] == "scan"
        st.free()


# ---- refusals ------------------------------------------------------------------------------------
def test_refusals():
    case = TC.parity_case("pool-24")
    nodes, pods, cfg = case["nodes"], case["pods"], case["cfg"]
    # (soft and hostname pods in one stream are refused by PERSISTENT whatever the policy, spec S15: without
    # the soft pods the restricting pods are the only reason left)
    hard = pods.copy()
    hard["anti_affinity"][(hard["anti_affinity"] & (1 << 16)) != 0] = A.NONE
    assert TC.restricting(hard).sum() >= 50
    with _open(cfg, "persistent") as s:
        s.load_nodes(nodes)
        st = s.prepare(hard)
        _raises(_abi.QS_EINVAL, "nodeTaintsPolicy Honor", st.run)
        assert all(np.array_equal(s.read_nodes()[k], nodes[k]) for k in nodes)
        _raises(_abi.QS_ESTATE, "prepared streams", s.set_topology_spread_node_taints_policy, "ignore")
        st.free()
        for bad in (2, -1, 7):
            _raises(_abi.QS_EINVAL, "QS_POLICY", s.set_topology_spread_node_taints_policy, bad)
        assert s.get_topology_spread_node_taints_policy() == _abi.QS_POLICY_HONOR
        # an explicit PERSISTENT serves the stream once its spread pods tolerate every bit
        plain = pods.copy()
        plain["tol_hard"][TC.spreads(plain)] = TC.ALL
        plain["anti_affinity"][(plain["anti_affinity"] & (1 << 16)) != 0] = A.NONE
        assert _stream(s, plain)[2]["engine_used"] == "persistent"
    with Scheduler(dict(enable_taint=0, enable_affinity=1)) as s:
        assert s.get_topology_spread_node_taints_policy() == _abi.QS_POLICY_IGNORE
        _raises(_abi.QS_EINVAL, "enable_taint", s.set_topology_spread_node_taints_policy, "honor")
        s.set_topology_spread_node_taints_policy("ignore")
        assert s.get_topology_spread_node_taints_policy() == _abi.QS_POLICY_IGNORE
    # 16-bit counts: a table that holds a node with max_pods 70,000 refuses the restricting pod, and serves one
    # that tolerates every bit
    with _open(cfg, "auto") as s:
        big = {k: v.copy() for k, v in nodes.items()}
        big["max_pods"][5] = 70000
        s.load_nodes(big)
        rs = pods[TC.restricting(pods)]
        _raises(_abi.QS_EINVAL, "65535", s.score_pod, rs[0])
        st = s.prepare(pods)
        _raises(_abi.QS_EINVAL, "65535", st.run)
        st.free()
        free = rs[:1].copy()
        free["tol_hard"] = TC.ALL
        free["anti_affinity"] = TC.SP1
        assert s.score_pod(free[0])["best"] >= 0


def test_tracking_off_ignores_the_policy():
    """The policy is read on a context that tracks only: with tracking off no record carries the bit and the
    stream runs where it ran before (PERSISTENT serves it)."""
    case = TC.parity_case("pool-64")
    got = {}
    for taints in ("honor", "ignore"):
        with Scheduler(dict(case["cfg"], engine="persistent")) as s:
            s.set_topology_spread_node_taints_policy(taints)
            s.load_nodes(case["nodes"])
            pl, keys, stats = _stream(s, case["pods"])
            got[taints] = (pl, keys, s.read_nodes())
            assert stats["engine_used"] == "persistent"
    assert_same(got["honor"][:2], got["ignore"][:2], got["honor"][2], got["ignore"][2])
    assert not np.array_equal(got["honor"][0], case["pl"])
