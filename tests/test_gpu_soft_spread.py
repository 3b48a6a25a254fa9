"""GPU parity of zone topology spread scoring (spec/semantics.md S14, ``QS_AA_SPREAD_SOFT(max_skew)``) on
the exact engines and the score path: PERSISTENT and SCAN, every feature class and both row layouts,
qs_score_pod / qs_score_pod_zone_scores across qs_reserve / qs_unreserve, the shared spread-app cap of
PERSISTENT, the weight, and the state across streams, save / restore and a new zone, against
tests/soft_spread_ref.py bit for bit (placements, per-pod keys, the final table, and the recorded state
as later probe pods see it).  The reference is pinned by spec/kat.md K37-K41
(tests/test_soft_spread_cpu.py).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import QschedError, Scheduler, _abi, aa_spread, aa_spread_soft, pods_from_struct, pods_to_struct  # noqa: E402

import antiaffinity_cases as C  # noqa: E402
import antiaffinity_ref as A  # noqa: E402
import soft_spread_cases as SC  # noqa: E402
import soft_spread_ref as R  # noqa: E402
import spread_ref as S  # noqa: E402
from test_gpu_parity import assert_same, run_oracle  # noqa: E402


def _probe_pods(pods, app):
    """Four pods of `app` asking for nothing: soft (max_skew 1), SPREAD(1), ZONE, HOSTNAME."""
    p = pods[:4].copy()
    for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "req_ext", "n_req_terms", "n_pref_terms", "sel"):
        if f in p.dtype.names:
            p[f] = 0
    p["tol_hard"] = p["tol_soft"] = np.uint64(0xFFFFFFFFFFFFFFFF)
    p["app"] = app
    p["anti_affinity"] = [aa_spread_soft(1), aa_spread(1), A.ZONE, A.HOSTNAME]
    return p


def _score_matches(s, nodes, pods, sp, j, state, cfg, scorer=None):
    """qs_score_pod / qs_score_pod_packed / qs_score_pod_zone_scores of pod j against the reference."""
    k = R.pod_keys(nodes, pods, j, state, cfg, scorer)
    feas = k != 0
    best = int(0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)) if feas.any() else -1
    zs = R.pod_zone_scores(nodes, pods, j, state, cfg, scorer)
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


def check_state(s, pods, final, state, apps, cfg, scorer):
    """The recorded state through the score path: soft / SPREAD / ZONE / HOSTNAME probe pods of `apps`
    against the reference's final table and state (feasible sets, totals, zone scores)."""
    for app in apps:
        probe = _probe_pods(pods, int(app))
        op = pods_from_struct(probe)
        for j in range(4):
            _score_matches(s, final, op, probe, j, state, cfg, scorer)


def run_tracked(nodes, pods, cfg, engine, wpts=2, track=True, check=None):
    with Scheduler(dict(cfg, engine=engine)) as s:
        if track:
            s.set_pod_anti_affinity(True)
        assert s.get_topology_spread_weight() == 2  # a new context
        s.set_topology_spread_weight(wpts)
        assert s.get_topology_spread_weight() == wpts
        s.load_nodes(nodes)
        st = s.prepare(pods)
        stats = st.run()
        pl, keys = st.results()
        st.free()
        final = s.read_nodes()
        if check is not None:
            state, ocfg, scorer = check
            check_state(s, pods, final, state, np.unique(pods["app"])[:3], ocfg, scorer)
    return pl, keys, final, stats


@pytest.mark.parametrize("name", list(SC.PARITY))
def test_parity(name):
    case = SC.parity_case(name)
    SC.check_conditions(case)  # from the reference alone, before the GPU runs
    scorer = C.scorer_of(case["kind"], case["ocfg"])
    g = run_tracked(case["nodes"], case["pods"], case["cfg"], case["engine"], case["wpts"],
                    check=(case["state"], case["ocfg"], scorer))
    assert_same(g[:2], (case["pl"], case["keys"]), g[2], case["final"])
    assert g[3]["engine_used"] == case["runs"], g[3]["engine_used"]
    assert g[3]["table_layout"] == ("wide" if "wide" in case["flags"] else "compact")


@pytest.mark.parametrize("name", ["persistent-24", "persistent-65", "persistent-1100", "norm-persistent", "most-persistent",
                                  "wide-most-persistent", "wide-norm-persistent"])
def test_scan_agrees_on_persistent_inputs(name):
    case = SC.parity_case(name)
    g = run_tracked(case["nodes"], case["pods"], case["cfg"], "scan", case["wpts"])
    assert_same(g[:2], (case["pl"], case["keys"]), g[2], case["final"])
    assert g[3]["engine_used"] == "scan"


@pytest.mark.parametrize("name,wpts", SC.WEIGHTS)
def test_weights(name, wpts):
    """Wpts = 0 (the term vanishes; the pods are still not filtered) and 100, on inputs of the table above."""
    case = SC.parity_case(name)
    ref = SC.reference(case["nodes"], case["pods"], case["ocfg"], case["kind"], wpts=wpts)
    assert not np.array_equal(ref[0], case["pl"])
    g = run_tracked(case["nodes"], case["pods"], case["cfg"], case["engine"], wpts,
                    check=(ref[3], case["ocfg"], C.scorer_of(case["kind"], case["ocfg"])))
    assert_same(g[:2], ref[:2], g[2], ref[2])
    assert g[3]["engine_used"] == case["runs"]


@pytest.mark.parametrize("engine", ["persistent", "scan"])
@pytest.mark.parametrize("build", [lambda: SC.tiny(1), lambda: SC.tiny(2), lambda: SC.tiny(3),
                                   lambda: SC.one_pod_per_node(64, 100), lambda: SC.one_pod_per_node(65, 100)],
                         ids=["1-node", "2-nodes", "3-nodes", "max-pods-1-64", "max-pods-1-65"])
def test_small_tables(build, engine):
    """Tables of 1-3 nodes in the zones {0, 5, 63} (one and two nodes: D is the domain count throughout,
    so only parity is checked), and max_pods = 1 on 64 / 65 nodes (the feasible zones shrink to nothing)."""
    nodes, pods = build()
    ref = R.run(nodes, pods, SC.ARRIVAL)
    g = run_tracked(nodes, pods, SC.ARRIVAL, engine, check=(ref[3], SC.ARRIVAL, None))
    assert_same(g[:2], ref[:2], g[2], ref[2])
    assert (ref[0] >= 0).any()


# ---- known answers -------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["persistent", "scan"])
@pytest.mark.parametrize("name", ["K37", "K38", "K39", "K40"])
def test_kat_streams(name, engine):
    nodes, pods, cfg, want_pl, want_tot, want_last = SC.kat(name)
    sp = pods_to_struct(pods)
    with Scheduler(dict(cfg, qos_sort=0, engine=engine)) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        first = s.prepare(sp[:-1])
        first.run()
        first.free()
        got = s.score_pod(sp[-1])  # the last pod on the score path: every node's total
        assert list(got["total"]) == want_last
        st = s.prepare(sp[-1:])
        st.run()
        pl, keys = st.results()
        st.free()
    assert int(pl[0]) == want_pl[-1] and int(keys[0]) == ((want_tot[-1] + 1) << 32) | (0xFFFFFFFF - want_pl[-1])
    pl, keys, _, _ = run_tracked(nodes, sp, dict(cfg, qos_sort=0), engine)
    assert list(pl) == want_pl
    assert [int(k) for k in keys] == [((t + 1) << 32) | (0xFFFFFFFF - n) for t, n in zip(want_tot, want_pl)]


def test_kat_k41_reserve_unreserve():
    nodes, pods, cfg, _, _, _ = SC.kat("K41")
    sp = pods_to_struct(pods)
    st = R.SoftSpreadState(nodes["zone"])
    with Scheduler(cfg) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        with pytest.raises(QschedError) as e:
            s.score_pod_zone_scores()
        assert e.value.status == _abi.QS_ESTATE
        for node, sign, want in SC.K41_STEPS:
            (s.reserve if sign > 0 else s.unreserve)(node, sp[1])  # (recorded whatever its kind)
            assert st.record(4, node, sign)
            A.reserve(nodes, pods, 1, node, sign)
            _score_matches(s, nodes, pods, sp, 0, st, cfg)
            assert list(s.score_pod_zone_scores()[:2]) == want
            _score_matches(s, nodes, pods, sp, 1, st, cfg)  # a pod of another kind: all -1
            assert (s.score_pod_zone_scores() == -1).all()


# qs_score_pod launches k_score_podg (1,024 nodes per workgroup; k_score_podg_max before it for a soft pod
# and in the normalizing classes): one workgroup at 300 nodes, three at 2,100.
@pytest.mark.parametrize("cfg,n,wide", [({}, 300, 0), (C.CFG4, 300, 0), (C.MOST, 300, 0),
                                        (dict(scan_soa_min_nodes=1), 300, 0), ({}, 2100, 0), (C.CFG4, 2100, 0),
                                        (C.MOST, 300, 1), (C.CFG4, 300, 1)],
                         ids=["default", "norm", "most", "soa", "grid", "grid-norm", "wide-most", "wide-norm"])
def test_score_reserve_unreserve_interleaved(cfg, n, wide):
    """qs_score_pod of soft and other pods across qs_reserve / qs_unreserve steps: feasible, total, best and
    the zone scores against the reference state after each call."""
    if wide:
        nodes, pods = (SC.wide_norm if cfg is C.CFG4 else SC.wide)(n, 60)
    else:
        nodes, pods = (SC.c4 if cfg is C.CFG4 else SC.c5)(n, 60, 6, 3)
    op = pods_from_struct(pods)
    ocfg = {k: v for k, v in cfg.items() if k != "scan_soa_min_nodes"}
    scorer = A.strategy_scorer(ocfg) if "scoring_strategy" in cfg else None
    on = {k: v.copy() for k, v in nodes.items()}
    st = R.SoftSpreadState(nodes["zone"])
    soft = [j for j in range(60) if R.is_soft(op["anti_affinity"][j])]
    held = []
    with Scheduler(cfg) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        for step, j in enumerate(range(60)):
            b = _score_matches(s, on, op, pods, j, st, ocfg, scorer)
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
                _score_matches(s, on, op, pods, soft[step % len(soft)], st, ocfg, scorer)
        final = s.read_nodes()
    for k in on:
        assert np.array_equal(final[k], on[k]), k


# ---- the spread-app cap of PERSISTENT, shared with SPREAD pods -------------------------------------
def _raises(status, word, fn, *a, **k):
    with pytest.raises(QschedError) as e:
        fn(*a, **k)
    assert e.value.status == status, e.value
    assert word in str(e.value), str(e.value)


def test_spread_app_cap():
    """65 distinct apps of soft and SPREAD pods: AUTO runs SCAN (bit-exact), an explicit PERSISTENT is
    QS_EINVAL; 64 run PERSISTENT."""
    for apps, runs in ((65, "scan"), (64, "persistent")):
        nodes, pods = SC.many_apps(300, 600, apps)
        ref = R.run(nodes, pods, SC.ARRIVAL)
        g = run_tracked(nodes, pods, SC.ARRIVAL, "auto")
        assert_same(g[:2], ref[:2], g[2], ref[2])
        assert g[3]["engine_used"] == runs
        if runs == "scan":
            with Scheduler(dict(SC.ARRIVAL, engine="persistent")) as s:
                s.set_pod_anti_affinity(True)
                s.load_nodes(nodes)
                st = s.prepare(pods)
                _raises(_abi.QS_EINVAL, "distinct apps", st.run)
                st.free()
                assert all(np.array_equal(s.read_nodes()[k], nodes[k]) for k in nodes)


def test_persistent_cap_of_the_normalizing_class():
    """The compact normalizing class keeps one node per lane with the score (1,024 nodes): at 1,100 nodes AUTO
    runs SCAN for a stream with soft pods (norm-auto-scan-1100 above) and PERSISTENT for one without."""
    case = SC.parity_case("norm-auto-scan-1100")
    plain = case["pods"].copy()
    plain["anti_affinity"] = np.where(R.is_soft(plain["anti_affinity"]), 0, plain["anti_affinity"])
    ref = S.run(case["nodes"], plain, case["ocfg"])
    with Scheduler(dict(case["cfg"], engine="auto")) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(case["nodes"])
        st = s.prepare(plain)
        stats = st.run()
        assert stats["engine_used"] == "persistent"
        assert_same(st.results(), ref[:2], s.read_nodes(), ref[2])
        st.free()
    with Scheduler(dict(case["cfg"], engine="persistent")) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(case["nodes"])
        st = s.prepare(case["pods"])
        _raises(_abi.QS_EINVAL, "at most 1024 nodes", st.run)
        st.free()


# ---- state ---------------------------------------------------------------------------------------
def test_two_streams_save_restore_and_a_new_zone():
    """Two streams in a row on one context, save / restore between them (the weight set after the save
    survives the restore), then an upsert that opens a new zone before the second stream runs again."""
    case = SC.parity_case("persistent-65")
    nodes, pods, cfg = case["nodes"], case["pods"], SC.ARRIVAL
    first, rest = pods[:40], pods[40:]
    ref1 = R.run(nodes, first, cfg, wpts=5)
    ref2 = R.run(ref1[2], rest, cfg, state=ref1[3])
    assert ref2[3].wpts == 5  # (the state carries the weight)
    free = int(np.flatnonzero((ref1[3].node.sum(axis=0) == 0) & (nodes["max_pods"] > 1))[0])
    moved = {k: v.copy() for k, v in ref1[2].items()}
    moved["zone"][free] = 9
    st3 = ref1[3].copy()
    st3.set_zones(moved["zone"])
    ref3 = R.run(moved, rest, cfg, state=st3)
    assert not np.array_equal(ref3[0], ref2[0])  # the new, empty zone changes the stream
    for engine in ("persistent", "scan"):
        with Scheduler(dict(cfg, engine=engine)) as s:
            s.set_pod_anti_affinity(True)
            s.load_nodes(nodes)
            s.save_table()  # (holds Wpts = 2)
            s.set_topology_spread_weight(5)
            s.restore_table()
            a = s.prepare(first)
            a.run()
            assert_same(a.results(), ref1[:2], s.read_nodes(), ref1[2])
            s.save_table()
            b = s.prepare(rest)
            _raises(_abi.QS_ESTATE, "prepared streams", s.set_topology_spread_weight, 7)
            for _ in range(2):
                b.run()
                assert_same(b.results(), ref2[:2], s.read_nodes(), ref2[2])
                s.restore_table()
            row = {f: moved[f][free] for f in moved}
            s.upsert(free, row)
            b.run()
            assert_same(b.results(), ref3[:2], s.read_nodes(), ref3[2])
            a.free()
            b.free()
            assert s.get_topology_spread_weight() == 5


# ---- interface -----------------------------------------------------------------------------------
def test_tracking_off_ignores_the_flag(oracle):
    case = SC.parity_case("persistent-24")
    nodes, pods = case["nodes"], case["pods"]
    o = run_oracle(oracle, nodes, pods, SC.ARRIVAL)
    for engine in ("persistent", "scan", "lookahead"):
        g = run_tracked(nodes, pods, SC.ARRIVAL, engine, track=False)
        assert_same(g[:2], o[:2], g[2], o[2])
        assert g[3]["engine_used"] == engine
    assert not np.array_equal(o[0], case["pl"])
    with Scheduler(SC.ARRIVAL) as s:
        s.load_nodes(nodes)
        soft = int(np.flatnonzero(R.is_soft(pods["anti_affinity"]))[0])
        plain = pods[soft:soft + 1].copy()
        plain["anti_affinity"] = 0
        a, b = s.score_pod(pods[soft]), s.score_pod(plain[0])
        assert np.array_equal(a["total"], b["total"]) and a["best"] == b["best"]
        assert (a["zone_scores"] == -1).all()


def test_interface_errors():
    case = SC.parity_case("persistent-24")
    nodes, pods = case["nodes"], case["pods"]
    soft = _abi.QS_AA_SOFT
    with Scheduler(dict(SC.ARRIVAL, batch_pods=1)) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        one = pods[:1].copy()
        for bad, word in ((A.NONE | soft, "zero"), (A.HOSTNAME | soft, "zero"), (A.ZONE | soft, "zero"),
                          (3 | soft, "max_skew"), (3 | (32 << 8) | soft, "max_skew"), (3 | (1 << 8) | (soft << 1), "max_skew"),
                          (3 | (1 << 8) | soft | (1 << 13), "max_skew")):
            one["anti_affinity"] = bad
            _raises(_abi.QS_EINVAL, word, s.prepare, one)
            _raises(_abi.QS_EINVAL, word, s.score_pod, one[0])
            _raises(_abi.QS_EINVAL, word, s.reserve, 0, one[0])
        for w in (-1, 101):
            _raises(_abi.QS_EINVAL, "0..100", s.set_topology_spread_weight, w)
        assert s.get_topology_spread_weight() == 2
        st = s.prepare(pods)
        _raises(_abi.QS_ESTATE, "prepared streams", s.set_topology_spread_weight, 3)
        _raises(_abi.QS_EINVAL, "QS_MODE_BATCHED", st.run, mode="batched")
        assert all(np.array_equal(s.read_nodes()[k], nodes[k]) for k in nodes)
        st.run()  # ... and the exact run of the same stream is fine
        assert np.array_equal(st.results()[0], case["pl"])
        st.free()
        only_soft = pods[R.is_soft(pods["anti_affinity"])][:8].copy()
        st = s.prepare(only_soft)
        _raises(_abi.QS_EINVAL, "QS_MODE_BATCHED", st.run, mode="batched")
        st.free()
    for engine in ("lookahead", "allreduce"):
        with Scheduler(dict(SC.ARRIVAL, engine=engine)) as s:
            s.set_pod_anti_affinity(True)
            s.load_nodes(nodes)
            st = s.prepare(pods)
            _raises(_abi.QS_EINVAL, "anti-affinity", st.run)
            st.free()
