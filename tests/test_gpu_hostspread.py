"""GPU parity of hostname topology spread (spec/semantics.md S15, ``QS_AA_SPREAD_HOSTNAME(max_skew)``) on
the exact engines and the score path: PERSISTENT and SCAN, every feature class and both row layouts, tables
with and without the column-major copy, qs_score_pod / qs_reserve / qs_unreserve, the app cap of
PERSISTENT, and the (app, node) counts
across streams that do and do not maintain them, batched runs, save / restore and an appended node,
against tests/hostspread_ref.py bit for bit (placements, per-pod keys, the final table, and the recorded
state as later probe pods see it).  The reference is pinned by spec/kat.md K42-K47
(tests/test_hostspread_cpu.py).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import (QschedError, Scheduler, _abi, aa_spread_hostname, pods_from_struct,  # noqa: E402
                    pods_to_struct)

import antiaffinity_ref as A  # noqa: E402
import hostspread_cases as HC  # noqa: E402
import hostspread_ref as H  # noqa: E402
from test_gpu_parity import assert_same, run_oracle  # noqa: E402


def _probe_pods(pods, app):
    """Four pods of `app` asking for nothing: HOSTSPREAD(1), HOSTSPREAD(2), ZONE, HOSTNAME."""
    p = pods[:4].copy()
    for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "req_ext", "n_req_terms", "n_pref_terms", "sel",
              "tol_hard", "tol_soft"):
        if f in p.dtype.names:
            p[f] = 0
    p["tol_hard"] = p["tol_soft"] = np.uint64(0xFFFFFFFFFFFFFFFF)
    p["app"] = app
    p["anti_affinity"] = [aa_spread_hostname(1), aa_spread_hostname(2), A.ZONE, A.HOSTNAME]
    return p


def check_state(s, pods, final, state, apps):
    """The recorded state through the score path: the feasible sets of probe pods of `apps` against the
    reference's final table and state."""
    for app in apps:
        probe = _probe_pods(pods, int(app))
        op = pods_from_struct(probe)
        for j in range(4):
            want = A.pod_keys(final, op, j, state, {}) != 0
            got = s.score_pod(probe[j])["feasible"]
            assert np.array_equal(got, want), (app, j)


def run_tracked(nodes, pods, cfg, engine, track=True, state=None):
    with Scheduler(dict(cfg, engine=engine)) as s:
        if track:
            s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        st = s.prepare(pods)
        stats = st.run()
        pl, keys = st.results()
        st.free()
        final = s.read_nodes()
        if state is not None:
            check_state(s, pods, final, state, np.unique(pods["app"])[:12])
    return pl, keys, final, stats


@pytest.mark.parametrize("name", list(HC.PARITY))
def test_parity(name):
    case = HC.parity_case(name)
    HC.check_conditions(case)  # from the reference alone, before the GPU runs
    g = run_tracked(case["nodes"], case["pods"], case["cfg"], case["engine"], state=case["state"])
    assert_same(g[:2], (case["pl"], case["keys"]), g[2], case["final"])
    assert g[3]["engine_used"] == case["runs"], g[3]["engine_used"]
    assert g[3]["table_layout"] == ("wide" if "wide" in case["flags"] else "compact")


# ---- known answers -------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["persistent", "scan"])
@pytest.mark.parametrize("name", ["K42", "K43", "K44", "K45", "K47"])
def test_kat_streams(name, engine):
    nodes, pods, cfg, want_pl = HC.kat(name)
    ref = H.run(nodes, pods, cfg)
    assert list(ref[0]) == want_pl
    pl, keys, _, stats = run_tracked(nodes, pods_to_struct(pods), cfg, engine)
    assert list(pl) == want_pl
    assert np.array_equal(keys, ref[1])
    assert stats["engine_used"] == engine


def _score_matches(s, nodes, pods, sp, j, state, cfg, scorer=None):
    """qs_score_pod / qs_score_pod_packed of pod j against the reference under `state`."""
    k = A.pod_keys(nodes, pods, j, state, cfg, scorer)
    feas = k != 0
    best = int(0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)) if feas.any() else -1
    got = s.score_pod(sp[j])
    assert np.array_equal(got["feasible"], feas), j
    assert got["best"] == best
    assert np.array_equal(got["total"], np.where(feas, (k >> np.uint64(32)).astype(np.int64) - 1, -1))
    assert (got["scores"][~feas] == 0).all()
    bp, packed = s.score_pod_packed(sp[j])
    assert bp == best and np.array_equal(packed != 0xFFFFFFFF, feas)
    return best


def test_kat_k46_reserve_unreserve():
    nodes, pods, cfg, _ = HC.kat("K46")
    sp = pods_to_struct(pods)
    st = H.HostSpreadState(nodes["zone"])
    with Scheduler(cfg) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        for node, sign, want in HC.K46_STEPS:
            (s.reserve if sign > 0 else s.unreserve)(node, sp[1])  # (recorded whatever its kind)
            assert st.record(4, node, sign)
            A.reserve(nodes, pods, 1, node, sign)
            _score_matches(s, nodes, pods, sp, 0, st, cfg)
            assert list(np.flatnonzero(s.score_pod(sp[0])["feasible"])) == want


# qs_score_pod launches k_score_podg (1,024 nodes per workgroup; before it k_score_podg_max for the
# minimum, and in the normalizing classes once more for the maxima): one workgroup at 300 nodes, three at
# 2,100, whose last one is ragged (52 real nodes: idle threads must not feed the minimum).
@pytest.mark.parametrize("cfg,n", [({}, 300), (HC.C.CFG4, 300), (HC.C.MOST, 300), (dict(scan_soa_min_nodes=1), 300),
                                   ({}, 2100), (HC.C.CFG4, 2100), ({}, 8), (HC.C.CFG4, 8)],
                         ids=["default", "norm", "most", "soa", "grid", "grid-norm", "tiny", "tiny-norm"])
def test_score_reserve_unreserve_interleaved(cfg, n):
    """qs_score_pod of every pod across qs_reserve / qs_unreserve steps, against the reference state after
    each call.  The first qs_reserve of a hostname-spread pod, or the first qs_score_pod of one, allocates
    the counts from what the mirror holds by then.  At 8 nodes the minimum rises above 0."""
    P = 60 if n > 8 else 120
    nodes, pods = HC.c4(n, P, apps=7 if n > 8 else 3, zones=3)
    op = pods_from_struct(pods)
    ocfg = {k: v for k, v in cfg.items() if k != "scan_soa_min_nodes"}
    scorer = A.strategy_scorer(ocfg) if "scoring_strategy" in cfg else None
    on = {k: v.copy() for k, v in nodes.items()}
    st = H.HostSpreadState(nodes["zone"])
    host = [j for j in range(P) if H.is_hostkey(op["anti_affinity"][j])]
    assert len(host) >= 10
    held = []
    with Scheduler(cfg) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        for step, j in enumerate(range(P)):
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
                _score_matches(s, on, op, pods, host[step % len(host)], st, ocfg, scorer)
        final = s.read_nodes()
    for k in on:
        assert np.array_equal(final[k], on[k]), k
    if n == 8:
        assert max(int(st.node[a].min()) for a in np.unique(op["app"][host])) >= 1


# ---- the app cap of PERSISTENT -----------------------------------------------------------------------
def _raises(status, word, fn, *a, **k):
    with pytest.raises(QschedError) as e:
        fn(*a, **k)
    assert e.value.status == status, e.value
    assert word in str(e.value), str(e.value)


def test_host_spread_app_cap():
    """17 distinct hostname-spread apps: AUTO runs SCAN (bit-exact), an explicit PERSISTENT is QS_EINVAL and
    leaves the table alone; 16 run PERSISTENT.  A stream that holds soft pods as well runs SCAN likewise."""
    for apps, runs in ((17, "scan"), (16, "persistent")):
        nodes, pods = HC.many_apps(300, 600, apps)
        ref = H.run(nodes, pods, HC.ARRIVAL)
        g = run_tracked(nodes, pods, HC.ARRIVAL, "auto", state=ref[3])
        assert_same(g[:2], ref[:2], g[2], ref[2])
        assert g[3]["engine_used"] == runs
        if runs == "scan":
            with Scheduler(dict(HC.ARRIVAL, engine="persistent")) as s:
                s.set_pod_anti_affinity(True)
                s.load_nodes(nodes)
                st = s.prepare(pods)
                _raises(_abi.QS_EINVAL, "distinct apps", st.run)
                st.free()
                assert all(np.array_equal(s.read_nodes()[k], nodes[k]) for k in nodes)
    import soft_spread_ref as R
    mixed = pods.copy()
    mixed["anti_affinity"][::5] = R.spread_soft(1)
    with Scheduler(dict(HC.ARRIVAL, engine="auto")) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        st = s.prepare(mixed)
        assert st.run()["engine_used"] == "scan"
        st.free()
    with Scheduler(dict(HC.ARRIVAL, engine="persistent")) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        st = s.prepare(mixed)
        _raises(_abi.QS_EINVAL, "QS_AA_SPREAD_SOFT", st.run)
        st.free()


# ---- validity of the counts across launches ----------------------------------------------------------
@pytest.mark.parametrize("engine,runs", [("auto", "persistent"), ("scan", "scan")])
def test_counts_across_streams_batched_restore_and_append(engine, runs):
    """The (app, node) counts through every writer of recorded pods: a stream of NONE pods (the array does
    not exist yet), a stream with hostname-spread pods of the same apps (allocated and filled from the
    mirror), a batched run (stale), a third exact stream (rebuilt), save, more pods, restore (rebuilt from
    the reinstated mirror), and an appended node (count 0: the minimum back to 0).  Each step against the
    reference state.  Under PERSISTENT every stream leaves the array stale; under SCAN the commit keeps it."""
    case = HC.parity_case("persistent-24")
    nodes, pods, cfg = case["nodes"], case["pods"], HC.ARRIVAL
    host = H.is_hostkey(pods["anti_affinity"]) == 1
    apps = np.unique(pods["app"][host])
    a_pods = pods[:150].copy()
    a_pods["anti_affinity"] = A.NONE
    b_pods, d_pods, e_pods = pods[150:330], pods[330:480], pods[480:]
    # the batched run: NONE pods of the hostname-spread apps, a few of them (batched mode is not
    # order-exact, so the reference takes the device's placements as given)
    c_pods = pods[host][:24].copy()
    c_pods["anti_affinity"] = A.NONE
    ref_a = H.run(nodes, a_pods, cfg)
    ref_b = H.run(ref_a[2], b_pods, cfg, state=ref_a[3])
    with Scheduler(dict(cfg, engine=engine, batch_pods=8)) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        sa = s.prepare(a_pods)
        assert sa.run()["engine_used"] == runs
        assert_same(sa.results(), ref_a[:2], s.read_nodes(), ref_a[2])
        sb = s.prepare(b_pods)
        assert sb.run()["engine_used"] == runs
        assert_same(sb.results(), ref_b[:2], s.read_nodes(), ref_b[2])
        check_state(s, pods, ref_b[2], ref_b[3], apps)
        # batched: record what the device placed
        sc = s.prepare(c_pods)
        sc.run(mode="batched")
        pl_c = sc.results()[0]
        on, st = {k: v.copy() for k, v in ref_b[2].items()}, ref_b[3].copy()
        oc = pods_from_struct(c_pods)
        for j, node in enumerate(pl_c):
            if node >= 0:
                A.reserve(on, oc, j, int(node))
                st.record(int(oc["app"][j]), int(node))
        assert (pl_c >= 0).any()
        final = s.read_nodes()
        for k in on:
            assert np.array_equal(final[k], on[k]), k
        ref_d = H.run(on, d_pods, cfg, state=st)
        sd = s.prepare(d_pods)
        assert sd.run()["engine_used"] == runs
        assert_same(sd.results(), ref_d[:2], s.read_nodes(), ref_d[2])
        check_state(s, pods, ref_d[2], ref_d[3], apps)
        s.save_table()
        ref_e = H.run(ref_d[2], e_pods, cfg, state=ref_d[3])
        se = s.prepare(e_pods)
        se.run()
        assert_same(se.results(), ref_e[:2], s.read_nodes(), ref_e[2])
        s.restore_table()
        check_state(s, pods, ref_d[2], ref_d[3], apps)
        se.run()  # the same pods again from the restored state
        assert_same(se.results(), ref_e[:2], s.read_nodes(), ref_e[2])
        s.restore_table()
        # an appended node enters with count 0 and pulls every minimum to 0
        n = len(nodes["zone"])
        grown = {k: np.concatenate([v, v[:1]]) for k, v in ref_d[2].items()}
        for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "pods"):
            grown[f][n] = 0
        grown["req_ext"][n] = 0
        st_g = ref_d[3].copy()
        st_g.set_zones(grown["zone"])
        assert max(int(ref_d[3].node[a].min()) for a in apps) >= 1  # some minimum was above 0
        assert all(int(st_g.node[a].min()) == 0 for a in apps)
        for q in (sa, sb, sc, sd, se):
            q.free()
        s.upsert(n, {f: grown[f][n] for f in grown})
        check_state(s, pods, grown, st_g, apps)
        ref_g = H.run(grown, e_pods, cfg, state=st_g)
        assert not np.array_equal(ref_g[0], ref_e[0])
        sg = s.prepare(e_pods)
        sg.run()
        assert_same(sg.results(), ref_g[:2], s.read_nodes(), ref_g[2])
        sg.free()


# ---- interface -----------------------------------------------------------------------------------
def test_tracking_off_ignores_the_kind(oracle):
    case = HC.parity_case("persistent-300")
    nodes, pods = case["nodes"], case["pods"]
    o = run_oracle(oracle, nodes, pods, HC.ARRIVAL)
    for engine in ("persistent", "scan", "lookahead"):
        g = run_tracked(nodes, pods, HC.ARRIVAL, engine, track=False)
        assert_same(g[:2], o[:2], g[2], o[2])
        assert g[3]["engine_used"] == engine
    assert not np.array_equal(o[0], case["pl"])


def test_interface_errors():
    case = HC.parity_case("persistent-300")
    nodes, pods = case["nodes"], case["pods"]
    hk = _abi.QS_AA_HOSTKEY
    with Scheduler(dict(HC.ARRIVAL, batch_pods=1)) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        one = pods[:1].copy()
        for bad, word in ((A.NONE | hk, "zero"), (A.HOSTNAME | hk, "zero"), (A.ZONE | hk, "zero"),
                          (aa_spread_hostname(1) | _abi.QS_AA_SOFT, "QS_AA_SOFT"), (3 | hk, "max_skew"),
                          (3 | hk | (1 << 19), "max_skew"), (3 | (1 << 8) | (1 << 17), "max_skew"), (4 | hk | (1 << 8), "kind")):
            one["anti_affinity"] = bad
            _raises(_abi.QS_EINVAL, word, s.prepare, one)
            _raises(_abi.QS_EINVAL, word, s.score_pod, one[0])
            _raises(_abi.QS_EINVAL, word, s.reserve, 0, one[0])
        st = s.prepare(pods)
        _raises(_abi.QS_EINVAL, "QS_MODE_BATCHED", st.run, mode="batched")
        assert all(np.array_equal(s.read_nodes()[k], nodes[k]) for k in nodes)
        st.run()  # ... and the exact run of the same stream is fine
        assert np.array_equal(st.results()[0], case["pl"])
        st.free()
        # 16-bit counts: a node with max_pods above 65,535 is refused once the context keeps them
        row = {f: nodes[f][0] for f in nodes}
        row["max_pods"] = 70000
        _raises(_abi.QS_EINVAL, "65535", s.upsert, 0, row)
    with Scheduler(HC.ARRIVAL) as s:
        s.set_pod_anti_affinity(True)
        big = {k: v.copy() for k, v in nodes.items()}
        big["max_pods"][5] = 70000
        s.load_nodes(big)
        one = pods[:1].copy()
        one["anti_affinity"] = aa_spread_hostname(1)
        _raises(_abi.QS_EINVAL, "65535", s.score_pod, one[0])
        one["anti_affinity"] = A.HOSTNAME  # ... and every other kind is served
        assert s.score_pod(one[0])["best"] >= 0
