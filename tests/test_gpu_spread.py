"""GPU parity of zone topology spread (spec/semantics.md S13, ``QS_AA_SPREAD(max_skew)``) on the exact
engines and the score path: PERSISTENT and SCAN, every feature class and both row layouts,
qs_score_pod / qs_reserve / qs_unreserve, the spread-app cap of PERSISTENT, and the state across
streams, save / restore and a new zone, against tests/spread_ref.py bit for bit (placements, per-pod
keys, the final table, and the recorded (app, zone) / presence state as later probe pods see it).
The reference is pinned by spec/kat.md K32-K36 (tests/test_spread_cpu.py).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import QschedError, Scheduler, _abi, aa_spread, pods_from_struct, pods_to_struct  # noqa: E402

import antiaffinity_ref as A  # noqa: E402
import spread_cases as SC  # noqa: E402
import spread_ref as S  # noqa: E402
from test_gpu_parity import assert_same, run_oracle  # noqa: E402


def _probe_pods(pods, app):
    """Three pods of `app` asking for nothing: SPREAD(1), ZONE, HOSTNAME."""
    p = pods[:3].copy()
    for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "req_ext", "n_req_terms", "n_pref_terms", "sel",
              "tol_hard", "tol_soft"):
        if f in p.dtype.names:
            p[f] = 0
    p["tol_hard"] = p["tol_soft"] = np.uint64(0xFFFFFFFFFFFFFFFF)
    p["app"] = app
    p["anti_affinity"] = [aa_spread(1), A.ZONE, A.HOSTNAME]
    return p


def check_state(s, pods, final, state, apps):
    """The recorded state through the score path: the feasible sets of SPREAD / ZONE / HOSTNAME probe pods
    of `apps` against the reference's final table and state."""
    for app in apps:
        probe = _probe_pods(pods, int(app))
        op = pods_from_struct(probe)
        for j in range(3):
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
            check_state(s, pods, final, state, np.unique(pods["app"]))
    return pl, keys, final, stats


@pytest.mark.parametrize("name", list(SC.PARITY))
def test_parity(name):
    case = SC.parity_case(name)
    SC.check_conditions(case)  # from the reference alone, before the GPU runs
    g = run_tracked(case["nodes"], case["pods"], case["cfg"], case["engine"], state=case["state"])
    assert_same(g[:2], (case["pl"], case["keys"]), g[2], case["final"])
    assert g[3]["engine_used"] == case["runs"], g[3]["engine_used"]
    assert g[3]["table_layout"] == ("wide" if "wide" in case["flags"] else "compact")


@pytest.mark.parametrize("name", ["persistent-24", "persistent-1100", "norm-persistent", "most-persistent"])
def test_scan_agrees_on_persistent_inputs(name):
    case = SC.parity_case(name)
    g = run_tracked(case["nodes"], case["pods"], case["cfg"], "scan")
    assert_same(g[:2], (case["pl"], case["keys"]), g[2], case["final"])
    assert g[3]["engine_used"] == "scan"


# ---- known answers -------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["persistent", "scan"])
@pytest.mark.parametrize("name", ["K32", "K33", "K34", "K35"])
def test_kat_streams(name, engine):
    nodes, pods, cfg, want_pl, want_tot = SC.kat(name)
    pl, keys, _, _ = run_tracked(nodes, pods_to_struct(pods), cfg, engine)
    assert list(pl) == want_pl
    assert [int(k) for k in keys] == [((t + 1) << 32) | (0xFFFFFFFF - n) for t, n in zip(want_tot, want_pl)]


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


def test_kat_k36_reserve_unreserve():
    nodes, pods, cfg, _, _ = SC.kat("K36")
    sp = pods_to_struct(pods)
    st = S.SpreadState(nodes["zone"])
    with Scheduler(cfg) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        for node, sign, want in SC.K36_STEPS:
            (s.reserve if sign > 0 else s.unreserve)(node, sp[1])  # (recorded whatever its kind)
            assert st.record(4, node, sign)
            A.reserve(nodes, pods, 1, node, sign)
            assert _score_matches(s, nodes, pods, sp, 0, st, cfg) == want[0]
            assert list(np.flatnonzero(s.score_pod(sp[0])["feasible"])) == want


# qs_score_pod launches k_score_podg (1,024 nodes per workgroup; the normalizing classes k_score_podg_max
# before it): one workgroup at 300 nodes, three at 2,100.  (k_score_pod1, the single-workgroup form,
# carries the same filter but no call of the C ABI launches it.)
@pytest.mark.parametrize("cfg,n", [({}, 300), (SC.C.CFG4, 300), (SC.C.MOST, 300), (dict(scan_soa_min_nodes=1), 300),
                                   ({}, 2100), (SC.C.CFG4, 2100)],
                         ids=["default", "norm", "most", "soa", "grid", "grid-norm"])
def test_score_reserve_unreserve_interleaved(cfg, n):
    """qs_score_pod of SPREAD pods across qs_reserve / qs_unreserve steps, against the reference state
    after each call, tables with and without the column-major copy, one workgroup and several.

    Only k_score_podg(_max) runs here.  k_score_pod1 is compiled with the same filter, but the host always
    passes the device words of the grid form, so no call of the C ABI executes it and nothing tests it."""
    nodes, pods = SC.c4(n, 60, apps=6, zones=3)
    op = pods_from_struct(pods)
    ocfg = {k: v for k, v in cfg.items() if k != "scan_soa_min_nodes"}
    scorer = A.strategy_scorer(ocfg) if "scoring_strategy" in cfg else None
    on = {k: v.copy() for k, v in nodes.items()}
    st = S.SpreadState(nodes["zone"])
    spread = [j for j in range(60) if S.kind_of(op["anti_affinity"][j]) == S.SPREAD]
    assert len(spread) >= 10
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
                _score_matches(s, on, op, pods, spread[step % len(spread)], st, ocfg, scorer)
        final = s.read_nodes()
    for k in on:
        assert np.array_equal(final[k], on[k]), k


# ---- the spread-app cap of PERSISTENT ---------------------------------------------------------------
def test_spread_app_cap():
    """65 distinct spread apps: AUTO runs SCAN (bit-exact), an explicit PERSISTENT is QS_EINVAL; 64 run
    PERSISTENT."""
    for apps, runs in ((65, "scan"), (64, "persistent")):
        nodes, pods = SC.many_apps(300, 600, apps)
        ref = S.run(nodes, pods, SC.ARRIVAL)
        g = run_tracked(nodes, pods, SC.ARRIVAL, "auto", state=ref[3])
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


# ---- state ---------------------------------------------------------------------------------------
def test_two_streams_save_restore_and_a_new_zone():
    """Two streams in a row on one context, save / restore between them, then an upsert that opens a new
    zone (the minimum drops to 0) before the second stream runs again."""
    case = SC.parity_case("persistent-300")
    nodes, pods, cfg = case["nodes"], case["pods"], SC.ARRIVAL
    first, rest = pods[:700], pods[700:]
    ref1 = S.run(nodes, first, cfg)
    ref2 = S.run(ref1[2], rest, cfg, state=ref1[3])
    # node 299 holds no recorded pod after `first` in the reference? pick one that does not
    free = int(np.flatnonzero(ref1[3].node.sum(axis=0) == 0)[0])
    moved = {k: v.copy() for k, v in ref1[2].items()}
    moved["zone"][free] = 9
    st3 = ref1[3].copy()
    st3.set_zones(moved["zone"])
    ref3 = S.run(moved, rest, cfg, state=st3)
    assert not np.array_equal(ref3[0], ref2[0])  # the new, empty zone changes the stream
    for engine in ("persistent", "scan"):
        with Scheduler(dict(cfg, engine=engine)) as s:
            s.set_pod_anti_affinity(True)
            s.load_nodes(nodes)
            a = s.prepare(first)
            a.run()
            assert_same(a.results(), ref1[:2], s.read_nodes(), ref1[2])
            s.save_table()
            b = s.prepare(rest)
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


# ---- interface -----------------------------------------------------------------------------------
def _raises(status, word, fn, *a, **k):
    with pytest.raises(QschedError) as e:
        fn(*a, **k)
    assert e.value.status == status, e.value
    assert word in str(e.value), str(e.value)


def test_tracking_off_ignores_spread(oracle):
    case = SC.parity_case("persistent-300")
    nodes, pods = case["nodes"], case["pods"]
    o = run_oracle(oracle, nodes, pods, SC.ARRIVAL)
    for engine in ("persistent", "scan", "lookahead"):
        g = run_tracked(nodes, pods, SC.ARRIVAL, engine, track=False)
        assert_same(g[:2], o[:2], g[2], o[2])
        assert g[3]["engine_used"] == engine
    assert not np.array_equal(o[0], case["pl"])


def test_interface_errors():
    case = SC.parity_case("persistent-300")
    nodes, pods = case["nodes"], case["pods"]
    with Scheduler(dict(SC.ARRIVAL, batch_pods=1)) as s:
        s.set_pod_anti_affinity(True)
        s.load_nodes(nodes)
        one = pods[:1].copy()
        for bad, word in ((3, "max_skew"), (3 | (32 << 8), "max_skew"), (3 | (1 << 13), "max_skew"),
                          (4 | (1 << 8), "kind"), (A.ZONE | (1 << 8), "zero"), (A.NONE | (1 << 16), "zero"),
                          (A.HOSTNAME | (1 << 30), "zero"), (-1, "kind")):
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
