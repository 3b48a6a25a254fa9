"""GPU parity of the preemption dry run (spec/semantics.md S18): qs_preempt_pod, qs_node_pods, qs_evict and
the pod registry behind them against tests/preempt_ref.py, bit for bit: the chosen node, the victims in
walk order with every field, the victims per node of every node, and the registry of every node; then the
round a caller makes of the answer (evict the victims, score, reserve) against the reference's table.
The inputs and what each is for are in tests/preempt_cases.py; the reference is pinned by spec/kat.md
K59-K67 (tests/test_preempt_cpu.py).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import POD_DTYPE, QschedError, Scheduler, _abi, synth_generate  # noqa: E402

import preempt_cases as C  # noqa: E402
import preempt_ref as R  # noqa: E402

TABLE_COLS = ("req_cpu", "req_mem", "req_ext", "nz_cpu", "nz_mem", "pods")


def open_case(c, **cfg):
    s = Scheduler(dict(c.get("cfg", C.ON), **cfg))
    s.set_preemption(True)
    s.set_preemption_policy(c["policy"])
    s.load_nodes(c["nodes"])
    for node, pod in c["fill"]:
        s.reserve(node, pod)
    return s


def assert_registry(s, ref, nodes=None):
    for i in (range(ref.n) if nodes is None else nodes):
        assert R.victims_equal(s.node_pods(i), ref.node_pods(i)), i


def assert_table(s, ref):
    got = s.read_nodes()
    for f in TABLE_COLS:
        assert np.array_equal(got[f], ref.t[f]), f


def assert_answer(s, pod, want):
    node, victims, nvict_n = s.preempt_pod(pod, per_node=True)
    assert np.array_equal(nvict_n, want[2]), np.flatnonzero(nvict_n != want[2])[:8]
    assert node == want[0]
    assert R.victims_equal(victims, want[1])
    node2, victims2 = s.preempt_pod(pod)  # (the call without the per-node array: the same answer)
    assert node2 == node and R.victims_equal(victims2, want[1])


@pytest.mark.parametrize("name", C.KATS)
def test_known_answers(name):
    k = C.kat(name)
    with open_case(k) as s:
        ref = C.kat_ref(k)
        assert_answer(s, k["pod"], ref.preempt(k["pod"]))
        assert_registry(s, ref)


@pytest.mark.parametrize("name", C.CASES)
def test_parity(name):
    c = C.case(name)
    ref, answers = C.case_ref(name)
    with open_case(c) as s:
        # the layout the case is for, read off a stream whose one pod fits nowhere (nothing is registered)
        huge = np.array([C.mk_pod(1 << 23, 0, 0, 0)], POD_DTYPE)
        placement, stats = s.schedule(huge, with_stats=True)
        assert placement[0] == -1 and stats["table_layout"] == ("wide" if name.startswith("wide") else "compact")
        assert_registry(s, ref)
        assert_table(s, ref)
        for pod, want in zip(c["pods"], answers):
            assert_answer(s, pod, want)
        assert_table(s, ref)  # the dry run changes no state
        assert_registry(s, ref, range(0, ref.n, 7))


@pytest.mark.parametrize("name", ["n65", "wide", "qos"])
def test_round(name):
    """evict the victims, score, reserve: the node is feasible and the table and registry follow the
    reference; the next dry run starts from the new registry (only the touched columns are uploaded)."""
    import copy
    c = C.case(name)
    ref = copy.deepcopy(C.case_ref(name)[0])
    with open_case(c) as s:
        for pod in (c["pods"][0], c["pods"][1], c["pods"][-1 if name == "wide" else 7]):
            node, victims, nvict_n = ref.preempt(pod)
            assert_answer(s, pod, (node, victims, nvict_n))
            if node < 0:
                continue
            for e in victims:
                assert ref.evict(node, e["seq"])
                s.evict(node, e["seq"])
            out = s.score_pod(pod)
            assert out["feasible"][node]
            s.reserve(node, pod)
            ref.reserve(node, pod)
            assert_table(s, ref)
            assert_registry(s, ref, [node])
        assert_registry(s, ref)


def test_both_policies_one_table():
    a, b = C.kat("K64a"), C.kat("K64b")
    with open_case(a) as s:
        assert_answer(s, a["pod"], C.kat_ref(a).preempt(a["pod"]))
        s.set_preemption_policy("qos")  # re-sorts the registry
        assert s.get_preemption_policy() == _abi.QS_PREEMPT_BY_QOS
        assert_answer(s, b["pod"], C.kat_ref(b).preempt(b["pod"]))
        assert_registry(s, C.kat_ref(b))
    # a larger table: the same registry walked under the other policy
    c = C.case("qos")
    ref, answers = C.case_ref("qos")
    other = C.new_ref(dict(c, policy=0))
    for node, pod in c["fill"]:
        other.reserve(node, pod)
    assert any(C.answers_differ(x, other.preempt(p)) for p, x in zip(c["pods"], answers))
    with open_case(dict(c, policy=0)) as s:
        for pod in c["pods"]:
            assert_answer(s, pod, other.preempt(pod))
        s.set_preemption_policy(1)
        for pod, want in zip(c["pods"], answers):
            assert_answer(s, pod, want)
        assert_registry(s, ref, range(0, ref.n, 5))


@pytest.mark.parametrize("engine", ["persistent", "scan"])
def test_registry_from_a_stream(engine):
    """An exact stream appends its placed pods in decision order; replaying its placements through
    qs_reserve on a second context gives the same qs_node_pods, and the dry run the same answer."""
    nodes, pods = synth_generate(1, 100, 3000)
    pods["priority"] = np.random.default_rng(5).choice(C.PRIOS, len(pods))
    with Scheduler({"engine": engine}) as s, Scheduler({}) as t:
        for x in (s, t):
            x.set_preemption(True)
            x.load_nodes(nodes)
        placement = s.schedule(pods)
        assert (placement >= 0).sum() > 100
        ref = R.Ref(nodes, False, False)
        ref.place_stream(pods, placement)
        for j in R.qos_order(pods):
            if placement[j] >= 0:
                t.reserve(int(placement[j]), pods[j])
        assert_table(s, ref)
        for x in (s, t):
            assert_registry(x, ref)
        big = C.mk_pod(3000, 4 * C.GI, C.I32_MAX, 2)
        want = ref.preempt(big)
        for x in (s, t):
            assert_answer(x, big, want)


def test_batched_stream_registers_its_pods():
    nodes, pods = synth_generate(1, 100, 600)
    with Scheduler({}) as s:
        s.set_preemption(True)
        s.load_nodes(nodes)
        placement = s.schedule(pods, mode="batched")
        ref = R.Ref(nodes, False, False)
        ref.place_stream(pods, placement)
        assert_registry(s, ref)


def test_registry_off_changes_nothing():
    """With the registry off a stream's placements and final table equal those of a context that never
    heard of it, and nothing is recorded; switching it off does not clear what is there."""
    nodes, pods = synth_generate(1, 100, 800)
    with Scheduler({}) as s, Scheduler({}) as t:
        s.load_nodes(nodes)
        t.load_nodes(nodes)
        s.set_preemption(True)
        s.reserve(3, pods[0])
        t.reserve(3, pods[0])
        s.set_preemption(False)
        assert not s.get_preemption()
        a, b = s.schedule(pods), t.schedule(pods)
        assert np.array_equal(a, b)
        fa, fb = s.read_nodes(), t.read_nodes()
        for f in fa:
            assert np.array_equal(fa[f], fb[f]), f
        assert [len(s.node_pods(i)) for i in range(100)] == [0] * 3 + [1] + [0] * 96
        with pytest.raises(QschedError) as e:
            s.preempt_pod(pods[1])
        assert e.value.status == _abi.QS_ESTATE


def test_save_restore_load_and_unreserve():
    k = C.kat("K61")
    with open_case(k) as s:
        ref = C.kat_ref(k)
        s.save_table()
        ref.save()
        extra = C.mk_pod(100, C.GI, 9, 0)
        s.reserve(1, extra)
        ref.reserve(1, extra)
        s.evict(0, 1)
        ref.evict(0, 1)
        assert_registry(s, ref)
        assert_answer(s, k["pod"], ref.preempt(k["pod"]))
        s.restore_table()
        ref.restore()
        assert_registry(s, ref)
        assert_table(s, ref)
        assert_answer(s, k["pod"], ref.preempt(k["pod"]))
        s.reserve(0, extra)  # the counter came back with the snapshot: seq 6 again
        ref.reserve(0, extra)
        assert int(s.node_pods(0)["seq"].max()) == 6
        assert_registry(s, ref)
        # qs_unreserve: the highest seq among equal entries; no equal entry: QS_EINVAL, nothing changed
        twin = k["fill"][3][1]  # node 1 holds two equal pods (seq 4, 5)
        s.unreserve(1, twin)
        assert ref.unreserve(1, twin)
        assert sorted(s.node_pods(1)["seq"]) == [3, 4]
        with pytest.raises(QschedError) as e:
            s.unreserve(1, C.mk_pod(500, C.GI, 2, 1))
        assert e.value.status == _abi.QS_EINVAL
        assert_registry(s, ref)
        assert_table(s, ref)
        s.load_nodes(k["nodes"])  # a load empties the registry
        assert all(len(s.node_pods(i)) == 0 for i in range(2))
        assert s.preempt_pod(k["pod"])[0] == -1


def test_status_codes():
    k = C.kat("K59")
    with open_case(k) as s:
        ref = C.kat_ref(k)
        # qs_evict of an absent entry, of a node outside the table
        for node, seq in ((0, 99), (0, 0), (5, 1)):
            with pytest.raises(QschedError) as e:
                s.evict(node, seq)
            assert e.value.status == _abi.QS_EINVAL
        with pytest.raises(QschedError) as e:
            s.node_pods(1)
        assert e.value.status == _abi.QS_EINVAL
        with pytest.raises(QschedError) as e:
            s.set_preemption_policy(2)
        assert e.value.status == _abi.QS_EINVAL
        bad = k["pod"].copy()
        bad["qos"] = 3  # what check_pod rejects
        with pytest.raises(QschedError) as e:
            s.preempt_pod(bad)
        assert e.value.status == _abi.QS_EINVAL
        # an upsert below the sums over the node's entries (4000m in three pods)
        row = {f: int(ref.t[f][0]) for f in ("alloc_cpu", "alloc_mem", "max_pods", "req_cpu", "req_mem", "nz_cpu",
                                             "nz_mem", "pods")}
        for f, v in (("req_cpu", 3999), ("pods", 2), ("nz_mem", 0)):
            with pytest.raises(QschedError) as e:
                s.upsert(0, dict(row, **{f: v}))
            assert e.value.status == _abi.QS_EINVAL
        s.upsert(0, dict(row, req_cpu=4500, nz_cpu=4500, pods=4, alloc_cpu=8000))  # more than the entries: fine
        ref.t["req_cpu"][0] = ref.t["nz_cpu"][0] = 4500
        ref.t["pods"][0], ref.t["alloc_cpu"][0] = 4, 8000
        assert_answer(s, k["pod"], ref.preempt(k["pod"]))
        # prepared streams pin the switch
        st = s.prepare(np.zeros(1, POD_DTYPE))
        with pytest.raises(QschedError) as e:
            s.set_preemption(False)
        assert e.value.status == _abi.QS_ESTATE
        st.free()
        s.set_preemption(False)
        # a preemptor with an anti-affinity kind on a context that tracks pod anti-affinity
        s.set_preemption(True)
        s.set_pod_anti_affinity(True)
        aa = k["pod"].copy()
        aa["anti_affinity"] = 1
        with pytest.raises(QschedError) as e:
            s.preempt_pod(aa)
        assert e.value.status == _abi.QS_EINVAL
        assert s.preempt_pod(k["pod"])[0] == 0
    with Scheduler({"virtual_shards": 2, "engine": "lookahead"}) as s:
        with pytest.raises(QschedError) as e:
            s.set_preemption(True)
        assert e.value.status == _abi.QS_EINVAL


def test_more_entries_than_victims_fit():
    """A node with 257 entries: QS_EINVAL that names the node; at 256 the call answers."""
    nodes = C.mk_nodes([100000, 4000], max_pods=300)
    tiny = C.mk_pod(100, 64 * C.MI, 0, 0)
    with Scheduler({}) as s:
        s.set_preemption(True)
        s.load_nodes(nodes)
        ref = R.Ref(nodes, False, False)
        for _ in range(256):
            s.reserve(0, tiny)
            ref.reserve(0, tiny)
        big = C.mk_pod(99000, C.GI, 5, 2)
        want = ref.preempt(big)
        assert want[0] == 0 and len(want[1]) == 246
        assert_answer(s, big, want)
        s.reserve(0, tiny)
        with pytest.raises(QschedError) as e:
            s.preempt_pod(big)
        assert e.value.status == _abi.QS_EINVAL and "node 0" in str(e.value)
        s.unreserve(0, tiny)
        assert_answer(s, big, want)


def test_evict_with_anti_affinity_tracking():
    """qs_evict removes the anti-affinity record as qs_unreserve does: the node opens again for a
    HOSTNAME pod of the app."""
    nodes = C.mk_nodes([4000, 4000])
    with Scheduler({}) as s:
        s.set_pod_anti_affinity(True)
        s.set_preemption(True)
        s.load_nodes(nodes)
        held = C.mk_pod(1000, C.GI, 0, 1, app=7)
        s.reserve(0, held)
        probe = held.copy()
        probe["anti_affinity"] = 1
        assert list(s.score_pod(probe)["feasible"]) == [False, True]
        s.evict(0, int(s.node_pods(0)["seq"][0]))
        assert list(s.score_pod(probe)["feasible"]) == [True, True]
        assert int(s.read_nodes()["pods"][0]) == 0


def test_table_limit():
    """The registry covers tables up to 2^17 nodes: switching it on above that, and qs_preempt_pod after a
    larger load with the registry already on, are QS_EINVAL; exactly 2^17 nodes are accepted."""
    limit = 1 << 17
    over, at = C.mk_nodes([1000] * (limit + 1), mem=C.GI), C.mk_nodes([1000] * limit, mem=C.GI)
    pod = C.mk_pod(500, C.MI * 64, 5, 2)
    with Scheduler({}) as s:
        s.load_nodes(over)
        with pytest.raises(QschedError) as e:
            s.set_preemption(True)
        assert e.value.status == _abi.QS_EINVAL and not s.get_preemption()
        s.load_nodes(at)
        s.set_preemption(True)
        s.reserve(limit - 1, C.mk_pod(1000, C.MI * 64, 1, 0))
        node, victims = s.preempt_pod(pod)
        assert node == limit - 1 and [int(v) for v in victims["seq"]] == [1]
        s.load_nodes(over)  # the registry stays on; the call refuses the table
        with pytest.raises(QschedError) as e:
            s.preempt_pod(pod)
        assert e.value.status == _abi.QS_EINVAL


def test_slot_growth_after_the_first_upload():
    """A list that outgrows the device copy's slots after the first dry run (8 -> 9 -> 17 entries): the copy
    is reallocated and every node's list uploaded again, the other node's included."""
    nodes = C.mk_nodes([1700, 3000])
    with Scheduler({}) as s:
        s.set_preemption(True)
        s.load_nodes(nodes)
        ref = R.Ref(nodes, False, False)

        def add(node, cpu, prio, k):
            for _ in range(k):
                p = C.mk_pod(cpu, 64 * C.MI, prio, 1)
                s.reserve(node, p)
                ref.reserve(node, p)
        add(0, 100, 3, 8)
        add(1, 1000, 1, 3)
        pods = [C.mk_pod(1000, C.GI, 10, 2), C.mk_pod(1200, C.GI, 2, 2), C.mk_pod(300, C.GI, 10, 2)]
        for grow in (0, 1, 8):
            add(0, 100, 4, grow)
            for p in pods:
                assert_answer(s, p, ref.preempt(p))
        assert len(s.node_pods(0)) == 17
        assert_registry(s, ref)


def test_evict_a_hostname_spread_holder():
    """The registry does not keep a pod's anti-affinity kind: qs_evict of a QS_AA_SPREAD_HOSTNAME pod still
    lowers the (app, node) count its kind reads, as qs_unreserve of that pod would."""
    from qsched import aa_spread_hostname
    nodes = C.mk_nodes([4000, 4000])
    with Scheduler({}) as s:
        s.set_pod_anti_affinity(True)
        s.set_preemption(True)
        s.load_nodes(nodes)
        held = C.mk_pod(1000, C.GI, 0, 1, app=7)
        held["anti_affinity"] = aa_spread_hostname(1)
        s.reserve(0, held)
        s.reserve(0, held)
        assert list(s.score_pod(held)["feasible"]) == [False, True]  # 2 + 1 - 0 > 1
        s.evict(0, 2)
        assert list(s.score_pod(held)["feasible"]) == [False, True]  # 1 + 1 - 0 > 1
        s.evict(0, 1)
        assert list(s.score_pod(held)["feasible"]) == [True, True]
        assert int(s.read_nodes()["pods"][0]) == 0 and len(s.node_pods(0)) == 0
