"""``nodeAffinityPolicy: Honor`` of the topology spread constraints (spec/semantics.md S16;
qs_set_topology_spread_node_affinity_policy), no GPU:

* the two symbols, the header text, and the status of a null context or pointer;
* the known answers K48-K52 of spec/kat.md through tests/honor_spread_ref.py, under both policies;
* properties of the reference: under IGNORE, and for pods that do not restrict, it is the reference of S13 /
  S14 / S15;
* the conditions that make the parity inputs of tests/test_gpu_honor_spread.py worth running.
"""
import ctypes
import os

import numpy as np
import pytest

import qsched
from qsched import _abi

import antiaffinity_ref as A
import honor_spread_cases as HC
import honor_spread_ref as HR
import hostspread_cases as HSC
import hostspread_ref as H
import soft_spread_cases as SSC
import spread_cases as SC
import spread_ref as S


def key(total, node):
    return ((total + 1) << 32) | (0xFFFFFFFF - node)


# ---- the interface -------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    lib = qsched.load()
    for s in ("qs_set_topology_spread_node_affinity_policy", "qs_get_topology_spread_node_affinity_policy"):
        assert s in _abi.EXPORTED and hasattr(lib, s), s
    assert (_abi.QS_POLICY_IGNORE, _abi.QS_POLICY_HONOR) == (0, 1) == (HR.IGNORE, HR.HONOR)
    assert qsched.POLICIES == {"ignore": 0, "honor": 1}
    assert _abi.QS_ABI_VERSION == 3 and lib.qs_struct_size(3) == _abi.POD_DTYPE.itemsize


def test_header_declares_the_additions():
    here = os.path.dirname(os.path.abspath(__file__))
    h = open(os.path.join(here, "..", "include", "qsched.h")).read()
    assert "#define QS_ABI_VERSION 3" in h
    for s in ("typedef enum qs_node_inclusion_policy { QS_POLICY_IGNORE = 0, QS_POLICY_HONOR = 1 } qs_node_inclusion_policy;",
              "QS_API qs_status qs_set_topology_spread_node_affinity_policy(qs_ctx *ctx, int32_t policy);",
              "QS_API qs_status qs_get_topology_spread_node_affinity_policy(qs_ctx *ctx, int32_t *policy);",
              "apis/core#TopologySpreadConstraint.NodeAffinityPolicy", "common.go#matchNodeInclusionPolicies",
              "filtering.go#calPreFilterState", "scoring.go#PreScore", "spec S16", "per context"):
        assert s in h, s


def test_null_context_and_null_pointer_are_statuses():
    lib = qsched.load()
    v = ctypes.c_int32(7)
    assert lib.qs_set_topology_spread_node_affinity_policy(None, _abi.QS_POLICY_HONOR) == _abi.QS_EINVAL
    assert lib.qs_get_topology_spread_node_affinity_policy(None, ctypes.byref(v)) == _abi.QS_EINVAL
    assert lib.qs_get_topology_spread_node_affinity_policy(None, None) == _abi.QS_EINVAL
    assert v.value == 7


# ---- known answers ------------------------------------------------------------------------------
# winners' totals under HONOR (0 = unschedulable): LeastAllocated + BalancedAllocation of the 8-core nodes
# with 0 / 1 / 2 pods on them (274 / 250 / 224, spec/kat.md K42), the S14 term where a soft pod wins
KAT_TOTALS = {"K48": [274, 274, 250], "K49": [274, 274, 274], "K50": [274, 250, 474, 474], "K51": [274, 274, 250],
              "K52": [274, 274, 274]}


@pytest.mark.parametrize("name", list(KAT_TOTALS))
def test_kat_streams(name):
    nodes, pods, cfg, honor, ignore = HC.kat(name)
    pl, keys, _, st = HR.run(nodes, pods, cfg)
    assert list(pl) == honor
    assert [int(k) for k in keys] == [key(t, n) if n >= 0 else 0 for t, n in zip(KAT_TOTALS[name], honor)]
    assert list(HR.run(nodes, pods, cfg, policy=HR.IGNORE)[0]) == ignore
    assert list(HR.run(nodes, pods, cfg, variant="ignore")[0]) == ignore
    assert int(st.node[3].sum()) == sum(n >= 0 for n in honor)


def test_kat_k48_the_domains_alone_decide():
    """The counts are the same under either rule (every pod of the app sits in M): Honor's domains place the
    third pod, and the variant with Honor's counts over all zones of the table strands it."""
    nodes, pods, cfg, honor, _ = HC.kat("K48")
    assert list(HR.run(nodes, pods, cfg, variant="domains_only")[0]) == honor
    assert list(HR.run(nodes, pods, cfg, variant="counts_only")[0]) == [0, 1, -1]


def test_kat_k49_the_counts_alone_decide():
    """Both zones hold a node of M: the domains are the table's, and the pod outside M is what differs."""
    nodes, pods, cfg, honor, ignore = HC.kat("K49")
    assert list(HR.run(nodes, pods, cfg, variant="counts_only")[0]) == honor
    assert list(HR.run(nodes, pods, cfg, variant="domains_only")[0]) == ignore


def test_kat_k50_zone_scores():
    nodes, pods, cfg, honor, ignore = HC.kat("K50")
    for policy, want_pl in ((HR.HONOR, honor), (HR.IGNORE, ignore)):
        on = {k: v.copy() for k, v in nodes.items()}
        st = HR.HonorState(nodes["zone"], nodes["label_bits"], policy)
        log = []
        for j in range(4):
            zs = HR.pod_zone_scores(on, pods, j, st, cfg)
            if j >= 2:
                assert tuple(zs[:2]) == HC.K50_ZONE_SCORES[policy][j - 2] and (zs[2:] == -1).all()
                st.log = log
            k = HR.pod_keys(on, pods, j, st, cfg)
            st.log = None
            n = 0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)
            assert n == want_pl[j]
            A.reserve(on, pods, j, n)
            st.record(3, n)
        # (D, domains of the table, mn, mx) of the two soft pods: cH changes mn / mx
        assert [e[2:] for e in log] == ([(0, 0), (0, 1)] if policy == HR.HONOR else [(0, 3), (1, 3)])
        assert all(e[:2] == (2, 2) for e in log)


def test_kat_k51_the_hostname_minimum_runs_over_m():
    nodes, pods, cfg, honor, ignore = HC.kat("K51")
    assert list(HR.run(nodes, pods, cfg, variant="domains_only")[0]) == honor
    assert list(HR.run(nodes, pods, cfg, variant="counts_only")[0]) == ignore
    assert list(H.run(nodes, pods, cfg)[0]) == ignore


def test_kat_k52_is_s13():
    nodes, pods, cfg, honor, _ = HC.kat("K52")
    pl, keys, _, _ = S.run(nodes, pods, cfg)
    got = HR.run(nodes, pods, cfg)
    assert list(pl) == honor and np.array_equal(got[0], pl) and np.array_equal(got[1], keys)


# ---- properties of the reference ----------------------------------------------------------------
def test_match_is_the_node_affinity_filter():
    """M(pod) against the oracle's own filter: a pod asking for nothing is feasible exactly on M."""
    case = HC.parity_case("spread-70-default-compact")
    nodes, pods = case["nodes"], qsched.pods_from_struct(case["pods"])
    free = {k: v.copy() for k, v in pods.items()}
    for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "req_ext", "anti_affinity"):
        free[f][:] = 0
    open_ = {k: v.copy() for k, v in nodes.items()}
    open_["max_pods"][:] = 110
    seen = set()
    for j in range(60):
        m = HR.matches(nodes["label_bits"], pods, j)
        assert np.array_equal(A.oracle_scorer(case["cfg"])(open_, free, j) != 0, m), j
        assert HR.restricts(pods, j) or m.all()
        seen.add(int(m.sum()))
    assert len(seen) >= 4  # several different node sets, the whole table among them


@pytest.mark.parametrize("mod,name", [(SC, "scan-700"), (SSC, "scan-700"), (HSC, "scan-24"), (HSC, "norm-scan")],
                         ids=["s13", "s14", "s15", "s15-norm"])
def test_on_the_older_parity_inputs_the_reference_is_the_older_reference(mod, name):
    """The parity inputs of S13 / S14 / S15.  Where none of their spread pods restricts (config 5 has no
    selectors), HONOR is the older reference; where some do (config 4), IGNORE is."""
    case = mod.parity_case(name)
    nodes, pods, cfg = case["nodes"], case["pods"], case["ocfg"]
    policy = HR.IGNORE if HC.restricting(pods).any() else HR.HONOR
    assert (policy == HR.IGNORE) == (name == "norm-scan")
    got = HR.run(nodes, pods, cfg, HC.C.scorer_of(case["kind"], cfg), policy=policy)
    assert np.array_equal(got[0], case["pl"]) and np.array_equal(got[1], case["keys"])


def test_an_appended_node_opens_a_domain():
    nodes, pods, cfg, honor, _ = HC.kat("K48")
    pl, _, final, st = HR.run(nodes, pods, cfg)
    one = {k: v[:1] for k, v in pods.items()}
    st.set_pod(one, 0)
    assert list(st.infeasible(3, HC.SP1)) == [True, False, False]  # cH = (2, 1), m = 1
    grown = {k: np.concatenate([v, v[:1]]) for k, v in final.items()}
    grown["zone"][3] = 7
    st.set_table(grown["zone"], grown["label_bits"])
    st.set_pod(one, 0)
    assert st.pod_domains()[[0, 1, 2, 7]].tolist() == [True, True, False, True]
    assert list(st.infeasible(3, HC.SP1)) == [True, True, False, False]  # m drops to 0


# ---- the GPU file's inputs, from the reference alone ---------------------------------------------
@pytest.mark.parametrize("name", list(HC.PARITY))
def test_parity_inputs_meet_their_conditions(name):
    HC.check_conditions(HC.parity_case(name))
