"""``nodeTaintsPolicy: Honor`` of the topology spread constraints (spec/semantics.md S17;
qs_set_topology_spread_node_taints_policy), no GPU:

* the two symbols, the header text, and the status of a null context or pointer;
* the known answers K53-K58 of spec/kat.md through tests/taint_spread_ref.py, under both policies;
* properties of the reference: under IGNORE, and for pods that tolerate every bit, it is the reference of S16;
* the conditions that make the parity inputs of tests/test_gpu_taint_spread.py worth running;
* the resource budget of the kernels that carry the widened predicate, from the code objects.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import qsched
from qsched import _abi

import antiaffinity_ref as A
import honor_spread_cases as HC
import honor_spread_ref as HR
import taint_spread_cases as TC
import taint_spread_ref as TR


def key(total, node):
    return ((total + 1) << 32) | (0xFFFFFFFF - node)


# ---- the interface -------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    lib = qsched.load()
    for s in ("qs_set_topology_spread_node_taints_policy", "qs_get_topology_spread_node_taints_policy"):
        assert s in _abi.EXPORTED and hasattr(lib, s), s
    assert (_abi.QS_POLICY_IGNORE, _abi.QS_POLICY_HONOR) == (0, 1) == (TR.IGNORE, TR.HONOR)
    assert qsched.POLICIES == {"ignore": 0, "honor": 1}
    assert hasattr(qsched.Scheduler, "set_topology_spread_node_taints_policy")
    assert hasattr(qsched.Scheduler, "get_topology_spread_node_taints_policy")
    # the ABI version and the struct sizes stay
    assert _abi.QS_ABI_VERSION == 3 and lib.qs_struct_size(3) == _abi.POD_DTYPE.itemsize


def test_header_declares_the_additions():
    here = os.path.dirname(os.path.abspath(__file__))
    h = open(os.path.join(here, "..", "include", "qsched.h")).read()
    assert "#define QS_ABI_VERSION 3" in h
    for s in ("typedef enum qs_node_inclusion_policy { QS_POLICY_IGNORE = 0, QS_POLICY_HONOR = 1 } qs_node_inclusion_policy;",
              "QS_API qs_status qs_set_topology_spread_node_taints_policy(qs_ctx *ctx, int32_t policy);",
              "QS_API qs_status qs_get_topology_spread_node_taints_policy(qs_ctx *ctx, int32_t *policy);",
              "apis/core#TopologySpreadConstraint.NodeTaintsPolicy", "common.go#matchNodeInclusionPolicies",
              "FindMatchingUntoleratedTaint", "DoNotScheduleTaintsFilterFunc", "KEP-3094", "spec S17",
              "enable_taint = 0"):
        assert s in h, s


def test_null_context_and_null_pointer_are_statuses():
    lib = qsched.load()
    v = ctypes.c_int32(7)
    assert lib.qs_set_topology_spread_node_taints_policy(None, _abi.QS_POLICY_HONOR) == _abi.QS_EINVAL
    assert lib.qs_get_topology_spread_node_taints_policy(None, ctypes.byref(v)) == _abi.QS_EINVAL
    assert lib.qs_get_topology_spread_node_taints_policy(None, None) == _abi.QS_EINVAL
    assert v.value == 7


# ---- known answers ------------------------------------------------------------------------------
# winners' totals under HONOR (0 = unschedulable): LeastAllocated + BalancedAllocation of the 8-core nodes with
# 0 / 1 / 2 pods on them (274 / 250 / 224, spec/kat.md K42) plus 300 of TaintToleration on every node (no soft
# taint in these tables: raw 0 everywhere, normalized and reversed to 100, default weight 3), and the S14 term
# where a soft pod wins
KAT_TOTALS = {"K53": [574, 574, 574, 550], "K54": [574, 574, 550], "K55": [574, 574, 574],
              "K56": [574, 550, 774, 774], "K57": [574, 574, 550], "K58": [574, 574, 574]}


@pytest.mark.parametrize("name", TC.KATS)
def test_kat_streams(name):
    nodes, pods, cfg, policy, honor, ignore = TC.kat(name)
    pl, keys, _, st = TR.run(nodes, pods, cfg, policy=policy)
    assert list(pl) == honor
    assert [int(k) for k in keys] == [key(t, n) if n >= 0 else 0 for t, n in zip(KAT_TOTALS[name], honor)]
    assert list(TR.run(nodes, pods, cfg, policy=policy, taints_policy=TR.IGNORE)[0]) == ignore
    assert list(TR.run(nodes, pods, cfg, policy=policy, variant="ignore")[0]) == ignore
    assert int(st.node[3].sum()) == sum(n >= 0 for n in honor)


def test_kat_k53_the_tainted_node_pins_the_minimum_under_ignore():
    """Under Ignore the reference is S15's and S16's own: the fourth pod is stranded."""
    import hostspread_ref as H

    nodes, pods, cfg, _, honor, ignore = TC.kat("K53")
    assert list(H.run(nodes, pods, cfg)[0]) == ignore
    assert list(HR.run(nodes, pods, cfg, policy=HR.HONOR)[0]) == ignore  # (no selector: S16 changes nothing)
    assert list(TR.run(nodes, pods, cfg, variant="domains_only")[0]) == honor
    assert list(TR.run(nodes, pods, cfg, variant="counts_only")[0]) == ignore


def test_kat_k54_the_domains_alone_decide():
    nodes, pods, cfg, _, honor, ignore = TC.kat("K54")
    assert list(TR.run(nodes, pods, cfg, variant="domains_only")[0]) == honor
    assert list(TR.run(nodes, pods, cfg, variant="counts_only")[0]) == ignore


def test_kat_k55_the_counts_alone_decide():
    nodes, pods, cfg, _, honor, ignore = TC.kat("K55")
    assert list(TR.run(nodes, pods, cfg, variant="counts_only")[0]) == honor
    assert list(TR.run(nodes, pods, cfg, variant="domains_only")[0]) == ignore


def test_kat_k56_zone_scores():
    nodes, pods, cfg, policy, honor, ignore = TC.kat("K56")
    for tp, want_pl in ((TR.HONOR, honor), (TR.IGNORE, ignore)):
        on = {k: v.copy() for k, v in nodes.items()}
        st = TR.state_of(nodes, policy, tp)
        log = []
        for j in range(4):
            zs = TR.pod_zone_scores(on, pods, j, st, cfg)
            if j >= 2:
                assert tuple(zs[:2]) == TC.K56_ZONE_SCORES[tp][j - 2] and (zs[2:] == -1).all()
                st.log = log
            k = TR.pod_keys(on, pods, j, st, cfg)
            st.log = None
            n = 0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)
            assert n == want_pl[j]
            A.reserve(on, pods, j, n)
            st.record(3, n)
        # (D, domains of the table, mn, mx) of the two soft pods: cH changes mn / mx
        assert [e[2:] for e in log] == ([(0, 0), (0, 1)] if tp == TR.HONOR else [(0, 3), (1, 3)])
        assert all(e[:2] == (2, 2) for e in log)


def test_kat_k57_the_intersection_decides():
    """M_A = {0, 1, 2}, M_T = {0, 1, 3}: either policy alone leaves a node with count 0 in the set, and the
    third pod is stranded; only both place it."""
    nodes, pods, cfg, _, honor, stranded = TC.kat("K57")
    op = A.pods_dict(pods)
    ma, mt = HR.matches(nodes["label_bits"], op, 0), TR.tolerated(nodes["taint_hard"], op, 0)
    assert list(np.flatnonzero(ma)) == [0, 1, 2] and list(np.flatnonzero(mt)) == [0, 1, 3]
    got = {(a, t): list(TR.run(nodes, pods, cfg, policy=a, taints_policy=t)[0]) for a in (0, 1) for t in (0, 1)}
    assert got == {(1, 1): honor, (1, 0): stranded, (0, 1): stranded, (0, 0): stranded}
    assert list(TR.run(nodes, pods, cfg, policy=TR.HONOR, variant="affinity_only")[0]) == stranded
    assert list(HR.run(nodes, pods, cfg, policy=HR.HONOR)[0]) == stranded


def test_kat_k58_is_s13():
    import spread_ref as S

    nodes, pods, cfg, _, honor, _ = TC.kat("K58")
    pl, keys, _, _ = S.run(nodes, pods, cfg)
    got = TR.run(nodes, pods, cfg)
    assert list(pl) == honor and np.array_equal(got[0], pl) and np.array_equal(got[1], keys)


# ---- properties of the reference ----------------------------------------------------------------
def test_tolerated_is_the_taint_toleration_filter():
    """M_T(pod) against the oracle's own filter: a pod asking for nothing is feasible exactly on M_T."""
    case = TC.parity_case("pool-65-wide")
    nodes, pods = case["nodes"], qsched.pods_from_struct(case["pods"])
    free = {k: v.copy() for k, v in pods.items()}
    for f in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "req_ext", "anti_affinity"):
        free[f][:] = 0
    open_ = {k: v.copy() for k, v in nodes.items()}
    open_["max_pods"][:] = 110
    seen = set()
    for j in range(60):
        m = TR.tolerated(nodes["taint_hard"], pods, j)
        assert np.array_equal(A.oracle_scorer(case["cfg"])(open_, free, j) != 0, m), j
        seen.add(int(m.sum()))
    assert len(seen) == 3  # tol_hard 0, T1, all ones: three node sets, the whole table among them


@pytest.mark.parametrize("name", ["spread-70-norm-compact", "soft-300-norm-wide", "host-70-norm-compact"])
def test_under_ignore_the_reference_is_s16s(name):
    """S16's parity inputs of the normalizing class (no hard taint in the table, tol_hard 0): nodeTaintsPolicy
    IGNORE is S16's reference, and so is HONOR, because M_T is every node of the table."""
    case = HC.parity_case(name)
    for tp in (TR.IGNORE, TR.HONOR):
        got = TR.run(case["nodes"], case["pods"], case["cfg"], policy=TR.HONOR, taints_policy=tp)
        assert np.array_equal(got[0], case["pl"]) and np.array_equal(got[1], case["keys"])


def test_a_taint_added_to_a_node_leaves_the_set():
    nodes, pods, cfg, _, _, _ = TC.kat("K54")
    st = TR.state_of(nodes)
    op = A.pods_dict(pods)
    st.set_pod(op, 0)
    assert list(np.flatnonzero(st.M)) == [0, 1] and st.pod_domains()[[0, 1, 2]].tolist() == [True, True, False]
    th = nodes["taint_hard"].copy()
    th[1] = 1
    st.set_table(nodes["zone"], nodes["label_bits"], th)
    st.set_pod(op, 0)
    assert list(np.flatnonzero(st.M)) == [0] and st.pod_domains()[[0, 1, 2]].tolist() == [True, False, False]


# ---- the GPU file's inputs, from the reference alone ---------------------------------------------
@pytest.mark.parametrize("name", list(TC.PARITY))
def test_parity_inputs_meet_their_conditions(name):
    TC.check_conditions(TC.parity_case(name))


# ---- the kernels' budget, from the code objects --------------------------------------------------
def test_the_kernels_that_carry_the_predicate_keep_their_budget():
    """k_scan_norm / _key / _commit and k_score_podg(_max) of the two classes with kFeatAA and the normalizing
    plugins (119 compact, 127 wide), the only kernels the widened honor_match and pod_honor compile into: no
    scratch, no VGPR spill, at most 256 VGPRs."""
    from test_kernel_resources import LLVM, kernel_metadata
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("the ROCm LLVM tools are absent")
    seen = {}
    for n, f in kernel_metadata():
        m = re.search(r"(k_scan_norm|k_scan_key|k_scan_commit|k_score_podg_max|k_score_podg)ILj(\d+)E", n)
        if not m or int(m.group(2)) not in (119, 127):
            continue
        seen.setdefault(m.group(1), set()).add(int(m.group(2)))
        print(m.group(1), m.group(2), {k: f[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size",
                                                         "vgpr_spill_count") if k in f})
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["vgpr_count"] <= 256, (n[:60], f)
    assert len(seen) == 5 and all(v == {119, 127} for v in seen.values()), seen
