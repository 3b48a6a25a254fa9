"""Required pod anti-affinity in exact mode (spec/semantics.md S12), no GPU:

* tests/antiaffinity_ref.py against the batched oracle with ``batch = 1`` (placements, keys, final
  table) on folded config-5 inputs, with the conditions that make the inputs worth running;
* the known answers K27-K31 of spec/kat.md through the reference;
* the ABI additions (the two symbols, and a status for a null context);
* the register budget of the new PERSISTENT and SCAN instantiations, from the code-object metadata.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import qsched
from qsched import checks
from oracle import oracle as O
from qsched import _abi

import antiaffinity_ref as A
import antiaffinity_cases as C


def _equal_tables(a, b):
    return all(np.array_equal(a[k], b[k]) for k in b)


# ---- the reference against the batch-of-one oracle ----------------------------------------------
@pytest.mark.parametrize("n,p,apps,zones", [(300, 3000, 40, 4), (64, 600, 20, 3)])
def test_reference_equals_batched_oracle_of_one(n, p, apps, zones):
    """The fold of this test keeps the app ids small ((app % apps), the kind of an app = that of its
    first pod).  On this fold: n = 300, p = 3000: 2,833 pods placed differently from oracle.schedule,
    282 ZONE pods unschedulable; n = 64, p = 600: 520 and 50."""
    nodes, pods = O.generate(5, n, p)
    nodes, pods = A.fold(nodes, pods, apps, zones, 1, 0)
    pl, keys, final, state = A.run(nodes, pods)
    b = {k: v.copy() for k, v in nodes.items()}
    bpl, bkeys, batches = O.schedule_batched(b, pods, batch=1)
    assert np.array_equal(pl, bpl) and np.array_equal(keys, bkeys) and _equal_tables(final, b)
    e = {k: v.copy() for k, v in nodes.items()}
    epl, _, _ = O.schedule(e, pods)
    differ = int((pl != epl).sum())
    zone_unsched = int(((pl < 0) & (pods["anti_affinity"] == A.ZONE)).sum())
    print(f"n={n} p={p}: {differ} placed differently from oracle.schedule, {zone_unsched} ZONE pods unschedulable")
    assert differ >= 1 and zone_unsched >= 1
    # the recorded state is the placements'
    placed = pl >= 0
    want = np.zeros_like(state.node)
    np.add.at(want, (pods["app"][placed], pl[placed]), 1)
    assert np.array_equal(state.node, want)
    assert checks.batched_invariants(nodes, pods, pl, final)["anti_affinity"]


def test_parity_inputs_meet_their_conditions():
    """Every parity input of tests/test_gpu_antiaffinity.py, from the reference alone: a pod placed
    differently than under oracle.schedule, an unschedulable ZONE pod, and in the tight case an
    unschedulable HOSTNAME pod."""
    for name in C.PARITY:
        case = C.parity_case(name)
        C.check_conditions(case)


# ---- known answers ------------------------------------------------------------------------------
def key(total, node):
    return ((total + 1) << 32) | (0xFFFFFFFF - node)


@pytest.mark.parametrize("name", ["K27", "K28", "K29", "K30"])
def test_kat_streams(name):
    nodes, pods, cfg, want_pl, want_tot = C.kat(name)
    pl, keys, _, _ = A.run(nodes, pods, cfg)
    assert list(pl) == want_pl
    assert [int(k) for k in keys] == [key(t, n) if n >= 0 else 0 for t, n in zip(want_tot, want_pl)]
    # without the filter the second pod goes elsewhere (what the case is about)
    e = {k: v.copy() for k, v in nodes.items()}
    epl, _, _ = O.schedule(e, pods, cfg)
    assert list(epl) != want_pl


def test_kat_k30_against_the_larger_maximum():
    """K30's aside: normalized against the maximum of all three nodes node 2 would win."""
    nodes, pods, cfg, _, _ = C.kat("K30")
    A.reserve(nodes, pods, 0, 0)
    k, sc = O.score_pod(nodes, pods, 1, cfg)
    assert [int(x >> 32) - 1 for x in k] == [525, 400, 417]
    st = A.State(nodes["zone"])
    st.record(9, 0)
    k = A.pod_keys(nodes, pods, 1, st, cfg)
    assert [int(x >> 32) - 1 if x else -1 for x in k] == [-1, 458, 441]


def test_kat_k31_unreserve_reopens():
    nodes, pods, cfg, _, _ = C.kat("K31")
    st = A.State(nodes["zone"])
    H, Z = 0, 1

    def feas(j):
        return [i for i, k in enumerate(A.pod_keys(nodes, pods, j, st, cfg)) if k]

    def best(j):
        k = A.pod_keys(nodes, pods, j, st, cfg)
        return int(0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)) if k.max() else -1

    for node, sign, want in C.K31_STEPS:
        assert st.record(4, node, sign)
        A.reserve(nodes, pods, H, node, sign)
        assert feas(H) == want and feas(Z) == want
        assert best(H) == best(Z) == (want[0] if want else -1)
    assert not st.record(4, 0, -1)  # nothing of app 4 left on node 0: refused, nothing changes
    assert st.node.sum() == 0 and st.zcount.sum() == 0


def test_presence_survives_the_first_unreserve():
    st = A.State(np.array([0, 1]))
    st.record(3, 1)
    st.record(3, 1)
    assert st.record(3, 1, -1) and st.presence()[3, 1] and st.zcount[3, 1] == 1
    assert st.record(3, 1, -1) and not st.presence()[3, 1] and st.zcount[3, 1] == 0


# ---- ABI ----------------------------------------------------------------------------------------
def test_abi_additions():
    lib = qsched.load()
    for s in ("qs_set_pod_anti_affinity", "qs_get_pod_anti_affinity"):
        assert hasattr(lib, s) and s in _abi.EXPORTED
    assert lib.qs_set_pod_anti_affinity(None, 1) == _abi.QS_EINVAL  # null context: a status, no crash
    assert lib.qs_get_pod_anti_affinity(None, None) == _abi.QS_EINVAL
    assert lib.qs_struct_size(3) == _abi.POD_DTYPE.itemsize and _abi.QS_ABI_VERSION == 3
    assert hasattr(qsched.Scheduler, "set_pod_anti_affinity") and hasattr(qsched.Scheduler, "get_pod_anti_affinity")


# ---- kernel budget ------------------------------------------------------------------------------
AA = 64  # kFeatAA


def test_antiaffinity_kernels_are_built_within_the_register_budget():
    """libqsched.so carries k_persistent, the scan kernels and the score kernels for the six kFeatAA
    classes (compact / wide x default, general, general + normalizing), and no lookahead kernel for
    any of them; every persistent and scan instantiation without scratch or VGPR spills and within
    256 VGPRs, as tests/test_kernel_resources.py asserts for the resident stream."""
    from test_kernel_resources import LLVM, kernel_metadata
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("the ROCm LLVM tools are absent")

    def feat(name):
        m = re.search(r"ILj(\d+)E", name) or re.search(r"ELj(\d+)E", name)
        return int(m.group(1)) if m else 0

    meta = [(n, f) for n, f in kernel_metadata() if feat(n) & AA]
    classes = {68, 116, 119, 76, 124, 127}
    for kern in ("k_persistent", "k_scan_key", "k_scan_norm", "k_scan_commit", "k_score_pod1", "k_score_podg"):
        got = {feat(n) for n, _ in meta if kern + "I" in n}
        assert got == classes, (kern, got)
    assert {feat(n) for n, _ in meta if "k_scan_soaI" in n} == {68, 116}  # (compact rows, no normalizing plugin)
    assert not [n for n, _ in meta if "k_la_" in n or "k_batch_claim" in n]
    bad = [(n[:100], f) for n, f in meta if ("k_persistent" in n or "k_scan_" in n) and
           (f["private_segment_fixed_size"] or f["vgpr_spill_count"] or f["vgpr_count"] > 256)]
    assert not bad, bad
    assert any("k_aa_apply" in n for n, _ in kernel_metadata())
