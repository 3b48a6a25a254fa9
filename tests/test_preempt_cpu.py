"""Preemption dry run (spec/semantics.md S18) without a GPU: the reference tests/preempt_ref.py against the
hand-computed known answers K59-K67 of spec/kat.md, the conditions every parity case of
tests/preempt_cases.py states about itself (checked from the reference alone), and the C ABI of the
feature: the symbols, the victim record and the status codes of calls that never reach a device.
"""
import ctypes

import numpy as np
import pytest

import qsched
from qsched import _abi

import preempt_cases as C
import preempt_ref as R


@pytest.mark.parametrize("name", C.KATS)
def test_known_answers(name):
    k = C.kat(name)
    ref = C.kat_ref(k)
    node, victims, nvict_n = ref.preempt(k["pod"])
    assert node == k["node"]
    assert [e["seq"] for e in victims] == k["victims"]
    assert list(nvict_n) == k["nvict_n"]


def test_k59_wrong_variants():
    """The variants are wrong where the spec says so: K59's walk reprieves two of three pods, K60's choice
    puts the top victim before the count, K64's class decides under BY_QOS."""
    k = C.kat("K59")
    assert len(C.kat_ref(k).preempt(k["pod"], "no_reprieve")[1]) == 3
    k = C.kat("K60")
    assert C.kat_ref(k).preempt(k["pod"], "count_first")[0] == 0
    k = C.kat("K64b")
    assert C.kat_ref(k).preempt(k["pod"], "priority_only")[0] == 1
    # reprieve_low_first: walking K59's list from the least important pod keeps B and gives up A as well,
    # but on a node where the order matters the victims change
    nodes = C.mk_nodes([3000])
    ref = R.Ref(nodes)
    for cpu, prio in ((2000, 5), (1000, 0)):
        ref.reserve(0, C.mk_pod(cpu, C.GI, prio, 1))
    pod = C.mk_pod(1000, C.GI, 10, 2)
    assert [e["seq"] for e in ref.preempt(pod)[1]] == [2]                         # the priority-5 pod is reprieved
    assert [e["seq"] for e in ref.preempt(pod, "reprieve_low_first")[1]] == [1]   # ... or lost


def test_k67_evict_and_unreserve():
    """K67: qs_unreserve takes the highest seq among equal pods, qs_evict the named one; both give the
    row back what the entry added."""
    ref = R.Ref(C.mk_nodes([4000]))
    a, b = C.mk_pod(1000, C.GI, 0, 1), C.mk_pod(500, C.GI, 7, 1)
    for p in (a, b, a):
        ref.reserve(0, p)
    assert [e["seq"] for e in ref.node_pods(0)] == [2, 1, 3]
    assert ref.unreserve(0, a) and [e["seq"] for e in ref.node_pods(0)] == [2, 1]
    assert not ref.unreserve(0, C.mk_pod(1000, C.GI, 1, 1))  # no equal entry: nothing changes
    assert ref.evict(0, 2) and not ref.evict(0, 2)
    assert int(ref.t["req_cpu"][0]) == 1000 and int(ref.t["pods"][0]) == 1


@pytest.mark.parametrize("name", C.CASES)
def test_case_conditions(name):
    C.check_conditions(name)


def test_importance():
    assert R.importance(R.BY_PRIORITY, 2, C.I32_MIN) == 0
    assert R.importance(R.BY_PRIORITY, 0, C.I32_MAX) == (1 << 32) - 1
    assert R.importance(R.BY_QOS, 1, C.I32_MIN) == 1 << 32 > R.importance(R.BY_QOS, 0, C.I32_MAX)
    assert R.importance(R.BY_QOS, 2, -1) == (2 << 32) + (1 << 31) - 1


# ---- C ABI ---------------------------------------------------------------------------------------
NEW_SYMBOLS = ("qs_set_preemption", "qs_get_preemption", "qs_set_preemption_policy", "qs_get_preemption_policy",
               "qs_node_pods", "qs_preempt_pod", "qs_evict")


def test_abi_symbols_and_victim_record():
    lib = qsched.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _abi.EXPORTED
    assert lib.qs_struct_size(7) == 72 == _abi.VICTIM_DTYPE.itemsize
    assert _abi.VICTIM_DTYPE.fields["priority"][1] == 56 and _abi.VICTIM_DTYPE.fields["req_ext"][1] == 24
    assert lib.qs_struct_size(3) == 248  # qs_pod is untouched
    assert _abi.QS_ABI_VERSION == 3 and _abi.QS_MAX_VICTIMS == 256
    header = open(__import__("test_abi").HEADER).read()
    assert "#define QS_MAX_VICTIMS 256" in header and "#define QS_ABI_VERSION 3" in header


def test_status_codes_without_a_context():
    """Every new entry point returns QS_EINVAL for a null context (as the rest of the ABI does), and
    never crashes."""
    lib = qsched.load()
    v = ctypes.c_int32(0)
    n = ctypes.c_uint32(0)
    pod = np.zeros(1, _abi.POD_DTYPE)
    vic = np.zeros(_abi.QS_MAX_VICTIMS, _abi.VICTIM_DTYPE)
    assert lib.qs_set_preemption(None, 1) == _abi.QS_EINVAL
    assert lib.qs_get_preemption(None, ctypes.byref(v)) == _abi.QS_EINVAL
    assert lib.qs_set_preemption_policy(None, 1) == _abi.QS_EINVAL
    assert lib.qs_get_preemption_policy(None, ctypes.byref(v)) == _abi.QS_EINVAL
    assert lib.qs_node_pods(None, 0, None, 0, ctypes.byref(n)) == _abi.QS_EINVAL
    assert lib.qs_preempt_pod(None, pod.ctypes.data, ctypes.byref(v), vic.ctypes.data, ctypes.byref(n),
                              None) == _abi.QS_EINVAL
    assert lib.qs_evict(None, 0, 1) == _abi.QS_EINVAL
