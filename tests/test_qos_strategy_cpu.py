"""One NodeResourcesFit scoring strategy per QoS class (spec/semantics.md S9 "Strategy per QoS class",
qs_set_scoring_strategy_qos), no GPU:

* tests/qos_strategy_ref.py with the three classes equal against tests/strategy_ref.py;
* the known answers K24-K26 of spec/kat.md against the reference and the C++ CPU reference plugins
  (tests/native/qos_strategy_driver);
* the framework runtime with three profiles, each with its own NodeResourcesFit instance, against the
  reference on a small cluster;
* the ABI additions;
* discrimination: on the inputs of tests/test_gpu_qos_strategy.py the per-class configuration places
  differently from every one-strategy configuration it is built from (otherwise the GPU parity tests
  would show nothing).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import qsched
from qsched import _abi

import qos_strategy_cases as C
import qos_strategy_ref as QR
import strategy_ref as R
from test_gpu_strategy import STRATEGIES  # (the values only: nothing here needs a GPU)
from test_strategy_cpu import CLUSTER_CFG, ZERO_MOD, small_cluster, strategy_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "native", "qos_strategy_driver")
GIB, MIB = 1 << 30, 1 << 20


def driver(*args):
    if not os.path.exists(DRIVER):
        pytest.fail("tests/native/qos_strategy_driver is not built (make -C custom-k8s-scheduler_amd)")
    out = subprocess.run([DRIVER, *map(str, args)], check=True, capture_output=True, text=True).stdout
    return [int(x) for x in out.split()]


def three_args(per):
    """The driver's three strategies in class order from a qos_strategies dict."""
    cs = QR.class_cfgs(dict(qos_strategies=per))
    return [v for c in cs for v in strategy_args(c)]


# ---- the reference with the classes equal -------------------------------------------------------
@pytest.mark.parametrize("strat", list(STRATEGIES))
def test_equal_classes_are_the_uniform_reference(strat):
    nodes, pods = small_cluster(77)
    assert set(pods["qos"].tolist()) == {0, 1, 2}
    want = R.run(nodes, pods, dict(CLUSTER_CFG, **STRATEGIES[strat]))
    per = {q: STRATEGIES[strat] for q in QR.QOS}
    for cfg in (dict(CLUSTER_CFG, qos_strategies=per),            # every class listed
                dict(CLUSTER_CFG, **STRATEGIES[strat]),           # none listed: the context-wide one
                dict(CLUSTER_CFG, **STRATEGIES[strat], qos_strategies={1: STRATEGIES[strat]})):
        got = QR.run(nodes, pods, cfg)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        for k in want[2]:
            assert np.array_equal(got[2][k], want[2][k]), k


# ---- known answers (spec/kat.md K24-K26) --------------------------------------------------------
KAT_MIX = {"BestEffort": C.MOST, "Burstable": C.rtcr(C.FALL30), "Guaranteed": C.LEAST}
# name, qos, pod (req cpu, req MiB, nz cpu, nz MiB), fit score per node, total per node, winner
KAT = [
    ("K24", 0, (0, 0, 100, 200), (51, 12), (151, 110), 0),
    ("K25", 1, (200, 512, 200, 512), (0, 50), (99, 199), 1),
    ("K26", 2, (1000, 4096, 1000, 4096), (25, 63), (175, 287), 1),
]


def kat_cluster(qos, pod):
    """Two nodes of 4000 m / 16 GiB: node 0 holds 2000 m / 8 GiB (fuller), node 1 400 m / 2 GiB."""
    from oracle import oracle as O
    nodes, pods = O.empty_cluster(2, 1)
    nodes["max_pods"][:] = 110
    nodes["alloc_cpu"][:], nodes["alloc_mem"][:] = 4000, 16 * GIB
    nodes["req_cpu"][:] = nodes["nz_cpu"][:] = (2000, 400)
    nodes["req_mem"][:] = nodes["nz_mem"][:] = (8 * GIB, 2 * GIB)
    nodes["pods"][:] = (10, 2)
    pods["req_cpu"][0], pods["req_mem"][0] = pod[0], pod[1] * MIB
    pods["nz_cpu"][0], pods["nz_mem"][0] = pod[2], pod[3] * MIB
    pods["qos"][0] = qos
    return nodes, pods


@pytest.mark.parametrize("name,qos,pod,fit,total,winner", KAT, ids=[k[0] for k in KAT])
def test_kat_reference(name, qos, pod, fit, total, winner):
    nodes, pods = kat_cluster(qos, pod)
    ok, sc, tot, best = QR.score_pod(nodes, pods, 0, dict(qos_strategies=KAT_MIX))
    assert ok.all() and tuple(sc[:, 0]) == fit and tuple(tot) == total and best == winner
    pl, keys, _ = QR.run(nodes, pods, dict(qos_strategies=KAT_MIX))
    assert pl[0] == winner and int(keys[0]) == ((total[winner] + 1) << 32) | (0xFFFFFFFF - winner)


@pytest.mark.parametrize("name,qos,pod,fit,total,winner", KAT, ids=[k[0] for k in KAT])
def test_kat_cpu_plugins(name, qos, pod, fit, total, winner):
    nodes, pods = kat_cluster(qos, pod)
    for i in range(2):
        ent = [(int(nodes["alloc_cpu"][i]), int(nodes["nz_cpu"][i] + pods["nz_cpu"][0]), 1),
               (int(nodes["alloc_mem"][i]), int(nodes["nz_mem"][i] + pods["nz_mem"][0]), 1)]
        assert driver("kat", qos, *three_args(KAT_MIX), 2, *[v for e in ent for v in e]) == [fit[i]]


# ---- the framework runtime with three profiles --------------------------------------------------
@pytest.mark.parametrize("per", [C.MIX, C.TWO_TABLES, KAT_MIX], ids=["mix", "two-tables", "kat-mix"])
def test_three_profiles_place_like_the_reference(per):
    seed = 77
    nodes, pods = small_cluster(seed)
    pl, keys, _ = QR.run(nodes, pods, dict(CLUSTER_CFG, qos_strategies=per))
    assert (pl >= 0).sum() > 50
    out = driver("loop", seed, 60, 150, ZERO_MOD, *three_args(per))
    cpl, ctot, cqos = out[:150], out[150:300], out[300:]
    assert cqos == pods["qos"].tolist() and set(cqos) == {0, 1, 2}
    assert cpl == list(pl)
    scored = [j for j in range(150) if ctot[j] >= 0]
    assert len(scored) > 100
    assert [((ctot[j] + 1) << 32) | (0xFFFFFFFF - cpl[j]) for j in scored] == [int(keys[j]) for j in scored]
    # ... and unlike the one-strategy configurations it is built from
    for u in C.uniform_cfgs(dict(qos_strategies=per)):
        assert not np.array_equal(R.run(nodes, pods, dict(CLUSTER_CFG, **u))[0], pl), u


# ---- ABI ----------------------------------------------------------------------------------------
def test_abi_additions():
    """libqsched.so exports the per-class setter and getter (it did not before they were added)."""
    lib = qsched.load()
    raw = ctypes.CDLL(_abi.LIB_PATH)
    for s in ("qs_set_scoring_strategy_qos", "qs_get_scoring_strategy_qos"):
        assert hasattr(raw, s), s
        assert s in _abi.EXPORTED
    assert lib.qs_struct_size(6) == ctypes.sizeof(_abi.QsScoringStrategy)  # the struct is unchanged
    assert lib.qs_struct_size(0) == ctypes.sizeof(_abi.QsConfig)
    assert _abi.QS_ABI_VERSION == 3
    st = _abi.QsScoringStrategy()
    assert lib.qs_set_scoring_strategy_qos(None, 0, ctypes.byref(st)) == _abi.QS_EINVAL  # null context: a status
    assert lib.qs_get_scoring_strategy_qos(None, 0, ctypes.byref(st)) == _abi.QS_EINVAL


# ---- discrimination on the GPU tests' inputs ----------------------------------------------------
def differs_from_its_uniforms(case):
    nodes, pods, cfg, ref = case
    assert (ref[0] >= 0).sum() > len(ref[0]) // 2
    for u in C.uniform_cfgs(cfg):
        base = {k: v for k, v in cfg.items() if k != "qos_strategies"}
        pl = R.run(nodes, pods, dict(base, **u))[0]
        assert not np.array_equal(pl, ref[0]), u


@pytest.mark.parametrize("lst", list(C.LISTS))
@pytest.mark.parametrize("prof", list(C.PROFILES))
def test_mix_differs_engines(prof, lst):
    nodes, pods, cfg, ref = C.engines_case(prof, lst)
    assert C.windows_hold_every_class(pods["qos"])
    differs_from_its_uniforms((nodes, pods, cfg, ref))


def test_mix_differs_sorted():
    differs_from_its_uniforms(C.engines_case("fit-balanced", "gpu5", 1))


def test_mix_differs_two_tables():
    differs_from_its_uniforms(C.two_tables_case())


def test_mix_differs_ties():
    case = C.ties_case()
    assert len(C.uniform_cfgs(case[2])) == 2  # LeastAllocated (Guaranteed, Burstable) and MostAllocated
    differs_from_its_uniforms(case)


def test_mix_differs_wide():
    differs_from_its_uniforms(C.wide_case())
