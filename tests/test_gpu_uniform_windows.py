"""The resident ring resolver's barrier-free path for windows of identical pods.

Every case runs the resident lookahead stream twice — as shipped and with QS_RES_UNIFORM=0 (the
general one-barrier-per-pod path) — and each run must be resident and equal the CPU oracle bit for
bit: placements, per-pod 64-bit keys, final node table.  The run as shipped must report uniform
windows (stats["uniform_windows"], qs_stream_uniform_windows), so that no case can pass on the
general path alone; the other run must report none.  That figure is a host-side count of the windows
flagged in the bitmap the launch was given: la_stream_res_takes_uniform gates both the bitmap and the
choice of the uniform-window kernel, so a count above zero means that kernel ran with a bitmap — it is
not a device-side record that the branch was taken.  The shapes are small (64-200 nodes, 100-300
pods) and are the places the path can go wrong: a lane that wins more pods of a window than a
ladder has rungs (several rounds), rungs that turn infeasible in the middle of a ladder, a stream
whose tail finds no node, mixed and uniform windows following each other with inherited slots both
ways, a short last window, a record change in the middle of a window, and every ring class
(extended resources, wide rows, configurable scoring resources).  The protocol itself is checked on
the CPU by tests/test_uniform_window_model.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import Scheduler, pods_from_struct, pods_to_struct, synth_generate  # noqa: E402

from oracle import oracle as O  # noqa: E402
from rescfg import GPU_CFG  # noqa: E402
from test_gpu_parity import assert_same, run_gpu  # noqa: E402

GIB, MIB, KI = 1 << 30, 1 << 20, 1 << 10
VARIANTS = [{}, {"QS_RES_UNIFORM": "0"}]


def check(monkeypatch, nodes, pods, cfg=None, K=0, env=None, windows=None):
    """pods: the canonical dict.  windows: how many uniform windows the run as shipped must report
    (default: at least one).  Returns the oracle's placements."""
    cfg = cfg or {}
    sp = pods_to_struct(pods)
    on = {k: v.copy() for k, v in nodes.items()}
    pl, keys, _ = O.schedule(on, pods_from_struct(sp), dict(O.DEFAULT_CONFIG, **cfg), nthreads=16)
    for var in VARIANTS:
        with monkeypatch.context() as m:
            for k, v in dict(env or {}, **var).items():
                m.setenv(k, v)
            g = run_gpu(nodes, sp, cfg, "lookahead", lookahead=K)
        assert g[3]["resident"] == 1, var
        assert g[3]["resident_path"] & 1, var  # the ring form with 32-bit keys
        if var:
            assert g[3]["uniform_windows"] == 0, var
        elif windows is None:
            assert g[3]["uniform_windows"] > 0, var
        else:
            assert g[3]["uniform_windows"] == windows, var
        assert_same(g[:2], (pl, keys), g[2], on)
    return pl


def identical(pods, lo, hi, req=(0, 0), ext0=0):
    """Pods lo..hi-1 identical: BestEffort (no requests, the non-zero defaults) or Guaranteed."""
    pods["req_cpu"][lo:hi] = req[0]
    pods["req_mem"][lo:hi] = req[1]
    pods["nz_cpu"][lo:hi] = req[0] or O.DEF_CPU
    pods["nz_mem"][lo:hi] = req[1] or O.DEF_MEM
    pods["req_ext"][lo:hi] = 0
    pods["req_ext"][lo:hi, 0] = ext0
    pods["qos"][lo:hi] = 2 if req[0] and req[1] else 0
    pods["priority"][lo:hi] = 0


def g2_nodes(n, seed=None):
    return synth_generate(2, n, 8, seed)[0]


def blank_pods(p):
    return O.empty_cluster(1, p)[1]


def test_identical_besteffort(monkeypatch):
    pods = blank_pods(200)
    identical(pods, 0, 200)
    check(monkeypatch, g2_nodes(120), pods)


def test_one_large_node_takes_several_rounds(monkeypatch):
    """One node far larger than the rest: its lane takes more pods of a window than a ladder has rungs."""
    nodes, _ = O.empty_cluster(70, 1)
    nodes["alloc_cpu"][:] = 2000
    nodes["alloc_mem"][:] = 4 * GIB
    nodes["max_pods"][:] = 110
    nodes["alloc_cpu"][13] = 64000
    nodes["alloc_mem"][13] = 512 * GIB
    nodes["max_pods"][13] = 500
    pods = blank_pods(200)
    identical(pods, 0, 200)
    pl = check(monkeypatch, nodes, pods)
    # the oracle's placements: with kResUniR = 6 rungs a ladder, more than 16 pods of the first
    # window on one lane take at least three rounds
    assert np.count_nonzero(pl[:32] == 13) > 16


def test_max_pods_and_unschedulable_tail(monkeypatch):
    """max_pods 1-3: rungs turn infeasible in the middle of a ladder; the tail finds no node."""
    rng = np.random.default_rng(11)
    nodes = g2_nodes(80)
    nodes["max_pods"][:] = rng.integers(1, 4, 80)
    nodes["pods"][:] = 0
    pods = blank_pods(250)
    identical(pods, 0, 250)
    pl = check(monkeypatch, nodes, pods)
    assert (pl == -1).sum() == 250 - int(nodes["max_pods"].sum())


def test_guaranteed_by_cpu_and_by_memory(monkeypatch):
    """Identical Guaranteed pods with requests: some nodes fill up by cpu, others by memory."""
    rng = np.random.default_rng(13)
    nodes, _ = O.empty_cluster(64, 1)
    nodes["alloc_cpu"][:] = rng.integers(1000, 8000, 64)
    nodes["alloc_mem"][:] = rng.integers(2, 17, 64) * GIB
    nodes["max_pods"][:] = 110
    pods = blank_pods(300)
    identical(pods, 0, 300, req=(1500, 3 * GIB))
    pl = check(monkeypatch, nodes, pods)
    assert (pl == -1).any() and (pl >= 0).any()


def test_mixed_uniform_mixed(monkeypatch):
    """qos_sort = 0: two mixed windows, two uniform ones, a window whose record changes in its
    middle (general path), mixed windows, and a short last window (300 = 9 * 32 + 12)."""
    nodes, sp = synth_generate(2, 150, 300)
    pods = pods_from_struct(sp)
    identical(pods, 64, 144)
    # windows of 32: pods 64-95 and 96-127 are uniform; 128-159 changes its record at pod 144
    pl = check(monkeypatch, nodes, pods, dict(qos_sort=0), windows=2)
    assert (pl >= 0).all()


def test_two_uniform_types_and_short_uniform_window(monkeypatch):
    """Two windows of BestEffort pods, then Guaranteed ones to the end: 150 = 4 * 32 + 22, so the
    last uniform window is short."""
    pods = blank_pods(150)
    identical(pods, 0, 64)
    identical(pods, 64, 150, req=(250, 512 * MIB))
    check(monkeypatch, g2_nodes(100), pods, dict(qos_sort=0), windows=5)


def test_ext_class(monkeypatch):
    """Identical pods that request an extended resource (the ext class; config-4 nodes)."""
    nodes = synth_generate(4, 200, 8)[0]
    assert (nodes["alloc_ext"][:, 0] > 0).any()
    pods = blank_pods(300)
    identical(pods, 0, 300, req=(200, 256 * MIB), ext0=1)
    pl = check(monkeypatch, nodes, pods)
    assert (pl >= 0).any()


def test_wide_layout(monkeypatch):
    """Odd-Ki allocatable memory: the table takes the wide layout (f64 memory columns)."""
    nodes = g2_nodes(90)
    nodes["alloc_mem"][:] = ((nodes["alloc_mem"] // KI) | 1) * KI
    pods = blank_pods(200)
    identical(pods, 0, 200)
    sp = pods_to_struct(pods)
    assert run_gpu(nodes, sp, {}, "lookahead")[3]["table_layout"] == "wide"
    check(monkeypatch, nodes, pods)


def test_configurable_resources(monkeypatch):
    """LeastAllocated {cpu:1, memory:1, ext0:5}, Balanced over [cpu, memory, ext0]."""
    nodes = synth_generate(4, 160, 8)[0]
    pods = blank_pods(250)
    identical(pods, 0, 250, req=(300, 512 * MIB), ext0=1)
    check(monkeypatch, nodes, pods, dict(GPU_CFG))


def test_generic_scorers(monkeypatch):
    """QS_FAST_ALLOC=0: the key waves with the zero-allocatable terms."""
    pods = blank_pods(200)
    identical(pods, 0, 200)
    check(monkeypatch, g2_nodes(120), pods, env={"QS_FAST_ALLOC": "0"})


@pytest.mark.parametrize("env", VARIANTS, ids=["uniform", "general"])
def test_record_timestamps(monkeypatch, env):
    """Per-pod decision stamps from either path: one per pod, in stream order."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nodes = g2_nodes(120)
    pods = blank_pods(200)
    identical(pods, 0, 200)
    sp = pods_to_struct(pods)
    on = {k: v.copy() for k, v in nodes.items()}
    pl, keys, _ = O.schedule(on, pods_from_struct(sp), nthreads=16)
    with Scheduler(dict(engine="lookahead", record_timestamps=1)) as s:
        s.load_nodes(nodes)
        st = s.prepare(sp)
        stats = st.run()
        g = st.results()
        stamps = st.stamps()
        st.free()
        final = s.read_nodes()
    assert stats["resident"] == 1 and (stats["uniform_windows"] > 0) == (not env)
    assert_same(g, (pl, keys), final, on)
    assert (stamps > 0).all() and (np.diff(stamps.astype(np.int64)) >= 0).all()
