"""Every path qs_stream_run can take for one small stream, pinned by what the run reports.

One shape throughout: 100 nodes x 200 pods (synthetic config 1, and config 4 with the normalizing
plugins).  With the default window K = 32 that is 7 windows, the last one partial (8 pods): the window
loop, both list parities and the short last window all run.  Each arm asserts oracle-exact placements,
keys and final table (as tests/test_gpu_parity.py does) and the qs_stats fields that identify the path:
engine_used, batches, resident, resident_path and, under config.profile_kernels, the launches counted
per bracket (stats["kernels"]: persistent, scan, select, resolve).

The ALLREDUCE, mailbox and timeout-recovery paths are pinned by tests/test_gpu_shard.py,
tests/test_gpu_mailbox.py and tests/test_gpu_recovery.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import Scheduler, pods_from_struct, synth_generate  # noqa: E402

import hostspread_cases as HC  # noqa: E402
import hostspread_ref as H  # noqa: E402
from test_gpu_hostspread import run_tracked  # noqa: E402
from test_gpu_parity import CFG4, assert_same, run_oracle  # noqa: E402

N, P, K = 100, 200, 32
NWIN = (P + K - 1) // K
assert NWIN == 7 and P % K == 8

PROFILES = {"fit": (1, {}), "norm": (4, CFG4)}
# qs_stats::resident_path of the default resident launch: Fit + Balanced carries 32-bit keys (bit 0) and
# skips the zero-allocatable terms (bit 1); the normalizing resolver reports neither
RESIDENT_PATH = {"fit": 3, "norm": 0}


@pytest.fixture(scope="module")
def cases(oracle):
    """Per profile: nodes, pods, configuration and the oracle's (placements, keys, final table)."""
    out = {}
    for name, (config, cfg) in PROFILES.items():
        nodes, pods = synth_generate(config, N, P)
        out[name] = (nodes, pods, cfg, run_oracle(oracle, nodes, pods, cfg))
    return out


def run_once(case, **cfg):
    nodes, pods, base, ref = case
    with Scheduler(dict(base, **cfg)) as s:
        s.load_nodes(nodes)
        st = s.prepare(pods)
        stats = st.run()
        got = st.results()
        st.free()
        final = s.read_nodes()
    assert_same(got, ref[:2], final, ref[2])
    return stats


def launches(stats):
    return {k: v["launches"] for k, v in stats["kernels"].items()}


@pytest.mark.parametrize("profile", [0, 1])
def test_persistent(cases, profile):
    st = run_once(cases["fit"], engine="persistent", profile_kernels=profile)
    assert st["engine_used"] == "persistent" and st["batches"] == 1 and st["resident"] == 0
    assert launches(st) == ({"persistent": 1} if profile else {})


@pytest.mark.parametrize("profile", [0, 1])
def test_scan(cases, profile):
    st = run_once(cases["fit"], engine="scan", profile_kernels=profile)
    assert st["engine_used"] == "scan" and st["batches"] == P and st["resident"] == 0
    assert launches(st) == ({"scan": P} if profile else {})


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("name", list(PROFILES))
def test_lookahead_per_window(cases, monkeypatch, name, profile):
    monkeypatch.setenv("QS_RESIDENT", "0")
    st = run_once(cases[name], engine="lookahead", profile_kernels=profile)
    assert st["engine_used"] == "lookahead" and st["resident"] == 0 and st["resident_path"] == 0
    assert st["batches"] == NWIN
    assert launches(st) == ({"select": NWIN, "resolve": NWIN} if profile else {})


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("name", list(PROFILES))
def test_lookahead_resident(cases, name, profile):
    st = run_once(cases[name], engine="lookahead", profile_kernels=profile)
    assert st["engine_used"] == "lookahead" and st["resident"] == 1
    assert st["resident_path"] == RESIDENT_PATH[name]
    assert st["batches"] == NWIN
    assert launches(st) == ({"resolve": 1} if profile else {})


@pytest.mark.parametrize("name", list(PROFILES))
def test_lookahead_serial_graph_replay(cases, name):
    """Non-overlapped windows run as a captured graph: the first run of the prepared stream captures, the
    second (from the restored table) replays."""
    nodes, pods, cfg, ref = cases[name]
    with Scheduler(dict(cfg, engine="lookahead", lookahead_serial=1)) as s:
        s.load_nodes(nodes)
        s.save_table()
        st = s.prepare(pods)
        for _ in range(2):
            stats = st.run()
            assert stats["engine_used"] == "lookahead" and stats["resident"] == 0
            assert stats["batches"] == NWIN and launches(stats) == {}
            assert_same(st.results(), ref[:2], s.read_nodes(), ref[2])
            s.restore_table()
        st.free()


def test_batched_graph_replay(oracle, cases):
    nodes, pods, _, _ = cases["fit"]
    on = {k: v.copy() for k, v in nodes.items()}
    o_pl, o_keys, o_nb = oracle.schedule_batched(on, pods_from_struct(pods), batch=64, nthreads=16)
    with Scheduler({}) as s:
        s.load_nodes(nodes)
        s.save_table()
        st = s.prepare(pods)
        for _ in range(2):
            stats = st.run(mode="batched")
            assert stats["engine_used"] == "batched" and stats["resident"] == 0
            assert stats["batches"] >= (P + 63) // 64 and stats["batches"] == o_nb
            pl, keys = st.results()
            assert np.array_equal(pl, o_pl) and np.array_equal(keys, o_keys)
            final = s.read_nodes()
            for k in ("req_cpu", "req_mem", "req_ext", "nz_cpu", "nz_mem", "pods"):
                assert np.array_equal(final[k], on[k]), k
            s.restore_table()
        st.free()


@pytest.mark.parametrize("engine", ["auto", "persistent", "scan", "lookahead"])
def test_empty_node_table(cases, engine):
    """No node loaded, P > 0: no pod is placed and no kernel runs."""
    _, pods, _, _ = cases["fit"]
    with Scheduler(dict(engine=engine, profile_kernels=1)) as s:
        st = s.prepare(pods)
        stats = st.run()
        pl, keys = st.results()
        st.free()
    assert (pl == -1).all() and (keys == 0).all()
    assert stats["batches"] == 0 and stats["pods"] == P and launches(stats) == {}


@pytest.mark.parametrize("apps,runs", [(16, "persistent"), (17, "scan")])
def test_hostname_spread_auto_engine(apps, runs):
    """QS_AA_SPREAD_HOSTNAME pods on a context that tracks anti-affinity, engine AUTO: up to 16 apps fit
    the persistent workgroup's slots, 17 run SCAN."""
    nodes, pods = HC.many_apps(N, P, apps)
    ref = H.run(nodes, pods, HC.ARRIVAL)
    g = run_tracked(nodes, pods, HC.ARRIVAL, "auto")
    assert_same(g[:2], ref[:2], g[2], ref[2])
    assert g[3]["engine_used"] == runs
    assert g[3]["batches"] == (1 if runs == "persistent" else P)
