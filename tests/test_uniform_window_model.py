"""CPU model of the resident resolver's barrier-free path for windows of identical pods
(la_resolve4_stream's uniform-window branch is a transcription of it).

A window whose K pod records are identical is resolved from pod 0's list alone.  Every lane keeps a
ladder of R rungs, rung k = key(row + k * pod, pod): slot lanes (the nodes dirtied by the previous
window) from their slot rows, candidate lanes (pod 0's list entries that were clean at the window
start) from the candidate's row plus the pods the lane took so far.  Wave D takes the maximum of
the top rungs pod after pod, shifts the owner's ladder, and ends the round when the owner's ladder
is used up; the key waves then rebuild every ladder from the counts.  At the window end the
candidate lanes that took a pod become slots.

Scores come from the C oracle (or_score_pod), so this checks the PROTOCOL (one list for the window,
rungs, exhaustion, new and inherited slots) against the exact sequential oracle; the GPU tests
check the kernel.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_lookahead_model import chunks_of, merged_select, resolve_window_inherit

POD_RECORD_FIELDS = ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "req_ext", "qos")


def key_node(e):
    return 0xFFFFFFFF - (int(e) & 0xFFFFFFFF)


def reserve(nodes, pods, j, w, times=1):
    sn, sp = O._mk_nodes(nodes), O._mk_pods(pods)
    for _ in range(times):
        O.lib().or_reserve(O.ctypes.byref(sn), O.ctypes.byref(sp), j, w, 1)


def window_is_uniform(pods, order, s0, kend):
    """The host's rule: the window's device pod records are identical."""
    j0 = int(order[s0])
    return all(np.array_equal(pods[f][int(order[s0 + i])], pods[f][j0])
               for f in POD_RECORD_FIELDS for i in range(1, kend))


def ladders(nodes, pods, j, lanes, R):
    """rung k of every lane's node: its key for pod j with k more pods of that type on it."""
    scratch, _ = O.copy_cluster(nodes, pods)
    out = {w: [] for w in lanes}
    for _ in range(R):
        keys, _ = O.score_pod(scratch, pods, j)
        for w in lanes:
            out[w].append(int(keys[w]))
            reserve(scratch, pods, j, w)
    return out


def resolve_uniform_window(nodes, pods, order, s0, kend, list0, placement, inherited, R, stop=True):
    """The round / ladder protocol.  ``inherited``: the slot nodes at the window start (lane order).
    Returns (won nodes, rounds).  stop=False drops the exhaustion stop (the negative test)."""
    j = int(order[s0])  # every pod of the window has this record
    slots = list(inherited)
    cands = [key_node(e) for e in list0 if key_node(e) not in set(slots)]  # clean at the window start
    cnt_s = {w: 0 for w in slots}
    cnt_c = {w: 0 for w in cands}
    i, rounds = 0, 0
    while i < kend:
        rounds += 1
        assert rounds <= kend  # a round resolves at least one pod
        # keys phase: the table holds every lane's row + count * pod (deltas applied below)
        lad = ladders(nodes, pods, j, slots + cands, R)
        left = {w: R for w in slots + cands}
        d = {w: 0 for w in slots + cands}
        # D phase: no barrier between pods
        while i < kend:
            m = max([lad[w][0] for w in slots + cands], default=0)
            if m == 0:  # the state does not change: every later pod of the window fails too
                for k in range(i, kend):
                    placement[int(order[s0 + k])] = -1
                i = kend
                break
            w = key_node(m)  # (a slot lane is found first; a node is never in both sets)
            placement[int(order[s0 + i])] = w
            i += 1
            lad[w] = lad[w][1:] + [0]
            left[w] -= 1
            d[w] += 1
            if stop and left[w] == 0:
                break
        for w, k in d.items():  # the key waves apply the round's deltas
            reserve(nodes, pods, j, w, k)
            if w in cnt_s:
                cnt_s[w] += k
            else:
                cnt_c[w] += k
    won = [w for w in slots if cnt_s[w]] + [w for w in cands if cnt_c[w]]  # new slots in lane order
    return won, rounds


def model_schedule_uniform(nodes, pods, K, R, cfg=None, stop=True, stats=None):
    """The overlapped engine of test_lookahead_model (window w+1's lists are selected before window w
    resolves, L = 2K), with the uniform path for windows of identical pods."""
    cfg = cfg or O.DEFAULT_CONFIG
    order = O.py_order(pods, cfg)
    n = len(nodes["alloc_cpu"])
    placement = np.full(len(order), -2, np.int32)
    starts = list(range(0, len(order), K))
    pending = merged_select(nodes, pods, order, starts[0], K, 2 * K, chunks_of(n, 1))
    inherited = []
    for w, s0 in enumerate(starts):
        lists, kend = pending, min(K, len(order) - s0)
        if w + 1 < len(starts):
            pending = merged_select(nodes, pods, order, starts[w + 1], K, 2 * K, chunks_of(n, 1))
        if window_is_uniform(pods, order, s0, kend):
            inherited, rounds = resolve_uniform_window(nodes, pods, order, s0, kend, lists[0], placement,
                                                       inherited, R, stop)
            if stats is not None:
                stats.append(rounds)
        else:
            inherited = sorted(resolve_window_inherit(nodes, pods, order, s0, lists, placement, set(inherited)))
    return placement


def identical_pods_cluster(n, p, alloc_cpu, alloc_mem, max_pods, req=(0, 0)):
    """n nodes, p identical pods: BestEffort (req 0, non-zero defaults) or Guaranteed with req."""
    nodes, pods = O.empty_cluster(n, p)
    nodes["alloc_cpu"][:] = alloc_cpu
    nodes["alloc_mem"][:] = alloc_mem
    nodes["max_pods"][:] = max_pods
    pods["req_cpu"][:] = req[0]
    pods["req_mem"][:] = req[1]
    pods["nz_cpu"][:] = req[0] or O.DEF_CPU
    pods["nz_mem"][:] = req[1] or O.DEF_MEM
    pods["qos"][:] = 2 if req[0] and req[1] else 0
    return nodes, pods


def check_exact(nodes, pods, K, R, stats=None):
    ref_nodes, _ = O.copy_cluster(nodes, pods)
    ref, _, _ = O.schedule(ref_nodes, pods)
    got = model_schedule_uniform(nodes, pods, K, R, stats=stats)
    assert np.array_equal(got, ref)
    for k in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "pods"):
        assert np.array_equal(nodes[k], ref_nodes[k])


@pytest.mark.parametrize("K,R", [(8, 4), (16, 4), (32, 4), (32, 8), (32, 1)])
def test_mixed_stream_is_exact(K, R):
    """spec/synth.md config 2, QoS-sorted: mixed windows, then the BestEffort tail's uniform ones
    (with slots inherited from a mixed window and from a uniform one)."""
    nodes, pods = O.generate(2, 150, 1000)
    stats = []
    check_exact(nodes, pods, K, R, stats)
    assert len(stats) >= 2  # the tail really took the uniform path


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_streams_are_exact(seed):
    nodes, pods = O.generate(2, 90, 700, seed=0xABC000 + seed)
    stats = []
    check_exact(nodes, pods, 32, 4, stats)
    assert stats


def test_one_large_node_takes_several_rounds():
    """One node far larger than the rest wins more than R pods of a window: its ladder is used up
    and the window takes several rounds."""
    rng = np.random.default_rng(7)
    nodes, pods = identical_pods_cluster(70, 200, 4000, 16 * O.GIB, 110)
    nodes["alloc_cpu"][:] = rng.integers(2000, 6000, 70)
    nodes["alloc_cpu"][13] = 4_000_000
    nodes["alloc_mem"][13] = 4096 * O.GIB
    nodes["max_pods"][13] = 1000
    stats = []
    check_exact(nodes, pods, 32, 4, stats)
    assert max(stats) > 1


def test_rungs_turn_infeasible_and_the_tail_is_unschedulable():
    """max_pods 1-3: rungs turn infeasible in the middle of a ladder; the stream's tail finds no node."""
    rng = np.random.default_rng(11)
    nodes, pods = identical_pods_cluster(80, 200, 8000, 32 * O.GIB, 1)
    nodes["max_pods"][:] = rng.integers(1, 4, 80)
    nodes["alloc_cpu"][:] = rng.integers(1000, 9000, 80)
    check_exact(nodes, pods, 32, 4)


def test_guaranteed_pods_end_by_cpu_and_by_memory():
    rng = np.random.default_rng(13)
    nodes, pods = identical_pods_cluster(64, 300, 4000, 8 * O.GIB, 110, req=(500, 1 * O.GIB))
    nodes["alloc_cpu"][:] = rng.integers(1000, 8000, 64)   # some nodes end by cpu ...
    nodes["alloc_mem"][:] = rng.integers(2, 17, 64) * O.GIB  # ... others by memory
    check_exact(nodes, pods, 32, 8)


def test_without_the_exhaustion_stop_placements_are_wrong():
    """R rungs and no stop when a ladder is used up: the large node's key is missing from the pods
    after its R-th win, so they go elsewhere."""
    nodes, pods = identical_pods_cluster(70, 200, 3000, 16 * O.GIB, 110)
    nodes["alloc_cpu"][13] = 4_000_000
    nodes["alloc_mem"][13] = 4096 * O.GIB
    nodes["max_pods"][13] = 1000
    ref_nodes, _ = O.copy_cluster(nodes, pods)
    ref, _, _ = O.schedule(ref_nodes, pods)
    got = model_schedule_uniform(nodes, pods, 32, 4, stop=False)
    assert not np.array_equal(got, ref)
