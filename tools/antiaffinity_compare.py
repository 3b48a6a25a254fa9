#!/usr/bin/env python3
"""What required pod anti-affinity costs on the exact engines: config-5 pods with the
apps folded to 40 groups and the zones to 4, 100,000 pods on tables of 2,000 and 5,000 nodes.

Arms per table:
  batched1          QS_MODE_BATCHED with batch_pods = 1: the only route to the sequential semantics with
                    anti-affinity before qs_set_pod_anti_affinity (one select, merge and claim per pod);
                    the yardstick, and the one arm a tree without the call can run (--tree)
  aa_persistent     tracking on, QS_MODE_EXACT, QS_ENGINE_PERSISTENT (tables within its cap; else skipped)
  aa_scan           tracking on, QS_ENGINE_SCAN
  spread_persistent the aa_* arms with the ZONE apps' pods turned into SPREAD(1) (zone topology spread, spec S13,
  spread_scan       DESIGN.md §3.5), checked against tests/spread_ref.py; read beside aa_* of the same run
  soft_persistent   the spread_* arms with the SPREAD(1) pods turned soft (zone topology spread scoring, spec S14,
  soft_scan         DESIGN.md §3.6), checked against tests/soft_spread_ref.py; read beside spread_* of the same run
  hostspread_persistent  the aa_* arms with the HOSTNAME apps' pods turned into HOSTSPREAD(1) (hostname topology
  hostspread_scan   spread, spec S15), checked against tests/hostspread_ref.py; read beside aa_*
                    of the same run: the same pods under the one-per-node rule
  honor_spread_scan      the spread_scan / soft_scan / hostspread_scan streams with the NodeAffinity filter on
  honor_soft_scan        (enable_affinity = 1: the normalizing class), the nodes of zones 0 and 1 labelled and every
  honor_hostspread_scan  pod of the converted kind selecting that label (half of the four zones), under
                    nodeAffinityPolicy Honor (spec S16), checked against tests/honor_spread_ref.py;
  ignore_*_scan     the same three streams under the policy Ignore: honor_* against ignore_* is the cost of
                    the count pass (one more launch per restricting SPREAD / SPREAD_SOFT pod; none for hostname)
  taint_honor_spread_scan      the spread_scan / soft_scan / hostspread_scan streams with the TaintToleration filter
  taint_honor_soft_scan        on (enable_taint = 1: the normalizing class), the nodes of zones 2 and 3 tainted, the
  taint_honor_hostspread_scan  pods of the converted kind tolerating nothing and every other pod everything, under
                    nodeTaintsPolicy Honor (spec S17), checked against tests/taint_spread_ref.py;
  taint_ignore_*_scan  the same three streams under the policy Ignore
  plain_persistent  the same table and pods with tracking off (placements ignore anti-affinity):
  plain_scan        the cost of the filter and the recording is aa_* against plain_*

Each arm runs in a process of its own, is checked bit for bit on the first 2,000 pods scheduled as a
stream of their own (tracked arms and batched1 against tests/antiaffinity_ref.py, plain arms against
oracle.schedule), and prints the median wall of --steps runs of the prepared stream from the same saved
table (the first run warms up), as us per pod.  --tree DIR runs the arms against another checkout's
library and binding (the parent commit: batched1 and the plain arms).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ["batched1", "aa_persistent", "aa_scan", "spread_persistent", "spread_scan", "soft_persistent", "soft_scan",
        "hostspread_persistent", "hostspread_scan", "honor_spread_scan", "honor_soft_scan", "honor_hostspread_scan",
        "ignore_spread_scan", "ignore_soft_scan", "ignore_hostspread_scan", "taint_honor_spread_scan",
        "taint_honor_soft_scan", "taint_honor_hostspread_scan", "taint_ignore_spread_scan", "taint_ignore_soft_scan",
        "taint_ignore_hostspread_scan", "plain_persistent", "plain_scan"]


def paths(tree):
    # the library and binding of `tree`; the reference and its inputs always from this checkout
    for p in (os.path.join(ROOT, "tests"), tree, os.path.join(tree, "custom-k8s-scheduler_amd")):
        sys.path.insert(0, p)


def run_arm(n, p, arm, steps, prefix):
    import numpy as np

    import antiaffinity_ref as A
    from oracle import oracle as O
    from qsched import Scheduler, synth_generate

    nodes, pods = synth_generate(5, n, p)
    nodes, pods = A.fold(nodes, pods, 40, 4)
    policy = None  # honor_* / ignore_*: the arm behind the prefix with a selector on its spread pods
    taints = arm.startswith("taint_")  # taint_honor_* / taint_ignore_*: ... with a tainted half of the table
    if taints:
        arm = arm[len("taint_"):]
    if arm.startswith(("honor_", "ignore_")):
        policy, arm = arm.split("_", 1)
        out_arm = ("taint_" if taints else "") + policy + "_" + arm
    else:
        out_arm = arm
    soft = arm.startswith("soft_")
    spread = arm.startswith("spread_") or soft
    host = arm.startswith("hostspread_")
    tracked = arm.startswith("aa_") or spread or host
    if host:
        import hostspread_ref as H

        pods = pods.copy()
        pods["anti_affinity"][pods["anti_affinity"] == A.HOSTNAME] = H.spread_hostname(1)
    if spread:
        import spread_ref as S

        pods = pods.copy()
        kind = S.spread(1)
        if soft:
            import soft_spread_ref as R

            kind = R.spread_soft(1)
        pods["anti_affinity"][pods["anti_affinity"] == A.ZONE] = kind
    batched = arm == "batched1"
    engine = "auto" if batched else arm.split("_")[1]
    cfg = dict(engine=engine, batch_pods=1) if batched else dict(engine=engine)
    mode = "batched" if batched else "exact"
    out = dict(nodes=n, pods=p, arm=out_arm)
    if taints:
        import taint_spread_ref as TR

        nodes = {k: v.copy() for k, v in nodes.items()}
        nodes["taint_hard"][nodes["zone"] >= 2] = np.uint64(1 << 8)
        pods = pods.copy()
        pods["tol_hard"] = np.where((pods["anti_affinity"] & 0xFF) == 3, np.uint64(0), ~np.uint64(0))
        cfg["enable_taint"] = 1
    elif policy:
        import honor_spread_ref as HR

        nodes = {k: v.copy() for k, v in nodes.items()}
        nodes["label_bits"][nodes["zone"] < 2, 0] |= np.uint64(1 << 8)
        pods = pods.copy()
        pods["sel"][(pods["anti_affinity"] & 0xFF) == 3, 0] = np.uint64(1 << 8)
        cfg["enable_affinity"] = 1
    with Scheduler(cfg) as s:
        if tracked:
            s.set_pod_anti_affinity(True)
        if taints:
            if not hasattr(s, "set_topology_spread_node_taints_policy"):  # (--tree: a tree from before S17)
                out.update(skipped="no qs_set_topology_spread_node_taints_policy in this tree")
                return out
            s.set_topology_spread_node_taints_policy(policy)
        elif policy:
            if not hasattr(s, "set_topology_spread_node_affinity_policy"):  # (--tree: a tree from before S16)
                out.update(skipped="no qs_set_topology_spread_node_affinity_policy in this tree")
                return out
            s.set_topology_spread_node_affinity_policy(policy)
        s.load_nodes(nodes)
        s.save_table()
        try:
            head = s.prepare(pods[:prefix])
        except Exception as e:  # e.g. a tree from before QS_AA_SPREAD (--tree): the spread arms are skipped
            out.update(skipped=str(e))
            return out
        try:
            head.run(mode=mode)
        except Exception as e:  # e.g. PERSISTENT beyond its cap for this class
            head.free()
            out.update(skipped=str(e))
            return out
        pl, keys = head.results()
        head.free()
        if taints:
            ref = TR.run(nodes, pods[:prefix], dict(enable_taint=1),
                         taints_policy=TR.HONOR if policy == "honor" else TR.IGNORE)
        elif policy:
            ref = HR.run(nodes, pods[:prefix], dict(enable_affinity=1),
                         policy=HR.HONOR if policy == "honor" else HR.IGNORE)
        elif host:
            ref = H.run(nodes, pods[:prefix])
        elif soft:
            ref = R.run(nodes, pods[:prefix])
        elif spread:
            ref = S.run(nodes, pods[:prefix])
        elif tracked or batched:
            ref = A.run(nodes, pods[:prefix])
        else:
            on = {k: v.copy() for k, v in nodes.items()}
            ref = O.schedule(on, A.pods_dict(pods[:prefix]))
        out["prefix_ok"] = bool(np.array_equal(pl, ref[0]) and np.array_equal(keys, ref[1]))
        s.restore_table()
        st = s.prepare(pods)
        walls, stats = [], None
        for i in range(steps + 1):
            stats = st.run(mode=mode)
            if i:
                walls.append(stats["wall_s"])
            s.restore_table()
        st.free()
    wall = statistics.median(walls)
    out.update(ms_per_step=round(wall * 1e3, 3), ms_all=[round(w * 1e3, 3) for w in walls],
               us_per_pod=round(wall * 1e6 / p, 3), engine_used=stats["engine_used"], launches=int(stats["batches"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", default="2000,5000")
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--prefix", type=int, default=2000)
    ap.add_argument("--tree", default=ROOT, help="checkout whose library and binding run the arms")
    ap.add_argument("--one", nargs=2, metavar=("NODES", "ARM"), help="run one arm in this process")
    a = ap.parse_args()
    if a.one:
        paths(os.path.abspath(a.tree))
        print(json.dumps(run_arm(int(a.one[0]), a.pods, a.one[1], a.steps, a.prefix)), flush=True)
        return 0
    rows, bad = [], 0
    for n in (int(x) for x in a.nodes.split(",")):
        for arm in a.arms.split(","):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), arm, "--pods", str(a.pods),
                                "--steps", str(a.steps), "--prefix", str(a.prefix), "--tree", a.tree],
                               capture_output=True, text=True, timeout=420)
            if r.returncode != 0:
                # a failed arm may have left the device in a bad state: nothing more is started
                sys.stderr.write(r.stdout + r.stderr)
                print(f"arm {n}/{arm} exited with {r.returncode}; stopping", flush=True)
                return 1
            row = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            rows.append(row)
            bad += not row.get("prefix_ok", True)
    for n in sorted({r["nodes"] for r in rows}):
        base = next((r for r in rows if r["nodes"] == n and r["arm"] == "batched1" and "us_per_pod" in r), None)
        for r in rows:
            if r["nodes"] != n:
                continue
            if "skipped" in r:
                print(f"n {n:5d} {r['arm']:28s} skipped: {r['skipped'][:90]}")
                continue
            rel = f"x{r['us_per_pod'] / base['us_per_pod']:.3f} of batched1" if base else ""
            print(f"n {n:5d} {r['arm']:28s} {r['ms_per_step']:10.3f} ms  {r['us_per_pod']:8.3f} us/pod  {rel}  "
                  f"engine {r['engine_used']}  prefix {'ok' if r['prefix_ok'] else 'DIFFERS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
