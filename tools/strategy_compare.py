#!/usr/bin/env python3
"""What the MostAllocated / RequestedToCapacityRatio scorers cost: config 2's
5,000 x 100,000 stream and config 4's 5,000 x 150,000 under the three strategies, LOOKAHEAD engine.

Arms per configuration:
  least_default   LeastAllocated on the default kernels (config 4: the lists reduce only where no pod
                  requests a GPU, so this arm uses the default lists)
  least_res       LeastAllocated through the resource-list kernels (kFeatRes): config 4 with the GPU
                  list {cpu:1, memory:1, amd.com/gpu:5} / Balanced [cpu, memory, amd.com/gpu], which does
                  not reduce; config 2, whose pods request no extended resource, with QS_FORCE_RES=1
  most, rtcr_binpack, rtcr_three   the same lists as least_res under the new strategies
  mix             one strategy per QoS class: BestEffort MostAllocated, Burstable
                  RequestedToCapacityRatio (the three-segment shape), Guaranteed LeastAllocated, on the
                  same lists; checked against tests/qos_strategy_ref.py
least_res is the yardstick of the new scorers: the same kernel family with the same Balanced path.
--arms picks a subset (a comparison against another tree runs the arms both trees know).

Each arm runs in a process of its own (QS_FORCE_RES is read once), is checked bit for bit against
tests/strategy_ref.py on the first 2,000 pods scheduled as a stream of their own, and prints pods/s
(median of --steps runs of the prepared stream from the same saved table) with the resolver's counters.
Prints one JSON object per arm and a closing table of ratios against least_res.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-k8s-scheduler_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GPU_LIST = dict(fit_resources=[("cpu", 1), ("memory", 1), ("ext0", 5)], balanced_resources=["cpu", "memory", "ext0"])
THREE = [(0, 2), (40, 10), (70, 3), (100, 8)]
STRATS = {
    "least_default": {},
    "least_res": {},
    "most": dict(scoring_strategy="MostAllocated"),
    "rtcr_binpack": dict(scoring_strategy="RequestedToCapacityRatio", shape=[(0, 0), (100, 10)]),
    "rtcr_three": dict(scoring_strategy="RequestedToCapacityRatio", shape=THREE),
    "mix": dict(qos_strategies={"BestEffort": dict(scoring_strategy="MostAllocated"),
                                "Burstable": dict(scoring_strategy="RequestedToCapacityRatio", shape=THREE),
                                "Guaranteed": dict(scoring_strategy="LeastAllocated")}),
}
SIZES = {2: (5000, 100000), 4: (5000, 150000)}


def arm_cfg(config, arm):
    cfg = dict(enable_taint=1, enable_affinity=1) if config == 4 else {}
    if config == 4 and arm != "least_default":
        cfg.update(GPU_LIST)
    cfg.update(STRATS[arm])
    return cfg


def run_arm(config, arm, steps, prefix):
    import numpy as np

    import qos_strategy_ref as R  # (strategy_ref's loop; the same placements where no class is listed)
    from qsched import Scheduler, synth_generate

    n, p = SIZES[config]
    nodes, pods = synth_generate(config, n, p)
    cfg = arm_cfg(config, arm)
    out = dict(config=config, arm=arm, nodes=n, pods=p, force_res=os.environ.get("QS_FORCE_RES", "0"))
    with Scheduler(dict(cfg, engine="lookahead")) as s:
        s.load_nodes(nodes)
        s.save_table()
        head = s.prepare(pods[:prefix])
        head.run()
        pl, keys = head.results()
        head.free()
        ref = R.run(nodes, pods[:prefix], cfg)
        out["prefix_ok"] = bool(np.array_equal(pl, ref[0]) and np.array_equal(keys, ref[1]))
        s.restore_table()
        st = s.prepare(pods)
        walls, stats = [], None
        for i in range(steps + 1):  # the first run warms up
            stats = st.run()
            if i:
                walls.append(stats["wall_s"])
            s.restore_table()
        st.free()
    wall = statistics.median(walls)
    out.update(ms_per_step=round(wall * 1e3, 3), ms_all=[round(w * 1e3, 3) for w in walls],
               pods_per_s=round(p / wall, 1), resident=int(stats["resident"]),
               resident_path=int(stats["resident_path"]), windows=int(stats["batches"]),
               truncations=int(stats["truncations"]), resumed_windows=int(stats["resumed_windows"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--arms", default=",".join(STRATS))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--prefix", type=int, default=2000)
    ap.add_argument("--one", nargs=2, metavar=("CONFIG", "ARM"), help="run one arm in this process")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run_arm(int(a.one[0]), a.one[1], a.steps, a.prefix)), flush=True)
        return 0
    rows, bad = [], 0
    for config in (int(c) for c in a.configs.split(",")):
        for arm in a.arms.split(","):
            env = dict(os.environ)
            env.pop("QS_FORCE_RES", None)
            if config == 2 and arm != "least_default":
                env["QS_FORCE_RES"] = "1"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(config), arm, "--steps",
                                str(a.steps), "--prefix", str(a.prefix)], env=env, capture_output=True, text=True,
                               timeout=300)
            if r.returncode != 0:
                # a failed arm may have left the device in a bad state: nothing more is started
                sys.stderr.write(r.stdout + r.stderr)
                print(f"arm {config}/{arm} exited with {r.returncode}; stopping", flush=True)
                return 1
            row = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            rows.append(row)
            bad += not row["prefix_ok"]
    for config in sorted({r["config"] for r in rows}):
        base = next((r for r in rows if r["config"] == config and r["arm"] == "least_res"), None)
        for r in rows:
            if r["config"] == config and base:
                print(f"config {config} {r['arm']:14s} {r['ms_per_step']:9.3f} ms  {r['pods_per_s'] / 1e6:6.3f} M pods/s  "
                      f"x{r['ms_per_step'] / base['ms_per_step']:.3f} of least_res  resident {r['resident']} "
                      f"truncations {r['truncations']} resumed {r['resumed_windows']}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
