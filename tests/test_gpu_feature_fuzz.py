"""Device parity of the feature fuzz (tests/feature_fuzz.py): the adversarial clusters of
tests/golden/fuzz_cases.json under the scoring strategies, one strategy per QoS class, configurable
resource lists, required anti-affinity (spec S12) and zone topology spread (S13), bit for bit against
tests/strategy_ref.py, tests/qos_strategy_ref.py and tests/spread_ref.py: placements, per-pod keys,
the final table, the layout the table took, and for the tracked arms the engine that ran and the
recorded state as probe pods see it.  The conditions that make these inputs worth running are asserted
from the references alone in tests/test_feature_fuzz_cpu.py.

One test covers the 14 to 24 small streams of one (arm, engine, memory grid); every selected case runs
on every engine of its arm.  The references are computed once per process.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import POD_DTYPE, Scheduler, pods_to_struct  # noqa: E402

import antiaffinity_ref as AA  # noqa: E402
import feature_fuzz as F  # noqa: E402
from test_gpu_adversarial import ENGINES, LAYOUTS, check_same, engine_cfg, gpu_stream  # noqa: E402
from test_gpu_spread import check_state  # noqa: E402

TRACKED_ENGINES = {"persistent": ("persistent", {}), "scan": ("scan", {}),
                   "scan_soa": ("scan", dict(scan_soa_min_nodes=1))}
FINAL = ("req_cpu", "req_mem", "req_ext", "nz_cpu", "nz_mem", "pods")


def check_layout(tag, x, stats):
    assert stats["table_layout"] == ("compact" if x["compact"] else "wide"), tag


def check_scores(tag, s, pod, want):
    """qs_score_pod and qs_score_pod_packed of one pod against (feasible, scores, total, best)."""
    feas, sc, total, best = want
    got = s.score_pod(pod)
    assert np.array_equal(got["feasible"], feas), tag
    np.testing.assert_array_equal(got["scores"], sc, err_msg=tag)
    assert np.array_equal(got["total"], total), tag
    assert got["best"] == best, tag
    bp, packed = s.score_pod_packed(pod)
    assert bp == best, tag
    word = (sc[:, 0] | (sc[:, 1] << 8) | (sc[:, 2] << 16) | (sc[:, 3] << 24)).astype(np.uint32)
    assert np.array_equal(packed, np.where(feas, word, np.uint32(0xFFFFFFFF))), tag


@pytest.mark.parametrize("arm", F.ARMS)
def test_wide_cases(arm):
    """Each arm reaches the wide layout (check_layout below asserts the layout of every case)."""
    assert F.wide_cases(arm) >= F.WIDE_FLOOR


@pytest.mark.parametrize("grid", F.GRIDS)
@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("arm", F.STREAM_ARMS)
def test_stream(arm, engine, grid):
    """Strategy, per-QoS and list arms on the six engines of the adversarial fuzz."""
    for i in F.selection(arm, grid):
        x, r = F.inputs(arm, i), F.reference(arm, i)
        tag = f"{arm} {engine} case {i} (seed {x['case']['seed']})"
        got = gpu_stream(x["nodes"], pods_to_struct(x["pods"]), engine_cfg(engine, x["case"], x["gcfg"]))
        check_same(tag, got, r["pl"], r["keys"], r["final"])
        check_layout(tag, x, got[3])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("grid", F.GRIDS)
@pytest.mark.parametrize("arm", F.STREAM_ARMS)
def test_score_pod(arm, grid, layout):
    """The score path on rows and on the column-major copy: the first three pods of each case."""
    for i in F.selection(arm, grid):
        x = F.inputs(arm, i)
        arr = pods_to_struct(x["pods"])  # (an empty stream scores no pod)
        with Scheduler(dict(x["gcfg"], **LAYOUTS[layout])) as s:
            s.load_nodes(x["nodes"])
            for j in range(min(3, x["case"]["p"])):
                check_scores(f"{arm} {layout} case {i} pod {j}", s, arr[j], F.score_reference(arm, i, j))


@pytest.mark.parametrize("grid", F.GRIDS)
@pytest.mark.parametrize("engine", list(TRACKED_ENGINES))
@pytest.mark.parametrize("arm", list(F.TRACKED_ARMS))
def test_tracked_stream(arm, engine, grid):
    """S12 + S13 with tracking on: the stream, the engine that ran, the layout, the recorded state of
    every app of the case, then the score path of the first three pods under that state."""
    name, extra = TRACKED_ENGINES[engine]
    for i in F.selection(arm, grid):
        x, r = F.inputs(arm, i), F.reference(arm, i)
        tag = f"{arm} {engine} case {i} (seed {x['case']['seed']})"
        arr = pods_to_struct(x["pods"])
        with Scheduler(dict(x["gcfg"], engine=name, **extra)) as s:
            s.set_pod_anti_affinity(True)
            s.load_nodes(x["nodes"])
            st = s.prepare(arr)
            stats = st.run()
            pl, keys = st.results()
            st.free()
            final = s.read_nodes()
            check_same(tag, (pl, keys, final), r["pl"], r["keys"], r["final"])
            assert stats["engine_used"] == name, tag
            check_layout(tag, x, stats)
            # (check_state takes its probe pods from the first three records: pad the short streams)
            check_state(s, np.concatenate([arr, np.zeros(3, POD_DTYPE)]), r["final"], r["state"],
                        np.unique(x["pods"]["app"]))
            for j in range(min(3, x["case"]["p"])):
                want = F.score_reference(arm, i, j, r["final"], r["state"])
                k = AA.pod_keys(r["final"], x["pods"], j, r["state"], x["ocfg"], F.scorer(arm, x["ocfg"]))
                assert np.array_equal(want[0], k != 0), tag
                assert np.array_equal(want[2], np.where(k != 0, (k >> np.uint64(32)).astype(np.int64) - 1, -1)), tag
                check_scores(f"{tag} pod {j}", s, arr[j], want)
