"""QS_MODE_BATCHED with batches of one pod (spec S11; the sequential semantics with anti-affinity that
spec S12 also gives) on both sides of the batch count up to which a stream is replayed as one HIP graph
(8,192 batches; longer streams are enqueued directly): placements, keys and the final table against
the batched oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from qsched import Scheduler, pods_from_struct  # noqa: E402

import antiaffinity_cases as C  # noqa: E402


@pytest.mark.parametrize("p", [8000, 8192, 8193, 9000])
def test_batches_of_one(oracle, p):
    nodes, pods = C.c5(300, p)
    with Scheduler(dict(batch_pods=1)) as s:
        s.load_nodes(nodes)
        st = s.prepare(pods)
        stats = st.run(mode="batched")
        pl, keys = st.results()
        st.free()
        final = s.read_nodes()
    on = {k: v.copy() for k, v in nodes.items()}
    opl, okeys, batches = oracle.schedule_batched(on, pods_from_struct(pods), batch=1)
    assert stats["engine_used"] == "batched" and stats["batches"] == batches == p
    assert np.array_equal(pl, opl) and np.array_equal(keys, okeys)
    for k in on:
        assert np.array_equal(final[k], on[k]), k
