"""Zone topology spread (spec/semantics.md S13, ``QS_AA_SPREAD(max_skew)``), no GPU:

* the known answers K32-K36 of spec/kat.md through tests/spread_ref.py;
* properties of the reference: ``max_skew = 31`` on few pods is the unfiltered stream, ``SPREAD(1)`` on
  an app with no more pods than domains places as ``ZONE`` does, every recorded pod counts;
* the conditions that make the parity inputs of tests/test_gpu_spread.py worth running;
* the binding's encoding helpers.
"""
import numpy as np
import pytest

import qsched
from oracle import oracle as O

import antiaffinity_cases as C
import antiaffinity_ref as A
import spread_cases as SC
import spread_ref as S


def key(total, node):
    return ((total + 1) << 32) | (0xFFFFFFFF - node)


# ---- known answers ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["K32", "K33", "K34", "K35"])
def test_kat_streams(name):
    nodes, pods, cfg, want_pl, want_tot = SC.kat(name)
    pl, keys, _, st = S.run(nodes, pods, cfg)
    assert list(pl) == want_pl
    assert [int(k) for k in keys] == [key(t, n) if n >= 0 else 0 for t, n in zip(want_tot, want_pl)]
    assert int(st.zcount[3].sum()) == len(want_pl)


def test_kat_k32_is_k28_with_the_fourth_replica_schedulable():
    nodes, pods, cfg, want_pl, _ = SC.kat("K32")
    z = {k: v.copy() for k, v in pods.items()}
    z["anti_affinity"][:] = A.ZONE
    assert list(S.run(nodes, z, cfg)[0]) == C.kat("K28")[3] == [0, 2, -1]
    assert want_pl == [0, 2, 1]


def test_kat_k33_differs_from_skew_one():
    nodes, pods, cfg, want_pl, _ = SC.kat("K33")
    one = {k: v.copy() for k, v in pods.items()}
    one["anti_affinity"][:] = S.spread(1)
    assert list(S.run(nodes, one, cfg)[0]) == [0, 2, 1, 2] != want_pl


def test_kat_k34_absent_zones_do_not_count():
    """Zone ids {0, 5, 63}: with the minimum over all 64 ids it stays 0 and the fourth pod finds no zone."""
    nodes, pods, cfg, want_pl, _ = SC.kat("K34")
    assert list(S.run(nodes, pods, cfg, all_zones=True)[0]) == [0, 1, 2, -1]
    assert want_pl[3] == 0


def test_kat_k35_a_none_pod_counts():
    nodes, pods, cfg, want_pl, _ = SC.kat("K35")
    rest = {k: v[1:].copy() for k, v in pods.items()}
    assert list(S.run(nodes, rest, cfg)[0]) == [0, 2]  # alone, the two SPREAD pods start at node 0
    assert want_pl[1:] == [2, 1]


def test_kat_k36_reserve_unreserve():
    nodes, pods, cfg, _, _ = SC.kat("K36")
    st = S.SpreadState(nodes["zone"])
    for node, sign, want in SC.K36_STEPS:
        assert st.record(4, node, sign)
        A.reserve(nodes, pods, 0, node, sign)
        k = A.pod_keys(nodes, pods, 0, st, cfg)
        assert [i for i, v in enumerate(k) if v] == want
        assert int(0xFFFFFFFF - (int(k.max()) & 0xFFFFFFFF)) == want[0]
    assert st.zcount.sum() == 0


# ---- properties of the reference ----------------------------------------------------------------
def test_skew_31_on_few_pods_is_the_unfiltered_stream():
    """At most 31 pods per app: c + 1 - m <= 31 always holds."""
    nodes, pods = SC.c5(300, 600)
    assert np.bincount(pods["app"]).max() <= 31
    p = pods.copy()
    p["anti_affinity"] = S.spread(31)
    e = {k: v.copy() for k, v in nodes.items()}
    epl, ekeys, _ = O.schedule(e, qsched.pods_from_struct(p), SC.ARRIVAL)
    pl, keys, final, _ = S.run(nodes, p, SC.ARRIVAL)
    assert np.array_equal(pl, epl) and np.array_equal(keys, ekeys)
    assert all(np.array_equal(final[k], e[k]) for k in e)


def test_spread_1_equals_zone_while_pods_fit_the_domains():
    """Apps with at most as many pods as domains, none of them unschedulable under ZONE: SPREAD(1) allows
    exactly the zones without a pod of the app (the minimum stays 0 until every domain holds one)."""
    nodes, pods = C.c5(300, 1500, apps=40, zones=4)
    pods = pods.copy()
    pods["app"] = 24 + 25 * ((np.arange(len(pods)) // 4) % 40)  # runs of four: 4 pods per app per 160
    pods = pods[:160]
    pods["anti_affinity"] = A.ZONE
    zpl = S.run(nodes, pods, SC.ARRIVAL)[0]
    assert (zpl >= 0).all()
    sp = pods.copy()
    sp["anti_affinity"] = S.spread(1)
    spl = S.run(nodes, sp, SC.ARRIVAL)[0]
    assert np.array_equal(zpl, spl)
    plain = pods.copy()
    plain["anti_affinity"] = 0
    assert not np.array_equal(S.run(nodes, plain, SC.ARRIVAL)[0], zpl)


def test_other_kinds_are_s12():
    case = C.parity_case("persistent-300")
    pl, keys, final, st = S.run(case["nodes"], case["pods"], case["ocfg"])
    assert np.array_equal(pl, case["pl"]) and np.array_equal(keys, case["keys"])
    assert np.array_equal(st.zcount, case["state"].zcount)


def test_parity_inputs_meet_their_conditions():
    for name in SC.PARITY:
        SC.check_conditions(SC.parity_case(name))


def test_cap_inputs():
    for apps in (64, 65):
        _, pods = SC.many_apps(300, 600, apps)
        assert len(np.unique(pods["app"])) == apps and (S.kind_of(pods["anti_affinity"]) == S.SPREAD).all()


# ---- the binding ----------------------------------------------------------------------------------
def test_encoding_helpers():
    assert qsched.QS_AA_SPREAD_ZONE == S.SPREAD == 3
    for s in (1, 2, 31):
        v = qsched.aa_spread(s)
        assert v == S.spread(s) == 3 | (s << 8)
        assert qsched.aa_kind(v) == 3 and qsched.aa_max_skew(v) == s
    for bad in (0, 32, -1):
        with pytest.raises(ValueError):
            qsched.aa_spread(bad)
    arr = np.array([0, 1, 2, S.spread(2)])
    assert list(qsched.aa_kind(arr)) == [0, 1, 2, 3] and list(qsched.aa_max_skew(arr)) == [0, 0, 0, 2]
