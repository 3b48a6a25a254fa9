"""Hostname topology spread (spec/semantics.md S15, ``QS_AA_SPREAD_HOSTNAME(max_skew)``), no GPU:

* the known answers K42-K47 of spec/kat.md through tests/hostspread_ref.py, and what the two wrong
  variants of the reference (``min_zero``, ``feasible_only``) make of them;
* properties of the reference: every other kind is S13's, ``max_skew = 31`` on few pods is the unfiltered
  stream, ``HOSTSPREAD(1)`` on an app with no more pods than nodes places as ``HOSTNAME`` does;
* the header, the binding's helper, and the register budget of the kernels that carry the filter;
* the conditions that make the parity inputs of tests/test_gpu_hostspread.py worth running.
"""
import os
import re

import numpy as np
import pytest

import qsched
from oracle import oracle as O
from qsched import _abi

import antiaffinity_cases as C
import antiaffinity_ref as A
import hostspread_cases as HC
import hostspread_ref as H
import spread_cases as SC
import spread_ref as S


def key(total, node):
    return ((total + 1) << 32) | (0xFFFFFFFF - node)


# winners' totals of the known-answer streams (spec/kat.md; 0 = unschedulable)
KAT_TOTALS = {"K42": [274, 200], "K43": [274, 274, 250], "K44": [274, 274, 0], "K45": [274, 274, 250, 250, 224],
              "K47": [274, 250, 200]}


# ---- known answers ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(KAT_TOTALS))
def test_kat_streams(name):
    nodes, pods, cfg, want_pl = HC.kat(name)
    pl, keys, _, st = H.run(nodes, pods, cfg)
    assert list(pl) == want_pl
    assert [int(k) for k in keys] == [key(t, n) if n >= 0 else 0 for t, n in zip(KAT_TOTALS[name], want_pl)]
    assert int(st.node[3].sum()) == sum(n >= 0 for n in want_pl)


def test_kat_k42_the_filter_moves_the_second_pod():
    nodes, pods, cfg, want_pl = HC.kat("K42")
    plain = {k: v.copy() for k, v in pods.items()}
    plain["anti_affinity"][:] = A.NONE
    assert list(H.run(nodes, plain, cfg)[0]) == [0, 0] and want_pl == [0, 1]


def test_kat_k43_min_zero_strands_the_third_pod():
    nodes, pods, cfg, want_pl = HC.kat("K43")
    assert list(H.run(nodes, pods, cfg, variant="min_zero")[0]) == [0, 1, -1]
    assert want_pl[2] == 0


def test_kat_k44_feasible_only_places_the_third_pod():
    nodes, pods, cfg, want_pl = HC.kat("K44")
    assert list(H.run(nodes, pods, cfg, variant="feasible_only")[0]) == [0, 1, 0]
    assert want_pl[2] == -1


def test_kat_k45_every_recorded_pod_counts():
    """With both the NONE and the HOSTNAME pod counted, cnt = (1, 1), m = 1 and the first HOSTSPREAD pod finds
    both nodes open (and takes node 0).  Without either of them cnt = (1, 0) and node 1 alone is open."""
    nodes, pods, cfg, want_pl = HC.kat("K45")
    for drop, first in ((0, 1), (1, 1)):
        rest = {k: np.delete(v, drop, axis=0) for k, v in pods.items()}
        st = H.HostSpreadState(nodes["zone"])
        on = {k: v.copy() for k, v in nodes.items()}
        H.schedule(on, {k: v[:1] for k, v in rest.items()}, cfg, state=st)
        k = A.pod_keys(on, rest, 1, st, cfg)
        assert list(np.flatnonzero(k != 0)) == [first]
    assert want_pl[2:] == [0, 1, 0]


def test_kat_k46_reserve_unreserve():
    nodes, pods, cfg, _ = HC.kat("K46")
    st = H.HostSpreadState(nodes["zone"])
    for node, sign, want in HC.K46_STEPS:
        assert st.record(4, node, sign)
        A.reserve(nodes, pods, 1, node, sign)
        k = A.pod_keys(nodes, pods, 0, st, cfg)
        assert [i for i, v in enumerate(k) if v] == want
    # the third step is an Unreserve that lowers m from 1 to 0 and closes node 0 again
    assert HC.K46_STEPS[1][2] == [0, 1] and HC.K46_STEPS[2][1:] == (-1, [1])


def test_kat_k47_differs_from_skew_one():
    nodes, pods, cfg, want_pl = HC.kat("K47")
    one = {k: v.copy() for k, v in pods.items()}
    one["anti_affinity"][:] = HC.HS1
    assert list(H.run(nodes, one, cfg)[0]) == [0, 1, 0] != want_pl


# ---- properties of the reference ----------------------------------------------------------------
def test_other_kinds_are_s13():
    case = SC.parity_case("persistent-300")
    pl, keys, final, st = H.run(case["nodes"], case["pods"], case["ocfg"])
    assert np.array_equal(pl, case["pl"]) and np.array_equal(keys, case["keys"])
    assert np.array_equal(st.node, case["state"].node)


def test_skew_31_on_few_pods_is_the_unfiltered_stream():
    """At most 31 pods per app: cnt + 1 - m <= 31 always holds."""
    nodes, pods = HC.c5(300, 600)
    assert np.bincount(pods["app"]).max() <= 31
    p = pods.copy()
    p["anti_affinity"] = H.spread_hostname(31)
    e = {k: v.copy() for k, v in nodes.items()}
    epl, ekeys, _ = O.schedule(e, qsched.pods_from_struct(p), HC.ARRIVAL)
    pl, keys, final, _ = H.run(nodes, p, HC.ARRIVAL)
    assert np.array_equal(pl, epl) and np.array_equal(keys, ekeys)
    assert all(np.array_equal(final[k], e[k]) for k in e)


def test_hostspread_1_equals_hostname_while_pods_fit_the_nodes():
    """Apps with fewer pods than nodes: the minimum stays 0, and HOSTSPREAD(1) allows exactly the nodes
    without a pod of the app."""
    nodes, pods = C.c5(300, 1500)
    pods = pods.copy()
    assert np.bincount(pods["app"]).max() < 300
    pods["anti_affinity"] = A.HOSTNAME
    hpl = H.run(nodes, pods, HC.ARRIVAL)[0]
    sp = pods.copy()
    sp["anti_affinity"] = HC.HS1
    assert np.array_equal(H.run(nodes, sp, HC.ARRIVAL)[0], hpl)
    plain = pods.copy()
    plain["anti_affinity"] = 0
    assert not np.array_equal(H.run(nodes, plain, HC.ARRIVAL)[0], hpl)


def test_an_appended_node_enters_with_count_zero():
    nodes, pods, cfg, _ = HC.kat("K43")
    pl, _, final, st = H.run(nodes, pods, cfg)
    assert int(st.node[3].min()) == 1
    st.set_zones(np.concatenate([nodes["zone"], [0]]))
    assert st.node.shape[1] == 3 and int(st.node[3].min()) == 0
    assert list(st.infeasible(3, HC.HS1)) == [True, True, False]


# ---- the header, the binding, the kernels -----------------------------------------------------------
def test_encoding():
    assert _abi.QS_AA_HOSTKEY == qsched.QS_AA_HOSTKEY == H.HOSTKEY == 0x40000
    assert _abi.QS_ABI_VERSION == 3 and qsched.load().qs_struct_size(3) == _abi.POD_DTYPE.itemsize
    for s in (1, 2, 31):
        v = qsched.aa_spread_hostname(s)
        assert v == H.spread_hostname(s) == 3 | (s << 8) | (1 << 18)
        assert qsched.aa_kind(v) == 3 and qsched.aa_max_skew(v) == s
        assert qsched.aa_is_hostkey(v) == 1 and qsched.aa_is_soft(v) == 0
    assert qsched.aa_is_hostkey(qsched.aa_spread(1)) == 0 and qsched.aa_is_hostkey(qsched.aa_spread_soft(1)) == 0
    for bad in (0, 32, -1):
        with pytest.raises(ValueError):
            qsched.aa_spread_hostname(bad)
    arr = np.array([0, 1, S.spread(2), H.spread_hostname(2)])
    assert list(qsched.aa_is_hostkey(arr)) == [0, 0, 0, 1]


def test_header_declares_the_additions():
    here = os.path.dirname(os.path.abspath(__file__))
    h = open(os.path.join(here, "..", "include", "qsched.h")).read()
    assert "#define QS_ABI_VERSION 3" in h
    for s in ("#define QS_AA_HOSTKEY ((int32_t)0x40000)", "QS_AA_SPREAD_HOSTNAME(max_skew)", "QS_AA_IS_HOSTKEY(x)",
              "spec S15"):
        assert s in h, s
    assert "QS_AA_SPREAD_ZONE = 3" in h and not re.search(r"QS_AA_\w+ = 4", h)  # the kind stays 3


def _kernel_lds(names):
    """{kernel name: .group_segment_fixed_size} of the kernels of libqsched.so whose name contains one of
    `names` (tests/test_kernel_resources.py reads the same notes, without this field)."""
    import subprocess
    import tempfile
    from test_kernel_resources import LIB, LLVM, MAGIC
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", LIB, os.path.join(d, "x")],
                       check=True, capture_output=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        for i, a in enumerate(starts):
            b = starts[i + 1] if i + 1 < len(starts) else len(data)
            part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"b{i}.co")
            open(part, "wb").write(data[a:b])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True,
                           capture_output=True)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if any(x in name for x in names):
                    out[name] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    return out


def test_the_kernels_that_carry_the_filter_keep_their_budget():
    """The SCAN and score kernels of the six kFeatAA classes (k_scan_norm / _key / _commit,
    k_score_podg(_max)) stay without scratch and VGPR spills with the count test in them, and k_hc_scatter
    is there.  k_persistent<..., SOFT = false, HOST = true> exists for the six classes up to the caps
    persistent_cap<F, false, true> gives them (compact normalizing: one node per lane; every other class its
    usual cap), each without scratch or VGPR spills, within 256 VGPRs and within 160 KiB of LDS; no
    instantiation carries both trailing parameters."""
    from test_kernel_resources import LLVM, kernel_metadata
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("the ROCm LLVM tools are absent")
    meta = kernel_metadata()
    seen = {}
    for n, f in meta:
        m = re.search(r"(k_scan_norm|k_scan_key|k_scan_commit|k_score_podg_max|k_score_podg)ILj(\d+)E", n)
        if not m or not int(m.group(2)) & 64:
            continue
        seen.setdefault(m.group(1), set()).add(int(m.group(2)))
        assert not (f["private_segment_fixed_size"] or f["vgpr_spill_count"] or f["vgpr_count"] > 256), (n[:60], f)
    classes = {68, 116, 119, 76, 124, 127}
    assert all(seen[k] == classes for k in seen) and len(seen) == 5, seen
    assert any("k_hc_scatter" in n for n, _ in meta)
    host = {}
    for n, f in meta:
        m = re.search(r"k_persistentILi(\d+)ELi(\d+)ELj(\d+)ELb([01])ELb([01])E", n)
        if "k_persistentI" not in n:
            continue
        assert m, n[:80]  # every instantiation names both trailing parameters
        assert not (m.group(4) == "1" and m.group(5) == "1"), n[:80]
        if m.group(5) == "1":
            host.setdefault(int(m.group(3)), set()).add(int(m.group(1)) * int(m.group(2)))
            assert not (f["private_segment_fixed_size"] or f["vgpr_spill_count"] or f["vgpr_count"] > 256), (n[:60], f)
    small = {64, 128, 256, 512, 1024}
    assert host == {68: small | {2048, 3072}, 116: small | {2048}, 119: small,
                    76: small | {2048}, 124: small | {2048}, 127: small}
    lds = _kernel_lds(["k_persistentI"])
    assert lds and max(lds.values()) <= 163840
    big = max(v for n, v in lds.items() if re.search(r"ELb0ELb1E", n))
    print(f"largest k_persistent<..., HOST> group segment: {big} B")
    assert big > 65536  # (the three-nodes-per-lane instantiation: 96 KB of counts)


# ---- the GPU file's inputs, from the reference alone ---------------------------------------------
@pytest.mark.parametrize("name", list(HC.PARITY))
def test_parity_inputs_meet_their_conditions(name):
    HC.check_conditions(HC.parity_case(name))


def test_some_input_reaches_a_minimum_of_two():
    case = HC.parity_case("persistent-3")
    host = np.unique(case["pods"]["app"][H.is_hostkey(case["pods"]["anti_affinity"]) == 1])
    assert max(int(case["state"].node[a].min()) for a in host) >= 2
    assert int(case["state"].node.max()) >= 4  # counts well beyond a presence bit


def test_engine_rule_inputs():
    for apps in (16, 17):
        _, pods = HC.many_apps(300, 600, apps)
        assert len(np.unique(pods["app"])) == apps and (H.is_hostkey(pods["anti_affinity"]) == 1).all()
