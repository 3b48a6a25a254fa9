"""Zone topology spread scoring (spec/semantics.md S14, ``QS_AA_SPREAD_SOFT(max_skew)``) without a GPU:
the known answers K37-K41 of spec/kat.md through the reference (tests/soft_spread_ref.py), LOGTAB against
an 80-digit evaluation, the ABI additions, the register budget of the k_persistent instantiations that
carry the score, and, from the reference alone, that every input of tests/test_gpu_soft_spread.py can
tell the score from its absence and from two wrong variants of it.
"""
import ctypes
import decimal
import math
import os
import re

import numpy as np
import pytest

import qsched
from qsched import _abi, pods_to_struct

import antiaffinity_ref as A
import soft_spread_cases as SC
import soft_spread_ref as R
import spread_ref as S


# ---- LOGTAB --------------------------------------------------------------------------------------
def _ln(k, ctx):
    return ctx.ln(decimal.Decimal(k))


def test_logtab_is_the_correctly_rounded_logarithm():
    """LOGTAB[D] is the double nearest to ln(D + 2): its distance from the 80-digit value is below half
    an ulp, and it is what math.log returns here."""
    ctx = decimal.Context(prec=80)
    assert len(R.LOGTAB) == 65
    for D in range(1, 65):
        v = R.LOGTAB[D]
        assert v == math.log(D + 2)
        exact = _ln(D + 2, ctx)
        err = abs(ctx.subtract(decimal.Decimal(v), exact))  # (a double converts to Decimal exactly)
        half_ulp = decimal.Decimal(math.ulp(v)) / 2
        assert err < half_ulp, D
        for other in (math.nextafter(v, 0.0), math.nextafter(v, 10.0)):
            assert abs(ctx.subtract(decimal.Decimal(other), exact)) > err, D


def test_logtab_in_the_host_code_and_the_spec():
    here = os.path.dirname(os.path.abspath(__file__))
    want = [float.hex(v) for v in R.LOGTAB[1:]]
    for path in ("../custom-k8s-scheduler_amd/csrc/qs_host.cpp", "../spec/semantics.md"):
        text = open(os.path.join(here, path)).read()
        got = re.findall(r"0x1\.[0-9a-f]{13}p\+[0-9]", text)
        assert got == want, path


# ---- known answers -------------------------------------------------------------------------------
def _last_totals(nodes, pods, cfg, **kw):
    """Per-node totals (-1 = infeasible) of the last pod after the pods before it ran as a stream."""
    n = len(pods["qos"])
    first = {k: v[:n - 1] for k, v in pods.items()}
    _, _, on, st = R.run(nodes, first, dict(cfg, qos_sort=0), **kw)
    k = R.pod_keys(on, pods, n - 1, st, cfg)
    return [int(x >> np.uint64(32)) - 1 if x else -1 for x in k]


@pytest.mark.parametrize("name", ["K37", "K38", "K39", "K40"])
def test_kat_streams(name):
    nodes, pods, cfg, want_pl, want_tot, want_last = SC.kat(name)
    pl, keys, _, _ = R.run(nodes, pods, dict(cfg, qos_sort=0))
    assert list(pl) == want_pl
    assert [int(k >> np.uint64(32)) - 1 for k in keys] == want_tot
    assert _last_totals(nodes, pods, cfg) == want_last


def test_kat_k38_rounds_and_k39_takes_feasible_zones_only():
    """The wrong variants give other totals on the known answers that pin them."""
    nodes, pods, cfg, _, _, want = SC.kat("K38")
    assert _last_totals(nodes, pods, cfg, truncate=True) == [450, 350, 350, 374] != want
    nodes, pods, cfg, _, _, want = SC.kat("K39")
    assert _last_totals(nodes, pods, cfg, all_domains=True) == [250, 250, 316, -1] != want
    # c = 6, D = 1: 6 ln 3 = 6.59 rounds to 7 and truncates to 6 (PTS is 100 either way: one zone)
    c = np.zeros(A.MAX_ZONES, np.int64)
    c[9] = 6
    assert R.zone_scores(c, [9], 1)[1:] == (1, 7, 7) and R.zone_scores(c, [9], 1, truncate=True)[1:] == (1, 6, 6)
    assert R.zone_scores(c, [9], 1)[0][9] == 100


def test_kat_k41_reserve_unreserve():
    nodes, pods, cfg, _, _, _ = SC.kat("K41")
    st = R.SoftSpreadState(nodes["zone"])
    for node, sign, want in SC.K41_STEPS:
        assert st.record(4, node, sign)
        A.reserve(nodes, pods, 1, node, sign)
        z = R.pod_zone_scores(nodes, pods, 0, st, cfg)
        assert list(z[:2]) == want and (z[2:] == -1).all()
    assert st.zcount.sum() == 0


def test_a_soft_pod_is_not_filtered_and_every_other_kind_scores_as_before():
    nodes, pods, cfg, _, _, _ = SC.kat("K38")
    st = R.SoftSpreadState(nodes["zone"])
    for _ in range(40):
        st.record(3, 1)
    assert (R.pod_keys(nodes, pods, 3, st, cfg) != 0).all()  # SPREAD(1) would leave zone 1 out
    assert np.array_equal(R.pod_keys(nodes, pods, 0, st, cfg), A.pod_keys(nodes, pods, 0, st, cfg))


# ---- ABI -----------------------------------------------------------------------------------------
def test_abi_additions():
    lib = qsched.load()
    for s in ("qs_set_topology_spread_weight", "qs_get_topology_spread_weight", "qs_score_pod_zone_scores"):
        assert hasattr(lib, s) and s in _abi.EXPORTED
    w = ctypes.c_int32(0)
    z = (ctypes.c_int32 * 64)()
    assert lib.qs_set_topology_spread_weight(None, 2) == _abi.QS_EINVAL  # null context: a status, no crash
    assert lib.qs_get_topology_spread_weight(None, ctypes.byref(w)) == _abi.QS_EINVAL
    assert lib.qs_score_pod_zone_scores(None, z) == _abi.QS_EINVAL
    assert lib.qs_struct_size(3) == _abi.POD_DTYPE.itemsize and _abi.QS_ABI_VERSION == 3
    for m in ("set_topology_spread_weight", "get_topology_spread_weight", "score_pod_zone_scores"):
        assert hasattr(qsched.Scheduler, m)
    # the macros keep their values for every existing input, and the flag sits above max_skew
    assert qsched.aa_spread_soft(5) == 3 | (5 << 8) | (1 << 16) == R.spread_soft(5)
    assert qsched.aa_kind(qsched.aa_spread_soft(5)) == 3 and qsched.aa_max_skew(qsched.aa_spread_soft(31)) == 31
    assert qsched.aa_is_soft(qsched.aa_spread_soft(1)) == 1 and qsched.aa_is_soft(qsched.aa_spread(1)) == 0
    for bad in (0, 32):
        with pytest.raises(ValueError):
            qsched.aa_spread_soft(bad)


def _header():
    here = os.path.dirname(os.path.abspath(__file__))
    return open(os.path.join(here, "..", "include", "qsched.h")).read()


def test_header_declares_the_additions():
    h = _header()
    assert "#define QS_ABI_VERSION 3" in h
    for s in ("QS_AA_SPREAD_SOFT(max_skew)", "qs_set_topology_spread_weight(qs_ctx *ctx, int32_t w)",
              "qs_get_topology_spread_weight(qs_ctx *ctx, int32_t *w)",
              "qs_score_pod_zone_scores(qs_ctx *ctx, int32_t out[QS_MAX_ZONES])"):
        assert s in h, s


# ---- kernel budget ------------------------------------------------------------------------------
def test_soft_persistent_kernels_are_built_within_the_register_budget():
    """libqsched.so carries k_persistent with the trailing SOFT parameter for the six kFeatAA classes up
    to the caps persistent_cap<F, true> gives them (compact normalizing: one node per lane; every other
    class its usual cap), each without scratch or VGPR spills and within 256 VGPRs; and the instantiations
    without the parameter are still there for every size they had."""
    from test_kernel_resources import LLVM, kernel_metadata
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("the ROCm LLVM tools are absent")
    meta = [(n, f) for n, f in kernel_metadata() if "k_persistentI" in n]
    soft = {}
    plain = {}
    for n, f in meta:
        m = re.search(r"k_persistentILi(\d+)ELi(\d+)ELj(\d+)E(Lb1E)?", n)
        npt, bs, feat = int(m.group(1)), int(m.group(2)), int(m.group(3))
        if not feat & 64:
            continue
        (soft if m.group(4) else plain).setdefault(feat, set()).add(npt * bs)
        assert not (f["private_segment_fixed_size"] or f["vgpr_spill_count"] or f["vgpr_count"] > 256), (n[:60], f)
    small = {64, 128, 256, 512, 1024}
    assert soft == {68: small | {2048, 3072}, 116: small | {2048}, 119: small,
                    76: small | {2048}, 124: small | {2048}, 127: small}
    assert plain == {68: small | {2048, 3072}, 116: small | {2048}, 119: small | {2048},
                     76: small | {2048}, 124: small | {2048}, 127: small}


# ---- the GPU file's inputs, from the reference alone ---------------------------------------------
@pytest.mark.parametrize("name", list(SC.PARITY))
def test_parity_inputs_tell_the_score_apart(name):
    SC.check_conditions(SC.parity_case(name))
