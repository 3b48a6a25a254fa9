// qs_kernels_aa.inc — instantiations of the kernels of qs_kernels.hpp with required pod
// anti-affinity (kFeatAA, spec/semantics.md S12): the PERSISTENT and SCAN engines and the score
// path; no lookahead kernel (DESIGN.md §3.4).  Included by qs_kernels_aa.hip (compact rows,
// QS_AA_WIDE 0) and qs_kernels_aa_wide.hip (wide rows, 1), translation units of their own, so every
// instantiation without the bit compiles from the code it compiled from before.  Three feature
// classes each: the default class (Fit + Balanced (+ ext), LeastAllocated), and the general class
// (the configurable-resource, per-pod-strategy scorers, whose LeastAllocated form over the default
// lists gives the default scores) without and with the normalizing plugins.  The dispatchers of
// qs_kernels.hip route every launch whose DevCfg carries kFeatAA here.
#include "qs_kernels.hpp"

#if QS_AA_WIDE
#define QS_AA_FN(name) aa_wide_##name
#else
#define QS_AA_FN(name) aa_compact_##name
#endif

namespace qs {

namespace {
constexpr uint32_t kAD = (QS_AA_WIDE ? kFeatWide : 0u) | kFeatAA | kFeatExt;
constexpr uint32_t kAG = kAD | kFeatRes | kFeatStrat;
constexpr uint32_t kAN = kAG | kFeatTaint | kFeatAffinity;
}  // namespace

#if !QS_AA_WIDE
// Reserve / Unreserve bookkeeping of one pod (qs_reserve / qs_unreserve on a context that tracks pod
// anti-affinity): one thread; the presence bit with plain stores, the (app, zone) count with an atomic add.
__global__ void k_aa_apply(DevTable t, uint32_t node, uint32_t app, int32_t sign, uint32_t clear_bit) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || !t.apps || node >= t.n || app >= kMaxApps) return;
    uint32_t *wp = t.apps + (size_t)(app >> 5) * t.cap + node;
    const uint32_t bit = 1u << (app & 31u);
    if (sign > 0) *wp = *wp | bit;
    else if (clear_bit) *wp = *wp & ~bit;
    atomicAdd(&t.zcount[app * kMaxZones + (uint32_t)t.zone[node]], sign > 0 ? 1 : -1);
    // ... and the (app, node) count of spec S15 where the context keeps them (the host has checked that
    // an Unreserve finds a recorded pod)
    uint16_t *hc = aa_hcount(t);
    if (hc) {
        uint16_t *cp = hc + (size_t)app * t.cap + node;
        *cp = (uint16_t)(*cp + (sign > 0 ? 1 : -1));
    }
}

// The (app, node) counts rebuilt from the host mirror's sparse map (spec S15): the array has been
// zeroed; entry k goes to cell idx[k] (= app * cap + node, below `cells`).
__global__ void k_hc_scatter(uint16_t *hc, const uint32_t *idx, const uint16_t *val, uint32_t m, uint32_t cells) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < m && idx[k] < cells) hc[idx[k]] = val[k];
}
#endif

hipError_t QS_AA_FN(persistent)(const DevTable &t, const void *pods, const DPodX *podx, uint32_t P,
                                const DevCfg &c, int32_t *on, uint64_t *ok, uint64_t *st, hipStream_t stream) {
    if (!t.apps) return hipErrorInvalidValue;
    if (c.feat & kFeatHost) {  // the stream holds hostname-spread pods (spec S15) and no soft pod
        if (c.feat & kFeatSoft) return hipErrorInvalidValue;
        if (c.feat & kFeatNorm) return persistent_f<kAN, false, true>(t, pods, podx, P, c, on, ok, st, stream);
        if (c.feat & kFeatRes) return persistent_f<kAG, false, true>(t, pods, podx, P, c, on, ok, st, stream);
        return persistent_f<kAD, false, true>(t, pods, podx, P, c, on, ok, st, stream);
    }
    if (c.feat & kFeatSoft) {  // the stream holds soft-spread pods (spec S14)
        if (c.feat & kFeatNorm) return persistent_f<kAN, true>(t, pods, podx, P, c, on, ok, st, stream);
        if (c.feat & kFeatRes) return persistent_f<kAG, true>(t, pods, podx, P, c, on, ok, st, stream);
        return persistent_f<kAD, true>(t, pods, podx, P, c, on, ok, st, stream);
    }
    if (c.feat & kFeatNorm) return persistent_f<kAN>(t, pods, podx, P, c, on, ok, st, stream);
    if (c.feat & kFeatRes) return persistent_f<kAG>(t, pods, podx, P, c, on, ok, st, stream);
    return persistent_f<kAD>(t, pods, podx, P, c, on, ok, st, stream);
}

uint32_t QS_AA_FN(persistent_max_nodes)(uint32_t feat) {
    if (feat & kFeatHost)
        return (feat & kFeatNorm) ? persistent_cap<kAN, false, true>()
                                  : (feat & kFeatRes) ? persistent_cap<kAG, false, true>() : persistent_cap<kAD, false, true>();
    if (feat & kFeatSoft)
        return (feat & kFeatNorm) ? persistent_cap<kAN, true>()
                                  : (feat & kFeatRes) ? persistent_cap<kAG, true>() : persistent_cap<kAD, true>();
    return (feat & kFeatNorm) ? persistent_cap<kAN>() : (feat & kFeatRes) ? persistent_cap<kAG>() : persistent_cap<kAD>();
}

hipError_t QS_AA_FN(scan_pod)(const DevTable &t, const void *pods, const DPodX *podx, uint32_t s,
                              const DevCfg &c, void *scratch, int32_t *on, uint64_t *ok, uint64_t *st,
                              uint8_t *feas, int32_t *score, int32_t *total, int part, hipStream_t stream) {
    if (!t.apps) return hipErrorInvalidValue;
    if (c.feat & kFeatNorm)
        return scan_pod_f<kAN>(t, pods, podx, s, c, scratch, on, ok, st, feas, score, total, part, stream);
    if (c.feat & kFeatRes)
        return scan_pod_f<kAG>(t, pods, podx, s, c, scratch, on, ok, st, feas, score, total, part, stream);
    return scan_pod_f<kAD>(t, pods, podx, s, c, scratch, on, ok, st, feas, score, total, part, stream);
}

hipError_t QS_AA_FN(score_pod1)(const DevTable &t, const void *pod, const DPodX *podx, const DevCfg &c,
                                uint8_t *hout, uint64_t *gs, uint64_t seq, uint32_t pidx, const HostRow &prow,
                                hipStream_t stream) {
    if (!t.apps) return hipErrorInvalidValue;
    if (c.feat & kFeatNorm) return score_pod1_f<kAN>(t, pod, podx, c, hout, gs, seq, pidx, prow, stream);
    if (c.feat & kFeatRes) return score_pod1_f<kAG>(t, pod, podx, c, hout, gs, seq, pidx, prow, stream);
    return score_pod1_f<kAD>(t, pod, podx, c, hout, gs, seq, pidx, prow, stream);
}

}  // namespace qs

#undef QS_AA_FN
