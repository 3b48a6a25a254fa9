// qs_kernels_strat.inc — instantiations of the kernels of qs_kernels.hpp for the MostAllocated and
// RequestedToCapacityRatio scoring strategies (kFeatStrat, spec/semantics.md S5 "Scoring
// strategies"; which of the two is a kernel argument: DevCfg::strat_tab(), a table for
// RequestedToCapacityRatio, none for MostAllocated).  Included by
// qs_kernels_strat.hip (compact rows, QS_STRAT_WIDE 0) and qs_kernels_strat_wide.hip (wide rows, 1),
// translation units of their own, so every LeastAllocated instantiation compiles from the code it
// compiled from before; two feature classes each: Fit + Balanced (+ ext), and the normalizing
// profile (TaintToleration / NodeAffinity).  The dispatchers of qs_kernels.hip route every launch
// whose DevCfg carries kFeatStrat here.
#include "qs_kernels.hpp"

#if QS_STRAT_WIDE
#define QS_STRAT_FN(name) strat_wide_##name
#else
#define QS_STRAT_FN(name) strat_compact_##name
#endif

namespace qs {

namespace {
constexpr uint32_t kSF = (QS_STRAT_WIDE ? kFeatWide : 0u) | kFeatExt | kFeatRes | kFeatStrat;
constexpr uint32_t kSN = kSF | kFeatTaint | kFeatAffinity;
}  // namespace

hipError_t QS_STRAT_FN(persistent)(const DevTable &t, const void *pods, const DPodX *podx, uint32_t P,
                                 const DevCfg &c, int32_t *on, uint64_t *ok, uint64_t *st, hipStream_t stream) {
    if (c.feat & kFeatNorm) return persistent_f<kSN>(t, pods, podx, P, c, on, ok, st, stream);
    return persistent_f<kSF>(t, pods, podx, P, c, on, ok, st, stream);
}

uint32_t QS_STRAT_FN(persistent_max_nodes)(uint32_t feat) {
    return (feat & kFeatNorm) ? persistent_cap<kSN>() : persistent_cap<kSF>();
}

hipError_t QS_STRAT_FN(scan_pod)(const DevTable &t, const void *pods, const DPodX *podx, uint32_t s,
                               const DevCfg &c, void *scratch, int32_t *on, uint64_t *ok, uint64_t *st,
                               uint8_t *feas, int32_t *score, int32_t *total, int part, hipStream_t stream) {
    if (c.feat & kFeatNorm)
        return scan_pod_f<kSN>(t, pods, podx, s, c, scratch, on, ok, st, feas, score, total, part, stream);
    return scan_pod_f<kSF>(t, pods, podx, s, c, scratch, on, ok, st, feas, score, total, part, stream);
}

hipError_t QS_STRAT_FN(score_pod1)(const DevTable &t, const void *pod, const DPodX *podx, const DevCfg &c,
                                 uint8_t *hout, uint64_t *gs, uint64_t seq, uint32_t pidx, const HostRow &prow,
                                 hipStream_t stream) {
    if (c.feat & kFeatNorm) return score_pod1_f<kSN>(t, pod, podx, c, hout, gs, seq, pidx, prow, stream);
    return score_pod1_f<kSF>(t, pod, podx, c, hout, gs, seq, pidx, prow, stream);
}

hipError_t QS_STRAT_FN(la_window)(const DevTable &t, const void *pods, const DPodX *podx, uint32_t s0, uint32_t P,
                                const DevCfg &c, const LaGeom &geo, const LaBufs &bf, int32_t *on, uint64_t *ok,
                                uint64_t *st, uint64_t *diag, hipStream_t stream, int part) {
    if (c.feat & kFeatNorm) return la_window_f<kSN>(t, pods, podx, s0, P, c, geo, bf, on, ok, st, diag, stream, part);
    return la_window_f<kSF>(t, pods, podx, s0, P, c, geo, bf, on, ok, st, diag, stream, part);
}

hipError_t QS_STRAT_FN(la_stream_res)(const DevTable &t, const void *pods, const DPodX *podx, const DevCfg &c,
                                    uint32_t P, const LaGeom &geo, uint64_t *lists0, uint64_t *clists0,
                                    uint32_t lwords, uint32_t cwords, uint4 *npart, NormInfo *norm, uint32_t *stat,
                                    unsigned long long *nfall, int32_t *on, uint64_t *ok, uint64_t *st, void *ctl,
                                    uint32_t sel_blocks, uint64_t *rdiag, const ResShard &rsh, hipStream_t stream) {
    if (c.feat & kFeatNorm)
        return la_stream_res_f<kSN>(t, pods, podx, c, P, geo, lists0, clists0, lwords, cwords, npart, norm, stat, nfall,
                                    on, ok, st, ctl, sel_blocks, rdiag, rsh, stream);
    return la_stream_res_f<kSF>(t, pods, podx, c, P, geo, lists0, clists0, lwords, cwords, npart, norm, stat, nfall, on,
                                ok, st, ctl, sel_blocks, rdiag, rsh, stream);
}

int QS_STRAT_FN(la_stream_res_per_cu)(const LaGeom &geo, uint32_t feat, uint32_t n) {
    return (feat & kFeatNorm) ? la_stream_res_per_cu<kSN>(geo, n) : la_stream_res_per_cu<kSF>(geo, n);
}

}  // namespace qs

#undef QS_STRAT_FN
