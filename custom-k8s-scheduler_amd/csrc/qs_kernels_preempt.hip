// qs_kernels_preempt.hip — the preemption dry run (spec/semantics.md S18): for one
// unschedulable pod, the victims every node would give up and the node to preempt on (UP
// plugins/defaultpreemption#SelectVictimsOnNode, framework/preemption/preemption.go#
// pickOneNodeForPreemption), as two plain launches over the device copy of the pod registry.
//
// The registry holds canonical int64 quantities (millicores, bytes, counts), whatever the table's
// layout: a lane widens its node row once (compact memory << shift, wide memory from its f64 integer)
// and every comparison of the dry run is 64-bit integer arithmetic.  No reciprocal, no rounding.
// No workgroup waits for another inside a kernel: the launch boundary orders the two passes.
#include "qs_device.hpp"
#include "qs_launch.hpp"

namespace qs {

constexpr uint32_t kPreBlock = 256, kPreMaxBlocks = 1024;

// The choice key of spec S18, smaller is better, compared field by field: k0 = class << 62 | hi
// (class 0: a candidate without victims, 1: with victims, 2: no candidate; hi < 2^35), k1 = sum << 9 |
// nvict (sum < 2^43, nvict <= 256), k2 = ~start (the highest start wins), idx = the node.
// (a kernel argument type: named in namespace qs, so the kernels' symbols are the same in both passes)
struct PKey {
    uint64_t k0, k1, k2;
    uint32_t idx;
};

namespace {

__device__ __forceinline__ PKey pkey_none() { return PKey{2ull << 62, 0ull, 0ull, 0xFFFFFFFFu}; }
__device__ __forceinline__ bool pkey_less(const PKey &a, const PKey &b) {
    if (a.k0 != b.k0) return a.k0 < b.k0;
    if (a.k1 != b.k1) return a.k1 < b.k1;
    if (a.k2 != b.k2) return a.k2 < b.k2;
    return a.idx < b.idx;
}
__device__ __forceinline__ PKey pkey_min(const PKey &a, const PKey &b) {
    const bool l = pkey_less(b, a);
    return PKey{l ? b.k0 : a.k0, l ? b.k1 : a.k1, l ? b.k2 : a.k2, l ? b.idx : a.idx};
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, kWave);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, kWave);
    return ((uint64_t)hi << 32) | lo;
}
// Every lane of the wave must be active; the result is the wave's minimum in every lane.
__device__ __forceinline__ PKey wave_min_pkey(PKey k) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        PKey o;
        o.k0 = shfl_xor_u64(k.k0, m);
        o.k1 = shfl_xor_u64(k.k1, m);
        o.k2 = shfl_xor_u64(k.k2, m);
        o.idx = (uint32_t)__shfl_xor((int)k.idx, m, kWave);
        k = pkey_min(k, o);
    }
    return k;
}
// The workgroup's minimum, valid in thread 0.
__device__ __forceinline__ PKey block_min_pkey(PKey k) {
    __shared__ PKey red[kPreBlock / kWave];
    k = wave_min_pkey(k);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = k;
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t w = 1; w < kPreBlock / kWave; ++w) k = pkey_min(k, red[w]);
    return k;
}

// One node row in canonical units.
struct CRow {
    int64_t ac, am, rc, rm, np, mp, ae0, re0, ae1, re1;
};
// NodeResourcesFit.Filter of spec S4 (fits() of qs_device.hpp on canonical quantities)
__device__ __forceinline__ bool cfits(const CRow &r, const PreemptPod &p) {
    bool ok = r.np < r.mp;
    ok &= (p.rc <= 0) | (p.rc <= r.ac - r.rc);
    ok &= (p.rm <= 0) | (p.rm <= r.am - r.rm);
    ok &= (p.re0 == 0) | (p.re0 <= r.ae0 - r.re0);
    ok &= (p.re1 == 0) | (p.re1 <= r.ae1 - r.re1);
    return ok;
}

// The dry run of node i (spec S18 steps 1-5).  Returns the node's choice key; *nv = its victims (-1: no
// candidate).  EMIT: the victims' slot numbers go to `slots_out` in walk order (one lane, k_preempt_pick).
// The slot loops run to the table-wide rv.slots under a per-lane length mask: bounded and wave-uniform.
template <bool WIDE, bool EMIT>
__device__ __forceinline__ PKey dry_run(const DevTable &t, const RegView &rv, const PreemptPod &pp, const DPodX &px,
                                        uint32_t i, int32_t *nv, uint32_t *slots_out) {
    constexpr uint32_t F = kFeatExt | kFeatTaint | kFeatAffinity | (WIDE ? kFeatWide : 0u);
    const RowT<F> r = load_row<F>(t, i);
    const RowX x = load_rowx<F>(t, i);
    // step 1: the static filters, through feasible() on a row and a pod that pass Fit by construction
    // (the host's pod extension record is neutral for a disabled plugin, compact_podx)
    Row r0 = empty_row<0u>();
    r0.mp = 1;
    DPod p0{};
    p0.flags = pp.flags;
    const bool resolvable = feasible<kFeatTaint | kFeatAffinity>(r0, x, p0, px);
    CRow c;
    c.ac = r.ac; c.rc = r.rc; c.np = r.np; c.mp = r.mp;
    if constexpr (WIDE) {
        c.am = (int64_t)r.am; c.rm = (int64_t)r.rm;
    } else {
        c.am = (int64_t)r.am << pp.shift; c.rm = (int64_t)r.rm << pp.shift;
    }
    c.ae0 = x.ae0; c.re0 = x.re0; c.ae1 = x.ae1; c.re1 = x.re1;
    const uint32_t slots = rv.slots;
    const uint32_t len = min(rv.len[i], slots);
    const size_t cs = (size_t)slots * rv.cap;  // elements per column
    const uint64_t *base = rv.col + i;
    // step 2 + 3: the entries less important than the pod form a suffix of the sorted list; take them all out
    uint32_t cnt = 0;
    for (uint32_t s = 0; s < slots; ++s) {
        if (s < len) {
            const uint64_t *e = base + (size_t)s * rv.cap;
            if (e[kRegImp * cs] < pp.imp) {
                c.rc -= (int64_t)e[kRegCpu * cs];
                c.rm -= (int64_t)e[kRegMem * cs];
                c.re0 -= (int64_t)e[kRegExt0 * cs];
                c.re1 -= (int64_t)e[kRegExt1 * cs];
                ++cnt;
            }
        }
    }
    c.np -= (int64_t)cnt;
    const bool cand = resolvable & (cnt != 0u) & cfits(c, pp);
    // step 4: the reprieve walk, most important first
    const uint32_t first = len - cnt;
    uint32_t nvict = 0;
    uint64_t hi = 0, sum = 0, start = 0;
    for (uint32_t s = 0; s < slots; ++s) {
        if (cand && s >= first && s < len) {
            const uint64_t *e = base + (size_t)s * rv.cap;
            CRow b = c;
            b.rc += (int64_t)e[kRegCpu * cs];
            b.rm += (int64_t)e[kRegMem * cs];
            b.re0 += (int64_t)e[kRegExt0 * cs];
            b.re1 += (int64_t)e[kRegExt1 * cs];
            b.np += 1;
            if (cfits(b, pp)) {
                c = b;  // reprieved
            } else {
                const uint64_t imp = e[kRegImp * cs];
                if (nvict == 0u) {
                    hi = imp;
                    start = e[kRegSeq * cs];  // (walk order: the lowest seq among the victims of importance hi)
                }
                sum += imp;
                if (EMIT && nvict < kPreemptMaxVictims) slots_out[nvict] = s;
                ++nvict;
            }
        }
    }
    *nv = cand ? (int32_t)nvict : -1;
    if (!cand) return pkey_none();
    if (nvict == 0u) return PKey{0ull, 0ull, 0ull, i};
    return PKey{(1ull << 62) | hi, (sum << 9) | (uint64_t)nvict, ~start, i};
}

}  // namespace

// One lane per node, grid-stride; one candidate record per workgroup.
template <bool WIDE>
__global__ void __launch_bounds__(kPreBlock) k_preempt_nodes(DevTable t, RegView rv, PreemptPod pp, const DPodX *podx,
                                                             int32_t *nvict_n, PKey *rec) {
    const DPodX px = load_vgpr(podx);
    PKey best = pkey_none();
    // (the bound is rounded up to whole workgroups so that every lane reaches the reductions)
    const uint32_t step = gridDim.x * kPreBlock;
    for (uint32_t i0 = blockIdx.x * kPreBlock; i0 < t.n; i0 += step) {
        const uint32_t i = i0 + threadIdx.x;
        if (i < t.n) {
            int32_t nv;
            const PKey k = dry_run<WIDE, false>(t, rv, pp, px, i, &nv, nullptr);
            if (nvict_n) nvict_n[i] = nv;
            best = pkey_min(best, k);
        }
    }
    best = block_min_pkey(best);
    if (threadIdx.x == 0) rec[blockIdx.x] = best;
}

// One workgroup: the minimum of the records, then one lane re-walks the winner's list for its victims.
template <bool WIDE>
__global__ void __launch_bounds__(kPreBlock) k_preempt_pick(DevTable t, RegView rv, PreemptPod pp, const DPodX *podx,
                                                            const PKey *rec, uint32_t nrec, PreemptOut *out) {
    PKey best = pkey_none();
    for (uint32_t k = threadIdx.x; k < nrec; k += kPreBlock) best = pkey_min(best, rec[k]);
    best = block_min_pkey(best);
    if (threadIdx.x != 0) return;
    if (best.idx >= t.n) {
        out->node = -1;
        out->nvict = 0;
        return;
    }
    const DPodX px = *podx;
    int32_t nv;
    (void)dry_run<WIDE, true>(t, rv, pp, px, best.idx, &nv, out->slot);
    out->node = (int32_t)best.idx;
    out->nvict = nv < 0 ? 0u : min((uint32_t)nv, kPreemptMaxVictims);
}

// Registry entries from the host's staging buffer into the slot-major device copy, and the lengths of
// the nodes they belong to.  Every index is checked against the copy's extent.
__global__ void k_preempt_scatter(uint64_t *col, uint32_t *len, uint32_t slots, uint32_t cap, const RegItem *items,
                                  uint32_t m, const uint32_t *lnode, const uint32_t *lval, uint32_t k) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t cs = (size_t)slots * cap;
    if (j < m) {
        const RegItem it = items[j];
        if (it.node < cap && it.slot < slots) {
#pragma unroll
            for (uint32_t q = 0; q < kRegCols; ++q) col[q * cs + (size_t)it.slot * cap + it.node] = it.v[q];
        }
    }
    if (j < k && lnode[j] < cap) len[lnode[j]] = min(lval[j], slots);
}

size_t preempt_scratch_bytes() { return sizeof(PKey) * kPreMaxBlocks; }

hipError_t launch_preempt(const DevTable &t, bool wide, const RegView &rv, const PreemptPod &pp, const DPodX *px,
                          int32_t *nvict_n, void *scratch, PreemptOut *out, hipStream_t stream) {
    if (t.n == 0 || t.n > rv.cap || rv.slots == 0 || rv.slots > kPreemptMaxVictims || !rv.col || !rv.len ||
        !(wide ? (const void *)t.wrows : (const void *)t.rows))
        return hipErrorInvalidValue;
    const uint32_t want = (t.n + kPreBlock - 1) / kPreBlock;
    const uint32_t blocks = want < kPreMaxBlocks ? want : kPreMaxBlocks;
    PKey *rec = static_cast<PKey *>(scratch);
    if (wide) {
        hipLaunchKernelGGL(k_preempt_nodes<true>, dim3(blocks), dim3(kPreBlock), 0, stream, t, rv, pp, px, nvict_n, rec);
        hipLaunchKernelGGL(k_preempt_pick<true>, dim3(1), dim3(kPreBlock), 0, stream, t, rv, pp, px, rec, blocks, out);
    } else {
        hipLaunchKernelGGL(k_preempt_nodes<false>, dim3(blocks), dim3(kPreBlock), 0, stream, t, rv, pp, px, nvict_n, rec);
        hipLaunchKernelGGL(k_preempt_pick<false>, dim3(1), dim3(kPreBlock), 0, stream, t, rv, pp, px, rec, blocks, out);
    }
    return hipGetLastError();
}

hipError_t launch_preempt_scatter(uint64_t *col, uint32_t *len, uint32_t slots, uint32_t cap, const RegItem *items,
                                  uint32_t m, const uint32_t *lnode, const uint32_t *lval, uint32_t k,
                                  hipStream_t stream) {
    const uint32_t work = m > k ? m : k;
    if (work == 0) return hipSuccess;
    hipLaunchKernelGGL(k_preempt_scatter, dim3((work + 255) / 256), dim3(256), 0, stream, col, len, slots, cap, items,
                       m, lnode, lval, k);
    return hipGetLastError();
}

}  // namespace qs
