// qs_key32.hpp — the resident resolver's 32-bit keys.
//
// A 64-bit key is pack_key(tv, node) = tv << 32 | (0xFFFFFFFF - node) with tv = total + 1 (0 = none).
// Where tv < 2^10 and node < 2^22 (the host's k32 rule: 100 * wmax + 1 < 1024 and n <= 2^22) the same
// order fits 32 bits:  k32 = tv << 22 | (0x3FFFFF - node), 0 = none.  u32 order on k32 equals u64
// order on pack_key, so the ring resolver carries k32 from the entry loader to the published winner
// and expands a pod's result once per window.
//
// Plain integer code without device builtins: the kernels include it, and tests/native/key32_sweep.cpp
// sweeps it on the CPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define QS_K32_FN __host__ __device__ __forceinline__
#else
#define QS_K32_FN inline
#endif

namespace qs {

constexpr uint32_t kK32NodeBits = 22;
constexpr uint32_t kK32NodeMask = (1u << kK32NodeBits) - 1u;  // 0x3FFFFF

// the score half alone (a slot's key before its node is or-ed in); tv = total + 1, 0 = infeasible
QS_K32_FN uint32_t k32_score(uint32_t tv) { return tv << kK32NodeBits; }
// the node half: 0x3FFFFF - node
QS_K32_FN uint32_t k32_low(uint32_t node) { return kK32NodeMask - node; }
QS_K32_FN uint32_t k32_pack(uint32_t tv, uint32_t node) { return k32_score(tv) | k32_low(node); }
QS_K32_FN uint32_t k32_node(uint32_t k) { return kK32NodeMask - (k & kK32NodeMask); }
// a 64-bit key or list entry (low word 0xFFFFFFFF - node, node < 2^22) as k32; 0 -> 0
QS_K32_FN uint32_t k32_from_key(uint64_t key) {
    return ((uint32_t)(key >> 32) << kK32NodeBits) | ((uint32_t)key & kK32NodeMask);
}
// back to the 64-bit key; 0 -> 0
QS_K32_FN uint64_t k32_to_key(uint32_t k) {
    return k ? ((uint64_t)(k >> kK32NodeBits) << 32) | (uint64_t)(0xFFFFFFFFu - k32_node(k)) : 0ull;
}

}  // namespace qs
