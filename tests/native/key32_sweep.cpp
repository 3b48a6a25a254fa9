// CPU sweep of the resident resolver's 32-bit key helpers (custom-k8s-scheduler_amd/csrc/qs_key32.hpp)
// against the 64-bit key format pack_key(tv, node) = tv << 32 | (0xFFFFFFFF - node):
//   convert(pack_key) == pack32, expand(pack32) == pack_key, a64 < b64 <=> a32 < b32, 0 <-> 0,
// for every tv in [0, 1024) x the edge nodes, and 1 M random pairs.  Prints "ok ..." or the first failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../custom-k8s-scheduler_amd/csrc/qs_key32.hpp"

static uint64_t pack_key(uint32_t tv, uint32_t idx) { return ((uint64_t)tv << 32) | (uint64_t)(0xFFFFFFFFu - idx); }
// the keys of (tv, node) in both widths; tv == 0 is "none": 0 in both
static uint64_t key64(uint32_t tv, uint32_t node) { return tv ? pack_key(tv, node) : 0ull; }
static uint32_t key32(uint32_t tv, uint32_t node) { return tv ? qs::k32_pack(tv, node) : 0u; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int check_one(uint32_t tv, uint32_t node) {
    const uint64_t k64 = key64(tv, node);
    const uint32_t k32 = key32(tv, node);
    if (qs::k32_from_key(k64) != k32) { printf("FAIL convert tv=%u node=%u\n", tv, node); return 1; }
    if (qs::k32_to_key(k32) != k64) { printf("FAIL expand tv=%u node=%u\n", tv, node); return 1; }
    if (tv) {
        if (qs::k32_node(k32) != node) { printf("FAIL node tv=%u node=%u\n", tv, node); return 1; }
        if ((qs::k32_score(tv) | qs::k32_low(node)) != k32) { printf("FAIL halves tv=%u node=%u\n", tv, node); return 1; }
        // a list entry converts the same way whatever its score half
        if ((k32 >> 22) != tv) { printf("FAIL score tv=%u node=%u\n", tv, node); return 1; }
    }
    return 0;
}
static int check_order(uint32_t ta, uint32_t na, uint32_t tb, uint32_t nb) {
    const uint64_t a64 = key64(ta, na), b64 = key64(tb, nb);
    const uint32_t a32 = key32(ta, na), b32 = key32(tb, nb);
    if ((a64 < b64) != (a32 < b32) || (a64 == b64) != (a32 == b32)) {
        printf("FAIL order (%u,%u) (%u,%u)\n", ta, na, tb, nb);
        return 1;
    }
    return 0;
}

int main() {
    const uint32_t edge[] = {0u, 1u, 2u, (1u << 21) - 1u, (1u << 21) + 1u, (1u << 22) - 2u, (1u << 22) - 1u};
    const int ne = (int)(sizeof edge / sizeof edge[0]);
    if (qs::k32_from_key(0ull) != 0u || qs::k32_to_key(0u) != 0ull) { printf("FAIL zero\n"); return 1; }
    unsigned long long n = 0;
    for (uint32_t tv = 0; tv < 1024; ++tv)
        for (int i = 0; i < ne; ++i) {
            if (check_one(tv, edge[i])) return 1;
            ++n;
        }
    // order over the edge grid: neighbouring scores x every pair of edge nodes
    for (uint32_t tv = 0; tv < 1024; ++tv)
        for (uint32_t tb = tv > 0 ? tv - 1 : 0; tb <= tv + 1 && tb < 1024; ++tb)
            for (int i = 0; i < ne; ++i)
                for (int j = 0; j < ne; ++j) {
                    if (check_order(tv, edge[i], tb, edge[j])) return 1;
                    ++n;
                }
    for (int k = 0; k < 1000000; ++k) {
        const uint64_t r = rng(), q = rng();
        const uint32_t ta = (uint32_t)(r & 1023u), na = (uint32_t)(r >> 20) & 0x3FFFFFu;
        // half of the pairs share the score, so the node half decides
        const uint32_t tb = (q & 1u) ? ta : (uint32_t)((q >> 1) & 1023u), nb = (uint32_t)(q >> 20) & 0x3FFFFFu;
        if (check_one(ta, na) || check_one(tb, nb) || check_order(ta, na, tb, nb)) return 1;
        ++n;
    }
    printf("ok %llu cases\n", n);
    return 0;
}
