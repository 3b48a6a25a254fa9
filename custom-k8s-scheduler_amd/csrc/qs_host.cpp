// qs_host.cpp — libqsched host runtime: the C ABI of include/qsched.h over the gfx950 kernels.
//
// Responsibilities:
//  * authoritative int64 host mirror of the node table (UP framework/types.go#NodeInfo) with
//    per-row generations (qs_node_upsert diff), rebuilt onto the device on demand;
//  * compaction to the device layout (spec S10): memory in units of 2^u bytes, int32 columns,
//    per-node reciprocals RN_f64(1/alloc), RN_f32(1/alloc);
//  * pod precompute (spec S2/S3/S8/S9): QoSSort order, per-QoS weights, compact pod records;
//  * engine dispatch (persistent / scan / lookahead) on one HIP stream per context;
//  * error handling: every entry point catches everything and returns a qs_status.
#include "../../include/qsched.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <new>
#include <string>
#include <vector>
#include <functional>
#include <condition_variable>
#include <thread>

#include "qs_ctx.hpp"

using namespace qs;

using namespace qs_host;

namespace {

// ---- environment knobs of the stream-run path (qs_stream_run and its engines) ----------------------
// Every getenv of that path is here.  (The score path's QS_UNPACK_* / QS_SCORE_DIAG and QS_FORCE_RES
// stay with their code.)
char env_char(const char *name) {  // the value's first character; 0: unset or empty
    const char *e = getenv(name);
    return e ? e[0] : 0;
}
bool env_is(const char *name, char v) { return env_char(name) == v; }
int env_int(const char *name) {
    const char *e = getenv(name);
    return e ? atoi(e) : 0;
}

// Read once per process, on first use: tests and tools set these from outside the process only.
struct ProcKnobs {
    bool overlap_off = env_is("QS_LA_OVERLAP", '0');          // 0: serial lookahead windows
    bool resolver_waves1 = env_is("QS_RESOLVER_WAVES", '1');  // 1: single-wave resolver (serial windows)
    bool diag = env_is("QS_DIAG", '1');                       // 1: diagnostic resolver, shader-clock stamps on stderr
    bool handoff_off = env_is("QS_HANDOFF", '0');             // 0: cross-stream events, no in-kernel window hand-off
    char graph = env_char("QS_GRAPH");  // '1': force graph replay (sharded and hand-off runs too); '0': never capture
    // n: a host sync every n windows / batches (profiling aid: bounds the launches in flight under counter
    // collection).  Clamped to >= 0: batched mode used to cast a negative n to a period of 2^32 - |n|, which
    // no reachable batch count is a multiple of, so it never synced either.
    uint32_t sync_every = (uint32_t)std::max(0, env_int("QS_SYNC_EVERY"));
    uint32_t res_sel = (uint32_t)std::max(0, env_int("QS_RES_SEL"));  // n > 0: selector workgroups of the resident launch
    bool res_diag = [] {  // 1 | 2: the resident resolver's time split on stderr (the digit itself: RunKnobs::sel_diag)
        const char d = env_char("QS_RES_DIAG");
        return d == '1' || d == '2';
    }();
};
const ProcKnobs &proc_knobs() {
    static const ProcKnobs k;
    return k;
}

// Read at the start of every run: tests and A/B timing switch these per case inside one process.
struct RunKnobs {
    bool norm_waves1 = env_is("QS_NORM_WAVES", '1');            // 1: single-wave normalizing resolver
    bool resident_off = env_is("QS_RESIDENT", '0');             // 0: per-window launches
    bool res_k32_off = env_is("QS_RES_K32", '0');               // 0: the resident resolver's 64-bit key path
    bool fast_alloc_off = env_is("QS_FAST_ALLOC", '0');         // 0: generic scorers (zero-allocatable terms kept)
    bool res_uniform_off = env_is("QS_RES_UNIFORM", '0');       // 0: no uniform windows
    bool fused_merge_off = env_is("QS_BATCH_FUSED_MERGE", '0');  // 0: batched mode's separate k_la_merge launch
    const char *inject = getenv("QS_INJECT_FAULT");             // test hooks (inject_once; tests/test_gpu_recovery.py)
    bool hosttime = getenv("QS_HOSTTIME") != nullptr;           // set: the lookahead enqueue's host time on stderr
    bool norm_diag = getenv("QS_NORM_DIAG") != nullptr;         // set: rescans and resumed windows on stderr
    bool sel_diag = env_is("QS_RES_DIAG", '1');                 // 1 (not 2): the selectors stamp too
};

uint32_t feat_of(const qs_config &c) {
    uint32_t f = 0;
    if (c.enable_taint) f |= kFeatTaint;
    if (c.enable_affinity) f |= kFeatAffinity;
    return f;
}

void check_cfg(const qs_config &c) {
    if (c.abi_version != QS_ABI_VERSION) fail(QS_EINVAL, "qs_config.abi_version mismatch");
    if (c.fit_weight_cpu < 0 || c.fit_weight_mem < 0 || c.fit_weight_cpu > 65535 ||
        c.fit_weight_mem > 65535)
        fail(QS_EINVAL, "fit weights out of range");
    int64_t wmax = 0;
    for (int q = 0; q < 3; q++) {
        if (c.w_fit[q] < 0 || c.w_bal[q] < 0 || c.w_fit[q] > 65535 || c.w_bal[q] > 65535)
            fail(QS_EINVAL, "plugin weights must be in [0, 65535]");
        wmax = std::max<int64_t>(wmax, (int64_t)c.w_fit[q] + c.w_bal[q]);
    }
    if (c.w_taint < 0 || c.w_affinity < 0 || c.w_taint > 65535 || c.w_affinity > 65535)
        fail(QS_EINVAL, "plugin weights must be in [0, 65535]");
    // scoring-resource lists (UP apis/config/validation/validation_pluginargs.go#validateResources:
    // known resource, no duplicates, weight 1..100)
    if (c.n_fit_resources < 0 || c.n_fit_resources > QS_MAX_SCORE_RES)
        fail(QS_EINVAL, "n_fit_resources must be in [0, 4]");
    if (c.n_balanced_resources < 0 || c.n_balanced_resources > QS_MAX_SCORE_RES)
        fail(QS_EINVAL, "n_balanced_resources must be in [0, 4]");
    uint32_t seen = 0;
    for (int i = 0; i < c.n_fit_resources; i++) {
        const int32_t r = c.fit_resources[i].resource;
        if (r < QS_RES_CPU || r > QS_RES_EXT1) fail(QS_EINVAL, "fit_resources: unknown resource");
        if (seen & (1u << r)) fail(QS_EINVAL, "fit_resources: duplicate resource");
        seen |= 1u << r;
        if (c.fit_resources[i].weight < 1 || c.fit_resources[i].weight > 100)
            fail(QS_EINVAL, "fit_resources: weight must be in [1, 100]");
    }
    seen = 0;
    for (int i = 0; i < c.n_balanced_resources; i++) {
        const int32_t r = c.balanced_resources[i];
        if (r < QS_RES_CPU || r > QS_RES_EXT1) fail(QS_EINVAL, "balanced_resources: unknown resource");
        if (seen & (1u << r)) fail(QS_EINVAL, "balanced_resources: duplicate resource");
        seen |= 1u << r;
    }
    // total + 1 must fit the 32-bit score half of the packed key (spec S6/S7)
    const int64_t tmax = 100 * (wmax + (c.enable_taint ? c.w_taint : 0) +
                                (c.enable_affinity ? c.w_affinity : 0));
    if (tmax >= 0x7FFFFFFF) fail(QS_EINVAL, "weighted total would overflow the packed key");
}

// LeastAllocated weight per scoring resource (index qs_resource; 0 = not in the list): the list,
// or the default [cpu: fit_weight_cpu, memory: fit_weight_mem]
void fit_weights(const qs_config &c, int64_t w[5]) {
    for (int r = 0; r < 5; r++) w[r] = 0;
    if (c.n_fit_resources == 0) {
        w[QS_RES_CPU] = c.fit_weight_cpu;
        w[QS_RES_MEMORY] = c.fit_weight_mem;
        return;
    }
    for (int i = 0; i < c.n_fit_resources; i++) w[c.fit_resources[i].resource] = c.fit_resources[i].weight;
}

// The BalancedAllocation list as 4-bit ids in list order (DevCfg::bal); default [cpu, memory].
uint32_t balanced_ids(const qs_config &c) {
    if (c.n_balanced_resources == 0) return QS_RES_CPU | (QS_RES_MEMORY << 4);
    uint32_t b = 0;
    for (int i = 0; i < c.n_balanced_resources; i++) b |= (uint32_t)c.balanced_resources[i] << (4 * i);
    return b;
}

// Does a stream (or pod) need the resource-list form of the scorers (kFeatRes, spec S5 "Scoring
// resources")?  Not when the lists reduce to the two-resource form the default kernels compute:
// LeastAllocated over cpu / memory with any weights, BalancedAllocation over exactly {cpu, memory}
// (its two-fraction std is symmetric in the order).  Extended resources drop out of both lists when
// no pod of the stream requests them (a scalar resource with podRequest == 0 is skipped).
uint32_t res_feat(const qs_config &c, bool has_ext) {
    // QS_FORCE_RES=1 (measurements, tools/strategy_compare.py): never reduce, so that
    // LeastAllocated runs the kernel family the other strategies run, on the same lists.  Read once.
    static const bool force = getenv("QS_FORCE_RES") && getenv("QS_FORCE_RES")[0] == '1';
    if (force) return kFeatRes | kFeatExt;
    int64_t w[5];
    fit_weights(c, w);
    bool generic = has_ext && (w[QS_RES_EXT0] != 0 || w[QS_RES_EXT1] != 0);
    uint32_t set = 0;
    const uint32_t b = balanced_ids(c);
    for (int i = 0; i < QS_MAX_SCORE_RES; i++) {
        const uint32_t id = (b >> (4 * i)) & 15u;
        if (id == QS_RES_CPU || id == QS_RES_MEMORY || (has_ext && id >= QS_RES_EXT0)) set |= 1u << id;
    }
    generic |= set != ((1u << QS_RES_CPU) | (1u << QS_RES_MEMORY));
    return generic ? (kFeatRes | kFeatExt) : 0u;
}
// A stream (or pod) runs the kFeatStrat kernels, whatever the lists are, when some pod of it belongs
// to a QoS class whose strategy is not LeastAllocated; otherwise every pod of it scores
// LeastAllocated and it reduces as res_feat says (the same kind of exact reduction: the kFeatStrat
// kernels compute the kFeatRes score for such a pod).
uint32_t strat_feat(const qs_ctx *c, const qs_pod *pods, uint32_t p) {
    if (c->strat[0].type == QS_STRATEGY_LEAST_ALLOCATED && c->strat[1].type == QS_STRATEGY_LEAST_ALLOCATED &&
        c->strat[2].type == QS_STRATEGY_LEAST_ALLOCATED)
        return 0u;
    for (uint32_t j = 0; j < p; j++)
        if (c->strat[pods[j].qos].type != QS_STRATEGY_LEAST_ALLOCATED) return kFeatStrat | kFeatRes | kFeatExt;
    return 0u;
}

// Feature set of an exact stream or qs_score_pod call on a context that tracks pod anti-affinity
// (spec S12; qs_kernels_aa.inc): kFeatAA on every one, also a stream without anti-affinity pods, whose
// pods must still be recorded.  Fit + Balanced (+ ext) LeastAllocated is the default class; everything
// else runs the general class, the configurable-resource scorers with the per-pod strategy, whose
// LeastAllocated form over the default lists gives the default scores (as QS_FORCE_RES relies on).
uint32_t aa_feat(uint32_t feat) {
    const uint32_t wide = feat & kFeatWide;
    if ((feat & ~(kFeatWide | kFeatExt)) == 0) return kFeatAA | kFeatExt | wide;
    const uint32_t norm = (feat & (kFeatTaint | kFeatAffinity)) ? (kFeatTaint | kFeatAffinity) : 0u;
    return kFeatAA | kFeatExt | kFeatRes | kFeatStrat | wide | norm;
}
void aa_check_table(const qs_ctx *c) {
    if (c->dev_valid && !c->dt.apps)
        fail(QS_EINVAL, "pod anti-affinity tracking keeps its state for tables up to 2^20 nodes");
}

DevCfg make_devcfg(const qs_config &c) {
    DevCfg d{};
    int64_t w[5];
    fit_weights(c, w);
    d.wc = (int32_t)w[QS_RES_CPU];
    d.wm = (int32_t)w[QS_RES_MEMORY];
    d.we0 = (int32_t)w[QS_RES_EXT0];
    d.we1 = (int32_t)w[QS_RES_EXT1];
    d.bal = balanced_ids(c);
    auto rcp = [](int64_t v) { return v > 0 ? 1.0 / (double)v : 0.0; };  // RN_f64(1/v)
    d.yd_both = rcp(w[QS_RES_CPU] + w[QS_RES_MEMORY]);
    d.yd_c = rcp(w[QS_RES_CPU]);
    d.yd_m = rcp(w[QS_RES_MEMORY]);
    // a disabled plugin weighs 0 (the kernels of the normalizing class evaluate both plugins; the
    // pod records of a disabled plugin are neutral, see compact_pod / compact_podx)
    d.wtt = c.enable_taint ? c.w_taint : 0;
    d.wna = c.enable_affinity ? c.w_affinity : 0;
    d.feat = feat_of(c);
    d.ba_skip_be = c.balanced_skip_besteffort ? 1u : 0u;
    return d;
}

// memory unit shift for the table (<= 20, the MiB granularity of every k8s "Mi"/"Gi" quantity)
int table_shift(const Mirror &m) {
    int s = 20;
    for (uint32_t i = 0; i < m.n; i++) {
        s = std::min(s, ctz64(m.am[i]));
        s = std::min(s, ctz64(m.rm[i]));
        s = std::min(s, ctz64(m.zm[i]));
    }
    return s;
}

// Nodes whose allocatable cpu or memory is 0 (qs_ctx::zero_alloc; DevCfg::all_alloc is set for a
// launch when there are none).  Kept wherever allocatable values enter the mirror: the load scans
// like table_shift, an upsert adjusts the count by its row, a restore recounts the snapshot's
// mirror.  Reservations and the kernels never change an allocatable column.  Every rank of a sharded
// context loads the whole table, so its count covers every rank's nodes.
bool zero_alloc_row(const Mirror &m, uint32_t i) { return m.ac[i] <= 0 || m.am[i] <= 0; }
uint32_t count_zero_alloc(const Mirror &m) {
    uint32_t z = 0;
    for (uint32_t i = 0; i < m.n; i++) z += zero_alloc_row(m, i) ? 1u : 0u;
    return z;
}

void check_range(int64_t v, const char *what, uint32_t i, int64_t limit = kLimit) {
    if (v < 0 || v > limit)
        fail(QS_EINVAL, std::string("node ") + std::to_string(i) + ": " + what + " = " + std::to_string(v) +
                            " outside the device range [0, " + std::to_string(limit) + "]");
}

// Value ranges every layout needs (cpu, counts and extended resources are int32 columns in both;
// memory is bounded by the wide layout's f64 exactness, kWideMemLimit).
void check_row_values(const Mirror &m, uint32_t i) {
    check_range(m.ac[i], "alloc_cpu", i);
    check_range(m.rc[i], "req_cpu", i);
    check_range(m.zc[i], "nz_cpu", i);
    check_range(m.np[i], "pods", i);
    check_range(m.mp[i], "max_pods", i);
    check_range(m.am[i], "alloc_mem", i, kWideMemLimit);
    check_range(m.rm[i], "req_mem", i, kWideMemLimit);
    check_range(m.zm[i], "nz_mem", i, kWideMemLimit);
    for (int k = 0; k < QS_MAX_EXT; k++) {
        check_range(m.ae[(size_t)i * QS_MAX_EXT + k], "alloc_ext", i);
        check_range(m.re[(size_t)i * QS_MAX_EXT + k], "req_ext", i);
    }
    if (m.zone[i] < 0 || m.zone[i] >= (int32_t)kMaxZones)
        fail(QS_EINVAL, "node " + std::to_string(i) + ": zone outside [0, 64)");
}

// Compact layout possible at this shift: every memory quantity is a multiple of 2^shift (true by
// construction of the shift) and below 2^24 units.
bool row_compact_ok(const Mirror &m, uint32_t i, int shift) {
    return (m.am[i] >> shift) <= kLimit && (m.rm[i] >> shift) <= kLimit && (m.zm[i] >> shift) <= kLimit;
}

HostRow compact_row(const Mirror &m, uint32_t i, int shift, bool wide) {
    HostRow r{};
    check_row_values(m, i);
    if (!wide && !row_compact_ok(m, i, shift))
        fail(QS_EINVAL, "node " + std::to_string(i) + ": memory outside the compact layout");  // cannot happen
    r.zone = m.zone[i];
    r.ac = (int32_t)m.ac[i];
    r.rc = (int32_t)m.rc[i];
    r.zc = (int32_t)m.zc[i];
    r.np = (int32_t)m.np[i];
    r.mp = (int32_t)m.mp[i];
    r.yc = r.ac ? 1.0 / (double)r.ac : 0.0;  // RN(1/alloc): IEEE division on the host
    if (wide) {
        r.wam = (double)m.am[i];
        r.wrm = (double)m.rm[i];
        r.wzm = (double)m.zm[i];
        r.ym = m.am[i] ? 1.0 / r.wam : 0.0;
    } else {
        r.am = (int32_t)(m.am[i] >> shift);
        r.rm = (int32_t)(m.rm[i] >> shift);
        r.zm = (int32_t)(m.zm[i] >> shift);
        r.ym = r.am ? 1.0 / (double)r.am : 0.0;
    }
    r.ae0 = (int32_t)m.ae[(size_t)i * QS_MAX_EXT + 0];
    r.ae1 = (int32_t)m.ae[(size_t)i * QS_MAX_EXT + 1];
    r.re0 = (int32_t)m.re[(size_t)i * QS_MAX_EXT + 0];
    r.re1 = (int32_t)m.re[(size_t)i * QS_MAX_EXT + 1];
    r.th = m.th[i];
    r.ts = m.ts[i];
    r.lb0 = m.lb[(size_t)i * 2];
    r.lb1 = m.lb[(size_t)i * 2 + 1];
    return r;
}

// Table layout inside ctx->tbl: cap rows (64 B compact, 80 B wide), cap mask rows of 32 B, cap zone
// ids, then (tables up to kAaMaxNodes) the anti-affinity state: kAppWords x cap app words and the
// (app, zone) counts.  Returns the size; assigns the pointers when base != nullptr.
size_t carve(DevTable &t, uint32_t cap, bool wide, char *base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    if (wide) {
        t.rows = nullptr;
        t.wrows = (DRowW *)take((size_t)cap * sizeof(DRowW));
    } else {
        t.wrows = nullptr;
        t.rows = (DRow *)take((size_t)cap * sizeof(DRow));
    }
    t.masks = (DMask *)take((size_t)cap * sizeof(DMask));
    t.zone = (int32_t *)take((size_t)cap * 4);
    t.cap = cap;
    if (cap <= kAaMaxNodes) {
        t.apps = (uint32_t *)take((size_t)kAppWords * cap * 4);
        // ... and behind the counts, in the same allocation (so qs_table_save / restore carry them), the
        // two rows of spec S13: the domain flags and the spread apps of the PERSISTENT stream in flight
        t.zcount = (int32_t *)take((size_t)(kMaxApps + kSpreadRows) * kMaxZones * 4);
    } else {
        t.apps = nullptr;
        t.zcount = nullptr;
    }
    return off;
}

DRow to_drow(const HostRow &r) {
    DRow d;
    d.ac = r.ac; d.am = r.am; d.rc = r.rc; d.rm = r.rm; d.zc = r.zc; d.zm = r.zm;
    d.np = r.np; d.mp = r.mp; d.yc = r.yc; d.ym = r.ym;
    d.ae0 = r.ae0; d.re0 = r.re0; d.ae1 = r.ae1; d.re1 = r.re1;
    return d;
}

uint32_t soa_min_nodes(const qs_ctx *c) {
    const int32_t v = c->cfg.scan_soa_min_nodes;
    return v == 0 ? kSoaMinNodes : (v < 0 ? 0xFFFFFFFFu : (uint32_t)v);
}

DRowW to_drow_wide(const HostRow &r) {
    DRowW d;
    d.ac = r.ac; d.rc = r.rc; d.zc = r.zc; d.np = r.np;
    d.am = r.wam; d.rm = r.wrm; d.zm = r.wzm; d.ym = r.ym;
    d.yc = r.yc; d.mp = r.mp; d.pad = 0;
    d.ae0 = r.ae0; d.re0 = r.re0; d.ae1 = r.ae1; d.re1 = r.re1;
    return d;
}

// LOGTAB of spec S14: entry D - 1 is the IEEE double nearest to ln(D + 2), D = 1..64 (the topology
// normalizing weight of UP podtopologyspread/scoring.go#topologyNormalizingWeight for D domains).
// tests/golden/soft_spread_logtab.json holds the same 64 values; tests/test_soft_spread_cpu.py checks
// them against an 80-digit evaluation.
const double kLogTab[kMaxZones] = {
    0x1.193ea7aad030bp+0, 0x1.62e42fefa39efp+0, 0x1.9c041f7ed8d33p+0, 0x1.cab0bfa2a2002p+0,
    0x1.f2272ae325a57p+0, 0x1.0a2b23f3bab73p+1, 0x1.193ea7aad030bp+1, 0x1.26bb1bbb55516p+1,
    0x1.32ee3b77f374cp+1, 0x1.3e116bcd39e7dp+1, 0x1.485042b318c51p+1, 0x1.51cca16d7bba7p+1,
    0x1.5aa16394d481fp+1, 0x1.62e42fefa39efp+1, 0x1.6aa6bc1fa7f7ap+1, 0x1.71f7b3a6b9186p+1,
    0x1.78e360604b32cp+1, 0x1.7f7427b73e391p+1, 0x1.85b2e946faeb1p+1, 0x1.8ba74773dc5c8p+1,
    0x1.9157dfdd1b3f0p+1, 0x1.96ca77c922cf9p+1, 0x1.9c041f7ed8d33p+1, 0x1.a1094eaf01acdp+1,
    0x1.a5ddfb8038490p+1, 0x1.aa85ad6964a23p+1, 0x1.af038cbcdfe1fp+1, 0x1.b35a6f90bd69bp+1,
    0x1.b78ce48912b5ap+1, 0x1.bb9d3beb8c86bp+1, 0x1.bf8d8f4d5b8d1p+1, 0x1.c35fc81b90df6p+1,
    0x1.c715a530ff3c5p+1, 0x1.cab0bfa2a2002p+1, 0x1.ce328ee3ac7bdp+1, 0x1.d19c6c5c341a8p+1,
    0x1.d4ef968880dd6p+1, 0x1.d82d33b32720dp+1, 0x1.db565458eac4ep+1, 0x1.de6bf542e3d2dp+1,
    0x1.e16f01614ec11p+1, 0x1.e460536fc5443p+1, 0x1.e740b76a3c9a4p+1, 0x1.ea10ebd90426cp+1,
    0x1.ecd1a2f90f0b6p+1, 0x1.ef8383c50bb75p+1, 0x1.f2272ae325a57p+1, 0x1.f4bd2b7ac1bafp+1,
    0x1.f7460ff5100ffp+1, 0x1.f9c25aaaea949p+1, 0x1.fc32868223cabp+1, 0x1.fe97077c2130cp+1,
    0x1.0078259bafef3p+2, 0x1.019f5cb2a6c50p+2, 0x1.02c15a1ad9a59p+2, 0x1.03de4c5c6464dp+2,
    0x1.04f65f9c72979p+2, 0x1.0609bdc65328bp+2, 0x1.07188eb126c0dp+2, 0x1.0822f8427dcebp+2,
    0x1.09291e8e3181bp+2, 0x1.0a2b23f3bab73p+2, 0x1.0b29293942975p+2, 0x1.0c234da4a23a6p+2,
};

// The three rows of spec S14 behind the spread apps: LOGTAB and the plugin weight, as they go into
// `rows` (3 * kMaxZones words).
void fill_spread_cfg(const qs_ctx *c, int32_t *rows) {
    static_assert(sizeof kLogTab == 2 * kMaxZones * 4 && kSpreadRows == 5, "LOGTAB fills two rows, the weight a third");
    std::memset(rows, 0, 3 * kMaxZones * 4);
    std::memcpy(rows, kLogTab, sizeof kLogTab);
    rows[2 * kMaxZones] = c->w_pts;
    // words 2-3 of the weight's row: the address of the (app, node) counts of spec S15, null while the
    // context keeps none (aa_hcount in qs_kernels.hpp reads it)
    const uint64_t hp = (uint64_t)(uintptr_t)c->hcount.p;
    std::memcpy(rows + 2 * kMaxZones + 2, &hp, 8);
    // words 16-31: the hostname-spread apps of the PERSISTENT stream in flight (none: a stream writes its own)
    static_assert(kHostSpreadApps == 16, "one quarter row");
    for (uint32_t j = 0; j < kHostSpreadApps; j++) rows[2 * kMaxZones + 16 + j] = -1;
}
// ... written alone by qs_set_topology_spread_weight and after qs_table_restore (whose snapshot holds
// the weight of its save); every table upload writes them with the domain flags (write_domains).
void write_spread_cfg(qs_ctx *c) {
    if (!c->dt.zcount) return;
    int32_t rows[3 * kMaxZones];
    fill_spread_cfg(c, rows);
    HIPCHK(hipMemcpyAsync(c->dt.zcount + (size_t)(kMaxApps + 2) * kMaxZones, rows, sizeof rows, hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (rows lives on this stack)
}

// The rows behind the (app, zone) counts in one copy: the two of spec S13, the domain flags from the
// mirror's zone column and an empty spread-app list (a PERSISTENT stream writes its own before it
// launches), and the three of spec S14.
void write_domains(qs_ctx *c) {
    if (!c->dt.zcount) return;
    int32_t rows[kSpreadRows * kMaxZones];
    const uint64_t dom = c->m.domains();
    for (uint32_t z = 0; z < kMaxZones; z++) {
        rows[z] = (int32_t)((dom >> z) & 1u);
        rows[kMaxZones + z] = -1;
    }
    fill_spread_cfg(c, rows + 2 * kMaxZones);
    HIPCHK(hipMemcpyAsync(c->dt.zcount + (size_t)kMaxApps * kMaxZones, rows, sizeof rows, hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (rows lives on this stack)
}

// Hostname topology spread (spec S15): the device's uint16 pods per (app, node), 2 KB per node.
constexpr uint32_t kHcMaxNodes = 1u << 19;  // 1 GiB
constexpr int64_t kHcMaxPods = 65535;
// The sparse mirror map as the dense array's non-zero cells (no HIP call): cell app * cap + node.
void hc_cells(const Mirror &m, uint32_t cap, std::vector<uint32_t> &idx, std::vector<uint16_t> &val) {
    idx.clear();
    val.clear();
    for (const auto &e : m.aa_node) {
        const uint32_t app = (uint32_t)(e.first >> 32), node = (uint32_t)e.first;
        if (app >= kMaxApps || node >= m.n || node >= cap || e.second <= 0) continue;
        idx.push_back(app * cap + node);
        val.push_back((uint16_t)std::min<int64_t>(e.second, kHcMaxPods));
    }
}
// A table upload (load, re-layout, append, rebuild after a fault): the array follows the table's
// capacity and is stale; a table it cannot cover drops it (the next such pod is refused).
void hc_on_upload(qs_ctx *c) {
    c->hc_valid = false;
    if (!c->hcount.p) return;
    if (!c->dt.apps || c->cap > kHcMaxNodes) {
        (void)hipFree(c->hcount.p);
        c->hcount.p = nullptr;
        c->hcount.bytes = 0;
        return;
    }
    c->hcount.ensure((size_t)kMaxApps * c->cap * 2);
}
// Before every launch that reads the counts: allocate on first use, rebuild from the mirror when stale.
void ensure_hcount(qs_ctx *c) {
    aa_check_table(c);
    if (c->hcount.p && c->hc_valid) return;
    if (c->cap > kHcMaxNodes)
        fail(QS_EINVAL, "QS_AA_SPREAD_HOSTNAME (and a restricting spread pod under nodeAffinityPolicy / nodeTaintsPolicy Honor) keeps "
                        "2 KB of counts per node: tables up to 2^19 nodes");
    for (uint32_t i = 0; i < c->m.n; i++)
        if (c->m.mp[i] > kHcMaxPods)
            fail(QS_EINVAL, "QS_AA_SPREAD_HOSTNAME (and nodeAffinityPolicy / nodeTaintsPolicy Honor) counts pods per node in 16 bits: node " + std::to_string(i) +
                                " has max_pods above 65535");
    const size_t cells = (size_t)kMaxApps * c->cap;
    const void *before = c->hcount.p;
    c->hcount.ensure(cells * 2);
    HIPCHK(hipMemsetAsync(c->hcount.p, 0, cells * 2, c->stream));
    std::vector<uint32_t> idx;
    std::vector<uint16_t> val;
    hc_cells(c->m, c->cap, idx, val);
    if (!idx.empty()) {
        const uint32_t m = (uint32_t)idx.size();
        c->hc_idx.ensure((size_t)m * 4);
        c->hc_val.ensure((size_t)m * 2);
        HIPCHK(hipMemcpyAsync(c->hc_idx.p, idx.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->hc_val.p, val.data(), (size_t)m * 2, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_hc_scatter, dim3((m + 255) / 256), dim3(256), 0, c->stream, c->hcount.as<uint16_t>(),
                           c->hc_idx.as<uint32_t>(), c->hc_val.as<uint16_t>(), m, (uint32_t)cells);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(c->stream));  // (idx / val live on this stack)
    if (c->hcount.p != before) write_spread_cfg(c);  // the kernels find the array through the weight's row
    c->hc_valid = true;
}

// Upload the whole mirror to the device in the context's layout (c->wide, c->shift).
void upload_table(qs_ctx *c) {
    const uint32_t n = c->m.n;
    const uint32_t cap = std::max<uint32_t>(64, (n + 63) & ~63u);
    const bool wide = c->wide;
    const size_t need = carve(c->dt, cap, wide, nullptr);
    if (cap > c->cap || !c->tbl.p || need > c->tbl.bytes) {
        c->tbl.ensure(need);
        c->cap = std::max(cap, c->cap);
    }
    carve(c->dt, c->cap, wide, c->tbl.as<char>());
    c->dt.n = n;
    const bool soa = !wide && n > 0 && n >= soa_min_nodes(c);
    std::memset(&c->dt.soa, 0, sizeof c->dt.soa);
    std::vector<DRow> rows(wide ? 0 : n);
    std::vector<DRowW> wrows(wide ? n : 0);
    std::vector<DMask> masks(n);
    std::vector<int32_t> cols(soa ? (size_t)kSCols * c->cap : 0, 0);  // zero padding: infeasible
    for (uint32_t i = 0; i < n; i++) {
        const HostRow r = compact_row(c->m, i, c->shift, wide);
        if (wide) wrows[i] = to_drow_wide(r);
        else rows[i] = to_drow(r);
        masks[i] = DMask{r.th, r.ts, r.lb0, r.lb1};
        if (soa) {
            const int32_t f[kSCols] = {r.ac, r.am, r.rc, r.rm, r.zc, r.zm, r.np, r.mp, r.ae0, r.re0, r.ae1, r.re1};
            for (int k = 0; k < kSCols; k++) cols[(size_t)k * c->cap + i] = f[k];
        }
    }
    if (n) {
        if (wide) HIPCHK(hipMemcpyAsync(c->dt.wrows, wrows.data(), n * sizeof(DRowW), hipMemcpyHostToDevice, c->stream));
        else HIPCHK(hipMemcpyAsync(c->dt.rows, rows.data(), n * sizeof(DRow), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->dt.masks, masks.data(), n * sizeof(DMask), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->dt.zone, c->m.zone.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    }
    // a (re)loaded table starts with no pods recorded; what the mirror of a context that tracks pod
    // anti-affinity holds (spec S12) is rebuilt: a re-layout, or the recovery after a device fault
    std::vector<uint32_t> aw;
    hc_on_upload(c);  // (before write_domains, whose rows carry the array's address)
    if (c->dt.apps) {
        const bool rebuild = !c->m.aa_node.empty();
        if (rebuild) {
            aw.assign((size_t)kAppWords * c->cap, 0u);
            for (const auto &e : c->m.aa_node) {
                const uint32_t app = (uint32_t)(e.first >> 32), node = (uint32_t)e.first;
                if (node < n) aw[(size_t)(app >> 5) * c->cap + node] |= 1u << (app & 31u);
            }
            HIPCHK(hipMemcpyAsync(c->dt.apps, aw.data(), aw.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(c->dt.zcount, c->m.aa_zone.data(), (size_t)kMaxApps * kMaxZones * 4,
                                  hipMemcpyHostToDevice, c->stream));
        } else {
            HIPCHK(hipMemsetAsync(c->dt.apps, 0, (size_t)kAppWords * c->cap * 4, c->stream));
            HIPCHK(hipMemsetAsync(c->dt.zcount, 0, (size_t)kMaxApps * kMaxZones * 4, c->stream));
        }
        write_domains(c);
    }
    if (soa) {
        c->soa.ensure(cols.size() * 4);
        for (int k = 0; k < kSCols; k++) c->dt.soa.c[k] = c->soa.as<int32_t>() + (size_t)k * c->cap;
        HIPCHK(hipMemcpyAsync(c->soa.p, cols.data(), cols.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->reg_all = true;  // the registry's device copy is rebuilt with the table (spec S18)
    c->dev_valid = true;
    c->soa_valid = soa;
    c->mirror_stale = false;
}

// The SCAN engine reads the SoA copy: rebuild it after engines that only update the rows.
void ensure_soa(qs_ctx *c) {
    if (!c->dt.soa.c[0] || c->soa_valid) return;
    HIPCHK(launch_rows_to_soa(c->dt, c->stream));
    c->soa_valid = true;
}

void push_row(qs_ctx *c, uint32_t i, bool sync = true) {
    if (!c->dev_valid) return;
    const HostRow r = compact_row(c->m, i, c->shift, c->wide);
    hipLaunchKernelGGL(k_set_row, dim3(1), dim3(1), 0, c->stream, c->dt, i, r,
                       kFeatExt | kFeatTaint | kFeatAffinity);
    HIPCHK(hipGetLastError());
    if (sync) HIPCHK(hipStreamSynchronize(c->stream));
}

void flush_pending(qs_ctx *c) {
    if (c->pend == 0xFFFFFFFFu) return;
    const uint32_t i = c->pend;
    c->pend = 0xFFFFFFFFu;
    if (c->dev_valid && i < c->m.n) push_row(c, i, /*sync=*/false);
}

// Refresh the dynamic mirror columns from the device after stream runs (compact values are
// multiples of 2^shift by construction and wide values are exact f64 integers, so decoding is exact).
void sync_mirror(qs_ctx *c) {
    if (!c->mirror_stale || !c->dev_valid) return;
    const uint32_t n = c->m.n;
    Mirror &m = c->m;
    if (c->wide) {
        std::vector<DRowW> rows(n);
        if (n) HIPCHK(hipMemcpyAsync(rows.data(), c->dt.wrows, n * sizeof(DRowW), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (uint32_t i = 0; i < n; i++) {
            m.rc[i] = rows[i].rc;
            m.rm[i] = (int64_t)rows[i].rm;
            m.zc[i] = rows[i].zc;
            m.zm[i] = (int64_t)rows[i].zm;
            m.np[i] = rows[i].np;
            m.re[(size_t)i * QS_MAX_EXT] = rows[i].re0;
            m.re[(size_t)i * QS_MAX_EXT + 1] = rows[i].re1;
        }
    } else {
        std::vector<DRow> rows(n);
        if (n) HIPCHK(hipMemcpyAsync(rows.data(), c->dt.rows, n * sizeof(DRow), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (uint32_t i = 0; i < n; i++) {
            m.rc[i] = rows[i].rc;
            m.rm[i] = (int64_t)rows[i].rm << c->shift;
            m.zc[i] = rows[i].zc;
            m.zm[i] = (int64_t)rows[i].zm << c->shift;
            m.np[i] = rows[i].np;
            m.re[(size_t)i * QS_MAX_EXT] = rows[i].re0;
            m.re[(size_t)i * QS_MAX_EXT + 1] = rows[i].re1;
        }
    }
    c->mirror_stale = false;
}

int pod_min_shift(const qs_pod &p) { return std::min(ctz64(p.req_mem), ctz64(p.nz_mem)); }

void check_pod(const qs_pod &p, uint32_t j) {
    auto bad = [&](const char *w) {
        fail(QS_EINVAL, std::string("pod ") + std::to_string(j) + ": " + w);
    };
    if (p.qos < 0 || p.qos > 2) bad("qos must be 0..2");
    if (p.req_cpu < 0 || p.req_mem < 0 || p.nz_cpu < 0 || p.nz_mem < 0) bad("negative request");
    for (int k = 0; k < QS_MAX_EXT; k++)
        if (p.req_ext[k] < 0 || p.req_ext[k] > kLimit) bad("req_ext out of range");
    if (p.req_cpu > kLimit || p.nz_cpu > kLimit) bad("cpu request out of range");
    if (p.req_mem > kWideMemLimit || p.nz_mem > kWideMemLimit) bad("memory request above 2^46 bytes");
    if (p.n_req_terms < 0 || p.n_req_terms > QS_MAX_TERMS || p.n_pref_terms < 0 ||
        p.n_pref_terms > QS_MAX_TERMS)
        bad("term count out of range");
    for (int t = 0; t < p.n_pref_terms; t++)
        if (p.pref_weight[t] < 0 || p.pref_weight[t] > 100) bad("preferred term weight must be 0..100");
    if (p.app < 0 || p.app >= QS_MAX_APPS) bad("app outside [0, QS_MAX_APPS)");
    // one kind per pod in the low byte; QS_AA_SPREAD_ZONE carries max_skew in bits 8-12 (spec S13)
    const int32_t kind = QS_AA_KIND(p.anti_affinity);
    if (p.anti_affinity < 0 || kind > QS_AA_SPREAD_ZONE) bad("anti_affinity kind must be 0..3");
    if (kind == QS_AA_SPREAD_ZONE) {
        // ... and QS_AA_SOFT (spec S14) or QS_AA_HOSTKEY (spec S15) above it, the only bits above max_skew
        const int32_t skew = (p.anti_affinity & ~(QS_AA_SOFT | QS_AA_HOSTKEY)) >> 8;
        if (skew < 1 || skew > QS_MAX_SPREAD_SKEW) bad("anti_affinity: max_skew of QS_AA_SPREAD must be 1..31");
        if (QS_AA_IS_SOFT(p.anti_affinity) && QS_AA_IS_HOSTKEY(p.anti_affinity))
            bad("anti_affinity: QS_AA_SOFT and QS_AA_HOSTKEY exclude each other (no ScheduleAnyway form of the "
                "hostname spread)");
    } else if (p.anti_affinity != kind) {
        bad("anti_affinity: bits above the kind must be zero (only QS_AA_SPREAD carries max_skew, QS_AA_SOFT and "
            "QS_AA_HOSTKEY)");
    }
}
// (a soft-spread pod too, spec S14: k_persistent needs its app's counts like a SPREAD pod's)
bool pod_spreads(const qs_pod &p) { return QS_AA_KIND(p.anti_affinity) == QS_AA_SPREAD_ZONE; }
bool pod_soft_spread(const qs_pod &p) { return pod_spreads(p) && QS_AA_IS_SOFT(p.anti_affinity); }
// (spec S15: kind 3 on the host, so pod_spreads() holds and batched mode refuses it; its counts are per
// node, so it takes no slot among the zone-spread apps)
bool pod_host_spread(const qs_pod &p) { return pod_spreads(p) && QS_AA_IS_HOSTKEY(p.anti_affinity); }

// NodeAffinity disabled (config.enable_affinity = 0): the pod's required / preferred term counts are
// recorded as 0, so the normalizing kernels (which evaluate both plugins) neither filter nor score
// by affinity.  Bits 2-3: the strategy of the pod's QoS class (qs_scoring_strategy_type), which only
// the kFeatStrat scorer reads (check_pod has bounded qos to 0..2).  Bits 12-13: the anti-affinity kind;
// bits 26-30: max_skew of a QS_AA_SPREAD pod (0 for every other kind; spec S13, read by the kFeatAA
// kernels only).  Bit 31 stays the batched claim's.  A QS_AA_SPREAD_SOFT pod (spec S14) carries kind 0,
// so that no filter knows it, bit 14, and its max_skew; a QS_AA_SPREAD_HOSTNAME pod (spec S15) likewise
// kind 0, bit 15, and its max_skew.  Bit 11: a spread pod of any kind that restricts under
// nodeAffinityPolicy Honor (spec S16; pod_honors below), read by the kFeatAA kernels of the normalizing
// classes only.  Bit 7: a spread pod of any kind that restricts by taints under nodeTaintsPolicy Honor
// (spec S17; pod_honors_taints below), read by the same kernels.  (The score path's launcher marks its
// passes in bits 7 and 31 of its own copy; in the classes that read bit 7 of the record, in bit 31 alone.)
// A pod restricts when it has a nodeSelector or required node-affinity terms (spec S16); the policy is
// HONOR only on a context whose NodeAffinity filter is on, so M(pod) is what that filter admits.  It is
// read on a context that tracks only (tracking cannot change while prepared streams exist), so the
// records of every other context are what they were.
bool pod_honors_affinity(const qs_ctx *c, const qs_pod &p) {
    return c->aa_track && c->spread_policy == QS_POLICY_HONOR && c->cfg.enable_affinity && pod_spreads(p) &&
           ((p.sel[0] | p.sel[1]) != 0 || p.n_req_terms > 0);
}
// A pod restricts by taints when some hard taint bit is not tolerated: ~tol_hard != 0 (spec S17).  That
// is a property of the pod alone: M_T may still be every node of the table as it stands (no node carries
// such a bit), and the kernels then count what S13-S16 count, but no qs_node_upsert between prepare and
// run can leave a record that says otherwise.  HONOR only on a context whose TaintToleration filter is on.
bool pod_honors_taints(const qs_ctx *c, const qs_pod &p) {
    return c->aa_track && c->taints_policy == QS_POLICY_HONOR && c->cfg.enable_taint && pod_spreads(p) &&
           ~p.tol_hard != 0;
}
// ... by either predicate: what every host-side rule of S16 hangs on
bool pod_honors(const qs_ctx *c, const qs_pod &p) { return pod_honors_affinity(c, p) || pod_honors_taints(c, p); }
uint32_t pod_flags(const qs_ctx *c, const qs_pod &p) {
    const uint32_t aff = c->cfg.enable_affinity ? 1u : 0u;
    const bool soft = pod_soft_spread(p), host = pod_host_spread(p);
    return (uint32_t)p.qos | ((uint32_t)c->strat[p.qos].type << 2) | (aff * (uint32_t)p.n_req_terms << 4) |
           ((pod_honors_taints(c, p) ? 1u : 0u) << 7) | (aff * (uint32_t)p.n_pref_terms << 8) |
           ((pod_honors_affinity(c, p) ? 1u : 0u) << 11) |
           ((soft || host ? 0u : (uint32_t)QS_AA_KIND(p.anti_affinity)) << 12) | ((soft ? 1u : 0u) << 14) |
           ((host ? 1u : 0u) << 15) | ((uint32_t)p.app << 16) | ((uint32_t)QS_AA_MAX_SKEW(p.anti_affinity) << 26);
}

// Device pod record in the context's layout: DPod (compact, memory in 2^shift units) or DPodW
// (wide, memory in f64 bytes).  ensure_layout has already checked the ranges.
size_t pod_record_bytes(bool wide) { return wide ? sizeof(DPodW) : sizeof(DPod); }

void compact_pod(const qs_ctx *c, const qs_pod &p, uint32_t j, int shift, bool wide, void *dst) {
    check_pod(p, j);
    if (wide) {
        DPodW d{};
        d.rc = (int32_t)p.req_cpu;
        d.zc = (int32_t)p.nz_cpu;
        d.rm = (double)p.req_mem;
        d.zm = (double)p.nz_mem;
        d.re0 = (int32_t)p.req_ext[0];
        d.re1 = (int32_t)p.req_ext[1];
        d.wfit = (uint16_t)c->cfg.w_fit[p.qos];
        d.wbal = (uint16_t)c->cfg.w_bal[p.qos];
        d.flags = pod_flags(c, p);
        std::memcpy(dst, &d, sizeof d);
        return;
    }
    if ((p.req_mem >> shift) > kLimit || (p.nz_mem >> shift) > kLimit)
        fail(QS_EINVAL, "pod " + std::to_string(j) + ": memory request out of the compact range");  // cannot happen
    DPod d{};
    d.rc = (int32_t)p.req_cpu;
    d.rm = (int32_t)(p.req_mem >> shift);
    d.zc = (int32_t)p.nz_cpu;
    d.zm = (int32_t)(p.nz_mem >> shift);
    d.re0 = (int32_t)p.req_ext[0];
    d.re1 = (int32_t)p.req_ext[1];
    d.wfit = (uint16_t)c->cfg.w_fit[p.qos];
    d.wbal = (uint16_t)c->cfg.w_bal[p.qos];
    d.flags = pod_flags(c, p);
    std::memcpy(dst, &d, sizeof d);
}

// A disabled plugin's part of the record is neutral: TaintToleration off -> every taint tolerated
// (Filter passes, raw score 0); NodeAffinity off -> no nodeSelector (the term counts are 0 in the
// pod flags).
DPodX compact_podx(const qs_ctx *c, const qs_pod &p) {
    DPodX x{};
    const bool taint = c->cfg.enable_taint != 0, aff = c->cfg.enable_affinity != 0;
    x.tol_hard = taint ? p.tol_hard : ~0ull;
    x.tol_soft = taint ? p.tol_soft : ~0ull;
    x.sel0 = aff ? p.sel[0] : 0ull;
    x.sel1 = aff ? p.sel[1] : 0ull;
    for (int t = 0; t < QS_MAX_TERMS; t++) {
        x.req[t][0] = p.req_terms[t][0];
        x.req[t][1] = p.req_terms[t][1];
        x.pref[t][0] = p.pref_terms[t][0];
        x.pref[t][1] = p.pref_terms[t][1];
        x.pw[t] = p.pref_weight[t];
    }
    return x;
}

// spec S8 QoSSort: stable by (qos desc, priority desc, arrival asc)
std::vector<uint32_t> qos_order(const qs_pod *pods, uint32_t p, bool sort) {
    std::vector<uint32_t> o(p);
    for (uint32_t j = 0; j < p; j++) o[j] = j;
    if (sort)
        std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) {
            if (pods[a].qos != pods[b].qos) return pods[a].qos > pods[b].qos;
            return pods[a].priority > pods[b].priority;
        });
    return o;
}

void mirror_reserve(Mirror &m, uint32_t i, const qs_pod &p, int sign) {
    m.rc[i] += sign * p.req_cpu;
    m.rm[i] += sign * p.req_mem;
    for (int k = 0; k < QS_MAX_EXT; k++) m.re[(size_t)i * QS_MAX_EXT + k] += sign * p.req_ext[k];
    m.zc[i] += sign * p.nz_cpu;
    m.zm[i] += sign * p.nz_mem;
    m.np[i] += sign;
}

// ---- pod registry (spec S18) ------------------------------------------------------
// Importance of a pod under the context's policy, as an unsigned 64-bit value.
uint64_t reg_importance(int32_t policy, int32_t qos, int32_t priority) {
    const uint64_t base = (uint64_t)((int64_t)priority + (1LL << 31));
    return policy == QS_PREEMPT_BY_QOS ? ((uint64_t)(uint32_t)qos << 32) + base : base;
}
bool reg_more_important(const RegEntry &a, const RegEntry &b) {  // UP util.MoreImportantPod
    return a.imp != b.imp ? a.imp > b.imp : a.seq < b.seq;
}
// The device copy of node's list is stale.
void reg_touch(qs_ctx *c, uint32_t node) {
    if (c->reg_all) return;
    if (c->reg_mark.size() < c->m.n) c->reg_mark.resize(c->m.n, 0);
    if (node < c->reg_mark.size() && !c->reg_mark[node]) {
        c->reg_mark[node] = 1;
        c->reg_dirty.push_back(node);
    }
}
// ... of every node is (and the count of over-long lists is taken again)
void reg_stale(qs_ctx *c) {
    c->reg_all = true;
    c->reg_dirty.clear();
    c->reg_mark.clear();
    c->reg_long = 0;
    for (const auto &l : c->m.reg) c->reg_long += l.size() > QS_MAX_VICTIMS ? 1u : 0u;
}
// Every entry's importance under the context's policy and every list in its walk order again.
void reg_resort(qs_ctx *c) {
    for (auto &l : c->m.reg) {
        for (RegEntry &e : l) e.imp = reg_importance(c->preempt_policy, e.qos, e.priority);
        std::sort(l.begin(), l.end(), reg_more_important);
    }
    reg_stale(c);
}
std::vector<RegEntry> &reg_list(qs_ctx *c, uint32_t node) {
    if (c->m.reg.size() < c->m.n) c->m.reg.resize(c->m.n);
    return c->m.reg[node];
}
bool reg_holds(const qs_ctx *c, uint32_t node) { return node < c->m.reg.size() && !c->m.reg[node].empty(); }
void reg_append(qs_ctx *c, uint32_t node, const qs_pod &p) {
    auto &l = reg_list(c, node);
    RegEntry e{reg_importance(c->preempt_policy, p.qos, p.priority), ++c->m.reg_seq, p.req_cpu, p.req_mem, {},
               p.nz_cpu, p.nz_mem, p.priority, p.qos, p.app};
    for (int k = 0; k < QS_MAX_EXT; k++) e.re[k] = p.req_ext[k];
    // behind every entry at least as important (the new entry carries the highest seq)
    const auto it = std::upper_bound(l.begin(), l.end(), e, [](const RegEntry &a, const RegEntry &b) { return a.imp > b.imp; });
    l.insert(it, e);
    if (l.size() == (size_t)QS_MAX_VICTIMS + 1) ++c->reg_long;
    reg_touch(c, node);
}
void reg_erase(qs_ctx *c, uint32_t node, size_t at) {
    auto &l = reg_list(c, node);
    if (l.size() == (size_t)QS_MAX_VICTIMS + 1) --c->reg_long;
    l.erase(l.begin() + (ptrdiff_t)at);
    reg_touch(c, node);
}
// The entry of `node` with the highest seq whose fields equal the pod's (qs_unreserve), or the entry `seq`
// (qs_evict, seq != 0); -1: none.
ptrdiff_t reg_find(const qs_ctx *c, uint32_t node, const qs_pod *p, uint64_t seq) {
    if (node >= c->m.reg.size()) return -1;
    const auto &l = c->m.reg[node];
    ptrdiff_t at = -1;
    for (size_t k = 0; k < l.size(); k++) {
        const RegEntry &e = l[k];
        if (seq != 0) {
            if (e.seq == seq) return (ptrdiff_t)k;
            continue;
        }
        if (e.priority == p->priority && e.qos == p->qos && e.app == p->app && e.rc == p->req_cpu && e.rm == p->req_mem &&
            e.re[0] == p->req_ext[0] && e.re[1] == p->req_ext[1] && e.zc == p->nz_cpu && e.zm == p->nz_mem &&
            (at < 0 || e.seq > l[(size_t)at].seq))
            at = (ptrdiff_t)k;
    }
    return at;
}
qs_victim reg_victim(const RegEntry &e) {
    qs_victim v{};
    v.seq = e.seq;
    v.req_cpu = e.rc; v.req_mem = e.rm; v.nz_cpu = e.zc; v.nz_mem = e.zm;
    for (int k = 0; k < QS_MAX_EXT; k++) v.req_ext[k] = e.re[k];
    v.priority = e.priority; v.qos = e.qos; v.app = e.app;
    return v;
}
// A qs_node_upsert of a node that holds entries: the row may not claim less than they add up to.
void reg_check_row(const qs_ctx *c, uint32_t node, const qs_node_row &r) {
    int64_t rc = 0, rm = 0, zc = 0, zm = 0, re[QS_MAX_EXT] = {};
    const auto &l = c->m.reg[node];
    for (const RegEntry &e : l) {
        rc += e.rc; rm += e.rm; zc += e.zc; zm += e.zm;
        for (int k = 0; k < QS_MAX_EXT; k++) re[k] += e.re[k];
    }
    bool ok = r.req_cpu >= rc && r.req_mem >= rm && r.nz_cpu >= zc && r.nz_mem >= zm && r.pods >= (int64_t)l.size();
    for (int k = 0; k < QS_MAX_EXT; k++) ok = ok && r.req_ext[k] >= re[k];
    if (!ok)
        fail(QS_EINVAL, "node " + std::to_string(node) + ": the row's requested columns or pod count fall below the "
                        "sums over its " + std::to_string(l.size()) + " registered pods (spec S18)");
}
// The device copy brought up to date: the dirty nodes' columns through one staging copy and one scatter
// launch, or every node's after reg_stale / a reallocation.  slots = the longest list rounded up to a
// power of two, 8..QS_MAX_VICTIMS; growth reallocates.
void reg_sync_device(qs_ctx *c) {
    const uint32_t n = c->m.n, cap = c->cap;
    if (c->m.reg.size() < n) c->m.reg.resize(n);
    if (cap != c->reg_cap || !c->reg_dev.p) c->reg_all = true;
    // few dirty nodes: their columns; many: the whole copy (one pass, no marks to keep)
    if (!c->reg_all && (size_t)c->reg_dirty.size() * 4 > n) reg_stale(c);
    size_t longest = 0;
    if (c->reg_all) for (uint32_t i = 0; i < n; i++) longest = std::max(longest, c->m.reg[i].size());
    else for (uint32_t i : c->reg_dirty) if (i < n) longest = std::max(longest, c->m.reg[i].size());
    uint32_t slots = 8;
    while (slots < longest && slots < QS_MAX_VICTIMS) slots <<= 1;
    // growth: a new extent, every node again (no other list is longer than the old extent, so `slots` stands)
    if (!c->reg_all && slots > c->reg_slots) c->reg_all = true;
    if (c->reg_all) {
        c->reg_dev.ensure((size_t)kRegCols * slots * cap * 8 + (size_t)cap * 4);
        c->reg_slots = slots;
        c->reg_cap = cap;
        c->reg_dirty.clear();
        c->reg_mark.clear();
    }
    uint64_t *col = c->reg_dev.as<uint64_t>();
    uint32_t *len = reinterpret_cast<uint32_t *>(col + (size_t)kRegCols * c->reg_slots * cap);
    std::vector<RegItem> items;
    std::vector<uint32_t> lnode, lval;
    auto add = [&](uint32_t i) {
        const auto &l = c->m.reg[i];
        lnode.push_back(i);
        lval.push_back((uint32_t)std::min<size_t>(l.size(), c->reg_slots));
        for (uint32_t s = 0; s < l.size() && s < c->reg_slots; s++) {
            const RegEntry &e = l[s];
            items.push_back(RegItem{i, s, {e.imp, e.seq, (uint64_t)e.rc, (uint64_t)e.rm, (uint64_t)e.re[0], (uint64_t)e.re[1]}});
        }
    };
    if (c->reg_all) {
        if (cap) HIPCHK(hipMemsetAsync(len, 0, (size_t)cap * 4, c->stream));
        for (uint32_t i = 0; i < n; i++) if (!c->m.reg[i].empty()) add(i);
    } else {
        for (uint32_t i : c->reg_dirty) if (i < n) add(i);
    }
    if (!lnode.empty()) {
        const size_t ib = items.size() * sizeof(RegItem), lb = lnode.size() * 4;
        c->reg_stage.ensure(ib + 2 * lb + 16);
        char *st = c->reg_stage.as<char>();
        if (ib) HIPCHK(hipMemcpyAsync(st, items.data(), ib, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(st + ib, lnode.data(), lb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(st + ib + lb, lval.data(), lb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_preempt_scatter(col, len, c->reg_slots, cap, reinterpret_cast<const RegItem *>(st),
                                      (uint32_t)items.size(), reinterpret_cast<const uint32_t *>(st + ib),
                                      reinterpret_cast<const uint32_t *>(st + ib + lb), (uint32_t)lnode.size(), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));  // (the staging vectors leave scope)
    }
    for (uint32_t i : c->reg_dirty) if (i < c->reg_mark.size()) c->reg_mark[i] = 0;
    c->reg_dirty.clear();
    c->reg_all = false;
}

// Device layout for the mirror plus the pods about to be scored (spec S10):
//  * compact: every memory quantity of the table and the pods is a multiple of 2^shift bytes and
//    below 2^24 units, and no NonZeroRequested memory column can pass 2^31 units while the pods
//    are placed;
//  * wide otherwise (f64 memory columns in bytes: odd-Ki allocatable, decimal requests, ...).
// The layout only gets finer (smaller shift, compact -> wide) until the next qs_nodes_load.  Cpu
// columns are int32 in both layouts: a stream whose NonZeroRequested cpu could pass 2^31 m, or wide
// memory past 2^53 bytes, is rejected up front.  Re-uploads the table when the layout changes.
void ensure_layout(qs_ctx *c, const qs_pod *pods, uint32_t p, int extra_shift = 64) {
    const Mirror &m = c->m;
    int want = std::min(c->shift, extra_shift);
    int64_t mem_max = 0, nzm = 0, nzc = 0;
    for (uint32_t j = 0; j < p; j++) {
        want = std::min(want, pod_min_shift(pods[j]));
        mem_max = std::max({mem_max, pods[j].req_mem, pods[j].nz_mem});
        nzm = std::max(nzm, pods[j].nz_mem);
        nzc = std::max(nzc, pods[j].nz_cpu);
    }
    want = std::max(0, want);
    bool wide = c->wide;
    for (uint32_t i = 0; i < m.n; i++) {
        // pods this node can still take (+1: the evaluation of one more before Fit rejects it).
        // The resident resolver's uniform-window ladders (la_resolve4_stream) score up to kResUniR
        // pods past that point; those rungs may wrap, and are never read: the first infeasible rung
        // of a ladder is 0 and no rung behind it is ever reached.
        const __int128 more = (__int128)std::max<int64_t>(0, m.mp[i] - m.np[i]) + 1;
        if ((__int128)m.zc[i] + more * nzc > kGrowLimit32)
            fail(QS_EINVAL, "node " + std::to_string(i) + ": NonZeroRequested cpu could pass 2^31 m during the stream");
        if (!wide && (!row_compact_ok(m, i, want) ||
                      (__int128)(m.zm[i] >> want) + more * (nzm >> want) > kGrowLimit32))
            wide = true;
        if (wide && (__int128)m.zm[i] + more * nzm > kGrowLimitF64)
            fail(QS_EINVAL, "node " + std::to_string(i) + ": NonZeroRequested memory could pass 2^53 B during the stream");
    }
    if (!wide && (mem_max >> want) > kLimit) wide = true;
    if (wide != c->wide || (!wide && want < c->shift)) {
        sync_mirror(c);  // the device table is re-laid out from the mirror
        c->wide = wide;
        if (!wide) c->shift = want;
        c->dev_valid = false;
        c->saved = false;  // a snapshot of the old layout cannot be restored into the new one
    }
    if (!c->dev_valid) upload_table(c);
}

// The pod fits the device layout as it stands (spec S10), so scoring / reserving it needs no
// re-layout and no pass over the table: its memory quantities are multiples of the table's unit and
// below the compact range (or the table is wide).  Otherwise ensure_layout decides.
bool pod_fits_layout(const qs_ctx *c, const qs_pod &p) {
    if (!c->dev_valid) return false;
    if (c->wide) return true;  // check_pod bounded memory by kWideMemLimit
    return pod_min_shift(p) >= c->shift && (p.req_mem >> c->shift) <= kLimit && (p.nz_mem >> c->shift) <= kLimit;
}

// One mirror row, for rolling back a rejected upsert / reserve (the mirror must keep matching
// the device table).
struct RowSnap {
    int64_t ac, am, mp, rc, rm, zc, zm, np, ae[QS_MAX_EXT], re[QS_MAX_EXT];
    uint64_t th, ts, lb0, lb1, gen;
    int32_t zone;
};
RowSnap snap_row(const Mirror &m, uint32_t i) {
    RowSnap r{m.ac[i], m.am[i], m.mp[i], m.rc[i], m.rm[i], m.zc[i], m.zm[i], m.np[i], {}, {},
              m.th[i], m.ts[i], m.lb[2 * (size_t)i], m.lb[2 * (size_t)i + 1], m.gen[i], m.zone[i]};
    for (int k = 0; k < QS_MAX_EXT; k++) {
        r.ae[k] = m.ae[(size_t)i * QS_MAX_EXT + k];
        r.re[k] = m.re[(size_t)i * QS_MAX_EXT + k];
    }
    return r;
}
void put_row(Mirror &m, uint32_t i, const RowSnap &r) {
    m.ac[i] = r.ac; m.am[i] = r.am; m.mp[i] = r.mp; m.rc[i] = r.rc; m.rm[i] = r.rm;
    m.zc[i] = r.zc; m.zm[i] = r.zm; m.np[i] = r.np;
    for (int k = 0; k < QS_MAX_EXT; k++) {
        m.ae[(size_t)i * QS_MAX_EXT + k] = r.ae[k];
        m.re[(size_t)i * QS_MAX_EXT + k] = r.re[k];
    }
    m.th[i] = r.th; m.ts[i] = r.ts; m.lb[2 * (size_t)i] = r.lb0; m.lb[2 * (size_t)i + 1] = r.lb1;
    m.gen[i] = r.gen; m.zone[i] = r.zone;
}

// Test hooks for the recovery path (tests/test_gpu_recovery.py): QS_INJECT_FAULT=<entry> makes the
// next call of that entry point fail as a device error after its device work.  One-shot per
// context and hook (the environment itself is never modified by the library).  `e` is the run's
// RunKnobs::inject.
enum InjectHook : uint32_t { kInjStreamRun = 1u, kInjHandoff = 2u, kInjResidentStall = 4u };
bool inject_once(qs_ctx *c, const char *e, const char *name, uint32_t bit) {
    if (!e || std::strcmp(e, name) != 0 || (c->inject_used & bit)) return false;
    c->inject_used |= bit;
    return true;
}
void maybe_inject_fault(qs_ctx *c, const char *e, const char *entry) {
    if (inject_once(c, e, entry, kInjStreamRun))
        fail(QS_EDEVICE, std::string("injected device fault in ") + entry);
}

// A pending row (qs_reserve's fast path defers its device write to the next qs_score_pod launch)
// is written before any other device work of the context.
void flush_pending(qs_ctx *c);

template <class F>
qs_status guarded(qs_ctx *c, F &&f, bool keep_pending = false) {
    if (!c) return QS_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    try {
        if (!keep_pending) flush_pending(c);
        f();
        c->err.clear();
        return QS_OK;
    } catch (const QsError &e) {
        c->err = e.msg;
        if (e.st == QS_EDEVICE || e.st == QS_ETIMEOUT) {
            // failure recovery: the host mirror is authoritative — it is synced
            // after every stream, so it holds every placement the caller has been told about.
            // Drop the device table; the next call re-uploads it from the mirror.
            c->dev_valid = false;
            c->mirror_stale = false;
            c->saved = false;
            c->device_faults++;
        }
        return e.st;
    } catch (const std::bad_alloc &) {
        c->err = "out of host memory";
        return QS_ENOMEM;
    } catch (const std::exception &e) {
        c->err = e.what();
        return QS_EINVAL;
    } catch (...) {
        c->err = "unknown error";
        return QS_EINVAL;
    }
}

// Per-launch HIP-event timing on the library's stream (config.profile_kernels).
struct KernelTimer {
    bool on;
    hipStream_t stream, stream2;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[4];
    double secs[4] = {0, 0, 0, 0};
    uint64_t count[4] = {0, 0, 0, 0};
    KernelTimer(bool o, hipStream_t s, hipStream_t s2) : on(o), stream(s), stream2(s2) {}
    void begin(int k, hipStream_t s) {
        if (!on) return;
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        HIPCHK(hipEventRecord(a, s));
        ev[k].push_back({a, b});
    }
    void end(int k, hipStream_t s) {
        if (!on) return;
        HIPCHK(hipEventRecord(ev[k].back().second, s));
    }
    void finish() {
        if (!on) return;
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipStreamSynchronize(stream2));
        for (int k = 0; k < 4; k++) {
            for (auto &e : ev[k]) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, e.first, e.second));
                secs[k] += ms * 1e-3;
                count[k]++;
                (void)hipEventDestroy(e.first);
                (void)hipEventDestroy(e.second);
            }
            ev[k].clear();
        }
    }
};

uint32_t la_window(const qs_ctx *c);
bool la_overlap(const qs_ctx *c);

int pick_engine(const qs_ctx *c, uint32_t n, bool spread_over = false, bool host_over = false, bool honor = false) {
    int e = c->cfg.engine;
    const uint32_t feat = c->dc.feat;
    if (feat & kFeatAA) {
        // pod anti-affinity (spec S12): the engines whose kernels carry the filter
        if (e == QS_ENGINE_LOOKAHEAD || e == QS_ENGINE_ALLREDUCE)
            fail(QS_EINVAL, "pod anti-affinity tracking runs the PERSISTENT and SCAN engines only: the lookahead "
                            "lists and the per-pod all-reduce do not carry the anti-affinity filter");
        // zone topology spread (spec S13): a stream whose SPREAD pods belong to more apps than the
        // persistent workgroup keeps counts for (kSpreadApps) runs SCAN, like a table
        // above the node cap
        if (spread_over && e == QS_ENGINE_PERSISTENT)
            fail(QS_EINVAL, "PERSISTENT engine supports QS_AA_SPREAD / QS_AA_SPREAD_SOFT pods of at most " + std::to_string(kSpreadApps) +
                                " distinct apps per stream");
        // hostname topology spread (spec S15): the persistent workgroup keeps the (app, node) counts of at
        // most kHostSpreadApps apps in LDS, and has no instantiation with the soft-spread score as well
        if (host_over && e == QS_ENGINE_PERSISTENT)
            fail(QS_EINVAL, "PERSISTENT engine supports QS_AA_SPREAD_HOSTNAME pods of at most " +
                                std::to_string(kHostSpreadApps) + " distinct apps per stream, and not together "
                                "with QS_AA_SPREAD_SOFT pods");
        // nodeAffinityPolicy Honor (spec S16): the per-pod count pass over the nodes the pod's selector
        // admits exists on SCAN and the score path only
        if (honor && e == QS_ENGINE_PERSISTENT)
            fail(QS_EINVAL, "PERSISTENT engine does not count topology spread under nodeAffinityPolicy Honor or "
                            "nodeTaintsPolicy Honor: a stream that holds a spread pod with a nodeSelector or required "
                            "node-affinity terms (under nodeTaintsPolicy Honor: one that leaves a hard taint bit "
                            "untolerated) runs SCAN");
        if (e == QS_ENGINE_AUTO)
            e = n <= persistent_max_nodes(feat) && !spread_over && !host_over && !honor ? QS_ENGINE_PERSISTENT
                                                                                         : QS_ENGINE_SCAN;
    }
    if (e == QS_ENGINE_AUTO) {
        if (n > 0 && la_geometry(n, la_window(c), shard_plan(c).W, 2 * la_window(c)).G > 0)
            e = QS_ENGINE_LOOKAHEAD;
        else if (n <= persistent_max_nodes(feat)) e = QS_ENGINE_PERSISTENT;
        else e = QS_ENGINE_SCAN;
    }
    if (e == QS_ENGINE_BATCHED) fail(QS_EINVAL, "the batched engine runs through QS_MODE_BATCHED");
    if (e == QS_ENGINE_PERSISTENT && n > persistent_max_nodes(feat))
        fail(QS_EINVAL, "PERSISTENT engine supports at most " +
                            std::to_string(persistent_max_nodes(feat)) + " nodes for this profile");
    return e;
}

// Overlapped windows (select of window w+1 beside resolve of window w): on unless
// cfg.lookahead_serial or QS_LA_OVERLAP=0; needs 2K <= 64 dirty slots, i.e. K <= 32.
bool la_overlap(const qs_ctx *c) {
    if (proc_knobs().overlap_off) return false;
    return !c->cfg.lookahead_serial && la_window(c) <= 32;
}

LaGeom lookahead_geometry(const qs_ctx *c, uint32_t n, bool overlap) {
    const ShardPlan sp = shard_plan(c);
    const uint32_t K = la_window(c);
    LaGeom geo = la_geometry(n, K, sp.W, overlap ? 2 * K : K);
    geo.v0 = sp.v0;
    geo.nv = sp.nv;
    return geo;
}

uint32_t la_window(const qs_ctx *c) {
    int K = c->cfg.lookahead > 0 ? c->cfg.lookahead : 32;  // measured best on config 2
    return (uint32_t)std::min(64, std::max(1, K));
}

void percentile_stats(const std::vector<uint64_t> &st, qs_stats *s) {
    if (st.size() < 2) return;
    std::vector<double> d(st.size() - 1);
    for (size_t i = 1; i < st.size(); i++) d[i - 1] = (double)(st[i] - st[i - 1]) * 0.01;  // 100 MHz
    std::sort(d.begin(), d.end());
    auto pct = [&](double q) { return d[std::min(d.size() - 1, (size_t)(q * (double)(d.size() - 1) + 0.5))]; };
    s->p50_cycle_us = pct(0.50);
    s->p99_cycle_us = pct(0.99);
    s->max_cycle_us = d.back();
}

// =============================================================================================
// qs_stream_run: the run's plan, one function per engine, the post-run step
// =============================================================================================

// What one stream run does.  plan_run is the only place that sets c->dc.feat for a stream run.
struct RunPlan {
    int eng;           // the qs_engine that runs
    uint32_t feat;     // c->dc.feat of the run
    bool aa_exact;     // an exact stream of a tracking context: it carries the filter and records its pods
    bool spread_over;  // more SPREAD apps than k_persistent keeps zone counts for
    bool host_spread;  // the stream needs the per-(app, node) counts: hostname-spread pods, or restricting
                       // spread pods under nodeAffinityPolicy Honor (and the context tracks)
    bool host_over;    // hostname-spread pods of more apps than k_persistent's slots, or beside soft-spread pods
    bool honor;        // the stream holds a restricting spread pod under Honor (spec S16): it runs SCAN
};

RunPlan plan_run(qs_ctx *c, const qs_stream *s, qs_mode mode) {
    RunPlan p{};
    c->dc.feat = s->feat;
    // pod anti-affinity (spec S12): every exact stream of a tracking context carries the filter
    // and records its pods; batched mode filters and records by itself (S11, the same state)
    p.aa_exact = c->aa_track && mode == QS_MODE_EXACT;
    if (c->aa_track) aa_check_table(c);
    if (p.aa_exact) {
        c->dc.feat = aa_feat(s->feat);
        // soft-spread pods (spec S14): the k_persistent instantiations that carry the score, and their caps
        if (std::find(s->soft.begin(), s->soft.end(), 1) != s->soft.end()) c->dc.feat |= kFeatSoft;
    }
    // zone topology spread (spec S13): k_persistent keeps the counts of at most kSpreadApps apps
    p.spread_over = p.aa_exact && s->spread_apps > kSpreadApps;
    // hostname topology spread (spec S15): the k_persistent instantiations that keep the (app, node)
    // counts of the stream's hostname-spread apps in LDS (kFeatHost), for at most kHostSpreadApps apps
    // and no soft pod in the same stream
    const bool host_pods = p.aa_exact && s->host_pods != 0;
    const bool has_soft = p.aa_exact && (c->dc.feat & kFeatSoft) != 0;
    p.host_over = host_pods && (s->host_apps > kHostSpreadApps || has_soft);
    // nodeAffinityPolicy Honor (spec S16): a stream with a restricting spread pod counts over the
    // per-node array in a pass of its own, which SCAN has and k_persistent has not
    p.honor = p.aa_exact && s->honor_pods != 0;
    p.host_spread = host_pods || p.honor;
    if (host_pods && !p.host_over && !p.honor) c->dc.feat |= kFeatHost;
    p.eng = mode == QS_MODE_BATCHED ? QS_ENGINE_BATCHED
                                    : pick_engine(c, c->m.n, p.spread_over, p.host_over, p.honor);
    p.feat = c->dc.feat;
    return p;
}

// The device arrays a run reads and writes: the stream's pod records and its per-pod outputs.
struct RunIo {
    const void *dp;
    const DPodX *dx;
    int32_t *on;
    uint64_t *ok;
    uint64_t *st;  // config.record_timestamps, else nullptr
};

// A prepared stream's launch sequence as one HIP graph: replayed while `key` (every pointer and value
// the captured launches were given) equals the key it was captured under, captured again otherwise.
// enqueue(capturing) issues the sequence on c->stream.
using GraphKey = std::vector<uint8_t>;
void key_put(GraphKey &key, const void *p, size_t nb) {
    key.insert(key.end(), (const uint8_t *)p, (const uint8_t *)p + nb);
}
template <class F>
void replay_or_capture(qs_ctx *c, qs_stream *s, const GraphKey &key, F &&enqueue) {
    if (!s->gexec || s->gkey != key) {
        if (s->gexec) (void)hipGraphExecDestroy(s->gexec);
        s->gexec = nullptr;
        HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        try {
            enqueue(true);
        } catch (...) {
            hipGraph_t g = nullptr;
            (void)hipStreamEndCapture(c->stream, &g);
            if (g) (void)hipGraphDestroy(g);
            throw;
        }
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamEndCapture(c->stream, &g));
        const hipError_t ie = hipGraphInstantiate(&s->gexec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        HIPCHK(ie);
        s->gkey = key;
    }
    HIPCHK(hipGraphLaunch(s->gexec, c->stream));
}

// QS_MODE_BATCHED (spec S11): batches of B <= 64 pods; per batch one select + merge (each pod's
// 64 best keys against the batch-start table, anti-affinity included) and one claim kernel that
// resolves the batch, applies it and builds the next one on the device.  The ceil(P/B) batches of
// a stream are captured once as a HIP graph; the few pods still carried at the end (all their
// candidates claimed by earlier pods of their batch) run in extra batches.  Returns the batch count.
uint64_t run_batched(qs_ctx *c, qs_stream *s, const RunIo &io, const RunKnobs &kn, KernelTimer &kt) {
    const uint32_t n = c->m.n, P = s->p;
    for (int q = 0; q < 3; q++)
        if (c->strat[q].type != QS_STRATEGY_LEAST_ALLOCATED)
            fail(QS_EINVAL, "QS_MODE_BATCHED scores LeastAllocated only (qs_set_scoring_strategy[_qos]: class " +
                                std::to_string(q) + " has another strategy)");
    if (c->dc.feat & (kFeatTaint | kFeatAffinity))
        fail(QS_EINVAL, "QS_MODE_BATCHED supports the Fit + Balanced (+ extended resources) profile");
    if (!c->dt.apps) fail(QS_EINVAL, "QS_MODE_BATCHED keeps anti-affinity state for tables up to 2^20 nodes");
    if (c->world > 1 || c->cfg.virtual_shards > 1) fail(QS_EINVAL, "QS_MODE_BATCHED runs unsharded");
    if (batch_claim_lds(n) > 160 * 1024)
        fail(QS_EINVAL, "QS_MODE_BATCHED claims batches in LDS: tables up to 712,672 nodes");
    HIPCHK(batch_claim_prepare());
    const uint32_t B = c->cfg.batch_pods > 0 ? (uint32_t)std::min(64, c->cfg.batch_pods) : 64u;
    LaGeom geo = la_geometry(n, B, 1, 64);
    if (geo.G == 0) fail(QS_EINVAL, "no batched geometry for this table size");
    geo.waves = 4;
    geo.k32 = 0;
    const size_t lwords = (size_t)geo.K * 64 * geo.eplr;
    const size_t cwords = std::max<size_t>(1, (size_t)geo.K * geo.G * geo.L);
    c->lists.ensure(8 * lwords);
    c->clists.ensure(8 * cwords);
    c->bctrl.ensure(4 * 192);
    uint32_t *ctrl = c->bctrl.as<uint32_t>(), *bidx = ctrl + 64, *tickets = ctrl + 128;
    LaBufs bf{c->lists.as<uint64_t>(), c->clists.as<uint64_t>(), nullptr, nullptr, nullptr, nullptr,
              nullptr, bidx, ctrl};
    if (!kn.fused_merge_off) bf.tickets = tickets;
    auto batch = [&]() {
        kt.begin(2, c->stream);
        HIPCHK(launch_la_window(c->dt, io.dp, io.dx, 0, P, c->dc, geo, bf, io.on, io.ok, nullptr, nullptr, c->stream, 1));
        kt.end(2, c->stream);
        kt.begin(3, c->stream);
        HIPCHK(launch_batch_claim(c->dt, io.dp, bf.lists, ctrl, bidx, P, B, io.on, io.ok, c->stream));
        kt.end(3, c->stream);
    };
    const uint32_t nb0 = (P + B - 1) / B;
    // (the QS_SYNC_EVERY sync is not held back while capturing, unlike the lookahead's)
    auto enqueue = [&](bool /*capturing*/) {
        HIPCHK(hipMemsetAsync(bf.lists, 0, 8 * lwords, c->stream));
        HIPCHK(hipMemsetAsync(tickets, 0, 4 * 64, c->stream));
        HIPCHK(launch_batch_init(ctrl, bidx, P, B, c->stream));
        const uint32_t every = proc_knobs().sync_every;
        for (uint32_t b = 0; b < nb0; ++b) {
            batch();
            if (every && (b + 1) % every == 0 && !kt.on) HIPCHK(hipStreamSynchronize(c->stream));
        }
    };
    // A stream of very many batches (small batch_pods: 100,000 batches of one pod) is enqueued directly:
    // its graph would be one chain of a few nodes per batch, and instantiating a chain of some 10^5
    // nodes ended the process with a segmentation fault (10,000 batches instantiate and replay fine)
    constexpr uint32_t kBatchGraphMax = 8192;
    if (!kt.on && proc_knobs().graph != '0' && nb0 <= kBatchGraphMax) {
        GraphKey key;
        const void *ptrs[] = {c->dt.rows, c->dt.wrows, c->dt.apps, bf.lists, bf.clists, ctrl, io.dp, io.on, io.ok};
        key_put(key, ptrs, sizeof ptrs);
        key_put(key, &c->dt.n, sizeof c->dt.n);
        key_put(key, &c->dc, sizeof c->dc);
        key_put(key, &geo, sizeof geo);
        const int tag = 2;  // batched
        key_put(key, &tag, sizeof tag);
        key_put(key, &bf.tickets, sizeof bf.tickets);  // the merge form is read per run
        replay_or_capture(c, s, key, enqueue);
    } else {
        enqueue(false);
    }
    uint64_t batches = nb0;
    for (;;) {  // carried pods left after the planned batches
        uint32_t h[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(h, ctrl, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (h[0] == 0) break;
        if (batches > 2ull * P + 64) fail(QS_EDEVICE, "batched mode made no progress");  // cannot happen
        batch();
        ++batches;
    }
    c->soa_valid = false;
    return batches;
}

// SCAN: per pod one key scan (+ pre-pass) and one commit launch.  Returns the batch count (P).
uint64_t run_scan(qs_ctx *c, const qs_stream *s, const RunIo &io, bool aa_exact, KernelTimer &kt) {
    const uint32_t P = s->p;
    HIPCHK(hipMemsetAsync(c->scratch.p, 0, scan_scratch_bytes(), c->stream));
    ensure_soa(c);
    for (uint32_t k = 0; k < P; k++) {
        // (128: a soft-spread pod of a tracked stream, spec S14: the pre-pass in every class)
        // (256: a hostname-spread pod, spec S15: the pre-pass for the minimum of its app's counts)
        // (512: a restricting SPREAD / SPREAD_SOFT pod under nodeAffinityPolicy Honor, spec S16: the count
        // pass first; a hostname-spread pod's minimum launch reads the record's bit instead)
        const int sp = !aa_exact ? 0
                                 : (s->soft[k] ? 128 : s->hosts[k] ? 256 : 0) | (s->honors[k] && !s->hosts[k] ? 512 : 0);
        kt.begin(1, c->stream);  // the key scan alone (+ normalize pre-pass)
        HIPCHK(launch_scan_pod(c->dt, io.dp, io.dx, k, c->dc, c->scratch.p, io.on, io.ok, io.st,
                               nullptr, nullptr, nullptr, 1 | sp, c->stream));
        kt.end(1, c->stream);
        HIPCHK(launch_scan_pod(c->dt, io.dp, io.dx, k, c->dc, c->scratch.p, io.on, io.ok, io.st,
                               nullptr, nullptr, nullptr, 2 | sp, c->stream));
    }
    return P;
}

// ALLREDUCE, SURVEY.md §8(e) C1 as-is: per pod every rank scans its contiguous node shard over the
// rows, one ncclAllReduce(u64 max) of the packed key (C2: the two normalize maxima first), and every
// rank applies the same Reserve to its replicated table.
// virtual_shards = V > 1 on a one-rank communicator: this context scans all V node ranges of a V-rank
// world in turn into the same scratch (the maxima with atomicMax, the keys max-into-best), so the
// shard partition and the max over shards run exactly as V ranks would compute them (the test form of
// the multi-rank engine).  Returns the batch count (P).
uint64_t run_allreduce(qs_ctx *c, const qs_stream *s, const RunIo &io, KernelTimer &kt) {
    const uint32_t n = c->m.n, P = s->p;
    if (!c->comm)
        fail(QS_ESTATE, "the all-reduce engine needs an RCCL communicator (qs_open_shard with an id)");
    const uint32_t V = c->world == 1 && c->cfg.virtual_shards > 1 ? (uint32_t)c->cfg.virtual_shards : 1u;
    const uint32_t R = V > 1 ? V : (uint32_t)c->world;
    DevTable dt = c->dt;
    std::memset(&dt.soa, 0, sizeof dt.soa);  // rows only (the SoA copy is marked stale after the run)
    std::vector<uint32_t> sh(2 * (size_t)R);
    for (uint32_t r = 0; r < R; ++r) {
        sh[2 * r] = (uint32_t)((uint64_t)n * r / R);
        sh[2 * r + 1] = (uint32_t)((uint64_t)n * (r + 1) / R);
    }
    const uint32_t r0 = V > 1 ? 0u : (uint32_t)c->rank;  // this rank's range (V = 1)
    c->vshard.ensure(8 * (size_t)R);
    HIPCHK(hipMemcpy(c->vshard.p, sh.data(), 8 * (size_t)R, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(c->scratch.p, 0, scan_scratch_bytes(), c->stream));
    char *lohi = static_cast<char *>(c->scratch.p) + offsetof(ScanHead, lo);
    auto range = [&](uint32_t r) {
        return hipMemcpyAsync(lohi, c->vshard.as<uint32_t>() + 2 * r, 8, hipMemcpyDeviceToDevice, c->stream);
    };
    if (V == 1) HIPCHK(range(r0));
    ScanHead *sc = c->scratch.as<ScanHead>();
    const bool norm = (c->dc.feat & (kFeatTaint | kFeatAffinity)) != 0;
    for (uint32_t k = 0; k < P; k++) {
        kt.begin(1, c->stream);
        if (norm) {
            for (uint32_t v = 0; v < V; ++v) {
                if (V > 1) HIPCHK(range(v));
                HIPCHK(launch_scan_pod(dt, io.dp, io.dx, k, c->dc, c->scratch.p, io.on, io.ok, io.st, nullptr,
                                       nullptr, nullptr, 8, c->stream));
            }
            allreduce_max_u32(c, &sc->mt, 2, c->stream);
        }
        for (uint32_t v = 0; v < V; ++v) {
            if (V > 1) HIPCHK(range(v));
            HIPCHK(launch_scan_pod(dt, io.dp, io.dx, k, c->dc, c->scratch.p, io.on, io.ok, io.st, nullptr,
                                   nullptr, nullptr, 16 | 32, c->stream));
        }
        allreduce_max_u64(c, reinterpret_cast<uint64_t *>(&sc->best), 1, c->stream);
        HIPCHK(launch_scan_pod(dt, io.dp, io.dx, k, c->dc, c->scratch.p, io.on, io.ok, io.st, nullptr, nullptr,
                               nullptr, 64, c->stream));
        kt.end(1, c->stream);
    }
    return P;
}

// ---- LOOKAHEAD ---------------------------------------------------------------------------------
// One lookahead run: what la_setup works out and every later step reads.
struct LaRun {
    RunIo io;
    uint32_t n, P, nwin;
    LaGeom geo;
    size_t rank_entries;  // [K][GLp] list entries per shard
    size_t lwords;        // one window's lists
    size_t cwords;        // one window's chunk lists
    size_t nparts;        // one window's partial maxima (uint4; normalizing profiles)
    int nbuf;             // overlapped windows double-buffer the lists
    bool norm;            // normalizing profile: k_la_norm pre-pass
    bool overlap;         // select of window w+1 beside resolve of window w
    bool mbox;            // sharded over the peer-memory mailbox (c->comm: RCCL)
    bool handoff;         // per-window resolvers wait for their lists on a device word
    uint64_t seq_run;     // tags the hand-off and mailbox words of this run (0: neither in use)
    uint64_t *hw;         // the hand-off words {unused, ready, timeout flag}
    uint64_t *diag;       // QS_DIAG stamps, else nullptr
};

// Geometry, the waves / key-width choice, the transport checks, the per-window buffers and the
// hand-off words of a lookahead run.  `profiling`: config.profile_kernels brackets every launch.
LaRun la_setup(qs_ctx *c, const qs_stream *s, const RunIo &io, const RunKnobs &kn, bool profiling) {
    const ProcKnobs &pk = proc_knobs();
    LaRun r{};
    r.io = io;
    r.n = c->m.n;
    r.P = s->p;
    r.overlap = la_overlap(c);
    LaGeom &geo = r.geo;
    geo = lookahead_geometry(c, r.n, r.overlap);
    r.norm = (c->dc.feat & (kFeatTaint | kFeatAffinity)) != 0;
    // sharded transport: RCCL (c->comm) or the peer-memory mailbox (c->mbox_on)
    r.mbox = c->mbox_on && !c->comm;
    if (c->world > 1 && !c->comm && !r.mbox)
        fail(QS_ESTATE, "sharded context without a transport: pass an RCCL id to qs_open_shard "
                        "or connect the mailbox (qs_dist_mailbox_connect)");
    if (r.mbox && c->mbox_broken)
        fail(QS_ESTATE, "mailbox ranks out of step after a timeout: every rank must call "
                        "qs_dist_mailbox_connect again (between two barriers) before the next run");
    // normalizing profiles: k_la_norm pre-pass + the single-wave k_la_resolve_norm
    geo.waves = r.norm || (pk.resolver_waves1 && !r.overlap) ? 1u : 4u;
    // normalizing profiles: the four-wave resolver with its stop/resume hand-off
    // (overlapped windows, merged lists); QS_NORM_WAVES=1 keeps the single-wave kernel
    if (r.norm && r.overlap && geo.epl == 1 && !kn.norm_waves1) geo.waves = 4;
    int64_t wmax = 0;
    for (int q = 0; q < 3; q++) wmax = std::max<int64_t>(wmax, (int64_t)c->cfg.w_fit[q] + c->cfg.w_bal[q]);
    if (c->dc.feat & kFeatTaint) wmax += c->cfg.w_taint;       // every plugin scores <= 100
    if (c->dc.feat & kFeatAffinity) wmax += c->cfg.w_affinity;
    geo.k32 = (100 * wmax + 1 < 1024 && r.n <= (1u << 22)) ? 1u : 0u;
    if (geo.G == 0) fail(QS_EINVAL, "no lookahead geometry for this table size");
    r.rank_entries = (size_t)geo.K * 64 * geo.eplr;
    r.lwords = geo.W * r.rank_entries;
    r.cwords = std::max<size_t>(1, (size_t)geo.nv * geo.K * geo.G * geo.L);
    r.nbuf = r.overlap ? 2 : 1;
    c->lists.ensure(8 * r.lwords * r.nbuf);
    c->clists.ensure(8 * r.cwords * r.nbuf);
    c->dio.ensure(2 * kDioWords * 4);
    r.nparts = r.norm ? (size_t)geo.W * geo.K * geo.G : 1;
    c->npart.ensure(16 * r.nparts * r.nbuf);
    c->normi.ensure(16 * (size_t)geo.K * r.nbuf);
    c->nfall.ensure(16);
    c->nrec.ensure(4 * kDioWords);
    if (pk.diag) {
        c->diag.ensure(128);
        HIPCHK(hipMemsetAsync(c->diag.p, 0, 128, c->stream));
        r.diag = c->diag.as<uint64_t>();
    }
    // in-kernel window hand-off (overlapped, unsharded windows): the resolver of window w
    // waits for window w's lists on a device word instead of a cross-stream event, so
    // consecutive resolver launches follow each other on one stream (QS_HANDOFF=0: events)
    // Only for direct launches: under graph replay, dropping the per-window event edges
    // let the executor serialise the select chain behind the resolvers (measured 122 vs
    // 91 ms per config-2 stream), while direct launches on the two streams gain (88 ms).
    // So overlapped unsharded runs launch directly with the hand-off by default
    // (config 2: 1.147 M vs 1.075 M pods/s; config 4: 548 k vs 518 k); QS_GRAPH=1 forces
    // graph replay (and events), QS_HANDOFF=0 keeps events.
    // (not in profile_kernels runs: their per-launch events should bracket the
    // resolver's own time, not an in-kernel wait)
    const bool handoff_ok = r.overlap && !c->comm && !c->handoff_off && !profiling && !pk.handoff_off;
    r.handoff = handoff_ok && pk.graph != '1';
    if (!c->hand.p) {
        c->hand.ensure(32);
        HIPCHK(hipMemset(c->hand.p, 0, 32));
    }
    r.hw = c->hand.as<uint64_t>();
    c->dc.ready = r.handoff ? r.hw + 1 : nullptr;
    // the run's sequence number tags the hand-off and mailbox words (earlier runs compare
    // lower; every rank of a sharded job runs the same streams, so the numbers agree)
    r.seq_run = (r.handoff || r.mbox) ? ++c->run_seq : 0;
    c->dc.epoch = r.handoff ? r.seq_run : 0;
    c->last_waits = r.handoff || r.mbox;
    if (r.mbox && (uint64_t)geo.K * geo.G > kMbPartPerRank)
        fail(QS_EINVAL, "mailbox transport: K*G exceeds the mailbox partials capacity");
    c->dc.werr = r.handoff ? reinterpret_cast<uint32_t *>(r.hw + 2) : nullptr;
    r.nwin = (r.P + geo.K - 1) / geo.K;
    return r;
}

// The buffers of window w: the lists' parity half when windows overlap, the mailbox slot when sharded
// over it.
LaBufs la_bufs(qs_ctx *c, const LaRun &r, uint32_t w) {
    const int b = r.overlap ? (int)(w & 1) : 0;
    uint32_t *dio = c->dio.as<uint32_t>();
    LaBufs bf{c->lists.as<uint64_t>() + b * r.lwords, c->clists.as<uint64_t>() + b * r.cwords,
              c->npart.as<uint4>() + b * r.nparts, c->normi.as<NormInfo>() + (size_t)b * r.geo.K, nullptr, nullptr,
              c->nfall.as<unsigned long long>()};
    bf.rec = c->nrec.as<uint32_t>();
    if (r.mbox) {  // lists and partials live in this rank's mailbox, slot w % 3
        bf.lists = mbox_lists(c, w % 3);
        bf.npart = mbox_npart(c, w % 3);
    }
    if (r.overlap) {
        bf.dprev = dio + ((w + 1) & 1) * kDioWords;
        bf.dcur = dio + (w & 1) * kDioWords;
    }
    return bf;
}

// select (+ norm pre-pass, + merge, + the exchanges when sharded) of window w on stream `ss`
void la_select(qs_ctx *c, const LaRun &r, KernelTimer &kt, uint32_t w, hipStream_t ss) {
    const RunIo &io = r.io;
    const LaGeom &geo = r.geo;
    const LaBufs bf = la_bufs(c, r, w);
    kt.begin(2, ss);
    uint32_t *werr = reinterpret_cast<uint32_t *>(r.hw + 2);
    if (r.norm) {
        HIPCHK(launch_la_window(c->dt, io.dp, io.dx, w * geo.K, r.P, c->dc, geo, bf, io.on, io.ok, io.st, r.diag, ss, 4));
        if (c->comm) exchange_u32(c, (uint32_t *)bf.npart, 4 * (size_t)geo.K * geo.G, ss);
        else if (r.mbox) mbox_exchange(c, 0, w % 3, 16 * (size_t)geo.K * geo.G, 0, 0, (r.seq_run << 32) | (w + 1), werr, ss);
    }
    HIPCHK(launch_la_window(c->dt, io.dp, io.dx, w * geo.K, r.P, c->dc, geo, bf, io.on, io.ok, io.st, r.diag, ss, 1));
    kt.end(2, ss);
    if (c->comm) exchange_lists(c, bf.lists, r.rank_entries, ss);
    else if (r.mbox) mbox_exchange(c, 1, w % 3, 8 * r.rank_entries, geo.K, geo.L, (r.seq_run << 32) | (w + 1), werr, ss);
    if (r.handoff) HIPCHK(launch_ready_set(r.hw + 1, (c->dc.epoch << 32) | (w + 1), ss));
}

void la_resolve(qs_ctx *c, const LaRun &r, KernelTimer &kt, uint32_t w) {
    const RunIo &io = r.io;
    kt.begin(3, c->stream);
    HIPCHK(launch_la_window(c->dt, io.dp, io.dx, w * r.geo.K, r.P, c->dc, r.geo, la_bufs(c, r, w), io.on, io.ok,
                            io.st, r.diag, c->stream, 2));
    kt.end(3, c->stream);
}

// The per-window launch sequence of the whole stream, issued directly or into a capture.
void la_enqueue_windows(qs_ctx *c, const LaRun &r, KernelTimer &kt, bool capturing) {
    // QS_SYNC_EVERY (individual launches only)
    const uint32_t sync_every = capturing ? 0u : proc_knobs().sync_every;
    // the run's timeout word: cleared before every run that waits on device words (the
    // serial mailbox path too: a stale 1 would void every later run)
    if (r.handoff || r.mbox) HIPCHK(hipMemsetAsync(r.hw + 2, 0, 8, c->stream));
    HIPCHK(hipMemsetAsync(c->lists.p, 0, 8 * r.lwords * r.nbuf, c->stream));  // padding stays 0
    HIPCHK(hipMemsetAsync(c->dio.p, 0, 2 * kDioWords * 4, c->stream));
    HIPCHK(hipMemsetAsync(c->nfall.p, 0, 16, c->stream));
    if (!r.overlap) {
        for (uint32_t w = 0; w < r.nwin; ++w) {
            la_select(c, r, kt, w, c->stream);
            la_resolve(c, r, kt, w);
            if (sync_every && (w + 1) % sync_every == 0) HIPCHK(hipStreamSynchronize(c->stream));
        }
        return;
    }
    // select(w+1) on the second stream runs beside resolve(w): it reads the table
    // after resolve(w-1), so the resolver treats the nodes of window w as dirty too
    // (lists of L = 2K keys).  Event rings order the two chains.
    constexpr int R = 4;
    hipEvent_t esel[R], eres[R], est;
    for (int i = 0; i < R; ++i) {
        HIPCHK(hipEventCreateWithFlags(&esel[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&eres[i], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&est, hipEventDisableTiming));
    HIPCHK(hipEventRecord(est, c->stream));
    HIPCHK(hipStreamWaitEvent(c->stream2, est, 0));
    la_select(c, r, kt, 0, c->stream2);
    HIPCHK(hipEventRecord(esel[0], c->stream2));
    for (uint32_t w = 0; w < r.nwin; ++w) {
        if (w + 1 < r.nwin) {
            if (w >= 1) HIPCHK(hipStreamWaitEvent(c->stream2, eres[(w - 1) % R], 0));
            la_select(c, r, kt, w + 1, c->stream2);
            HIPCHK(hipEventRecord(esel[(w + 1) % R], c->stream2));
        }
        if (!r.handoff) HIPCHK(hipStreamWaitEvent(c->stream, esel[w % R], 0));
        la_resolve(c, r, kt, w);
        HIPCHK(hipEventRecord(eres[w % R], c->stream));
        if (sync_every && (w + 1) % sync_every == 0) {
            HIPCHK(hipStreamSynchronize(c->stream2));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    hipEvent_t eend = nullptr;
    if (r.handoff) {  // join the select stream (its last ready_set) back into the run
        HIPCHK(hipEventCreateWithFlags(&eend, hipEventDisableTiming));
        HIPCHK(hipEventRecord(eend, c->stream2));
        HIPCHK(hipStreamWaitEvent(c->stream, eend, 0));
    }
    for (int i = 0; i < R; ++i) {
        (void)hipEventDestroy(esel[i]);
        (void)hipEventDestroy(eres[i]);
    }
    (void)hipEventDestroy(est);
    if (eend) (void)hipEventDestroy(eend);
}

// The key of the captured per-window sequence (replay_or_capture).
GraphKey la_graph_key(const qs_ctx *c, const LaRun &r) {
    GraphKey key;
    const void *ptrs[] = {c->dt.rows, c->dt.wrows, c->dt.masks, c->lists.p, c->clists.p, c->dio.p, r.io.st,
                          (void *)c->comm, r.io.dp, r.io.dx, c->npart.p, c->normi.p, c->nfall.p};
    key_put(key, ptrs, sizeof ptrs);
    key_put(key, &c->dt.n, sizeof c->dt.n);
    key_put(key, &c->dc, sizeof c->dc);
    key_put(key, &r.geo, sizeof r.geo);
    key_put(key, &r.overlap, sizeof r.overlap);
    return key;
}

// Resident stream: the whole overlapped window sequence of an unsharded Fit +
// Balanced (+ extended) stream as ONE launch (resolver + selector workgroups handing off inside it);
// QS_RESIDENT=0 keeps per-window launches.
struct ResPlan {
    LaGeom rgeo;    // the launch's geometry (G == 0: none fits)
    uint32_t sel;   // selector workgroups
    bool resident;  // the run is one resident launch
};
ResPlan la_plan_resident(qs_ctx *c, const LaRun &r, const RunKnobs &kn) {
    const uint32_t feat = c->dc.feat, n = r.n;
    if (!c->cus) {
        int cu = 0;
        HIPCHK(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, c->device));
        c->cus = cu;
    }
    const uint32_t cus = (uint32_t)c->cus;
    // two selector workgroups per CU when the occupancy check admits them, else one
    // (normalizing profiles: the resident resolver is the four-wave one whatever the
    // per-window geometry picked — sharded contexts keep the single-wave kernel there,
    // epl > 1 — unless QS_NORM_WAVES=1 pins the single-wave path)
    LaGeom pgeo = r.geo;
    if (r.norm && r.overlap && !kn.norm_waves1) pgeo.waves = 4;
    if (kn.res_k32_off) pgeo.k32 = 0;
    ResPlan p{};
    LaGeom &rgeo = p.rgeo;
    rgeo = la_stream_res_plan(pgeo, feat, n, cus, 2);
    if (rgeo.G > 0 && rgeo.K * rgeo.G + 1 > la_stream_res_max_blocks(rgeo, feat, n, cus))
        rgeo = la_stream_res_plan(pgeo, feat, n, cus, 1);
    // one selector workgroup per (pod, chunk) task of a window, at most one per
    // remaining CU (they loop over the tasks otherwise); QS_RES_SEL overrides
    p.sel = rgeo.K * rgeo.G;
    if (proc_knobs().res_sel > 0) p.sel = proc_knobs().res_sel;
    // normalizing profiles: the G chunk tasks of a pod wait for each other's partial
    // maxima, so every task needs its own workgroup
    if (r.norm) p.sel = std::max(p.sel, rgeo.K * rgeo.G);
    // the launch's workgroups wait on each other: resident only when the occupancy
    // query guarantees that all 1 + sel of them run at once (VERDICT r2 missing #5)
    const bool coresident = rgeo.G > 0 && 1 + p.sel <= la_stream_res_max_blocks(rgeo, feat, n, cus);
    // unsharded contexts, and mailbox-sharded ones for Fit + Balanced (+ extended)
    // profiles: there the selectors exchange every pod's shard list through the peers'
    // mailboxes inside the launch (RCCL cannot be called in a kernel)
    const bool res_transport = c->world == 1 ? !r.mbox && !c->comm : r.mbox;
    const bool res_allowed = c->res_timeouts < 2 && !c->res_cooldown;
    p.resident = r.overlap && res_transport && res_allowed && !proc_knobs().diag && !kn.resident_off &&
                 rgeo.G > 0 && coresident;
    return p;
}

// Windows of identical pod records for the K a resident launch runs: the stream's bitmap on the
// device (rebuilt when K changed), or nullptr when the launch takes none (QS_RES_UNIFORM=0, the
// kernel class, no such window).  Sets s->uni_given.
const uint32_t *la_uniform_windows(qs_ctx *c, qs_stream *s, const LaGeom &rgeo, uint32_t W, const RunKnobs &kn) {
    const uint32_t P = s->p;
    s->uni_given = 0;
    if (kn.res_uniform_off || !la_stream_res_takes_uniform(rgeo, c->dc.feat, W) || s->run0.size() != P)
        return nullptr;
    if (s->uni_K != rgeo.K) {
        const uint32_t K = rgeo.K, nwin = (P + K - 1) / K;
        s->uni_bits.assign((nwin + 31) / 32 + 1, 0u);
        s->uni_count = 0;
        for (uint32_t w = 0; w < nwin; ++w) {
            const uint32_t s0 = w * K, last = std::min(P, s0 + K) - 1;
            if (s->run0[last] <= s0) {
                s->uni_bits[w >> 5] |= 1u << (w & 31);
                ++s->uni_count;
            }
        }
        s->d_uni.ensure(4 * s->uni_bits.size());
        HIPCHK(hipMemcpyAsync(s->d_uni.p, s->uni_bits.data(), 4 * s->uni_bits.size(),
                              hipMemcpyHostToDevice, c->stream));
        s->uni_K = K;
    }
    if (!s->uni_count) return nullptr;
    s->uni_given = s->uni_count;
    return s->d_uni.as<uint32_t>();
}

// QS_RES_DIAG: the resident resolver's time split (list waits / window bodies / between), from the
// launch's 128 diagnostic words.
void la_report_res_diag(const uint64_t *h, uint32_t sel) {
    const double nw = h[3] ? (double)h[3] : 1.0;
    fprintf(stderr, "QS_RES_DIAG resolver %.3f us per window; windows whose lists were not prefetched %llu of %llu (selectors %u)\n",
            h[1] * 0.01 / nw, (unsigned long long)h[4], (unsigned long long)h[3], sel);
    if (h[2])
        fprintf(stderr, "QS_RES_DIAG selector 0: done seen %.2f us, its task finished %.2f us after "
                        "the resolver's start of the window it overlaps (%llu windows)\n",
                h[13] * 0.01 / (double)h[2], h[14] * 0.01 / (double)h[2], (unsigned long long)h[2]);
    {
        std::vector<double> fin;
        for (uint32_t k = 0; k < std::min(sel, 64u); ++k)
            if (h[64 + k]) fin.push_back(h[64 + k] * 0.01);
        std::sort(fin.begin(), fin.end());
        if (!fin.empty()) {
            fprintf(stderr, "QS_RES_DIAG selectors' mean finish (us after window start), sorted:");
            for (double v : fin) fprintf(stderr, " %.1f", v);
            fprintf(stderr, "\n");
        }
    }
    if (h[36] + h[37] + h[38])
        fprintf(stderr, "QS_RES_DIAG B3 -> B1 busy (ns per window, without the B1 wait): D %.0f, A %.0f, "
                        "C %.0f\n", h[38] * 10.0 / nw, h[37] * 10.0 / nw, h[36] * 10.0 / nw);
    if (h[41])
        fprintf(stderr, "QS_RES_DIAG uniform windows %llu: %.2f us each from B1 to the window end, "
                        "%.2f rounds each; the other windows %.2f us each, boundaries included\n",
                (unsigned long long)h[41], h[40] * 0.01 / (double)h[41], (double)h[42] / (double)h[41],
                h[3] > h[41] ? (h[1] - h[40]) * 0.01 / (double)(h[3] - h[41]) : 0.0);
    if (h[33])
        fprintf(stderr, "QS_RES_DIAG last list of a window published %.2f us after the start of "
                        "the window before it (%llu windows; after 13 us %llu, after 15 us %llu)\n",
                h[32] * 0.01 / (double)h[33], (unsigned long long)h[33],
                (unsigned long long)h[34], (unsigned long long)h[35]);
    if (h[6])
        fprintf(stderr, "QS_RES_DIAG prefetch check: %llu windows short of lists, %.2f lists missing "
                        "on average\n", (unsigned long long)h[6], (double)h[5] / (double)h[6]);
    if (h[27] + h[28] + h[29] + h[30] + h[31])
        fprintf(stderr, "QS_RES_DIAG window boundary (ns per window, wave D): bookkeeping %.0f "
                        "-> B2 %.0f -> B3 %.0f -> B1 %.0f -> pod 0 decided %.0f\n",
                h[27] * 10.0 / nw, h[28] * 10.0 / nw, h[29] * 10.0 / nw, h[30] * 10.0 / nw,
                h[31] * 10.0 / nw);
    if (h[19])
        fprintf(stderr, "QS_RES_DIAG selector task (us): scoring %.2f chunk top-L %.2f publish/merge %.2f (tasks %llu, merges %llu)\n",
                h[16] * 0.01 / (double)h[19], h[17] * 0.01 / (double)h[19], h[18] * 0.01 / (double)h[19],
                (unsigned long long)h[19], (unsigned long long)h[20]);
    if (h[12])  // QS_RES_DIAG_BLOCK build: busy shader cycles per pod step by role
        fprintf(stderr, "QS_RES_DIAG busy cycles/step: D %.0f A %.0f B %.0f C %.0f (steps %llu)\n",
                h[8] / (double)h[12], h[9] / (double)h[12], h[10] / (double)h[12],
                h[11] / (double)h[12], (unsigned long long)h[12]);
    if (h[12])
        fprintf(stderr, "QS_RES_DIAG step marks: D argmax %.0f | A pub+reads %.0f applied %.0f | C reads %.0f keyC %.0f loads %.0f\n",
                h[26] / (double)h[12], h[21] / (double)h[12], h[22] / (double)h[12],
                h[23] / (double)h[12], h[24] / (double)h[12], h[25] / (double)h[12]);
}

// QS_DIAG: the per-window resolver's shader-clock stamps, from its 16 diagnostic words.
void la_report_diag(const uint64_t *h, const LaGeom &geo, uint32_t nwin) {
    const double np = h[5] ? (double)h[5] : 1.0;
    fprintf(stderr, geo.waves == 1 ? "QS_DIAG resolve cycles/pod: cand %.0f issue %.0f fresh %.0f wmax %.0f commit %.0f (pods %llu, G=%u E=%u epl=%u)\n"
                                   : "QS_DIAG resolve4 busy cycles/pod: D %.0f A %.0f B %.0f C %.0f (C row wait %.0f) (pods %llu, G=%u E=%u epl=%u)\n",
            h[0] / np, h[1] / np, h[2] / np, h[3] / np, h[4] / np,
            (unsigned long long)h[5], geo.G, geo.E, geo.epl);
    if (geo.waves == 4)
        fprintf(stderr, "QS_DIAG resolve4 pre-score cycles/pod: A %.0f C %.0f; per window: prologue %.0f epilogue %.0f\n",
                h[6] / np, h[7] / np, h[8] / (double)nwin, h[9] / (double)nwin);
}

// The resident launch of the run `r` as `rp` plans it.
void la_launch_resident(qs_ctx *c, qs_stream *s, const LaRun &r, const ResPlan &rp, const RunKnobs &kn,
                        KernelTimer &kt) {
    const RunIo &io = r.io;
    const LaGeom &rgeo = rp.rgeo;
    // what the resident geometry needs beyond la_setup's per-window sizes (DevBuf::ensure only grows, so
    // each buffer ends at the larger of the two needs): its hand-off counters; per window parity the
    // chunks' partial maxima and the pods' NormInfo of the normalizing profiles; the entry statics of the
    // lists; its own chunk lists (its chunks differ from the per-window select's), double-buffered
    const size_t rcw = std::max<size_t>(1, (size_t)rgeo.K * rgeo.G * rgeo.L);
    c->resctl.ensure(la_stream_res_ctl_bytes());
    c->npart.ensure(16 * 2 * (size_t)rgeo.K * rgeo.G);
    c->normi.ensure(16 * 2 * 64);
    c->nstat.ensure(4 * 2 * 128 * (size_t)rgeo.K);
    c->clists.ensure(8 * rcw * 2);
    // la_setup armed the per-window hand-off; the resident launch hands off inside the kernel: no ready
    // word or epoch, but always the timeout word
    c->dc.ready = nullptr;
    c->dc.epoch = 0;
    c->dc.werr = reinterpret_cast<uint32_t *>(r.hw + 2);
    c->last_waits = true;
    HIPCHK(hipMemsetAsync(c->lists.p, 0, 8 * r.lwords * r.nbuf, c->stream));  // padding stays 0
    HIPCHK(hipMemsetAsync(c->dio.p, 0, 2 * kDioWords * 4, c->stream));
    HIPCHK(hipMemsetAsync(c->resctl.p, 0, la_stream_res_ctl_bytes(), c->stream));
    HIPCHK(hipMemsetAsync(r.hw + 2, 0, 8, c->stream));
    HIPCHK(hipMemsetAsync(c->nfall.p, 0, 16, c->stream));  // {rescans, windows with a rescan}
    ResShard rsh{1u, 0u, 0ull, nullptr, 0ull, 0ull, 0ull, 0ull, 0ull};
    if (c->world > 1)
        rsh = ResShard{(uint32_t)c->world, (uint32_t)c->rank, r.seq_run, c->mbox_peers.as<char *>(),
                       kMbResHello, kMbResFlags, kMbResLists, kMbResNFlags, kMbResNorm};
    DevCfg dcr = c->dc;  // (the launch's copy: the test hooks never stick to the context)
    // test hook: a selector that never delivers window 3 (one-shot), so the
    // in-kernel timeout drain runs (tests/test_gpu_recovery.py)
    // (QS_INJECT_FAULT=resident_stall_always: every resident launch of the context)
    dcr.inject = (inject_once(c, kn.inject, "resident_stall", kInjResidentStall) ||
                  (kn.inject && std::strcmp(kn.inject, "resident_stall_always") == 0)) ? 1u : 0u;
    // (QS_INJECT_FAULT=resident_skew: this rank's selectors of windows 40-43 start 3 ms
    // late, so the ranks of a sharded run drift apart in the middle of the stream)
    if (kn.inject && std::strcmp(kn.inject, "resident_skew") == 0) dcr.inject = 2u;
    // sharded: window 0's waits cover a peer still in host-side prepare (5 s)
    dcr.first_ticks = c->world > 1 ? 500000000ull : 0ull;
    // no node with allocatable cpu or memory 0: the key waves skip those terms
    // (QS_FAST_ALLOC=0 keeps the generic scorers)
    dcr.all_alloc = c->zero_alloc == 0 && !kn.fast_alloc_off ? 1u : 0u;
    // what the launch runs (qs_stats::resident_path): the ring form carries 32-bit
    // keys, and its two-resource classes read the flag
    c->last_res_path = (!r.norm && rgeo.k32 ? 1 : 0) |
                       (!r.norm && !(c->dc.feat & kFeatRes) && dcr.all_alloc ? 2 : 0);
    dcr.sel_diag = kn.sel_diag ? 1u : 0u;
    uint64_t *rdiag = nullptr;
    if (proc_knobs().res_diag) {
        c->diag.ensure(1024);
        rdiag = c->diag.as<uint64_t>();
        HIPCHK(hipMemsetAsync(rdiag, 0, 1024, c->stream));
    }
    const uint32_t *uni = la_uniform_windows(c, s, rgeo, rsh.W, kn);
    kt.begin(3, c->stream);  // the one launch, under "resolve"
    HIPCHK(launch_la_stream_res(c->dt, io.dp, io.dx, dcr, r.P, rgeo, c->lists.as<uint64_t>(), c->clists.as<uint64_t>(),
                                (uint32_t)r.lwords, (uint32_t)rcw, c->npart.as<uint4>(),
                                c->normi.as<NormInfo>(), c->nstat.as<uint32_t>(),
                                c->nfall.as<unsigned long long>(), io.on, io.ok,
                                io.st, c->resctl.p, rp.sel, rdiag, rsh, c->stream, uni));
    kt.end(3, c->stream);
    if (rdiag) {
        uint64_t h[128] = {0};
        HIPCHK(hipMemcpyAsync(h, rdiag, 1024, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        la_report_res_diag(h, rp.sel);
    }
}

// LOOKAHEAD: windows of K pods, as one resident launch, a replayed graph of the per-window launches, or
// those launches issued directly.  Returns the batch count (the windows).
uint64_t run_lookahead(qs_ctx *c, qs_stream *s, const RunIo &io, const RunKnobs &kn, KernelTimer &kt) {
    const ProcKnobs &pk = proc_knobs();
    const LaRun r = la_setup(c, s, io, kn, kt.on);
    const auto th0 = std::chrono::steady_clock::now();
    // Replay the whole window sequence as one HIP graph (built on the first run of this
    // prepared stream): ~3 launches + 4 event operations per window would otherwise
    // be issued one host call at a time.  Not used for diagnostic runs.
    // Multi-rank contexts enqueue directly: RCCL collectives inside a captured graph
    // across ranks have not been observed on this pool yet; QS_GRAPH=1
    // forces capture for them.
    const bool graph_ok = !c->comm || pk.graph == '1';
    const bool use_graph = graph_ok && !r.handoff && !r.mbox && !kt.on && !pk.diag && pk.graph != '0';
    const ResPlan rp = la_plan_resident(c, r, kn);
    c->last_resident = rp.resident;
    // the per-window run after a resident timeout ends the cooldown (whatever it returns)
    if (!rp.resident) c->res_cooldown = false;
    if (rp.resident) {
        la_launch_resident(c, s, r, rp, kn, kt);
    } else if (use_graph) {
        replay_or_capture(c, s, la_graph_key(c, r),
                          [&](bool capturing) { la_enqueue_windows(c, r, kt, capturing); });
    } else {
        la_enqueue_windows(c, r, kt, false);
    }
    if (kn.hosttime)
        fprintf(stderr, "QS_HOSTTIME enqueue %.3f ms for %u windows (overlap %d)\n",
                std::chrono::duration<double>(std::chrono::steady_clock::now() - th0).count() * 1e3,
                r.nwin, (int)r.overlap);
    if (pk.diag) {
        uint64_t h[16] = {0};
        HIPCHK(hipMemcpyAsync(h, r.diag, 128, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        la_report_diag(h, r.geo, r.nwin);
    }
    return r.nwin;
}

// After the run's device work has finished (`ms` between the driver's two events): the timeout word,
// the mirror, the anti-affinity fold, the stream's validity and the stats.
void finish_run(qs_ctx *c, qs_stream *s, qs_mode mode, const RunPlan &plan, const RunKnobs &kn, KernelTimer &kt,
                uint64_t batches, float ms, qs_stats *stats) {
    const uint32_t n = c->m.n, P = s->p;
    const int eng = plan.eng;
    uint64_t rescans = 0, resumed = 0;
    if (eng == QS_ENGINE_LOOKAHEAD && c->last_waits) {
        uint64_t w = 0;  // a resolver gave up waiting for its window's lists (device hand-off)
        HIPCHK(hipMemcpy(&w, c->hand.as<uint64_t>() + 2, 8, hipMemcpyDeviceToHost));
        if (inject_once(c, kn.inject, "handoff", kInjHandoff)) w = 1;  // test hook: a timed-out hand-off
        if (w) {
            // the select stream did not run beside the resolvers (e.g. a profiler serialising
            // dispatches), or a mailbox peer never posted: the run's results and table updates
            // are void and the device table is rebuilt from the host mirror (guarded(), as for
            // a device fault); an unsharded context uses cross-stream events from now on
            if (c->last_resident) {
                ++c->res_timeouts;
                c->res_cooldown = true;
            } else if (!c->mbox_on) {
                c->handoff_off = true;
            }
            if (c->mbox_on && !c->comm) c->mbox_broken = true;
            fail(QS_ETIMEOUT, c->mbox_on ? "mailbox exchange timed out (a peer never posted its window)"
                                         : c->last_resident
                                               ? "resident lookahead stream timed out (a hand-off never arrived); "
                                                 "the next run uses per-window launches"
                                               : "lookahead window hand-off timed out (lists never published); "
                                                 "the context falls back to stream events");
        }
    }
    // a resident run that finished without a timeout: only CONSECUTIVE resident timeouts keep
    // the context on per-window launches (qs_ctx.hpp)
    if (eng == QS_ENGINE_LOOKAHEAD && c->last_resident) c->res_timeouts = 0;
    if (eng == QS_ENGINE_LOOKAHEAD && c->nfall.p) {
        uint64_t h[2] = {0, 0};
        HIPCHK(hipMemcpy(h, c->nfall.p, 16, hipMemcpyDeviceToHost));
        rescans = h[0];
        resumed = h[1];
        if (kn.norm_diag)
            fprintf(stderr, "QS_NORM_DIAG rescans %llu resumed windows %llu\n", (unsigned long long)h[0],
                    (unsigned long long)h[1]);
    }
    c->mirror_stale = true;
    if (eng != QS_ENGINE_SCAN) c->soa_valid = false;  // those engines update the rows only
    kt.finish();
    maybe_inject_fault(c, kn.inject, "stream_run");
    // keep the host mirror authoritative after every stream (one D2H of the rows, outside
    // the timed region): a later device fault rebuilds the table from it
    sync_mirror(c);
    if ((c->aa_track || c->preempt_on) && P > 0 && n > 0) {
        // fold the run's placements into the mirror's anti-affinity state (4 P bytes back, outside
        // wall_s): the mirror stays authoritative for save / restore and the recovery rebuild;
        // ... and into the pod registry (spec S18), in the stream's decision order
        std::vector<int32_t> node(P);
        HIPCHK(hipMemcpy(node.data(), s->d_node.p, 4 * (size_t)P, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < P; k++) {
            if (node[k] < 0 || (uint32_t)node[k] >= n) continue;
            const qs_pod &pod = s->pods[s->order[k]];
            if (c->aa_track) c->m.aa_add((uint32_t)pod.app, (uint32_t)node[k], +1);
            if (c->preempt_on) reg_append(c, (uint32_t)node[k], pod);
        }
    }
    s->aa_ran = plan.aa_exact;
    s->ran = true;
    s->mode_ran = (int)mode;
    s->epoch_after = ++c->table_epoch;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        for (int k = 0; k < 4; k++) {
            stats->kernel_s[k] = kt.secs[k];
            stats->kernel_launches[k] = kt.count[k];
        }
        stats->pods = P;
        stats->evals = (uint64_t)P * n;
        stats->wall_s = ms * 1e-3;
        stats->batches = batches;
        stats->truncations = rescans;
        stats->engine_used = eng;
        stats->table_layout = c->wide ? 1 : 0;
        stats->resumed_windows = resumed;
        stats->resident = (eng == QS_ENGINE_LOOKAHEAD && c->last_resident) ? 1 : 0;
        stats->resident_path = stats->resident ? c->last_res_path : 0;
        stats->device_faults = c->device_faults;
    }
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char *qs_version(void) { return "qsched 0.1 (gfx950)"; }

void qs_config_default(qs_config *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->abi_version = QS_ABI_VERSION;
    cfg->engine = QS_ENGINE_AUTO;
    cfg->fit_weight_cpu = 1;
    cfg->fit_weight_mem = 1;
    const int32_t wf[3] = {1, 2, 3}, wb[3] = {1, 1, 1};  // spec S9
    for (int q = 0; q < 3; q++) { cfg->w_fit[q] = wf[q]; cfg->w_bal[q] = wb[q]; }
    cfg->w_taint = 3;     // UP apis/config/v1/default_plugins.go TaintToleration weight
    cfg->w_affinity = 2;  // NodeAffinity weight
    cfg->qos_sort = 1;
}

qs_status qs_open(const qs_config *cfg, int device, qs_ctx **out) {
    g_open_err.clear();
    if (!cfg || !out) return open_failed(QS_EINVAL, "qs_open: null config or output pointer");
    *out = nullptr;
    qs_ctx *c = new (std::nothrow) qs_ctx();
    if (!c) return QS_ENOMEM;
    try {
        check_cfg(*cfg);
        c->cfg = *cfg;
        c->device = device;
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) fail(QS_EINVAL, "no such device");
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        c->dc = make_devcfg(c->cfg);
        c->scratch.ensure(scan_scratch_bytes());
        HIPCHK(hipMemset(c->scratch.p, 0, scan_scratch_bytes()));
    } catch (const QsError &e) {
        delete c;
        return open_failed(e.st, e.msg);
    } catch (...) {
        delete c;
        return open_failed(QS_EDEVICE, "qs_open: unexpected failure");
    }
    *out = c;
    return QS_OK;
}

qs_status qs_close(qs_ctx *c) {
    if (!c) return QS_EINVAL;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        if (c->comm) (void)ncclCommDestroy(c->comm);
        c->comm = nullptr;
        for (void *p : c->mbox_opened) (void)hipIpcCloseMemHandle(p);
        c->mbox_opened.clear();
        mbox_host_release(c);
        // streams still prepared outlive the context: they keep their own buffers and are freed later
        // by qs_stream_free, which must not reach for this context then
        for (qs_stream *ps : c->streams) ps->owner = nullptr;
        c->streams.clear();
    }
    hipStream_t s = c->stream, s2 = c->stream2;
    if (s2) (void)hipStreamSynchronize(s2);
    if (c->pin) (void)hipHostFree(c->pin);
    delete c;  // DevBuf destructors free device memory
    if (s) (void)hipStreamDestroy(s);
    if (s2) (void)hipStreamDestroy(s2);
    return QS_OK;
}

// The shape function as a table (UP helper/shape_score.go#BuildBrokenLinearFunction over scores scaled
// by 10): throws QS_EINVAL with the reason for a bad shape.
static void shape_table(const qs_shape_point *sh, uint32_t n, uint8_t table[101]) {
    if (!sh || !table) fail(QS_EINVAL, "shape: null pointer");
    if (n < 1 || n > QS_MAX_SHAPE) fail(QS_EINVAL, "shape: 1 to 16 points");
    for (uint32_t i = 0; i < n; i++) {
        if (sh[i].utilization < 0 || sh[i].utilization > 100) fail(QS_EINVAL, "shape: utilization must be in [0, 100]");
        if (sh[i].score < 0 || sh[i].score > 10) fail(QS_EINVAL, "shape: score must be in [0, 10]");
        if (i && sh[i].utilization <= sh[i - 1].utilization)
            fail(QS_EINVAL, "shape: utilization must be strictly increasing");
    }
    for (int64_t p = 0; p <= 100; p++) {
        int64_t v = (int64_t)sh[n - 1].score * 10;
        for (uint32_t i = 0; i < n; i++) {
            if (p > sh[i].utilization) continue;
            const int64_t s1 = (int64_t)sh[i].score * 10;
            if (i == 0) { v = s1; break; }
            const int64_t s0 = (int64_t)sh[i - 1].score * 10, u0 = sh[i - 1].utilization, u1 = sh[i].utilization;
            v = s0 + (s1 - s0) * (p - u0) / (u1 - u0);  // C++ integer division truncates, as Go's
            break;
        }
        table[p] = (uint8_t)v;
    }
}

qs_status qs_shape_table(const qs_shape_point *shape, uint32_t n, uint8_t table[101]) {
    try {
        shape_table(shape, n, table);
    } catch (const QsError &) {
        return QS_EINVAL;
    }
    return QS_OK;
}

// Validates one strategy and writes its device table (RequestedToCapacityRatio: the shape function;
// the other types take none and hold zeros).  Throws QS_EINVAL with the reason.
static void strategy_table(const qs_scoring_strategy *s, uint8_t tab[128]) {
    if (!s) fail(QS_EINVAL, "null scoring strategy");
    if (s->type != QS_STRATEGY_LEAST_ALLOCATED && s->type != QS_STRATEGY_MOST_ALLOCATED &&
        s->type != QS_STRATEGY_REQUESTED_TO_CAPACITY_RATIO)
        fail(QS_EINVAL, "unknown scoring strategy type");
    if (s->type != QS_STRATEGY_REQUESTED_TO_CAPACITY_RATIO && s->n_shape != 0)
        fail(QS_EINVAL, "a shape is given for a scoring strategy that takes none");
    std::memset(tab, 0, 128);
    if (s->type == QS_STRATEGY_REQUESTED_TO_CAPACITY_RATIO) {
        if (s->n_shape < 1 || s->n_shape > QS_MAX_SHAPE) fail(QS_EINVAL, "shape: 1 to 16 points");
        shape_table(s->shape, (uint32_t)s->n_shape, tab);
    }
}

// Stores the strategy of the classes q0..q1 (validated, tab its table) and uploads all three tables.
static void set_strategy(qs_ctx *c, int q0, int q1, const qs_scoring_strategy *s, const uint8_t tab[128]) {
    if (!c->streams.empty()) fail(QS_ESTATE, "the scoring strategy cannot change while prepared streams exist");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));  // no launch of this context still reads the tables
    alignas(16) uint8_t all[3 * 128];
    qs_scoring_strategy next[3] = {c->strat[0], c->strat[1], c->strat[2]};
    for (int q = 0; q < 3; q++) {
        if (q >= q0 && q <= q1) {
            next[q] = qs_scoring_strategy{};
            next[q].type = s->type;
            next[q].n_shape = s->n_shape;
            for (int i = 0; i < s->n_shape; i++) next[q].shape[i] = s->shape[i];
            std::memcpy(all + 128 * q, tab, 128);
        } else {
            uint8_t t[128];
            strategy_table(&c->strat[q], t);  // (valid: it was stored through here)
            std::memcpy(all + 128 * q, t, 128);
        }
    }
    c->strat_tab.ensure(sizeof all);
    HIPCHK(hipMemcpy(c->strat_tab.p, all, sizeof all, hipMemcpyHostToDevice));
    bool rtcr = false;
    for (int q = 0; q < 3; q++) {
        c->strat[q] = next[q];
        rtcr |= next[q].type == QS_STRATEGY_REQUESTED_TO_CAPACITY_RATIO;
    }
    // DevCfg: the tables when some class scores RequestedToCapacityRatio, else none (kFeatStrat kernels only)
    const uint64_t tp = rtcr ? (uint64_t)(uintptr_t)c->strat_tab.p : 0;
    c->dc.strat_tab_lo = (uint32_t)tp;
    c->dc.strat_tab_hi = (uint32_t)(tp >> 32);
}

qs_status qs_set_scoring_strategy(qs_ctx *c, const qs_scoring_strategy *s) {
    return guarded(c, [&] {
        uint8_t tab[128];
        strategy_table(s, tab);
        set_strategy(c, 0, 2, s, tab);
    });
}

qs_status qs_set_scoring_strategy_qos(qs_ctx *c, int32_t qos, const qs_scoring_strategy *s) {
    return guarded(c, [&] {
        if (qos < 0 || qos > 2) fail(QS_EINVAL, "qos must be 0 (BestEffort), 1 (Burstable) or 2 (Guaranteed)");
        uint8_t tab[128];
        strategy_table(s, tab);
        set_strategy(c, qos, qos, s, tab);
    });
}

qs_status qs_get_scoring_strategy_qos(qs_ctx *c, int32_t qos, qs_scoring_strategy *out) {
    return guarded(c, [&] {
        if (qos < 0 || qos > 2) fail(QS_EINVAL, "qos must be 0 (BestEffort), 1 (Burstable) or 2 (Guaranteed)");
        if (!out) fail(QS_EINVAL, "null scoring strategy");
        *out = c->strat[qos];
    });
}

qs_status qs_set_pod_anti_affinity(qs_ctx *c, int32_t on) {
    return guarded(c, [&] {
        if (!c->streams.empty())
            fail(QS_ESTATE, "pod anti-affinity tracking cannot change while prepared streams exist");
        if (on) {
            if (c->world > 1 || c->cfg.virtual_shards > 1)
                fail(QS_EINVAL, "pod anti-affinity tracking runs unsharded (qs_open_shard / virtual_shards > 1)");
            aa_check_table(c);
        }
        c->aa_track = on != 0;  // (the recorded state stays as it is)
    });
}

qs_status qs_get_pod_anti_affinity(qs_ctx *c, int32_t *on) {
    return guarded(c, [&] {
        if (!on) fail(QS_EINVAL, "null output");
        *on = c->aa_track ? 1 : 0;
    });
}

qs_status qs_set_topology_spread_weight(qs_ctx *c, int32_t w) {
    return guarded(c, [&] {
        if (!c->streams.empty())
            fail(QS_ESTATE, "the topology spread weight cannot change while prepared streams exist");
        if (w < 0 || w > 100) fail(QS_EINVAL, "the topology spread weight must be 0..100");
        c->w_pts = w;
        if (c->dev_valid) {
            HIPCHK(hipSetDevice(c->device));
            write_spread_cfg(c);
        }
    });
}

qs_status qs_get_topology_spread_weight(qs_ctx *c, int32_t *w) {
    return guarded(c, [&] {
        if (!w) fail(QS_EINVAL, "null output");
        *w = c->w_pts;
    });
}

qs_status qs_set_topology_spread_node_affinity_policy(qs_ctx *c, int32_t policy) {
    return guarded(c, [&] {
        if (!c->streams.empty())
            fail(QS_ESTATE, "the topology spread nodeAffinityPolicy cannot change while prepared streams exist");
        if (policy != QS_POLICY_IGNORE && policy != QS_POLICY_HONOR)
            fail(QS_EINVAL, "the topology spread nodeAffinityPolicy must be QS_POLICY_IGNORE or QS_POLICY_HONOR");
        if (policy == QS_POLICY_HONOR && !c->cfg.enable_affinity)
            fail(QS_EINVAL, "QS_POLICY_HONOR needs the NodeAffinity filter (config.enable_affinity = 1): it counts "
                            "the nodes that filter admits");
        c->spread_policy = policy;
    });
}

qs_status qs_get_topology_spread_node_affinity_policy(qs_ctx *c, int32_t *policy) {
    return guarded(c, [&] {
        if (!policy) fail(QS_EINVAL, "null output");
        *policy = c->spread_policy;
    });
}

qs_status qs_set_topology_spread_node_taints_policy(qs_ctx *c, int32_t policy) {
    return guarded(c, [&] {
        if (!c->streams.empty())
            fail(QS_ESTATE, "the topology spread nodeTaintsPolicy cannot change while prepared streams exist");
        if (policy != QS_POLICY_IGNORE && policy != QS_POLICY_HONOR)
            fail(QS_EINVAL, "the topology spread nodeTaintsPolicy must be QS_POLICY_IGNORE or QS_POLICY_HONOR");
        if (policy == QS_POLICY_HONOR && !c->cfg.enable_taint)
            fail(QS_EINVAL, "QS_POLICY_HONOR needs the TaintToleration filter (config.enable_taint = 1): it counts "
                            "the nodes that filter admits");
        c->taints_policy = policy;
    });
}

qs_status qs_get_topology_spread_node_taints_policy(qs_ctx *c, int32_t *policy) {
    return guarded(c, [&] {
        if (!policy) fail(QS_EINVAL, "null output");
        *policy = c->taints_policy;
    });
}

qs_status qs_score_pod_zone_scores(qs_ctx *c, int32_t *out) {
    return guarded(c, [&] {
        if (!out) fail(QS_EINVAL, "null output");
        if (!c->score_zs_valid) fail(QS_ESTATE, "no qs_score_pod / qs_score_pod_packed call yet");
        std::memcpy(out, c->score_zs, sizeof c->score_zs);
    }, /*keep_pending=*/true);
}

// (no context: why the calling thread's last qs_open / qs_open_shard failed, or "null context")
const char *qs_last_error(const qs_ctx *c) {
    if (c) return c->err.c_str();
    return g_open_err.empty() ? "null context" : g_open_err.c_str();
}

qs_status qs_nodes_load(qs_ctx *c, const qs_node_soa *nd, uint32_t n) {
    return guarded(c, [&] {
        if (!nd || !nd->alloc_cpu || !nd->alloc_mem) fail(QS_EINVAL, "alloc_cpu/alloc_mem required");
        HIPCHK(hipSetDevice(c->device));
        Mirror &m = c->m;
        m.resize(n);
        m.aa_clear();  // no pod recorded on a new table (spec S12)
        m.reg.clear();  // ... and none registered (spec S18; the sequence counter runs on)
        reg_stale(c);
        auto get = [](const int64_t *a, size_t i, int64_t d) { return a ? a[i] : d; };
        for (uint32_t i = 0; i < n; i++) {
            m.ac[i] = nd->alloc_cpu[i];
            m.am[i] = nd->alloc_mem[i];
            m.mp[i] = get(nd->max_pods, i, 110);
            m.rc[i] = get(nd->req_cpu, i, 0);
            m.rm[i] = get(nd->req_mem, i, 0);
            m.zc[i] = get(nd->nz_cpu, i, 0);
            m.zm[i] = get(nd->nz_mem, i, 0);
            m.np[i] = get(nd->pods, i, 0);
            for (int k = 0; k < QS_MAX_EXT; k++) {
                m.ae[(size_t)i * QS_MAX_EXT + k] = get(nd->alloc_ext, (size_t)i * QS_MAX_EXT + k, 0);
                m.re[(size_t)i * QS_MAX_EXT + k] = get(nd->req_ext, (size_t)i * QS_MAX_EXT + k, 0);
            }
            m.zone[i] = nd->zone ? nd->zone[i] : 0;
            m.th[i] = nd->taint_hard ? nd->taint_hard[i] : 0;
            m.ts[i] = nd->taint_soft ? nd->taint_soft[i] : 0;
            m.lb[2 * (size_t)i] = nd->label_bits ? nd->label_bits[2 * (size_t)i] : 0;
            m.lb[2 * (size_t)i + 1] = nd->label_bits ? nd->label_bits[2 * (size_t)i + 1] : 0;
        }
        for (uint32_t i = 0; i < n; i++) check_row_values(m, i);
        c->shift = table_shift(m);
        c->zero_alloc = count_zero_alloc(m);
        c->wide = false;
        for (uint32_t i = 0; i < n && !c->wide; i++) c->wide = !row_compact_ok(m, i, c->shift);
        c->dev_valid = false;
        c->saved = false;
        c->mirror_stale = false;
        ++c->table_epoch;
        upload_table(c);
    });
}

qs_status qs_nodes_read(qs_ctx *c, const qs_node_soa_out *o, uint32_t n) {
    return guarded(c, [&] {
        if (!o) fail(QS_EINVAL, "null output");
        if (n != c->m.n) fail(QS_EINVAL, "n does not match the loaded table");
        sync_mirror(c);
        const Mirror &m = c->m;
        auto put = [](int64_t *d, const std::vector<int64_t> &s) {
            if (d) std::memcpy(d, s.data(), s.size() * 8);
        };
        put(o->alloc_cpu, m.ac); put(o->alloc_mem, m.am); put(o->max_pods, m.mp);
        put(o->req_cpu, m.rc); put(o->req_mem, m.rm); put(o->nz_cpu, m.zc); put(o->nz_mem, m.zm);
        put(o->pods, m.np); put(o->alloc_ext, m.ae); put(o->req_ext, m.re);
        if (o->taint_hard) std::memcpy(o->taint_hard, m.th.data(), 8 * (size_t)n);
        if (o->taint_soft) std::memcpy(o->taint_soft, m.ts.data(), 8 * (size_t)n);
        if (o->label_bits) std::memcpy(o->label_bits, m.lb.data(), 16 * (size_t)n);
        if (o->zone) std::memcpy(o->zone, m.zone.data(), 4 * (size_t)n);
    });
}

qs_status qs_node_upsert(qs_ctx *c, uint32_t idx, const qs_node_row *r, uint64_t generation) {
    return guarded(c, [&] {
        if (!r) fail(QS_EINVAL, "null row");
        HIPCHK(hipSetDevice(c->device));
        sync_mirror(c);
        Mirror &m = c->m;
        if (idx > m.n) fail(QS_EINVAL, "idx beyond table end (append only at idx == n)");
        if (idx < m.n && generation != 0 && generation <= m.gen[idx]) return;  // already applied (UP NodeInfo.Generation diff)
        // validate the new row on its own before any state changes (a rejected row leaves the
        // mirror, the layout and the device table untouched)
        Mirror one;
        one.resize(1);
        one.ac[0] = r->alloc_cpu; one.am[0] = r->alloc_mem; one.mp[0] = r->max_pods;
        one.rc[0] = r->req_cpu; one.rm[0] = r->req_mem; one.zc[0] = r->nz_cpu; one.zm[0] = r->nz_mem;
        one.np[0] = r->pods;
        for (int k = 0; k < QS_MAX_EXT; k++) { one.ae[k] = r->alloc_ext[k]; one.re[k] = r->req_ext[k]; }
        one.th[0] = r->taint_hard; one.ts[0] = r->taint_soft;
        one.lb[0] = r->label_bits[0]; one.lb[1] = r->label_bits[1];
        one.zone[0] = r->zone;
        one.gen[0] = generation;
        check_row_values(one, 0);
        if (c->hcount.p && r->max_pods > kHcMaxPods)
            fail(QS_EINVAL, "max_pods above 65535 on a context that counts pods per (app, node) in 16 bits "
                            "(QS_AA_SPREAD_HOSTNAME, spec S15; nodeAffinityPolicy / nodeTaintsPolicy Honor, spec S16 / S17)");
        if (c->aa_track && idx < m.n && r->zone != m.zone[idx] && m.aa_holds(idx))
            fail(QS_EINVAL, "node " + std::to_string(idx) + " holds pods recorded for anti-affinity: its zone "
                            "cannot change while tracking is on");
        if (reg_holds(c, idx)) reg_check_row(c, idx, *r);
        const bool was_zero = idx < m.n && zero_alloc_row(m, idx);
        const bool zone_moves = idx < m.n && r->zone != m.zone[idx];  // (an append re-uploads the table)
        if (idx == m.n) {  // append one node
            // (the recorded anti-affinity state is moved aside, not copied with the columns)
            auto aa_node = std::move(m.aa_node);
            auto aa_zone = std::move(m.aa_zone);
            auto aa_pods = std::move(m.aa_pods);
            auto reg = std::move(m.reg);  // (the registry likewise, spec S18)
            m.aa_clear();
            m.reg.clear();
            Mirror old = m;
            m.resize(old.n + 1);
            m.reg = std::move(reg);
            m.aa_node = std::move(aa_node);
            m.aa_zone = std::move(aa_zone);
            m.aa_pods = std::move(aa_pods);
            auto cp = [&](std::vector<int64_t> &d, const std::vector<int64_t> &s) { std::copy(s.begin(), s.end(), d.begin()); };
            cp(m.ac, old.ac); cp(m.am, old.am); cp(m.mp, old.mp); cp(m.rc, old.rc); cp(m.rm, old.rm);
            cp(m.zc, old.zc); cp(m.zm, old.zm); cp(m.np, old.np); cp(m.ae, old.ae); cp(m.re, old.re);
            std::copy(old.th.begin(), old.th.end(), m.th.begin());
            std::copy(old.ts.begin(), old.ts.end(), m.ts.begin());
            std::copy(old.lb.begin(), old.lb.end(), m.lb.begin());
            std::copy(old.gen.begin(), old.gen.end(), m.gen.begin());
            std::copy(old.zone.begin(), old.zone.end(), m.zone.begin());
            c->dev_valid = false;
            c->saved = false;
        }
        put_row(m, idx, snap_row(one, 0));
        c->zero_alloc += (zero_alloc_row(m, idx) ? 1u : 0u) - (was_zero ? 1u : 0u);
        ++c->table_epoch;
        // the new row's memory may need a finer unit or the wide layout (re-upload), else one row
        const int want = std::min({ctz64(r->alloc_mem), ctz64(r->req_mem), ctz64(r->nz_mem)});
        const bool was_valid = c->dev_valid;
        const int old_shift = c->shift;
        const bool old_wide = c->wide;
        ensure_layout(c, nullptr, 0, want);
        if (was_valid && c->dev_valid && c->shift == old_shift && c->wide == old_wide) {
            push_row(c, idx);
            // a zone may have gained its first node or lost its last: the domains of spec S13 (every
            // other path re-uploads the table, upload_table writes them)
            if (zone_moves) write_domains(c);
        }
    });
}

// evict_seq != 0 (qs_evict, spec S18): an Unreserve of the registry entry with that sequence number, the pod
// rebuilt from the entry; 0: the pod is the caller's.
static qs_status reserve_impl(qs_ctx *c, uint32_t node, const qs_pod *p, int sign, uint64_t evict_seq = 0) {
    qs_pod from_entry;
    return guarded(c, [&] {
        ptrdiff_t reg_at = -1;
        if (evict_seq != 0) {
            reg_at = node < c->m.n ? reg_find(c, node, nullptr, evict_seq) : -1;
            if (reg_at < 0)
                fail(QS_EINVAL, "qs_evict: node " + std::to_string(node) + " holds no entry with seq " + std::to_string(evict_seq));
            const RegEntry &e = c->m.reg[node][(size_t)reg_at];
            std::memset(&from_entry, 0, sizeof from_entry);
            from_entry.req_cpu = e.rc; from_entry.req_mem = e.rm; from_entry.nz_cpu = e.zc; from_entry.nz_mem = e.zm;
            for (int k = 0; k < QS_MAX_EXT; k++) from_entry.req_ext[k] = e.re[k];
            from_entry.qos = e.qos; from_entry.priority = e.priority; from_entry.app = e.app;
            p = &from_entry;
        }
        if (!p) fail(QS_EINVAL, "null pod");
        if (node >= c->m.n) fail(QS_EINVAL, "node index out of range");
        check_pod(*p, 0);
        HIPCHK(hipSetDevice(c->device));
        const uint32_t app = (uint32_t)p->app;
        if (c->aa_track) {
            aa_check_table(c);
            if (sign < 0 && c->m.aa_count(app, node) == 0)
                fail(QS_EINVAL, "qs_unreserve: no pod of app " + std::to_string(app) + " is recorded on node " +
                                    std::to_string(node));
            // a hostname-spread pod (spec S15): the context keeps the (app, node) counts from here on
            // (k_aa_apply below maintains them)
            if (pod_host_spread(*p) && c->dev_valid) ensure_hcount(c);
        }
        if (c->preempt_on && sign < 0 && evict_seq == 0) {
            // the registry entry this Unreserve removes (spec S18): the latest one that equals the pod
            reg_at = reg_find(c, node, p, 0);
            if (reg_at < 0)
                fail(QS_EINVAL, "qs_unreserve: no registered pod of node " + std::to_string(node) + " equals this pod");
        }
        auto reg_record = [&] {  // (last: nothing after it fails)
            if (reg_at >= 0) reg_erase(c, node, (size_t)reg_at);
            else if (c->preempt_on && sign > 0) reg_append(c, node, *p);
        };
        sync_mirror(c);
        const RowSnap before = snap_row(c->m, node);
        mirror_reserve(c->m, node, *p, sign);
        ++c->table_epoch;
        // anti-affinity bookkeeping (spec S12), after the row's own path has succeeded: the mirror, then
        // one small kernel on the context's stream (a table that is not on the device is rebuilt
        // from the mirror by the next call that needs it)
        auto aa_record = [&] {
            if (!c->aa_track) return;
            const int32_t left = c->m.aa_add(app, node, sign);
            if (!c->dev_valid) return;
            hipLaunchKernelGGL(k_aa_apply, dim3(1), dim3(1), 0, c->stream, c->dt, node, app, (int32_t)sign,
                               left <= 0 ? 1u : 0u);
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) {
                c->m.aa_add(app, node, -sign);
                HIPCHK(le);
            }
        };
        // any failure from here on (a column driven negative, a layout the stream's growth
        // projection rejects, a device error while pushing the row) leaves the mirror as it was:
        // the caller was told the reservation failed
        try {
            check_row_values(c->m, node);  // e.g. an Unreserve that drives a column negative
            if (pod_fits_layout(c, *p) && (c->wide || row_compact_ok(c->m, node, c->shift))) {
                // the row changes in place: no device call now — the next qs_score_pod launch writes
                // it (and scores it from its argument), any other call writes it first
                if (c->pend != 0xFFFFFFFFu && c->pend != node) flush_pending(c);
                const uint32_t pend_before = c->pend;
                c->pend = node;
                try {
                    aa_record();
                } catch (...) {
                    c->pend = pend_before;
                    throw;
                }
                reg_record();
                return;
            }
            flush_pending(c);
            const bool was_valid = c->dev_valid;
            const int old_shift = c->shift;
            const bool old_wide = c->wide;
            ensure_layout(c, p, 1);
            if (was_valid && c->shift == old_shift && c->wide == old_wide) push_row(c, node);
            aa_record();
            reg_record();
        } catch (...) {
            put_row(c->m, node, before);
            throw;
        }
    }, /*keep_pending=*/true);
}
qs_status qs_reserve(qs_ctx *c, uint32_t node, const qs_pod *p) { return reserve_impl(c, node, p, +1); }
qs_status qs_unreserve(qs_ctx *c, uint32_t node, const qs_pod *p) { return reserve_impl(c, node, p, -1); }

// ---- preemption (spec S18) ----
qs_status qs_evict(qs_ctx *c, uint32_t node, uint64_t seq) {
    if (seq == 0) {
        if (!c) return QS_EINVAL;
        return guarded(c, [&] { fail(QS_EINVAL, "qs_evict: seq 0 names no entry"); }, /*keep_pending=*/true);
    }
    return reserve_impl(c, node, nullptr, -1, seq);
}

qs_status qs_set_preemption(qs_ctx *c, int32_t on) {
    return guarded(c, [&] {
        if (!c->streams.empty()) fail(QS_ESTATE, "the pod registry cannot be switched while prepared streams exist");
        if (on) {
            if (c->world > 1 || c->cfg.virtual_shards > 1)
                fail(QS_EINVAL, "the pod registry runs unsharded (qs_open_shard / virtual_shards > 1)");
            if (c->m.n > kRegMaxNodes) fail(QS_EINVAL, "the pod registry covers tables up to 2^17 nodes");
        }
        c->preempt_on = on != 0;  // (what is registered stays as it is)
    });
}

qs_status qs_get_preemption(qs_ctx *c, int32_t *on) {
    return guarded(c, [&] {
        if (!on) fail(QS_EINVAL, "null output");
        *on = c->preempt_on ? 1 : 0;
    });
}

qs_status qs_set_preemption_policy(qs_ctx *c, int32_t policy) {
    return guarded(c, [&] {
        if (policy != QS_PREEMPT_BY_PRIORITY && policy != QS_PREEMPT_BY_QOS) fail(QS_EINVAL, "unknown qs_preempt_policy");
        if (policy == c->preempt_policy) return;
        c->preempt_policy = policy;
        // (the saved registry follows when it is restored: qs_table_restore sorts what it reinstates)
        reg_resort(c);
    });
}

qs_status qs_get_preemption_policy(qs_ctx *c, int32_t *policy) {
    return guarded(c, [&] {
        if (!policy) fail(QS_EINVAL, "null output");
        *policy = c->preempt_policy;
    });
}

qs_status qs_node_pods(qs_ctx *c, uint32_t node, qs_victim *out, uint32_t cap, uint32_t *n) {
    return guarded(c, [&] {
        if (!n || (cap && !out)) fail(QS_EINVAL, "null output");
        if (node >= c->m.n) fail(QS_EINVAL, "node index out of range");
        *n = 0;
        if (node >= c->m.reg.size()) return;
        const auto &l = c->m.reg[node];
        *n = (uint32_t)l.size();
        for (uint32_t k = 0; k < l.size() && k < cap; k++) out[k] = reg_victim(l[k]);
    }, /*keep_pending=*/true);
}

qs_status qs_preempt_pod(qs_ctx *c, const qs_pod *pod, int32_t *node, qs_victim *victims, uint32_t *n_victims,
                         int32_t *nvict_n) {
    return guarded(c, [&] {
        if (!pod || !node || !victims || !n_victims) fail(QS_EINVAL, "null argument");
        if (!c->preempt_on) fail(QS_ESTATE, "the pod registry is off (qs_set_preemption)");
        check_pod(*pod, 0);
        if (c->aa_track && QS_AA_KIND(pod->anti_affinity) != QS_AA_NONE)
            fail(QS_EINVAL, "preemption for a pod with anti-affinity or topology spread on a context that tracks them "
                            "is not built (spec S18): removing victims would change the counts its filter reads");
        const uint32_t n = c->m.n;
        if (n > kRegMaxNodes) fail(QS_EINVAL, "the pod registry covers tables up to 2^17 nodes");
        *node = -1;
        *n_victims = 0;
        if (n == 0) return;
        if (c->reg_long)
            for (uint32_t i = 0; i < c->m.reg.size(); i++)
                if (c->m.reg[i].size() > QS_MAX_VICTIMS)
                    fail(QS_EINVAL, "node " + std::to_string(i) + " holds " + std::to_string(c->m.reg[i].size()) +
                                        " registered pods, more than QS_MAX_VICTIMS");
        HIPCHK(hipSetDevice(c->device));
        if (!c->dev_valid) upload_table(c);  // recovery after a device fault: rebuild from the mirror
        reg_sync_device(c);
        // the preemptor in canonical units: the dry run needs no layout the pod fits
        const DPodX dx = compact_podx(c, *pod);
        PreemptPod pp{pod->req_cpu, pod->req_mem, pod->req_ext[0], pod->req_ext[1],
                      reg_importance(c->preempt_policy, pod->qos, pod->priority), pod_flags(c, *pod), c->wide ? 0 : c->shift};
        constexpr size_t kOutBytes = (sizeof(PreemptOut) + 15) & ~(size_t)15;
        c->reg_out.ensure(kOutBytes + sizeof(DPodX));
        c->reg_rec.ensure(preempt_scratch_bytes());
        if (nvict_n) c->reg_nv.ensure((size_t)c->cap * 4);
        DPodX *dpx = reinterpret_cast<DPodX *>(c->reg_out.as<char>() + kOutBytes);
        HIPCHK(hipMemcpyAsync(dpx, &dx, sizeof dx, hipMemcpyHostToDevice, c->stream));
        const uint64_t *col = c->reg_dev.as<uint64_t>();
        const RegView rv{col, reinterpret_cast<const uint32_t *>(col + (size_t)kRegCols * c->reg_slots * c->reg_cap),
                         c->reg_slots, c->reg_cap};
        HIPCHK(launch_preempt(c->dt, c->wide, rv, pp, dpx, nvict_n ? c->reg_nv.as<int32_t>() : nullptr, c->reg_rec.p,
                              c->reg_out.as<PreemptOut>(), c->stream));
        PreemptOut po;
        HIPCHK(hipMemcpyAsync(&po, c->reg_out.p, sizeof po, hipMemcpyDeviceToHost, c->stream));
        if (nvict_n) HIPCHK(hipMemcpyAsync(nvict_n, c->reg_nv.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (po.node < 0) return;
        if ((uint32_t)po.node >= n || po.nvict > QS_MAX_VICTIMS) fail(QS_EDEVICE, "preemption dry run returned a record out of range");
        const auto &l = c->m.reg[(uint32_t)po.node];
        for (uint32_t k = 0; k < po.nvict; k++) {
            if (po.slot[k] >= l.size()) fail(QS_EDEVICE, "preemption dry run returned a slot out of range");
            victims[k] = reg_victim(l[po.slot[k]]);
        }
        *node = po.node;
        *n_victims = po.nvict;
    });
}

// The packed outputs of the one-launch score (pinned host memory, written by the kernel: one u32 of
// four byte scores per node, 0xFFFFFFFF = infeasible) into the caller's arrays, 16 nodes per step as
// vectors: feasible = not the sentinel, the four int32 plugin scores (0 where infeasible) and the
// QoS-weighted total (w = {wfit, wbal, wtt, wna}: the sums node_total forms, -1 where infeasible).
// Widening of the packed per-node words into qs_score_pod's arrays (only the planes asked for), 16
// nodes per iteration with clang vector types.  The body is compiled three times — for AVX-512BW,
// AVX2 and the baseline — and the widest one the host CPU supports is picked once (round 5: the
// copy-out form was 5-7 us of the 5,000-node call and ~40 us of the 50,000-node one, SSE2 only).
__attribute__((always_inline)) static inline void unpack_body(const uint32_t *pk, uint32_t n, const uint32_t w[4],
                                                              uint8_t *feas, int32_t *score, int32_t *total) {
    typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
    typedef int32_t i32x16 __attribute__((ext_vector_type(16)));
    typedef uint8_t u8x16 __attribute__((ext_vector_type(16)));
    typedef uint8_t u8x64 __attribute__((ext_vector_type(64)));
    typedef int32_t i32x64 __attribute__((ext_vector_type(64)));
    uint32_t i = 0;
    for (; i + 16 <= n; i += 16) {
        u32x16 v;
        std::memcpy(&v, pk + i, sizeof v);
        const i32x16 ok = v != kScoreInfeasible;  // -1 (all ones) where feasible
        const u32x16 z = v & (u32x16)ok;           // infeasible -> 0
        if (feas) {
            const u8x16 f = __builtin_convertvector(ok, u8x16) & (uint8_t)1;
            std::memcpy(feas + i, &f, sizeof f);
        }
        if (total) {
            const u32x16 t = (z & 255u) * w[0] + ((z >> 8) & 255u) * w[1] + ((z >> 16) & 255u) * w[2] + (z >> 24) * w[3];
            const i32x16 r = ((i32x16)t & ok) | ~ok;  // -1 where infeasible
            std::memcpy(total + i, &r, sizeof r);
        }
        if (score) {
            u8x64 b;
            std::memcpy(&b, &z, sizeof b);
            const i32x64 wd = __builtin_convertvector(b, i32x64);
            std::memcpy(score + 4 * (size_t)i, &wd, sizeof wd);
        }
    }
    for (; i < n; ++i) {
        const bool f = pk[i] != kScoreInfeasible;
        const uint32_t z = f ? pk[i] : 0u;
        if (feas) feas[i] = f;
        if (score)
            for (uint32_t k = 0; k < 4; ++k) score[4 * (size_t)i + k] = (int32_t)((z >> (8 * k)) & 255u);
        if (total)
            total[i] = f ? (int32_t)((z & 255u) * w[0] + ((z >> 8) & 255u) * w[1] + ((z >> 16) & 255u) * w[2] +
                                     (z >> 24) * w[3])
                         : -1;
    }
}
__attribute__((target("avx512f,avx512bw,avx512vl"))) static void unpack_avx512(const uint32_t *pk, uint32_t n,
                                                                               const uint32_t w[4], uint8_t *feas,
                                                                               int32_t *score, int32_t *total) {
    unpack_body(pk, n, w, feas, score, total);
}
__attribute__((target("avx2"))) static void unpack_avx2(const uint32_t *pk, uint32_t n, const uint32_t w[4],
                                                        uint8_t *feas, int32_t *score, int32_t *total) {
    unpack_body(pk, n, w, feas, score, total);
}
static void unpack_base(const uint32_t *pk, uint32_t n, const uint32_t w[4], uint8_t *feas, int32_t *score,
                        int32_t *total) {
    unpack_body(pk, n, w, feas, score, total);
}
// Large tables widen in parallel: a few helper threads (spinning ~50 us for the next call, then
// sleeping) take equal node ranges (multiples of 16) beside the calling thread (round 5: 50,000
// nodes, every output, was ~20 us of widening on one core).
class UnpackPool {
   public:
    static UnpackPool &get() {
        // never destroyed: its detached helpers may be blocked on cv_ at process exit, and
        // destroying a condition variable with waiters hangs the exit (glibc)
        static UnpackPool *p = new UnpackPool;
        return *p;
    }
    int parts() const { return (int)th_.size() + 1; }
    // fn(part) for part in [0, parts()); the caller runs part 0
    void run(const std::function<void(int)> &fn) {
        std::lock_guard<std::mutex> one(run_mu_);  // contexts in different threads take turns
        {
            std::lock_guard<std::mutex> g(mu_);
            fn_ = &fn;
            left_.store((int)th_.size(), std::memory_order_relaxed);
            gen_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
        fn(0);
        while (left_.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    }

   private:
    UnpackPool() {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const char *e = getenv("QS_UNPACK_THREADS");  // helper threads (default 7)
        const unsigned want = e ? (unsigned)std::max(0, atoi(e)) : 7u;
        const int helpers = (int)std::min(want, hw > 1 ? hw - 1 : 0u);
        for (int k = 0; k < helpers; ++k) th_.emplace_back([this, k] { loop(k + 1); });
        for (auto &t : th_) t.detach();  // process lifetime (no join at static destruction)
    }
    void loop(int part) {
        uint64_t seen = 0;
        for (;;) {
            const auto t0 = std::chrono::steady_clock::now();
            while (gen_.load(std::memory_order_acquire) == seen &&
                   std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(50))
                std::this_thread::yield();
            if (gen_.load(std::memory_order_acquire) == seen) {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return gen_.load(std::memory_order_acquire) != seen; });
            }
            seen = gen_.load(std::memory_order_acquire);
            (*fn_)(part);
            left_.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_, run_mu_;
    std::condition_variable cv_;
    std::atomic<uint64_t> gen_{0};
    std::atomic<int> left_{0};
    const std::function<void(int)> *fn_ = nullptr;
};

static void unpack_scores(const uint32_t *pk, uint32_t n, const uint32_t w[4], uint8_t *feas, int32_t *score,
                          int32_t *total) {
    using Fn = void (*)(const uint32_t *, uint32_t, const uint32_t *, uint8_t *, int32_t *, int32_t *);
    static const Fn fn = [] {
#if !defined(__HIP_DEVICE_COMPILE__)  // (this TU is also parsed for the device; the probe is host-only)
        __builtin_cpu_init();
        if (getenv("QS_UNPACK_BASE")) return (Fn)unpack_base;
        if (__builtin_cpu_supports("avx512bw") && __builtin_cpu_supports("avx512vl")) return (Fn)unpack_avx512;
        if (__builtin_cpu_supports("avx2")) return (Fn)unpack_avx2;
#endif
        return (Fn)unpack_base;
    }();
    static const uint32_t par_min = [] {
        const char *e = getenv("QS_UNPACK_PAR_MIN");  // nodes from which the widening runs in parallel
        return e ? (uint32_t)std::max(0, atoi(e)) : 16384u;
    }();
    if (n < par_min || (!score && !total) || UnpackPool::get().parts() < 2) {
        fn(pk, n, w, feas, score, total);
        return;
    }
    UnpackPool &pool = UnpackPool::get();
    const uint32_t parts = (uint32_t)pool.parts();
    const uint32_t per = ((n + parts - 1) / parts + 15) & ~15u;
    pool.run([&](int part) {
        const uint32_t b = std::min(n, (uint32_t)part * per), e = std::min(n, b + per);
        if (b < e)
            fn(pk + b, e - b, w, feas ? feas + b : nullptr, score ? score + 4 * (size_t)b : nullptr,
               total ? total + b : nullptr);
    });
}

// The one-launch score of one pod into the context's pinned buffer: pod by value,
// the previous Reserve's row folded in, outputs written by the kernel into pinned host memory,
// completion seen by polling its done word (no copy command, no stream sync).  Returns the packed
// per-node words (valid until the next call on the context); *wts = {wfit, wbal, wtt, wna}.
// QS_SCORE_DIAG=1: a qs_score_pod call slower than 500 us reports its host prep / launch / done-word
// wait / unpack split on stderr (the framework path's tail)
static const bool g_sdiag = getenv("QS_SCORE_DIAG") && getenv("QS_SCORE_DIAG")[0] == '1';
struct ScoreSplit { std::chrono::steady_clock::time_point ts, tl, t0, te; };
static thread_local ScoreSplit g_split;
static void score_diag_report(uint64_t seq, std::chrono::steady_clock::time_point tu) {
    auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    const ScoreSplit &s = g_split;
    if (us(s.ts, tu) > 500.0)
        std::fprintf(stderr, "QS_SCORE_DIAG call %llu: prep %.1f us, launch %.1f us, wait %.1f us, unpack %.1f us\n",
                     (unsigned long long)seq, us(s.ts, s.tl), us(s.tl, s.t0), us(s.t0, s.te), us(s.te, tu));
}

static const uint32_t *score_pod_launch(qs_ctx *c, const qs_pod *pod, uint32_t wts[5], int32_t *best) {
    if (g_sdiag) g_split.ts = std::chrono::steady_clock::now();
    // qs_score_pod_zone_scores answers for the last call, once it has succeeded: void until then
    c->score_zs_valid = false;
    if (!pod) fail(QS_EINVAL, "null pod");
    HIPCHK(hipSetDevice(c->device));
    check_pod(*pod, 0);
    if (!pod_fits_layout(c, *pod)) {
        flush_pending(c);  // (a re-layout re-uploads the table from the mirror)
        ensure_layout(c, pod, 1);
    }
    const uint32_t n = c->m.n;
    alignas(16) uint8_t dp[sizeof(DPodW)];
    compact_pod(c, *pod, 0, c->shift, c->wide, dp);
    if (c->wide) {
        const DPodW *q = reinterpret_cast<const DPodW *>(dp);
        wts[0] = q->wfit; wts[1] = q->wbal;
    } else {
        const DPod *q = reinterpret_cast<const DPod *>(dp);
        wts[0] = q->wfit; wts[1] = q->wbal;
    }
    DevCfg dc = c->dc;
    const bool pod_ext = pod->req_ext[0] || pod->req_ext[1];
    dc.feat = feat_of(c->cfg) | (pod_ext ? kFeatExt : 0u) | (c->wide ? kFeatWide | kFeatExt : 0u) |
              res_feat(c->cfg, pod_ext) | strat_feat(c, pod, 1);
    if (c->aa_track) {  // spec S12: the anti-affinity filter on the score path
        aa_check_table(c);
        dc.feat = aa_feat(dc.feat);
    }
    wts[2] = (dc.feat & kFeatTaint) ? (uint32_t)dc.wtt : 0u;
    wts[3] = (dc.feat & kFeatAffinity) ? (uint32_t)dc.wna : 0u;
    std::fill(std::begin(c->score_zs), std::end(c->score_zs), -1);
    wts[4] = 0u;
    if (n == 0 || !c->dev_valid) {
        if (best) *best = -1;
        c->score_zs_valid = true;
        return nullptr;
    }
    // a hostname-spread pod (spec S15) reads the (app, node) counts: allocated / rebuilt first
    // ... and so does a restricting spread pod of any kind under nodeAffinityPolicy Honor (spec S16)
    if (c->aa_track && (pod_host_spread(*pod) || pod_honors(c, *pod))) ensure_hcount(c);
    const DPodX dx = compact_podx(c, *pod);
    // (behind the packed words: the 64 zone scores of a soft-spread pod, spec S14)
    const size_t pb = score_pod1_pack_bytes(n) + kMaxZones * 4;
    const bool soft = c->aa_track && pod_soft_spread(*pod);
    if (c->pin_bytes < pb) {
        if (c->pin) (void)hipHostFree(c->pin);
        c->pin = nullptr;
        c->pin_bytes = 0;
        HIPCHK(hipHostMalloc(&c->pin, pb, hipHostMallocDefault));
        c->pin_bytes = pb;
        std::memset(c->pin, 0, pb);
    }
    if (!c->score_gs.p) {
        // (+ the feasible-zones word of a soft-spread pod, the minimum of a hostname-spread pod, and the
        // domain word and 64 counts of the Honor count pass, spec S16)
        c->score_gs.ensure(score_gs_bytes());
        HIPCHK(hipMemsetAsync(c->score_gs.p, 0, score_gs_bytes(), c->stream));
    }
    const uint32_t pidx = c->pend < n ? c->pend : 0xFFFFFFFFu;
    const HostRow prow = pidx < n ? compact_row(c->m, pidx, c->shift, c->wide) : HostRow{};
    const uint64_t seq = ++c->score_seq;
    const auto tl = std::chrono::steady_clock::now();
    HIPCHK(launch_score_pod1(c->dt, dp, &dx, dc, static_cast<uint8_t *>(c->pin), c->score_gs.as<uint64_t>(), seq,
                             pidx, prow, c->stream));
    c->pend = 0xFFFFFFFFu;
    // the done word: polled (bounded), then the stream is checked for an error
    volatile uint64_t *done = reinterpret_cast<volatile uint64_t *>(static_cast<uint8_t *>(c->pin) + 8);
    const auto t0 = std::chrono::steady_clock::now();
    while (*done != seq) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
            HIPCHK(hipStreamSynchronize(c->stream));  // a fault surfaces here
            if (*done != seq) fail(QS_EDEVICE, "qs_score_pod: the scoring kernel did not complete");
            break;
        }
    }
    if (g_sdiag) {
        g_split.tl = tl;
        g_split.t0 = t0;
        g_split.te = std::chrono::steady_clock::now();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    const uint8_t *h = static_cast<const uint8_t *>(c->pin);
    uint64_t kbest = 0;
    std::memcpy(&kbest, h, 8);
    if (best) *best = kbest ? (int32_t)(0xFFFFFFFFu - (uint32_t)kbest) : -1;
    if (soft) std::memcpy(c->score_zs, h + score_pod1_pack_bytes(n), sizeof c->score_zs);
    c->score_zs_valid = true;
    wts[4] = soft ? (uint32_t)c->w_pts : 0u;
    return reinterpret_cast<const uint32_t *>(h + 16);
}

qs_status qs_score_pod(qs_ctx *c, const qs_pod *pod, uint8_t *feas, int32_t *score, int32_t *total,
                       int32_t *best) {
    return guarded(c, [&] {
        uint32_t w[5];
        const uint32_t *pk = score_pod_launch(c, pod, w, best);
        if (pk) unpack_scores(pk, c->m.n, w, feas, score, total);
        if (pk && total && w[4]) {
            // a soft-spread pod (spec S14): the fifth score by the node's zone (a feasible node's zone
            // holds a feasible node, so its score is there)
            for (uint32_t i = 0; i < c->m.n; i++)
                if (total[i] >= 0) total[i] += (int32_t)w[4] * std::max(c->score_zs[c->m.zone[i]], 0);
        }
        if (g_sdiag && pk) score_diag_report(c->score_seq, std::chrono::steady_clock::now());
    }, /*keep_pending=*/true);
}

qs_status qs_score_pod_packed(qs_ctx *c, const qs_pod *pod, const uint32_t **packed, int32_t *best) {
    return guarded(c, [&] {
        uint32_t w[5];
        const uint32_t *pk = score_pod_launch(c, pod, w, best);
        if (packed) *packed = pk;
        if (g_sdiag && pk) score_diag_report(c->score_seq, std::chrono::steady_clock::now());
    }, /*keep_pending=*/true);
}

qs_status qs_stream_prepare(qs_ctx *c, const qs_pod *pods, uint32_t p, qs_stream **out) {
    if (!out) return QS_EINVAL;
    *out = nullptr;
    qs_stream *s = nullptr;
    qs_status st = guarded(c, [&] {
        if (p && !pods) fail(QS_EINVAL, "null pods");
        HIPCHK(hipSetDevice(c->device));
        s = new qs_stream();
        s->p = p;
        s->pods.assign(pods, pods + p);
        for (uint32_t j = 0; j < p; j++) check_pod(pods[j], j);
        ensure_layout(c, pods, p);
        s->shift = c->shift;
        s->wide = c->wide;
        s->feat = feat_of(c->cfg) | (c->wide ? kFeatWide | kFeatExt : 0u);
        bool has_ext = false;
        for (uint32_t j = 0; j < p && !has_ext; j++) has_ext = pods[j].req_ext[0] || pods[j].req_ext[1];
        if (has_ext) s->feat |= kFeatExt;
        s->feat |= res_feat(c->cfg, has_ext) | strat_feat(c, pods, p);
        s->order = qos_order(pods, p, c->cfg.qos_sort != 0);
        {  // the distinct apps of the SPREAD pods (spec S13), in arrival order.  k_persistent relies on
           // this: every SPREAD pod's app is in the row (pick_engine keeps a stream with more than
           // kSpreadApps of them off PERSISTENT); a pod whose app had no slot would be allowed no zone
            std::vector<uint8_t> seen(kMaxApps, 0);
            std::fill(std::begin(s->spread_row), std::end(s->spread_row), -1);
            for (uint32_t j = 0; j < p; j++) {
                // (a hostname-spread pod, spec S15, needs no zone counts and takes no slot)
                if (!pod_spreads(pods[j]) || pod_host_spread(pods[j]) || seen[(uint32_t)pods[j].app]) continue;
                seen[(uint32_t)pods[j].app] = 1;
                if (s->spread_apps < kSpreadApps) s->spread_row[s->spread_apps] = pods[j].app;
                ++s->spread_apps;
            }
        }
        const size_t rb = pod_record_bytes(c->wide);
        std::vector<uint8_t> dp(rb * std::max<uint32_t>(p, 1));
        const bool needx = feat_of(c->cfg) & (kFeatTaint | kFeatAffinity);
        std::vector<DPodX> dx(needx ? std::max<uint32_t>(p, 1) : 1);
        s->soft.assign(p, 0);
        s->hosts.assign(p, 0);
        s->honors.assign(p, 0);
        s->honor_pods = 0;
        s->host_pods = 0;
        s->host_apps = 0;
        std::fill(std::begin(s->host_row), std::end(s->host_row), -1);
        std::vector<uint8_t> host_seen(kMaxApps, 0);
        for (uint32_t k = 0; k < p; k++) {
            const uint32_t j = s->order[k];
            s->soft[k] = pod_soft_spread(pods[j]) ? 1 : 0;
            s->hosts[k] = pod_host_spread(pods[j]) ? 1 : 0;
            s->host_pods += s->hosts[k];
            s->honors[k] = pod_honors(c, pods[j]) ? 1 : 0;
            s->honor_pods += s->honors[k];
            if (s->hosts[k] && !host_seen[(uint32_t)pods[j].app]) {  // the distinct apps, for k_persistent's slots
                host_seen[(uint32_t)pods[j].app] = 1;
                if (s->host_apps < kHostSpreadApps) s->host_row[s->host_apps] = pods[j].app;
                ++s->host_apps;
            }
            compact_pod(c, pods[j], j, c->shift, c->wide, dp.data() + rb * k);
            if (needx) dx[k] = compact_podx(c, pods[j]);
        }
        // runs of byte-identical device records (a Deployment's replicas, the BestEffort tail of a
        // QoS-sorted stream): the resident resolver's uniform windows
        s->run0.resize(p);
        for (uint32_t k = 0; k < p; k++)
            s->run0[k] = k > 0 && std::memcmp(dp.data() + rb * k, dp.data() + rb * (k - 1), rb) == 0 ? s->run0[k - 1] : k;
        const size_t P1 = std::max<uint32_t>(p, 1);
        s->d_pods.ensure(rb * P1);
        s->d_podx.ensure(sizeof(DPodX) * dx.size());
        s->d_node.ensure(4 * P1);
        s->d_key.ensure(8 * P1);
        if (c->cfg.record_timestamps) s->d_stamp.ensure(8 * P1);
        HIPCHK(hipMemcpyAsync(s->d_pods.p, dp.data(), rb * p, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s->d_podx.p, dx.data(), sizeof(DPodX) * dx.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->streams.push_back(s);  // (last: nothing after it throws)
        s->owner = c;
    });
    if (st != QS_OK) {
        delete s;
        return st;
    }
    *out = s;
    return QS_OK;
}

qs_status qs_stream_run(qs_ctx *c, qs_stream *s, qs_mode mode, qs_stats *stats) {
    return guarded(c, [&] {
        if (!s) fail(QS_EINVAL, "null stream");
        if (mode != QS_MODE_EXACT && mode != QS_MODE_BATCHED) fail(QS_EINVAL, "unknown qs_mode");
        if (s->shift != c->shift || s->wide != c->wide) fail(QS_ESTATE, "node table re-laid out after prepare");
        if (mode == QS_MODE_BATCHED && (s->spread_apps != 0 || s->host_pods != 0))
            fail(QS_EINVAL, "QS_MODE_BATCHED does not know topology spread (QS_AA_SPREAD / QS_AA_SPREAD_SOFT / QS_AA_SPREAD_HOSTNAME pods, spec S13-S15): "
                            "run the stream in QS_MODE_EXACT on a context that tracks pod anti-affinity");
        HIPCHK(hipSetDevice(c->device));
        // from here on the device table (and d_node) may change even if this run fails part way
        // (e.g. a resident timeout): invalidate the stream's results and every other stream's FitError
        // replay now; only a successful run sets them again (finish_run)
        s->ran = false;
        s->mode_ran = -1;
        s->uni_given = 0;
        s->aa_ran = false;
        ++c->table_epoch;
        if (!c->dev_valid) upload_table(c);  // recovery after a device fault: rebuild from the mirror
        const uint32_t n = c->m.n, P = s->p;
        const RunKnobs kn;
        const RunPlan plan = plan_run(c, s, mode);
        // the (app, node) counts: brought up to date for a stream that reads them; kept by the tracked
        // SCAN commit alone, so every other run that records pods on a tracking context leaves them stale
        // (k_persistent loads them at entry and keeps its own in LDS)
        if (plan.host_spread && n > 0) ensure_hcount(c);
        if (c->aa_track && !(plan.aa_exact && plan.eng == QS_ENGINE_SCAN)) c->hc_valid = false;
        if (plan.host_spread && plan.eng == QS_ENGINE_PERSISTENT && n > 0 && P > 0)
            HIPCHK(hipMemcpyAsync(c->dt.zcount + (size_t)(kMaxApps + 4) * kMaxZones + 16, s->host_row,
                                  sizeof s->host_row, hipMemcpyHostToDevice, c->stream));
        if (plan.aa_exact && plan.eng == QS_ENGINE_PERSISTENT && n > 0 && P > 0)
            HIPCHK(hipMemcpyAsync(c->dt.zcount + (size_t)(kMaxApps + 1) * kMaxZones, s->spread_row,
                                  sizeof s->spread_row, hipMemcpyHostToDevice, c->stream));
        const RunIo io{s->d_pods.p, s->d_podx.as<DPodX>(), s->d_node.as<int32_t>(), s->d_key.as<uint64_t>(),
                       c->cfg.record_timestamps ? s->d_stamp.as<uint64_t>() : nullptr};
        uint64_t batches = 0;
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        // config.profile_kernels: bracket every launch with events (untimed diagnostic runs)
        KernelTimer kt(c->cfg.profile_kernels != 0, c->stream, c->stream2);
        HIPCHK(hipEventRecord(e0, c->stream));
        if (P > 0 && n == 0) {
            HIPCHK(hipMemsetAsync(io.on, 0xFF, 4 * (size_t)P, c->stream));
            HIPCHK(hipMemsetAsync(io.ok, 0, 8 * (size_t)P, c->stream));
        } else if (P > 0) {
            switch (plan.eng) {
            case QS_ENGINE_BATCHED: batches = run_batched(c, s, io, kn, kt); break;
            case QS_ENGINE_PERSISTENT:
                kt.begin(0, c->stream);
                HIPCHK(launch_persistent(c->dt, io.dp, io.dx, P, c->dc, io.on, io.ok, io.st, c->stream));
                kt.end(0, c->stream);
                batches = 1;
                break;
            case QS_ENGINE_SCAN: batches = run_scan(c, s, io, plan.aa_exact, kt); break;
            case QS_ENGINE_ALLREDUCE: batches = run_allreduce(c, s, io, kt); break;
            default: batches = run_lookahead(c, s, io, kn, kt); break;
            }
        }
        HIPCHK(hipEventRecord(e1, c->stream));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        finish_run(c, s, mode, plan, kn, kt, batches, ms, stats);
    });
}

qs_status qs_stream_results(qs_ctx *c, qs_stream *s, int32_t *placement, uint64_t *best_key) {
    return guarded(c, [&] {
        if (!s || !s->ran) fail(QS_ESTATE, "stream has not run");
        HIPCHK(hipSetDevice(c->device));
        const uint32_t P = s->p;
        std::vector<int32_t> node(P);
        std::vector<uint64_t> key(P);
        if (P) {
            HIPCHK(hipMemcpyAsync(node.data(), s->d_node.p, 4 * (size_t)P, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(key.data(), s->d_key.p, 8 * (size_t)P, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        for (uint32_t k = 0; k < P; k++) {
            const uint32_t j = s->order[k];
            if (placement) placement[j] = node[k];
            if (best_key) best_key[j] = key[k];
        }
    });
}

qs_status qs_stream_free(qs_ctx *c, qs_stream *s) {
    (void)c;
    if (s && s->owner) {  // (nullptr: its context closed first, qs_close detached it)
        std::lock_guard<std::mutex> lk(s->owner->mu);
        auto &v = s->owner->streams;
        v.erase(std::remove(v.begin(), v.end(), s), v.end());
    }
    delete s;
    return QS_OK;
}

qs_status qs_table_save(qs_ctx *c) {
    return guarded(c, [&] {
        if (!c->dev_valid) fail(QS_ESTATE, "no node table loaded");
        HIPCHK(hipSetDevice(c->device));
        sync_mirror(c);
        c->tbl_saved.ensure(c->tbl.bytes);
        HIPCHK(hipMemcpyAsync(c->tbl_saved.p, c->tbl.p, c->tbl.bytes, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->m_saved = c->m;
        c->saved_wide = c->wide;
        c->saved_shift = c->shift;
        c->saved = true;
    });
}

qs_status qs_table_restore(qs_ctx *c) {
    return guarded(c, [&] {
        if (!c->saved || !c->dev_valid || c->tbl_saved.bytes != c->tbl.bytes || c->saved_wide != c->wide ||
            c->saved_shift != c->shift)
            fail(QS_ESTATE, "no matching qs_table_save snapshot");
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemcpyAsync(c->tbl.p, c->tbl_saved.p, c->tbl.bytes, hipMemcpyDeviceToDevice, c->stream));
        write_spread_cfg(c);      // (the snapshot holds the topology spread weight of its save, and the
                                  // address of the (app, node) counts of its save)
        c->hc_valid = false;      // (rebuilt from the mirror reinstated below, spec S15)
        c->m = c->m_saved;        // the mirror of the snapshot (the pod registry and its counter with it, spec S18)
        reg_resort(c);            // (under the policy of now)
        c->zero_alloc = count_zero_alloc(c->m);
        c->mirror_stale = false;
        ++c->table_epoch;
        c->soa_valid = false;     // the SoA copy is rebuilt from the restored rows on demand
    });
}

qs_status qs_schedule_stream(qs_ctx *c, const qs_pod *pods, uint32_t p, qs_mode mode,
                             int32_t *placement, qs_stats *stats) {
    using clk = std::chrono::steady_clock;
    auto t0 = clk::now();
    qs_stream *s = nullptr;
    qs_status st = qs_stream_prepare(c, pods, p, &s);
    if (st != QS_OK) return st;
    auto t1 = clk::now();
    qs_stats local{};
    st = qs_stream_run(c, s, mode, &local);
    if (st != QS_OK) { qs_stream_free(nullptr, s); return st; }
    auto t2 = clk::now();
    st = qs_stream_results(c, s, placement, nullptr);
    if (st == QS_OK && c->cfg.record_timestamps && p > 1) {
        std::vector<uint64_t> stamps(p);
        if (hipMemcpy(stamps.data(), s->d_stamp.p, 8 * (size_t)p, hipMemcpyDeviceToHost) == hipSuccess)
            percentile_stats(stamps, &local);
    }
    auto t3 = clk::now();
    for (uint32_t j = 0; j < p && st == QS_OK; j++) {
        if (placement[j] >= 0) local.placed++;
        else local.unschedulable++;
    }
    qs_status st2 = qs_stream_free(c, s);
    if (st == QS_OK) st = st2;
    local.h2d_s = std::chrono::duration<double>(t1 - t0).count();
    local.d2h_s = std::chrono::duration<double>(t3 - t2).count();
    if (stats) *stats = local;
    return st;
}

size_t qs_struct_size(int which) {
    switch (which) {
        case 0: return sizeof(qs_config);
        case 1: return sizeof(qs_node_soa);
        case 2: return sizeof(qs_node_row);
        case 3: return sizeof(qs_pod);
        case 4: return sizeof(qs_container);
        case 5: return sizeof(qs_stats);
        case 6: return sizeof(qs_scoring_strategy);
        case 7: return sizeof(qs_victim);
        default: return 0;
    }
}

// FitError diagnosis (UP framework/types.go#FitError): the table at each requested pod's turn is the
// run's initial table (the final mirror minus every placed pod's delta) plus the deltas of the pods
// placed before it in stream order; each node's reasons follow spec S4/S5's filters in upstream's
// default order, NodeResourcesFit listing every insufficient resource (UP fit.go#fitsRequest).
// counts: m x QS_FIT_REASONS; tcounts (nullable): m x 64, the QS_FIT_TAINT nodes split by the first
// untolerated taint bit (the lowest set bit of taint_hard & ~tol_hard)
static qs_status fit_errors(qs_ctx *c, qs_stream *s, const uint32_t *pods, uint32_t mreq, uint32_t *counts,
                            uint32_t *tcounts) {
    return guarded(c, [&] {
        if (!s || !s->ran) fail(QS_ESTATE, "stream has not run");
        if (s->mode_ran != QS_MODE_EXACT) fail(QS_EINVAL, "FitError diagnosis covers exact streams");
        if (s->aa_ran)
            fail(QS_EINVAL, "FitError diagnosis does not cover streams run with pod anti-affinity tracking (the replay "
                            "would need the anti-affinity state at every pod's turn)");
        if (s->epoch_after != c->table_epoch) fail(QS_ESTATE, "the node table changed after the stream's run");
        if (mreq && (!pods || !counts)) fail(QS_EINVAL, "null pods / counts");
        const uint32_t P = s->p;
        for (uint32_t q = 0; q < mreq; q++)
            if (pods[q] >= P) fail(QS_EINVAL, "pod index out of range");
        std::memset(counts, 0, sizeof(uint32_t) * QS_FIT_REASONS * (size_t)mreq);
        if (tcounts) std::memset(tcounts, 0, sizeof(uint32_t) * 64 * (size_t)mreq);
        if (!mreq) return;
        HIPCHK(hipSetDevice(c->device));
        sync_mirror(c);
        std::vector<int32_t> node(P);
        if (P) HIPCHK(hipMemcpy(node.data(), s->d_node.p, 4 * (size_t)P, hipMemcpyDeviceToHost));
        // stream position -> requested slots (a pod may be requested twice)
        std::vector<std::vector<uint32_t>> want(P);
        std::vector<uint32_t> pos_of(P);
        for (uint32_t k = 0; k < P; k++) pos_of[s->order[k]] = k;
        for (uint32_t q = 0; q < mreq; q++) want[pos_of[pods[q]]].push_back(q);
        Mirror m = c->m;
        for (uint32_t k = 0; k < P; k++)
            if (node[k] >= 0) mirror_reserve(m, (uint32_t)node[k], s->pods[s->order[k]], -1);
        const bool taint = c->cfg.enable_taint != 0, aff = c->cfg.enable_affinity != 0;
        auto subset = [](const uint64_t *mask, const uint64_t *bits) {
            return (mask[0] & ~bits[0]) == 0 && (mask[1] & ~bits[1]) == 0;
        };
        for (uint32_t k = 0; k < P; k++) {
            const qs_pod &p = s->pods[s->order[k]];
            if (node[k] < 0 && !want[k].empty()) {
                uint32_t cnt[QS_FIT_REASONS] = {0};
                uint32_t tcnt[64] = {0};
                const bool any_req = p.req_cpu || p.req_mem || p.req_ext[0] || p.req_ext[1];
                for (uint32_t i = 0; i < m.n; i++) {
                    if (taint && (m.th[i] & ~p.tol_hard) != 0) {
                        ++cnt[QS_FIT_TAINT];
                        ++tcnt[__builtin_ctzll(m.th[i] & ~p.tol_hard)];
                        continue;
                    }
                    if (aff) {
                        const uint64_t *lb = &m.lb[2 * (size_t)i];
                        bool ok = subset(p.sel, lb);
                        if (ok && p.n_req_terms > 0) {
                            bool one = false;
                            for (int t = 0; t < p.n_req_terms; t++) one = one || subset(p.req_terms[t], lb);
                            ok = one;
                        }
                        if (!ok) { ++cnt[QS_FIT_AFFINITY]; continue; }
                    }
                    if (m.np[i] + 1 > m.mp[i]) ++cnt[QS_FIT_TOO_MANY_PODS];
                    if (!any_req) continue;
                    if (p.req_cpu > 0 && p.req_cpu > m.ac[i] - m.rc[i]) ++cnt[QS_FIT_CPU];
                    if (p.req_mem > 0 && p.req_mem > m.am[i] - m.rm[i]) ++cnt[QS_FIT_MEMORY];
                    for (int e = 0; e < QS_MAX_EXT; e++) {
                        const int64_t q = p.req_ext[e];
                        if (q != 0 && q > m.ae[(size_t)i * QS_MAX_EXT + e] - m.re[(size_t)i * QS_MAX_EXT + e])
                            ++cnt[QS_FIT_EXT0 + e];
                    }
                }
                for (uint32_t q : want[k]) {
                    std::memcpy(counts + (size_t)q * QS_FIT_REASONS, cnt, sizeof cnt);
                    if (tcounts) std::memcpy(tcounts + (size_t)q * 64, tcnt, sizeof tcnt);
                }
            }
            if (node[k] >= 0) mirror_reserve(m, (uint32_t)node[k], p, +1);
        }
    });
}

qs_status qs_stream_fit_errors(qs_ctx *c, qs_stream *s, const uint32_t *pods, uint32_t mreq, uint32_t *counts) {
    return fit_errors(c, s, pods, mreq, counts, nullptr);
}

qs_status qs_stream_fit_taints(qs_ctx *c, qs_stream *s, const uint32_t *pods, uint32_t mreq, uint32_t *counts,
                               uint32_t *taint_counts) {
    if (!taint_counts && mreq) return QS_EINVAL;
    return fit_errors(c, s, pods, mreq, counts, taint_counts);
}

qs_status qs_stream_stamps(qs_ctx *c, qs_stream *s, uint64_t *stamps) {
    return guarded(c, [&] {
        if (!s || !s->ran || !s->d_stamp.p) fail(QS_ESTATE, "no timestamps recorded");
        HIPCHK(hipMemcpy(stamps, s->d_stamp.p, 8 * (size_t)s->p, hipMemcpyDeviceToHost));
    });
}

qs_status qs_stream_uniform_windows(qs_ctx *c, qs_stream *s, uint32_t *windows) {
    return guarded(c, [&] {
        if (!s || !windows) fail(QS_EINVAL, "null stream or output");
        *windows = s->ran ? s->uni_given : 0u;
    });
}

}  // extern "C"
