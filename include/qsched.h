/*
 * qsched.h — C ABI of libqsched.so, the MI355X (gfx950) scheduling core.
 *
 * This is the drop-in boundary: the surface a kube-scheduler framework plugin
 * binds through cgo (or any FFI).  Plain C types only — no HIP, no torch, no C++.
 *
 * What each entry point replaces (upstream kube-scheduler v1.32, `UP <path>#<symbol>`; the mounted
 * reference /root/reference/README.md:1 is a title line, so there is no reference-side FFI to cite
 * beyond the north_star's "thin cgo C-ABI" in BASELINE.json:5):
 *   qs_open / qs_close        framework.Handle-scoped plugin state (UP cmd/kube-scheduler/app#WithPlugin
 *                             factory `func(ctx, runtime.Object, framework.Handle) (framework.Plugin, error)`)
 *   qs_set_scoring_strategy   NodeResourcesFitArgs.ScoringStrategy.Type / RequestedToCapacityRatio.Shape
 *                             (UP apis/config/types_pluginargs.go#ScoringStrategy; noderesources/fit.go#NewFit
 *                             picks the scorer from nodeResourceStrategyTypeMap)
 *   qs_set_scoring_strategy_qos  the same of one QoS class: upstream gives every KubeSchedulerProfile its own
 *                             NodeResourcesFitArgs.ScoringStrategy (UP apis/config/types.go#KubeSchedulerProfile.
 *                             PluginConfig; profile.NewMap builds one framework, and so one Fit instance, per
 *                             profile), and a QoS class is one profile here (spec S9)
 *   qs_nodes_load             Cache.UpdateSnapshot → Snapshot NodeInfo list (UP backend/cache#Snapshot)
 *   qs_node_upsert            per-NodeInfo Generation diff (UP framework/types.go#NodeInfo.Generation)
 *   qs_score_pod              PreFilter+Filter+PreScore+Score+NormalizeScore for ALL nodes of one pod
 *                             (UP framework/interface.go#{PreFilterPlugin,FilterPlugin,ScorePlugin,
 *                             ScoreExtensions}; UP schedule_one.go#{findNodesThatPassFilters,prioritizeNodes})
 *   qs_reserve / qs_unreserve ReservePlugin.Reserve / Unreserve → NodeInfo.AddPod / RemovePod
 *                             (UP framework/interface.go#ReservePlugin, framework/types.go#NodeInfo.update)
 *   qs_preempt_pod / qs_evict PostFilter of DefaultPreemption: the dry run over every node and the choice
 *                             (UP plugins/defaultpreemption#SelectVictimsOnNode, framework/preemption/
 *                             preemption.go#pickOneNodeForPreemption; spec/semantics.md S18)
 *   qs_schedule_stream        ScheduleOne loop with deterministic selectHost (UP schedule_one.go#
 *                             {ScheduleOne,schedulingCycle,selectHost,assume}; spec/semantics.md S7/S8)
 *
 * Semantics: spec/semantics.md.  Ownership: every pointer argument is borrowed for the duration of
 * the call only (cgo rule: C never retains Go pointers); outputs go to caller-allocated arrays of
 * the stated length.  Quantities are canonical int64 (millicores, bytes, counts).  Errors are
 * return codes, never exceptions or aborts; `qs_last_error` holds the message.  Unschedulable is
 * not an error: placement −1.  Threading: one mutex per context serialises every call.
 */
#ifndef QSCHED_H
#define QSCHED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define QS_API __attribute__((visibility("default")))
#else
#define QS_API
#endif

#define QS_ABI_VERSION 3
#define QS_MAX_EXT 2   /* extended resources per node/pod (e.g. amd.com/gpu) */
#define QS_MAX_TERMS 4 /* node-affinity terms per pod (required OR-terms, preferred terms) */
#define QS_MAX_APPS 1024 /* anti-affinity groups (batched mode, spec S11) */
#define QS_MAX_ZONES 64  /* topology zones (batched mode zone anti-affinity) */
#define QS_MAX_SCORE_RES 4 /* entries of a scoring-resource list (cpu, memory, ext 0, ext 1) */

typedef enum qs_status {
    QS_OK = 0,
    QS_EINVAL = 1,   /* bad argument / input outside the device layout's range */
    QS_EDEVICE = 2,  /* HIP or RCCL failure (message in qs_last_error) */
    QS_ETIMEOUT = 3, /* an in-kernel wait (lookahead lists, resident hand-off, mailbox peer) hit its
                        0.5 s bound; the run is void and the device table rebuilt from the mirror */
    QS_ENOMEM = 4,
    QS_ESTATE = 5 /* call out of order (e.g. no nodes loaded) */
} qs_status;

typedef enum qs_qos { QS_QOS_BESTEFFORT = 0, QS_QOS_BURSTABLE = 1, QS_QOS_GUARANTEED = 2 } qs_qos;

typedef enum qs_mode { QS_MODE_EXACT = 0, QS_MODE_BATCHED = 1 } qs_mode;

/* Required pod anti-affinity to the pod's own app group (the subset of UP plugins/interpodaffinity
 * that config 5 uses): none, per node (topologyKey hostname), per zone.  QS_MODE_BATCHED always
 * honours it (spec S11); exact streams, qs_score_pod and qs_reserve / qs_unreserve honour it on a
 * context that tracks it (qs_set_pod_anti_affinity, spec S12) and ignore it otherwise.
 * QS_AA_SPREAD_ZONE (spec S13) is the zone topologySpreadConstraint with whenUnsatisfiable:
 * DoNotSchedule over the pod's own app (UP plugins/podtopologyspread Filter; nodeAffinityPolicy Ignore
 * unless qs_set_topology_spread_node_affinity_policy says HONOR (spec S16), nodeTaintsPolicy Ignore
 * unless qs_set_topology_spread_node_taints_policy says HONOR (spec S17),
 * minDomains unset): a node is infeasible when taking it would leave its zone
 * more than max_skew pods of the app above the emptiest zone that holds a node of the table.  The kind
 * sits in the low byte of qs_pod.anti_affinity and max_skew (1..31) in bits 8-12: QS_AA_SPREAD(max_skew).
 * Upper bits must be zero for the other kinds; a pod has one kind.  Honoured like the other kinds on a
 * context that tracks; QS_MODE_BATCHED refuses a stream that holds such a pod (QS_EINVAL).
 * QS_AA_SPREAD_SOFT(max_skew) (spec S14) is the same constraint with whenUnsatisfiable: ScheduleAnyway
 * (UP plugins/podtopologyspread Score / NormalizeScore): kind 3 with the flag QS_AA_SOFT above max_skew.
 * Such a pod is not filtered by spread; on a context that tracks, every feasible node's total gains
 * Wpts * PTS(zone of the node), PTS in 0..100 from the app's recorded pods per zone over the zones that
 * hold a node feasible for the pod (qs_set_topology_spread_weight; qs_score_pod_zone_scores).
 * QS_AA_SPREAD_HOSTNAME(max_skew) (spec S15) is the DoNotSchedule constraint with topologyKey
 * kubernetes.io/hostname: kind 3 with the flag QS_AA_HOSTKEY, every node a domain of its own.  A node
 * is infeasible when taking it would leave it more than max_skew pods of the app above the emptiest
 * node of the table, whether the pod could take that node or not.  Exact streams run QS_ENGINE_PERSISTENT
 * for up to 16 distinct such apps per stream and no QS_AA_SPREAD_SOFT pod in the same stream (beyond
 * that AUTO runs SCAN and an explicit PERSISTENT returns QS_EINVAL) or QS_ENGINE_SCAN; the flag together with
 * QS_AA_SOFT, or on another kind, is QS_EINVAL; QS_MODE_BATCHED refuses the stream.  The context keeps
 * 2 KB of counts per node from the first such pod on: tables above 2^19 nodes, and tables with a node
 * whose max_pods exceeds 65,535, refuse the pod (QS_EINVAL). */
typedef enum qs_anti_affinity {
    QS_AA_NONE = 0, QS_AA_HOSTNAME = 1, QS_AA_ZONE = 2, QS_AA_SPREAD_ZONE = 3
} qs_anti_affinity;
#define QS_AA_SPREAD(max_skew) ((int32_t)(QS_AA_SPREAD_ZONE | ((max_skew) << 8)))
#define QS_AA_KIND(x) ((int32_t)((x) & 0xFF))
#define QS_AA_MAX_SKEW(x) ((int32_t)(((x) >> 8) & 0x1F))
#define QS_MAX_SPREAD_SKEW 31
#define QS_AA_SOFT ((int32_t)0x10000) /* only with QS_AA_SPREAD_ZONE: ScheduleAnyway (spec S14) */
#define QS_AA_SPREAD_SOFT(max_skew) ((int32_t)(QS_AA_SPREAD(max_skew) | QS_AA_SOFT))
#define QS_AA_IS_SOFT(x) ((int32_t)(((x) >> 16) & 1))
#define QS_AA_HOSTKEY ((int32_t)0x40000) /* bit 18 (bit 17 alone stays invalid); only with QS_AA_SPREAD_ZONE, without QS_AA_SOFT: the spread key is the node (spec S15) */
#define QS_AA_SPREAD_HOSTNAME(max_skew) ((int32_t)(QS_AA_SPREAD(max_skew) | QS_AA_HOSTKEY))
#define QS_AA_IS_HOSTKEY(x) ((int32_t)(((x) >> 18) & 1))

/* Scoring resources (spec/semantics.md S5 "Scoring resources"): cpu, memory, or one of the table's
 * two extended-resource columns (the caller interns e.g. "amd.com/gpu" as QS_RES_EXT0). */
typedef enum qs_resource { QS_RES_NONE = 0, QS_RES_CPU = 1, QS_RES_MEMORY = 2, QS_RES_EXT0 = 3, QS_RES_EXT1 = 4 } qs_resource;
/* One entry of NodeResourcesFitArgs.ScoringStrategy.Resources (UP apis/config#ResourceSpec{Name, Weight}). */
typedef struct qs_resource_spec {
    int32_t resource; /* qs_resource */
    int32_t weight;   /* 1..100 (UP apis/config/validation#validateResources) */
} qs_resource_spec;

/* NodeResourcesFitArgs.ScoringStrategy.Type (UP apis/config/types_pluginargs.go#ScoringStrategyType;
 * spec/semantics.md S5 "Scoring strategies"): LeastAllocated spreads (UP noderesources/
 * least_allocated.go#leastResourceScorer), MostAllocated bin-packs (UP most_allocated.go#
 * mostResourceScorer), RequestedToCapacityRatio scores each resource's utilisation through a
 * piecewise-linear shape (UP requested_to_capacity_ratio.go#requestedToCapacityRatioScorer,
 * helper/shape_score.go#BuildBrokenLinearFunction). */
typedef enum qs_scoring_strategy_type {
    QS_STRATEGY_LEAST_ALLOCATED = 0,
    QS_STRATEGY_MOST_ALLOCATED = 1,
    QS_STRATEGY_REQUESTED_TO_CAPACITY_RATIO = 2
} qs_scoring_strategy_type;
/* One point of RequestedToCapacityRatioParam.Shape (UP apis/config#UtilizationShapePoint):
 * utilization 0..100 strictly increasing along the shape, score 0..10 (MaxCustomPriorityScore). */
typedef struct qs_shape_point {
    int32_t utilization, score;
} qs_shape_point;
#define QS_MAX_SHAPE 16
typedef struct qs_scoring_strategy {
    int32_t type;    /* qs_scoring_strategy_type */
    int32_t n_shape; /* RequestedToCapacityRatio: 1..QS_MAX_SHAPE points; 0 for the other types */
    qs_shape_point shape[QS_MAX_SHAPE];
} qs_scoring_strategy;

/* Which device engine runs the exact stream (all are bit-exact; AUTO picks the fastest). */
typedef enum qs_engine {
    QS_ENGINE_AUTO = 0,
    QS_ENGINE_PERSISTENT = 1, /* one resident workgroup, node rows in registers (N <= 8192) */
    QS_ENGINE_SCAN = 2,       /* per-pod grid scan + finalize/reserve launch chain (any N) */
    QS_ENGINE_LOOKAHEAD = 3,  /* exact top-K lookahead: chip-wide stale scan + sequential resolve */
    QS_ENGINE_BATCHED = 4,    /* reported by qs_stats.engine_used for QS_MODE_BATCHED streams */
    QS_ENGINE_ALLREDUCE = 5   /* sharded contexts with an RCCL communicator: per pod every rank scans its
                                 node shard and the ranks max-reduce one packed key with
                                 ncclAllReduce(count 1, ncclUint64, ncclMax) (+ the two normalize maxima for
                                 TaintToleration / NodeAffinity); the as-is RCCL baseline of SURVEY.md §8(e) C1 */
} qs_engine;

typedef struct qs_config {
    uint32_t abi_version;        /* = QS_ABI_VERSION */
    int32_t engine;              /* qs_engine */
    int64_t fit_weight_cpu;      /* NodeResourcesFitArgs.ScoringStrategy.Resources cpu weight (1) */
    int64_t fit_weight_mem;      /* ... memory weight (1) */
    int32_t w_fit[3];            /* NodeResourcesFit plugin weight per QoS class [BE, Bu, G] */
    int32_t w_bal[3];            /* NodeResourcesBalancedAllocation weight per QoS class */
    int32_t w_taint;             /* TaintToleration weight (3) */
    int32_t w_affinity;          /* NodeAffinity weight (2) */
    int32_t enable_taint;        /* TaintToleration filter+score on */
    int32_t enable_affinity;     /* NodeAffinity filter+score on */
    int32_t balanced_skip_besteffort; /* 0 = v1.32 behaviour */
    int32_t qos_sort;            /* 1 = QoSSort order (spec S8), 0 = arrival order */
    int32_t lookahead;           /* pods per lookahead window (0 = default) */
    int32_t record_timestamps;   /* 1 = per-pod device timestamps for p50/p99 cycle latency */
    int32_t profile_kernels;     /* 1 = time every kernel launch with HIP events (qs_stats.kernel_s) */
    int32_t virtual_shards;      /* >1: run the sharded LOOKAHEAD protocol with this many node shards
                                    inside one process (no collective; parity testing of the
                                    multi-GPU layout on one device).  Ignored by qs_open_shard. */
    int32_t lookahead_serial;    /* 1 = LOOKAHEAD windows back to back; 0 (default) = the select of
                                    window w+1 overlaps the resolve of window w (needs lookahead <= 32) */
    int32_t scan_soa_min_nodes;  /* tables with at least this many nodes also keep the column-major
                                    copy the SCAN engine / qs_score_pod stream (0 = 65,536; -1 never) */
    int32_t batch_pods;          /* QS_MODE_BATCHED: pods per batch (0 = 64; at most 64) */
    /* NodeResourcesFitArgs.ScoringStrategy.Resources of the LeastAllocated strategy, in list order
     * (replaces UP apis/config/types_pluginargs.go#ScoringStrategy.Resources); 0 entries = the
     * default [cpu: fit_weight_cpu, memory: fit_weight_mem].  Distinct resources, weights 1..100. */
    int32_t n_fit_resources;
    qs_resource_spec fit_resources[QS_MAX_SCORE_RES];
    /* NodeResourcesBalancedAllocationArgs.Resources in list order (UP types_pluginargs.go#
     * NodeResourcesBalancedAllocationArgs); 0 entries = the default [cpu, memory].  With three or
     * more resources requested the score takes the mean / sqrt standard deviation (spec S5). */
    int32_t n_balanced_resources;
    int32_t balanced_resources[QS_MAX_SCORE_RES]; /* qs_resource */
    int32_t reserved[3];
} qs_config;

/* Canonical node table, structure of arrays, n entries each.  alloc_ext/req_ext are [n][QS_MAX_EXT],
 * label_bits is [n][2], zone is the node's topology zone id (< QS_MAX_ZONES; batched-mode zone
 * anti-affinity).  Optional columns may be NULL (read as 0). */
typedef struct qs_node_soa {
    const int64_t *alloc_cpu, *alloc_mem, *alloc_ext, *max_pods;
    const int64_t *req_cpu, *req_mem, *req_ext, *nz_cpu, *nz_mem, *pods;
    const uint64_t *taint_hard, *taint_soft, *label_bits;
    const int32_t *zone;
} qs_node_soa;

/* Same layout, writable (qs_nodes_read, qs_synth_generate). */
typedef struct qs_node_soa_out {
    int64_t *alloc_cpu, *alloc_mem, *alloc_ext, *max_pods;
    int64_t *req_cpu, *req_mem, *req_ext, *nz_cpu, *nz_mem, *pods;
    uint64_t *taint_hard, *taint_soft, *label_bits;
    int32_t *zone;
} qs_node_soa_out;

typedef struct qs_node_row {
    int64_t alloc_cpu, alloc_mem, alloc_ext[QS_MAX_EXT], max_pods;
    int64_t req_cpu, req_mem, req_ext[QS_MAX_EXT], nz_cpu, nz_mem, pods;
    uint64_t taint_hard, taint_soft, label_bits[2];
    int32_t zone, reserved;
} qs_node_row;

/* One pod, precomputed on the host (spec S2/S3; qs_pod_from_containers helps). */
typedef struct qs_pod {
    int64_t req_cpu, req_mem, req_ext[QS_MAX_EXT]; /* effective requests, missing -> 0 */
    int64_t nz_cpu, nz_mem;                        /* non-zero requests (defaults 100m / 200Mi) */
    int32_t qos;                                   /* qs_qos */
    int32_t priority;
    uint64_t tol_hard; /* interned taint bits tolerated for NoSchedule/NoExecute */
    uint64_t tol_soft; /* interned taint bits tolerated for PreferNoSchedule */
    uint64_t sel[2];   /* nodeSelector requirement bits (all must hold) */
    int32_t n_req_terms, n_pref_terms;
    uint64_t req_terms[QS_MAX_TERMS][2];  /* required node-affinity terms (OR of ANDs) */
    uint64_t pref_terms[QS_MAX_TERMS][2]; /* preferred terms */
    int32_t pref_weight[QS_MAX_TERMS];
    int32_t app;           /* anti-affinity group (< QS_MAX_APPS); with tracking on (spec S12) every
                              placed pod is recorded under it, whatever its anti_affinity */
    int32_t anti_affinity; /* qs_anti_affinity: required anti-affinity to the pod's own app (batched
                              mode; exact mode and the score path with tracking on, else ignored), or
                              QS_AA_SPREAD(max_skew): zone topology spread (spec S13; exact mode and the
                              score path with tracking on, else ignored; refused by batched mode) */
} qs_pod;

/* One container of a pod spec for qs_pod_from_containers (spec S2/S3). has_* = 0 means missing. */
typedef struct qs_container {
    int32_t kind; /* 0 regular, 1 init, 2 restartable init (sidecar) */
    int32_t has_req_cpu, has_req_mem, has_lim_cpu, has_lim_mem;
    int64_t req_cpu, req_mem, lim_cpu, lim_mem;
    int64_t req_ext[QS_MAX_EXT];
} qs_container;

typedef struct qs_stats {
    uint64_t pods, placed, unschedulable, evals;
    uint64_t batches, truncations;  /* lookahead windows run / pods resolved by an exact full
                                       rescan (normalizing profiles: a normalize maximum lost) */
    double wall_s;                  /* qs_stream_run wall, device-resident inputs */
    double h2d_s, d2h_s;            /* host<->device copies around it (qs_schedule_stream) */
    double p50_cycle_us, p99_cycle_us, max_cycle_us; /* per-pod decision interval (record_timestamps) */
    int32_t engine_used;
    int32_t table_layout;           /* device layout that ran: 0 compact (int32 columns, memory in
                                       2^u-byte units < 2^24), 1 wide (f64 memory columns in bytes) */
    uint64_t resumed_windows;       /* normalizing LOOKAHEAD: windows stopped for an exact rescan */
    uint64_t device_faults;         /* QS_EDEVICE results of this context so far (each one drops
                                       the device table; the next call rebuilds it from the mirror) */
    int32_t resident;               /* 1: LOOKAHEAD ran as one resident launch (resolver + selector
                                       workgroups, k_la_stream_res); 0: per-window launches */
    int32_t resident_path;          /* resident launch only, else 0: bit 0 the resolver ran with 32-bit
                                       keys end to end (ring form; QS_RES_K32=0 clears it), bit 1 its key
                                       waves ran without the zero-allocatable terms (no node with
                                       allocatable cpu or memory 0; QS_FAST_ALLOC=0 clears it) */
    /* per-kernel device time (config.profile_kernels = 1; HIP events on the library's stream):
     * [0] persistent, [1] scan (all per-pod kernels), [2] lookahead select, [3] lookahead resolve
     * (a resident stream is one launch, counted under [3]) */
    double kernel_s[4];
    uint64_t kernel_launches[4];
} qs_stats;

typedef struct qs_ctx qs_ctx;
typedef struct qs_stream qs_stream;

/* ---- lifecycle ---- */
QS_API void qs_config_default(qs_config *cfg);
QS_API qs_status qs_open(const qs_config *cfg, int device, qs_ctx **out);
/* Sharded context for one rank of `world` (one process per GPU, world <= 16).  nccl_id = 128 bytes
 * from qs_dist_unique_id on rank 0, broadcast by the caller (any out-of-band channel); NULL selects
 * the peer-memory mailbox transport instead (qs_dist_mailbox_connect before the first stream).  Every rank
 * loads the SAME full node table (qs_nodes_load) and the SAME pod stream; rank r scores only its
 * contiguous node shard [r*n/world, (r+1)*n/world), the per-window top-L lists are exchanged with
 * one RCCL all-gather over xGMI, and every rank resolves the window identically, so placements and
 * the node table stay identical on all ranks.  Collective calls happen inside
 * qs_stream_run: all ranks must call it with the same stream. */
QS_API qs_status qs_open_shard(const qs_config *cfg, int device, int rank, int world,
                        const uint8_t nccl_id[128], qs_ctx **out);
QS_API qs_status qs_dist_unique_id(uint8_t out[128]);
/* Peer-memory mailbox transport, the alternative to RCCL: open
 * every rank with qs_open_shard(..., nccl_id = NULL, ...), call qs_dist_mailbox_export on each rank
 * (allocates this rank's ~5 MB mailbox and returns its 64-byte IPC handle), exchange the handles
 * out of band, and call qs_dist_mailbox_connect with all `world` handles in rank order.  Per
 * lookahead window every rank then writes its list block (and, for TaintToleration/NodeAffinity
 * profiles, its partial maxima) straight into every peer's mailbox over xGMI and raises a flag
 * there (one hop), instead of an RCCL all-gather; a peer that never posts makes the run return
 * QS_ETIMEOUT (bound: 5 s for a run's first window, 0.5 s for the others).  All ranks must run the
 * same streams in the same order.  After QS_ETIMEOUT the ranks are out of step: every later run
 * returns QS_ESTATE until every rank has called qs_dist_mailbox_connect again (the caller places a
 * barrier of its own before and after that call on every rank), which restarts all mailboxes empty.
 * Replaces (with qs_open_shard) the per-pod ncclAllReduce exchange of SURVEY.md §8(e). */
QS_API qs_status qs_dist_mailbox_export(qs_ctx *ctx, uint8_t handle[64]);
QS_API qs_status qs_dist_mailbox_connect(qs_ctx *ctx, const uint8_t *handles /* world x 64 bytes */);
/* The scoring strategy of NodeResourcesFit for every later call on the context (qs_score_pod, streams
 * prepared afterwards, every exact engine); a new context scores LeastAllocated.  The resources and
 * weights stay those of qs_config (fit_resources, or fit_weight_cpu / fit_weight_mem); BalancedAllocation
 * is untouched.  QS_ESTATE while the context holds prepared streams (free them first); QS_EINVAL for an
 * unknown type, a bad shape (empty, more than QS_MAX_SHAPE points, utilization outside 0..100 or not
 * strictly increasing, score outside 0..10), or a shape given for a type that takes none.
 * QS_MODE_BATCHED runs LeastAllocated only: with another strategy set qs_stream_run returns QS_EINVAL. */
QS_API qs_status qs_set_scoring_strategy(qs_ctx *ctx, const qs_scoring_strategy *s);
/* The scoring strategy of one QoS class (qos 0 BestEffort, 1 Burstable, 2 Guaranteed; spec S9 "Strategy
 * per QoS class"): the fit score of a pod on every node is computed with the strategy of the pod's class,
 * type and shape both.  qs_set_scoring_strategy above sets all three classes.  The same validation and
 * QS_ESTATE rule; QS_EINVAL for qos outside 0..2.  A stream whose pods all belong to LeastAllocated
 * classes runs the kernels a default context runs.  QS_MODE_BATCHED returns QS_EINVAL while any class
 * has another strategy.  qs_get_scoring_strategy_qos returns what is stored for the class. */
QS_API qs_status qs_set_scoring_strategy_qos(qs_ctx *ctx, int32_t qos, const qs_scoring_strategy *s);
QS_API qs_status qs_get_scoring_strategy_qos(qs_ctx *ctx, int32_t qos, qs_scoring_strategy *out);
/* Required pod anti-affinity on the exact engines and the score path (spec S12), per context, off in a
 * new context (nothing changes anywhere while it is off).  on != 0: every later exact stream and
 * qs_score_pod call filters HOSTNAME / ZONE pods against the recorded (app, node) / (app, zone) state
 * (an infeasible node takes no part in the TaintToleration / NodeAffinity maxima), and every pod placed
 * by an exact or batched stream or by qs_reserve is recorded under its app; qs_unreserve removes one.
 * The state is that of batched mode on the same context (shared), empty after qs_nodes_load, kept by
 * qs_table_save / qs_table_restore and rebuilt after a device fault; switching tracking on or off does
 * not clear it, and nothing is recorded while it is off.  That holds for the host's record, from which
 * qs_unreserve, the zone rule below and every rebuild of the device state work; a batched stream still
 * marks the device state with tracking off (S11, as before), so pods it places then filter later pods
 * until the table is re-laid out or rebuilt, but qs_unreserve does not know them (QS_EINVAL) and a zone
 * change of their node is not refused.  Switch tracking on before the first stream whose pods should
 * count.  QS_AA_SPREAD(max_skew) pods (spec S13) filter against the same (app, zone) counts: every
 * recorded pod of the app counts, whatever its kind, and the minimum runs over the zones that hold a node
 * of the table (a qs_node_upsert that opens a new zone lowers it to 0).  Exact streams then run
 * QS_ENGINE_PERSISTENT (tables that fit it, and streams whose SPREAD pods belong to at most 64 distinct
 * apps; beyond that AUTO runs SCAN and an explicit PERSISTENT returns QS_EINVAL)
 * or QS_ENGINE_SCAN; an explicit QS_ENGINE_LOOKAHEAD / QS_ENGINE_ALLREDUCE makes
 * qs_stream_run return QS_EINVAL, as do qs_stream_fit_errors / qs_stream_fit_taints of a tracked run and
 * a qs_node_upsert that moves a node holding recorded pods to another zone.  QS_ESTATE while the context
 * holds prepared streams; QS_EINVAL (switching on) on a sharded context (qs_open_shard, virtual_shards
 * > 1) or when the loaded table keeps no anti-affinity state (more than 2^20 nodes), and for a null
 * output pointer. */
QS_API qs_status qs_set_pod_anti_affinity(qs_ctx *ctx, int32_t on);
QS_API qs_status qs_get_pod_anti_affinity(qs_ctx *ctx, int32_t *on);
/* Weight of the PodTopologySpread score (spec S14: Wpts, UP apis/config/v1/default_plugins.go weight 2)
 * of the context, 0..100, 2 in a new context.  Only QS_AA_SPREAD_SOFT pods on a context that tracks pod
 * anti-affinity get the term.  QS_ESTATE while the context holds prepared streams; QS_EINVAL outside
 * 0..100 and for null pointers. */
QS_API qs_status qs_set_topology_spread_weight(qs_ctx *ctx, int32_t w);
QS_API qs_status qs_get_topology_spread_weight(qs_ctx *ctx, int32_t *w);
/* nodeAffinityPolicy of the context's topology spread constraints (spec S16; UP
 * apis/core#TopologySpreadConstraint.NodeAffinityPolicy, podtopologyspread/common.go#matchNodeInclusionPolicies,
 * filtering.go#calPreFilterState, scoring.go#PreScore).  QS_POLICY_IGNORE (a new context; spec S13-S15 to
 * the letter): every node of the table counts.  QS_POLICY_HONOR (upstream's default): for a pod with a
 * nodeSelector or required node-affinity terms, only the nodes that pass them (the NodeAffinity filter's
 * predicate) are counted and make up the domains of QS_AA_SPREAD, QS_AA_SPREAD_SOFT and
 * QS_AA_SPREAD_HOSTNAME pods; a pod without either is treated as under IGNORE.  Upstream carries the field
 * per constraint; it is per context here, because qs_pod.anti_affinity has no free bit left that is not
 * already defined as invalid, and a cluster's manifests overwhelmingly share one value.  The policy is
 * read on a context that tracks pod anti-affinity only.  A stream that holds such a restricting spread
 * pod under HONOR runs QS_ENGINE_SCAN (AUTO picks it; an explicit QS_ENGINE_PERSISTENT returns
 * QS_EINVAL), and the context keeps the per-(app, node) counts of QS_AA_SPREAD_HOSTNAME with their limits
 * (tables up to 2^19 nodes, max_pods <= 65,535).  QS_ESTATE while the context holds prepared streams;
 * QS_EINVAL for an unknown policy, a null pointer, a null context, and for HONOR on a context opened with
 * enable_affinity = 0 (Honor presupposes that the NodeAffinity filter removes the nodes the selector does
 * not admit). */
typedef enum qs_node_inclusion_policy { QS_POLICY_IGNORE = 0, QS_POLICY_HONOR = 1 } qs_node_inclusion_policy;
QS_API qs_status qs_set_topology_spread_node_affinity_policy(qs_ctx *ctx, int32_t policy);
QS_API qs_status qs_get_topology_spread_node_affinity_policy(qs_ctx *ctx, int32_t *policy);
/* nodeTaintsPolicy of the context's topology spread constraints (spec S17; UP
 * apis/core#TopologySpreadConstraint.NodeTaintsPolicy, KEP-3094,
 * podtopologyspread/common.go#matchNodeInclusionPolicies, which calls FindMatchingUntoleratedTaint with
 * DoNotScheduleTaintsFilterFunc: NoSchedule and NoExecute taints).  QS_POLICY_IGNORE (a new context, and
 * upstream's default for this field; spec S13-S16 to the letter): tainted nodes count like any other.
 * QS_POLICY_HONOR: for a spread pod, only the nodes whose hard taints it tolerates (taint_hard & ~tol_hard
 * == 0, the TaintToleration filter's predicate) are counted and make up the domains of QS_AA_SPREAD,
 * QS_AA_SPREAD_SOFT and QS_AA_SPREAD_HOSTNAME pods.  Under both policies the node set is the intersection
 * of the two.  A tainted pool that a Deployment cannot use then no longer pins the minimum of its spread
 * at 0.  Like the affinity policy it is per context, and read on a context that tracks pod anti-affinity
 * only.  A pod restricts by taints when ~tol_hard != 0; a stream that holds such a spread pod under HONOR
 * runs QS_ENGINE_SCAN (AUTO picks it; an explicit QS_ENGINE_PERSISTENT returns QS_EINVAL) and the context
 * keeps the per-(app, node) counts with their limits, as under the affinity policy; a pod that tolerates
 * every bit is dispatched as before.  QS_ESTATE while the context holds prepared streams; QS_EINVAL for an
 * unknown policy, a null pointer, a null context, and for HONOR on a context opened with enable_taint = 0
 * (Honor presupposes that the TaintToleration filter removes the nodes outside the set). */
QS_API qs_status qs_set_topology_spread_node_taints_policy(qs_ctx *ctx, int32_t policy);
QS_API qs_status qs_get_topology_spread_node_taints_policy(qs_ctx *ctx, int32_t *policy);
QS_API qs_status qs_close(qs_ctx *ctx);
QS_API const char *qs_last_error(const qs_ctx *ctx);
QS_API const char *qs_version(void);

/* ---- node table (device-resident SoA, host mirror authoritative) ---- */
QS_API qs_status qs_nodes_load(qs_ctx *ctx, const qs_node_soa *nodes, uint32_t n);
QS_API qs_status qs_nodes_read(qs_ctx *ctx, const qs_node_soa_out *out, uint32_t n);
QS_API qs_status qs_node_upsert(qs_ctx *ctx, uint32_t idx, const qs_node_row *row, uint64_t generation);
/* Device-side snapshot of the whole node table (checkpoint/resume; bench resets between steps). */
QS_API qs_status qs_table_save(qs_ctx *ctx);
QS_API qs_status qs_table_restore(qs_ctx *ctx);
/* Reserve / Unreserve of one pod on one node.  With anti-affinity tracking on (spec S12) qs_reserve
 * also records the pod under pod->app on the node, and qs_unreserve removes one pod of that app from
 * it: the (app, zone) count drops by one and the presence bit clears with the node's last pod of the
 * app; unreserving an app with nothing recorded on the node returns QS_EINVAL and changes nothing. */
QS_API qs_status qs_reserve(qs_ctx *ctx, uint32_t node, const qs_pod *pod);
QS_API qs_status qs_unreserve(qs_ctx *ctx, uint32_t node, const qs_pod *pod);

/* ---- preemption dry run (spec S18) ----
 * The pod registry: which pods sit on which node, per context, off in a new context (nothing is recorded
 * and no call changes while it is off; replaces the per-node pod lists of UP framework/types.go#NodeInfo.Pods
 * that UP plugins/defaultpreemption reads).  While it is on, qs_reserve appends the pod it reserves to the
 * node's list and every stream, exact or batched, appends its placed pods in the stream's decision order
 * (on the host after the run, outside wall_s).  An entry carries seq, a context-wide counter from 1 (the
 * stand-in for upstream's pod StartTime), and the pod's priority, qos, app and requests.  Load that
 * qs_nodes_load or qs_node_upsert brought belongs to no entry and is never freed by preemption.
 * qs_nodes_load empties the registry; qs_table_save / qs_table_restore cover it, the counter included;
 * switching it on or off does not clear it.  With the registry on, qs_unreserve removes the entry of the
 * node with the highest seq whose fields equal the pod's (QS_EINVAL, nothing changed, when there is none),
 * and a qs_node_upsert whose requested columns or pod count fall below the sums over the node's entries
 * is QS_EINVAL.  QS_ESTATE while the context holds prepared streams; QS_EINVAL (switching on) on a
 * sharded context (qs_open_shard, virtual_shards > 1) or a table above 2^17 nodes, and for null pointers. */
QS_API qs_status qs_set_preemption(qs_ctx *ctx, int32_t on);
QS_API qs_status qs_get_preemption(qs_ctx *ctx, int32_t *on);
/* How pods rank against each other (spec S18 "Importance"), one policy per context.
 * QS_PREEMPT_BY_PRIORITY (a new context) is upstream's rule, the pod's priority alone
 * (UP framework/preemption/preemption.go, util.MoreImportantPod); QS_PREEMPT_BY_QOS ranks by QoS class
 * first, then priority: the order of spec S8 (QoSSort).  QS_EINVAL for an unknown policy or a null pointer. */
typedef enum qs_preempt_policy { QS_PREEMPT_BY_PRIORITY = 0, QS_PREEMPT_BY_QOS = 1 } qs_preempt_policy;
QS_API qs_status qs_set_preemption_policy(qs_ctx *ctx, int32_t policy);
QS_API qs_status qs_get_preemption_policy(qs_ctx *ctx, int32_t *policy);
/* One registry entry: a pod on a node, and a victim of a dry run. */
typedef struct qs_victim {
    uint64_t seq;
    int64_t req_cpu, req_mem, req_ext[QS_MAX_EXT], nz_cpu, nz_mem;
    int32_t priority, qos, app, reserved;
} qs_victim; /* qs_struct_size(7) */
#define QS_MAX_VICTIMS 256
/* The node's entries, most important first (importance descending, then seq ascending: the order of the
 * dry run's reprieve walk, UP util.MoreImportantPod over NodeInfo.Pods): *n = their number, of which the
 * first min(*n, cap) are written to out (nullable when cap = 0).  QS_EINVAL for a node outside the table. */
QS_API qs_status qs_node_pods(qs_ctx *ctx, uint32_t node, qs_victim *out, uint32_t cap, uint32_t *n);
/* The dry run for one pod over ALL nodes in one device pass (replaces UP plugins/defaultpreemption#
 * DefaultPreemption.PostFilter: framework/preemption#Evaluator.{findCandidates, DryRunPreemption},
 * defaultpreemption#SelectVictimsOnNode without PodDisruptionBudgets, and preemption.go#
 * pickOneNodeForPreemption; no candidate sampling, every node is evaluated).  *node = the chosen node or
 * -1; victims[QS_MAX_VICTIMS] / *n_victims = its victims in walk order; nvict_n (nullable, n entries) =
 * victims per node, -1 where the node is no candidate.  The call changes no state: the caller evicts
 * (qs_evict) and reserves.  QS_ESTATE with the registry off; QS_EINVAL for a pod qs_reserve would reject,
 * for a pod with an anti_affinity kind other than QS_AA_NONE on a context that tracks pod anti-affinity
 * (removing victims would change the counts its filter reads), and when a node holds more than
 * QS_MAX_VICTIMS entries (the message names the node). */
QS_API qs_status qs_preempt_pod(qs_ctx *ctx, const qs_pod *pod, int32_t *node, qs_victim *victims,
                                uint32_t *n_victims, int32_t *nvict_n);
/* Removes the entry `seq` of `node` (the caller has deleted that pod: UP framework/preemption#
 * Evaluator.prepareCandidate -> util.DeletePod, then NodeInfo.RemovePod): Unreserve with the recorded
 * requests and, with anti-affinity tracking on, of the recorded app, as qs_unreserve does.  QS_EINVAL
 * when the node holds no such entry. */
QS_API qs_status qs_evict(qs_ctx *ctx, uint32_t node, uint64_t seq);

/* ---- one pod, all nodes (framework-embedded path) ----
 * feasible_n (nullable): 1/0 per node; score_n (nullable): [n][4] {LeastAllocated, Balanced,
 * TaintToleration, NodeAffinity} normalized plugin scores (0 where infeasible); total_n (nullable):
 * QoS-weighted total per node (-1 where infeasible); best: node index of spec S7 or -1.
 * With anti-affinity tracking on (spec S12, S13) a node the pod's required anti-affinity or its zone
 * topology spread (QS_AA_SPREAD) excludes is infeasible like any other: 0 in feasible_n, zeros in score_n, -1 in total_n, 0xFFFFFFFF in the
 * packed words, and outside the normalize maxima. */
QS_API qs_status qs_score_pod(qs_ctx *ctx, const qs_pod *pod, uint8_t *feasible_n, int32_t *score_n,
                       int32_t *total_n, int32_t *best);
/* The same call without the per-node copy-out: *packed_n (nullable) points at n context-owned words,
 * valid until the next call on ctx, one per node: 0xFFFFFFFF = infeasible, else the four normalized
 * plugin scores as bytes (LeastAllocated | Balanced << 8 | TaintToleration << 16 | NodeAffinity << 24).
 * The words are what the kernel wrote into pinned host memory, so a plugin's per-node Filter / Score
 * lookups read them in place (UP framework/interface.go#ScorePlugin.Score is called per node). */
QS_API qs_status qs_score_pod_packed(qs_ctx *ctx, const qs_pod *pod, const uint32_t **packed_n, int32_t *best);
/* The fifth plugin score of the last qs_score_pod / qs_score_pod_packed call on ctx, per zone (spec S14):
 * out[z] = PTS of every node of zone z (0..100) for the zones that hold a node feasible for that pod, -1
 * for every other zone; all -1 when that pod was no QS_AA_SPREAD_SOFT pod or the context does not track.
 * score_n[n][4] and the packed words keep their four scores: a framework plugin looks this one up by the
 * node's zone.  total_n and best of that call include Wpts * PTS.  QS_ESTATE before any such call. */
QS_API qs_status qs_score_pod_zone_scores(qs_ctx *ctx, int32_t out[QS_MAX_ZONES]);

/* ---- exact stream ---- */
QS_API qs_status qs_schedule_stream(qs_ctx *ctx, const qs_pod *pods, uint32_t p, qs_mode mode,
                             int32_t *placement_p, qs_stats *stats);
/* Split form: prepare (host precompute + H2D), run (device only, timed; may run again, e.g. after
 * qs_table_restore), results (D2H of the last run). */
QS_API qs_status qs_stream_prepare(qs_ctx *ctx, const qs_pod *pods, uint32_t p, qs_stream **out);
QS_API qs_status qs_stream_run(qs_ctx *ctx, qs_stream *s, qs_mode mode, qs_stats *stats);
QS_API qs_status qs_stream_results(qs_ctx *ctx, qs_stream *s, int32_t *placement_p, uint64_t *best_key_p);
/* Frees the stream (ctx may be NULL).  A stream may also be freed after its context was closed. */
QS_API qs_status qs_stream_free(qs_ctx *ctx, qs_stream *s);
/* Per-pod device timestamps (100 MHz s_memrealtime ticks, stream order; record_timestamps = 1). */
QS_API qs_status qs_stream_stamps(qs_ctx *ctx, qs_stream *s, uint64_t *stamps_p);
/* How many of the last run's lookahead windows the resident launch was told hold identical pod
 * records; its ring resolver decides those without a barrier per pod.  0 for every other run, and
 * with QS_RES_UNIFORM=0. */
QS_API qs_status qs_stream_uniform_windows(qs_ctx *ctx, qs_stream *s, uint32_t *windows);
/* FitError diagnosis of an exact stream's unschedulable pods (replaces UP framework/types.go#FitError,
 * Diagnosis.NodeToStatusMap; the "0/N nodes are available: ..." message).  For each requested pod
 * (arrival index) the number of nodes that rejected it for each reason, against the table as it
 * stood when that pod was scheduled: the stream's device placements replayed over the host mirror.
 * A node counts under the first failing filter in upstream's default order (TaintToleration,
 * NodeAffinity, NodeResourcesFit) and, for NodeResourcesFit, under every insufficient resource
 * (UP noderesources/fit.go#fitsRequest).  counts = m x QS_FIT_REASONS; a placed pod gets zeros.
 * Call after qs_stream_run of an exact stream and before any other change to the table
 * (QS_ESTATE otherwise). */
typedef enum qs_fit_reason {
    QS_FIT_TOO_MANY_PODS = 0, /* "Too many pods" */
    QS_FIT_CPU = 1,           /* "Insufficient cpu" */
    QS_FIT_MEMORY = 2,        /* "Insufficient memory" */
    QS_FIT_EXT0 = 3,          /* "Insufficient <extended resource 0>" */
    QS_FIT_EXT1 = 4,          /* "Insufficient <extended resource 1>" */
    QS_FIT_TAINT = 5,         /* "node(s) had untolerated taint {key: value}" (split per taint:
                               * qs_stream_fit_taints) */
    QS_FIT_AFFINITY = 6,      /* "node(s) didn't match Pod's node affinity/selector" */
    QS_FIT_REASONS = 7
} qs_fit_reason;
QS_API qs_status qs_stream_fit_errors(qs_ctx *ctx, qs_stream *s, const uint32_t *pods, uint32_t m, uint32_t *counts);
/* The same counts, plus the QS_FIT_TAINT nodes split by taint (UP plugins/tainttoleration/
 * taint_toleration.go#Filter: "node(s) had untolerated taint {%s: %s}" names the FIRST untolerated
 * NoSchedule / NoExecute taint of the node, one reason string per distinct taint, which FitError.Error()
 * counts separately).  taint_counts = m x 64: per pod, per interned taint bit b, the nodes whose first
 * untolerated hard taint is bit b (the lowest set bit of taint_hard & ~tol_hard; the interning order
 * stands for the node's taint order, exact when every node lists its taints in interning order, as
 * the workload loader's and the synthetic generator's nodes do).  Row sums equal counts[QS_FIT_TAINT]. */
QS_API qs_status qs_stream_fit_taints(qs_ctx *ctx, qs_stream *s, const uint32_t *pods, uint32_t m, uint32_t *counts,
                                      uint32_t *taint_counts);

/* ---- host helpers (spec S2/S3, spec/synth.md) ---- */
QS_API qs_status qs_pod_from_containers(const qs_container *c, uint32_t nc, const int64_t *overhead_cpu_mem,
                                 qs_pod *out);
QS_API int32_t qs_compute_qos(const qs_container *c, uint32_t nc);
/* sizeof of the ABI structs for binding self-checks: 0 config, 1 node_soa, 2 node_row, 3 pod,
 * 4 container, 5 stats, 6 scoring_strategy, 7 victim. */
QS_API size_t qs_struct_size(int which);
/* The shape function of RequestedToCapacityRatio as a table (no context): validates the shape as
 * qs_set_scoring_strategy does and writes table[p] = raw(p) * 10 for the utilisation p = 0..100
 * (UP helper/shape_score.go#BuildBrokenLinearFunction with Go's truncating integer division, scores
 * scaled by MaxNodeScore / MaxCustomPriorityScore = 10).  QS_EINVAL for a bad shape or a null pointer. */
QS_API qs_status qs_shape_table(const qs_shape_point *shape, uint32_t n, uint8_t table[101]);
QS_API qs_status qs_synth_generate(int config, uint64_t seed, uint32_t n, uint32_t p,
                            const qs_node_soa_out *nodes, qs_pod *pods);

#ifdef __cplusplus
}
#endif
#endif /* QSCHED_H */
