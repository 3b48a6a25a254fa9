"""qsched — Python binding of libqsched.so (the gfx950 scheduling core behind include/qsched.h).

This is plumbing for tests and ``bench.py``; the product is the C ABI.  Every call goes through
the HIP library: if ``libqsched.so`` is missing, importing the binding succeeds but the first call
raises ``QschedLibraryMissing`` — there is no CPU fallback.

Data model (the same field names as include/qsched.h):
  * nodes: dict of numpy arrays (``alloc_cpu``, ``alloc_mem``, ``alloc_ext`` [n,2], ``max_pods``,
    ``req_cpu``, ``req_mem``, ``req_ext`` [n,2], ``nz_cpu``, ``nz_mem``, ``pods`` int64;
    ``taint_hard``, ``taint_soft`` uint64; ``label_bits`` [n,2] uint64);
  * pods: numpy structured array of ``POD_DTYPE`` (one ``qs_pod`` per element) or the equivalent
    dict of arrays (converted with ``pods_to_struct``).
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._abi import (ENGINES, ENGINE_NAMES, EXPORTED, LIB_PATH, POD_DTYPE, QS_ABI_VERSION,
                   QS_MAX_EXT, QS_MAX_SCORE_RES, QS_MAX_TERMS, QS_MODE_BATCHED, QS_MODE_EXACT, QS_OK,
                   RESOURCES, FIT_REASONS, QS_FIT_TAINT, QS_MAX_SHAPE, QOS_NAMES, STRATEGIES, QschedError,
                   QschedLibraryMissing, QsConfig, QsContainer, QsNodeRow, QsNodeSoa, QsScoringStrategy,
                   QsStats, load)

__all__ = ["Scheduler", "Config", "POD_DTYPE", "pods_to_struct", "pods_from_struct", "fit_error_message",
           "synth_generate", "shape_table", "dist_unique_id", "empty_nodes", "pod_from_containers", "compute_qos", "load",
           "QschedError", "QschedLibraryMissing", "ENGINES", "EXPORTED", "LIB_PATH",
           "aa_spread", "aa_spread_soft", "aa_spread_hostname", "aa_is_soft", "aa_is_hostkey", "QS_AA_HOSTKEY", "aa_kind", "aa_max_skew", "QS_AA_SOFT", "QS_MAX_ZONES", "QS_AA_NONE", "QS_AA_HOSTNAME", "QS_AA_ZONE", "QS_AA_SPREAD_ZONE",
           "QS_MAX_SPREAD_SKEW", "QS_POLICY_IGNORE", "QS_POLICY_HONOR", "POLICIES"]

from ._abi import (QS_POLICY_HONOR, QS_POLICY_IGNORE, QS_AA_HOSTKEY, QS_AA_HOSTNAME, QS_AA_NONE, QS_AA_SOFT, QS_AA_SPREAD_ZONE, QS_AA_ZONE,  # noqa: E402,F401
                   QS_MAX_SPREAD_SKEW, QS_MAX_ZONES)

from ._abi import (PREEMPT_POLICIES, QS_MAX_VICTIMS, QS_PREEMPT_BY_PRIORITY, QS_PREEMPT_BY_QOS,  # noqa: E402,F401
                   VICTIM_DTYPE)

__all__ += ["VICTIM_DTYPE", "QS_MAX_VICTIMS", "QS_PREEMPT_BY_PRIORITY", "QS_PREEMPT_BY_QOS", "PREEMPT_POLICIES"]

MODES = {"exact": QS_MODE_EXACT, "batched": QS_MODE_BATCHED}
POLICIES = {"ignore": QS_POLICY_IGNORE, "honor": QS_POLICY_HONOR}


def aa_spread(max_skew: int) -> int:
    """QS_AA_SPREAD(max_skew): the ``anti_affinity`` value of a pod under zone topology spread
    (``topologySpreadConstraints``, ``whenUnsatisfiable: DoNotSchedule``, spec S13), max_skew 1..31."""
    if not 1 <= int(max_skew) <= QS_MAX_SPREAD_SKEW:
        raise ValueError("max_skew must be 1..31")
    return QS_AA_SPREAD_ZONE | (int(max_skew) << 8)


def aa_spread_soft(max_skew: int) -> int:
    """QS_AA_SPREAD_SOFT(max_skew): the same constraint with ``whenUnsatisfiable: ScheduleAnyway`` (spec
    S14): the pod is not filtered by spread; every feasible node's total gains the PodTopologySpread
    score of its zone times ``Scheduler.set_topology_spread_weight``."""
    return aa_spread(max_skew) | QS_AA_SOFT


def aa_spread_hostname(max_skew: int) -> int:
    """QS_AA_SPREAD_HOSTNAME(max_skew): topology spread with ``topologyKey: kubernetes.io/hostname`` and
    ``whenUnsatisfiable: DoNotSchedule`` (spec S15): at most max_skew pods of the app more on any node
    than on the emptiest node of the table.  max_skew 1..31."""
    return aa_spread(max_skew) | QS_AA_HOSTKEY


def aa_is_hostkey(anti_affinity):
    """QS_AA_IS_HOSTKEY: the hostname-key flag (scalar or array)."""
    return (anti_affinity >> 18) & 1


def aa_is_soft(anti_affinity):
    """QS_AA_IS_SOFT: the ScheduleAnyway flag (scalar or array)."""
    return (anti_affinity >> 16) & 1


def aa_kind(anti_affinity):
    """QS_AA_KIND: the kind in the low byte (scalar or array)."""
    return anti_affinity & 0xFF


def aa_max_skew(anti_affinity):
    """QS_AA_MAX_SKEW: bits 8-12 (0 for every kind but QS_AA_SPREAD_ZONE)."""
    return (anti_affinity >> 8) & 0x1F
NODE_I64 = ["alloc_cpu", "alloc_mem", "max_pods", "req_cpu", "req_mem", "nz_cpu", "nz_mem", "pods"]


def _check(lib, ctx, st):
    if st != QS_OK:
        msg = lib.qs_last_error(ctx).decode() if ctx else ""
        raise QschedError(st, msg)


def _ptr(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "arrays passed to the C ABI must be C-contiguous"
    return a.ctypes.data


def empty_nodes(n: int):
    d = {f: np.zeros(n, np.int64) for f in NODE_I64}
    d["alloc_ext"] = np.zeros((n, QS_MAX_EXT), np.int64)
    d["req_ext"] = np.zeros((n, QS_MAX_EXT), np.int64)
    d["taint_hard"] = np.zeros(n, np.uint64)
    d["taint_soft"] = np.zeros(n, np.uint64)
    d["label_bits"] = np.zeros((n, 2), np.uint64)
    d["zone"] = np.zeros(n, np.int32)
    return d


def _soa(nodes, lib_out=False):
    s = QsNodeSoa()
    for f, _ in QsNodeSoa._fields_:
        a = nodes.get(f)
        if a is not None:
            want = (np.uint64 if f in ("taint_hard", "taint_soft", "label_bits") else
                    np.int32 if f == "zone" else np.int64)
            if a.dtype != want or not a.flags["C_CONTIGUOUS"]:
                if lib_out:
                    raise TypeError(f"output column {f} must be C-contiguous {want}")
                a = np.ascontiguousarray(a, dtype=want)
                nodes = dict(nodes)
                nodes[f] = a
        setattr(s, f, _ptr(a))
    return s, nodes  # keep the converted arrays alive with the struct


def pods_to_struct(pods) -> np.ndarray:
    """dict-of-arrays (oracle layout) or structured array -> contiguous POD_DTYPE array."""
    if isinstance(pods, np.ndarray) and pods.dtype == POD_DTYPE:
        return np.ascontiguousarray(pods)
    p = len(pods["req_cpu"])
    out = np.zeros(p, POD_DTYPE)
    for f in POD_DTYPE.names:
        if f in pods:
            out[f] = pods[f]
    return out


def pods_from_struct(arr: np.ndarray):
    return {f: np.ascontiguousarray(arr[f]) for f in POD_DTYPE.names}


class Config(dict):
    """qs_config as a dict; unspecified fields take qs_config_default()."""

    def to_c(self) -> QsConfig:
        lib = load()
        c = QsConfig()
        lib.qs_config_default(ctypes.byref(c))
        for k, v in self.items():
            if k == "engine" and isinstance(v, str):
                v = ENGINES[v]
            if k in ("w_fit", "w_bal"):
                for i in range(3):
                    getattr(c, k)[i] = int(v[i])
            elif k == "fit_resources":  # [(name | id, weight), ...] (spec S5 "Scoring resources")
                v = list(v or [])
                if len(v) > QS_MAX_SCORE_RES:
                    raise ValueError("at most 4 scoring resources")
                c.n_fit_resources = len(v)
                for i, (name, w) in enumerate(v):
                    c.fit_resources[i][0] = RESOURCES[name] if isinstance(name, str) else int(name)
                    c.fit_resources[i][1] = int(w)
            elif k == "balanced_resources":  # [name | id, ...]
                v = list(v or [])
                if len(v) > QS_MAX_SCORE_RES:
                    raise ValueError("at most 4 balanced resources")
                c.n_balanced_resources = len(v)
                for i, name in enumerate(v):
                    c.balanced_resources[i] = RESOURCES[name] if isinstance(name, str) else int(name)
            else:
                setattr(c, k, int(v))
        return c


class Scheduler:
    """One device context (``qs_ctx``) on one GPU."""

    def __init__(self, config=None, device: int = 0, shard=None):
        """shard = (rank, world, unique_id bytes) opens a node-sharded context (qs_open_shard):
        every rank loads the same full table and pod stream; RCCL exchanges the per-window lists.
        unique_id None: the peer-memory mailbox transport (mailbox_export / mailbox_connect)."""
        self.lib = load()
        config = dict(config or {})
        # NodeResourcesFitArgs.ScoringStrategy.Type / RequestedToCapacityRatio.Shape are not part of
        # qs_config: they are set on the open context (qs_set_scoring_strategy)
        strategy, shape = config.pop("scoring_strategy", None), config.pop("shape", None)
        # ... and per QoS class (one upstream profile each): {"BestEffort": dict(scoring_strategy=...,
        # shape=...), ...}, applied after a context-wide scoring_strategy
        qos_strategies = config.pop("qos_strategies", None)
        self.cfg = Config(config).to_c()
        ctx = ctypes.c_void_p()
        if shard is None:
            st = self.lib.qs_open(ctypes.byref(self.cfg), device, ctypes.byref(ctx))
        else:
            rank, world, uid = shard
            buf = None if uid is None else (ctypes.c_uint8 * 128).from_buffer_copy(bytes(uid))
            st = self.lib.qs_open_shard(ctypes.byref(self.cfg), device, rank, world, buf,
                                        ctypes.byref(ctx))
        if st != QS_OK:
            why = self.lib.qs_last_error(None)
            raise QschedError(st, "qs_open failed: " + (why.decode() if why else "no HIP device?"))
        self.ctx = ctx
        self.n = 0
        try:
            if strategy is not None or shape is not None:
                self.set_scoring_strategy(strategy or "LeastAllocated", shape)
            for q, sc in (qos_strategies or {}).items():
                self.set_scoring_strategy(sc.get("scoring_strategy") or "LeastAllocated", sc.get("shape"), qos=q)
        except Exception:
            self.close()
            raise

    @staticmethod
    def _qos_id(qos) -> int:
        return QOS_NAMES[qos] if isinstance(qos, str) else int(qos)

    def set_scoring_strategy(self, strategy, shape=None, qos=None):
        """qs_set_scoring_strategy: "LeastAllocated" | "MostAllocated" | "RequestedToCapacityRatio"
        (or the qs_scoring_strategy_type id) and, for the last, shape = [(utilization, score), ...].
        qos = "BestEffort" | "Burstable" | "Guaranteed" (or 0..2) sets the strategy of that QoS class
        only (qs_set_scoring_strategy_qos); None sets all three."""
        shape = list(shape or [])
        if len(shape) > QS_MAX_SHAPE:
            raise ValueError(f"at most {QS_MAX_SHAPE} shape points")
        st = QsScoringStrategy()
        st.type = STRATEGIES[strategy] if isinstance(strategy, str) else int(strategy)
        st.n_shape = len(shape)
        for i, (u, sc) in enumerate(shape):
            st.shape[i][0], st.shape[i][1] = int(u), int(sc)
        if qos is None:
            self._chk(self.lib.qs_set_scoring_strategy(self.ctx, ctypes.byref(st)))
        else:
            self._chk(self.lib.qs_set_scoring_strategy_qos(self.ctx, self._qos_id(qos), ctypes.byref(st)))

    def get_scoring_strategy(self, qos):
        """qs_get_scoring_strategy_qos: (strategy name, [(utilization, score), ...]) of one QoS class."""
        st = QsScoringStrategy()
        self._chk(self.lib.qs_get_scoring_strategy_qos(self.ctx, self._qos_id(qos), ctypes.byref(st)))
        name = {v: k for k, v in STRATEGIES.items()}[int(st.type)]
        return name, [(int(st.shape[i][0]), int(st.shape[i][1])) for i in range(int(st.n_shape))]

    def set_pod_anti_affinity(self, on=True):
        """qs_set_pod_anti_affinity: required pod anti-affinity (``app`` / ``anti_affinity``) on the
        exact engines, score_pod and reserve / unreserve (spec S12); off in a new context."""
        self._chk(self.lib.qs_set_pod_anti_affinity(self.ctx, 1 if on else 0))

    def get_pod_anti_affinity(self) -> bool:
        on = ctypes.c_int32(-1)
        self._chk(self.lib.qs_get_pod_anti_affinity(self.ctx, ctypes.byref(on)))
        return bool(on.value)

    def set_topology_spread_weight(self, weight: int):
        """qs_set_topology_spread_weight: the PodTopologySpread plugin weight of QS_AA_SPREAD_SOFT pods
        (spec S14), 0..100; 2 in a new context."""
        self._chk(self.lib.qs_set_topology_spread_weight(self.ctx, int(weight)))

    def get_topology_spread_weight(self) -> int:
        w = ctypes.c_int32(-1)
        self._chk(self.lib.qs_get_topology_spread_weight(self.ctx, ctypes.byref(w)))
        return int(w.value)

    def set_topology_spread_node_affinity_policy(self, policy):
        """qs_set_topology_spread_node_affinity_policy: "ignore" / "honor" (or QS_POLICY_*), spec S16.  Under
        "honor" a spread pod with a nodeSelector or required node-affinity terms counts, and takes its
        domains from, the nodes that pass them only; "ignore" in a new context."""
        pol = POLICIES[policy] if isinstance(policy, str) else int(policy)
        self._chk(self.lib.qs_set_topology_spread_node_affinity_policy(self.ctx, pol))

    def get_topology_spread_node_affinity_policy(self) -> int:
        v = ctypes.c_int32(-1)
        self._chk(self.lib.qs_get_topology_spread_node_affinity_policy(self.ctx, ctypes.byref(v)))
        return int(v.value)

    def set_topology_spread_node_taints_policy(self, policy):
        """qs_set_topology_spread_node_taints_policy: "ignore" / "honor" (or QS_POLICY_*), spec S17.  Under
        "honor" a spread pod counts, and takes its domains from, the nodes whose hard taints it tolerates
        only (needs enable_taint = 1); "ignore" in a new context."""
        pol = POLICIES[policy] if isinstance(policy, str) else int(policy)
        self._chk(self.lib.qs_set_topology_spread_node_taints_policy(self.ctx, pol))

    def get_topology_spread_node_taints_policy(self) -> int:
        v = ctypes.c_int32(-1)
        self._chk(self.lib.qs_get_topology_spread_node_taints_policy(self.ctx, ctypes.byref(v)))
        return int(v.value)

    def score_pod_zone_scores(self):
        """qs_score_pod_zone_scores: int32[QS_MAX_ZONES], the PodTopologySpread score per zone of the last
        score_pod / score_pod_packed call (-1: no feasible node there, or no soft-spread pod)."""
        z = np.full(QS_MAX_ZONES, -2, np.int32)
        self._chk(self.lib.qs_score_pod_zone_scores(self.ctx, _ptr(z)))
        return z

    def mailbox_export(self) -> bytes:
        """qs_dist_mailbox_export: this rank's 64-byte mailbox IPC handle (sharded contexts opened
        without an RCCL id)."""
        buf = (ctypes.c_uint8 * 64)()
        self._chk(self.lib.qs_dist_mailbox_export(self.ctx, buf))
        return bytes(buf)

    def mailbox_connect(self, handles):
        """qs_dist_mailbox_connect with every rank's handle, in rank order."""
        blob = b"".join(bytes(h) for h in handles)
        buf = (ctypes.c_uint8 * len(blob)).from_buffer_copy(blob)
        self._chk(self.lib.qs_dist_mailbox_connect(self.ctx, buf))

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.qs_close(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st):
        _check(self.lib, self.ctx, st)

    # ---- node table ----
    def load_nodes(self, nodes):
        s, keep = _soa(nodes)
        n = len(nodes["alloc_cpu"])
        self._chk(self.lib.qs_nodes_load(self.ctx, ctypes.byref(s), n))
        self.n = n
        del keep

    def read_nodes(self):
        out = empty_nodes(self.n)
        s, _ = _soa(out, lib_out=True)
        self._chk(self.lib.qs_nodes_read(self.ctx, ctypes.byref(s), self.n))
        return out

    def upsert(self, idx, row: dict, generation=0):
        r = QsNodeRow()
        for f, t in QsNodeRow._fields_:
            if f in row:
                v = row[f]
                if f in ("alloc_ext", "req_ext", "label_bits"):
                    for i, x in enumerate(v):
                        getattr(r, f)[i] = int(x)
                else:
                    setattr(r, f, int(v))
        self._chk(self.lib.qs_node_upsert(self.ctx, idx, ctypes.byref(r), generation))
        if idx == self.n:
            self.n += 1

    def save_table(self):
        self._chk(self.lib.qs_table_save(self.ctx))

    def restore_table(self):
        self._chk(self.lib.qs_table_restore(self.ctx))

    def reserve(self, node, pod):
        p = pods_to_struct(pod) if not isinstance(pod, np.void) else np.array([pod], POD_DTYPE)
        self._chk(self.lib.qs_reserve(self.ctx, node, _ptr(p)))

    def unreserve(self, node, pod):
        p = pods_to_struct(pod) if not isinstance(pod, np.void) else np.array([pod], POD_DTYPE)
        self._chk(self.lib.qs_unreserve(self.ctx, node, _ptr(p)))

    # ---- preemption (spec S18) ----
    def set_preemption(self, on=True):
        """qs_set_preemption: the pod registry (which pods sit on which node); off in a new context."""
        self._chk(self.lib.qs_set_preemption(self.ctx, 1 if on else 0))

    def get_preemption(self) -> bool:
        on = ctypes.c_int32(-1)
        self._chk(self.lib.qs_get_preemption(self.ctx, ctypes.byref(on)))
        return bool(on.value)

    def set_preemption_policy(self, policy):
        """qs_set_preemption_policy: "priority" (upstream's rule; a new context) or "qos" (QoS class, then
        priority: the order of spec S8), or a QS_PREEMPT_* value."""
        pol = PREEMPT_POLICIES[policy] if isinstance(policy, str) else int(policy)
        self._chk(self.lib.qs_set_preemption_policy(self.ctx, pol))

    def get_preemption_policy(self) -> int:
        v = ctypes.c_int32(-1)
        self._chk(self.lib.qs_get_preemption_policy(self.ctx, ctypes.byref(v)))
        return int(v.value)

    def node_pods(self, node):
        """qs_node_pods: the node's registry entries as a VICTIM_DTYPE array, most important first."""
        n = ctypes.c_uint32(0)
        self._chk(self.lib.qs_node_pods(self.ctx, node, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, VICTIM_DTYPE)
        if n.value:
            self._chk(self.lib.qs_node_pods(self.ctx, node, _ptr(out), n.value, ctypes.byref(n)))
        return out

    def preempt_pod(self, pod, per_node=False):
        """qs_preempt_pod: (node, victims) of the dry run for one pod, node -1 without a candidate and
        victims a VICTIM_DTYPE array in walk order; with per_node also the victims per node (int32[n], -1
        where the node is no candidate).  Changes no state: evict() the victims, then reserve()."""
        p = np.array([pod], POD_DTYPE) if isinstance(pod, np.void) else pods_to_struct(pod)[:1]
        node = ctypes.c_int32(-2)
        nv = ctypes.c_uint32(0)
        victims = np.zeros(QS_MAX_VICTIMS, VICTIM_DTYPE)
        nvict_n = np.full(self.n, -2, np.int32) if per_node else None
        self._chk(self.lib.qs_preempt_pod(self.ctx, _ptr(p), ctypes.byref(node), _ptr(victims), ctypes.byref(nv),
                                          _ptr(nvict_n)))
        res = (int(node.value), victims[:nv.value].copy())
        return res + (nvict_n,) if per_node else res

    def evict(self, node, seq):
        """qs_evict: remove the registry entry `seq` of `node` (Unreserve with the recorded requests)."""
        self._chk(self.lib.qs_evict(self.ctx, int(node), int(seq)))

    # ---- one pod, all nodes ----
    def score_pod(self, pod, outputs=True, out=None):
        """qs_score_pod: {"best"} and, with outputs, the per-node "feasible" / "scores" / "total"
        arrays and the per-zone "zone_scores" of a soft-spread pod (fresh copies, or the caller's reusable buffers from score_buffers() passed as
        `out`, filled in place).  outputs=False asks the library for the best node only."""
        p = np.array([pod], POD_DTYPE) if isinstance(pod, np.void) else pods_to_struct(pod)[:1]
        best = ctypes.c_int32(-2)
        if not outputs:
            self._chk(self.lib.qs_score_pod(self.ctx, _ptr(p), None, None, None, ctypes.byref(best)))
            return dict(best=best.value)
        if out is None:
            out = self.score_buffers()
        feas, score, total = out["feasible"], out["scores"], out["total"]
        if len(total) != self.n or score.shape != (self.n, 4) or feas.dtype != np.bool_:
            raise ValueError("score_pod: out buffers do not match the node table (use score_buffers())")
        self._chk(self.lib.qs_score_pod(self.ctx, _ptr(p), _ptr(feas), _ptr(score), _ptr(total),
                                        ctypes.byref(best)))
        # the fifth score per zone (spec S14): one more call, for a soft-spread pod only; all -1 otherwise
        soft = aa_is_soft(int(p["anti_affinity"][0]))
        zs = self.score_pod_zone_scores() if soft else np.full(QS_MAX_ZONES, -1, np.int32)
        return dict(feasible=feas, scores=score, total=total, best=best.value, zone_scores=zs)

    def score_pod_packed(self, pod):
        """qs_score_pod_packed: (best, packed) with packed a copy of the n per-node words (0xFFFFFFFF
        = infeasible, else the four plugin scores as bytes, LeastAllocated in the low byte)."""
        p = np.array([pod], POD_DTYPE) if isinstance(pod, np.void) else pods_to_struct(pod)[:1]
        best = ctypes.c_int32(-2)
        ptr = ctypes.POINTER(ctypes.c_uint32)()
        self._chk(self.lib.qs_score_pod_packed(self.ctx, _ptr(p), ctypes.byref(ptr), ctypes.byref(best)))
        packed = np.ctypeslib.as_array(ptr, shape=(self.n,)).copy() if self.n and ptr else np.zeros(0, np.uint32)
        return best.value, packed

    def score_buffers(self):
        """Output arrays for score_pod(..., out=...) sized to the current table (feasible is a bool
        array the library fills with 0 / 1 bytes)."""
        return dict(feasible=np.zeros(self.n, np.bool_), scores=np.zeros((self.n, 4), np.int32),
                    total=np.zeros(self.n, np.int32))

    # ---- exact stream ----
    def schedule(self, pods, with_stats=False, mode="exact"):
        arr = pods_to_struct(pods)
        placement = np.empty(len(arr), np.int32)
        stats = QsStats()
        self._chk(self.lib.qs_schedule_stream(self.ctx, _ptr(arr), len(arr), MODES[mode],
                                              _ptr(placement), ctypes.byref(stats)))
        return (placement, stats.as_dict()) if with_stats else placement

    def prepare(self, pods):
        arr = pods_to_struct(pods)
        h = ctypes.c_void_p()
        self._chk(self.lib.qs_stream_prepare(self.ctx, _ptr(arr), len(arr), ctypes.byref(h)))
        return Stream(self, h, len(arr))


class Stream:
    """A prepared pod stream (device-resident pod records): run() is the timed device path."""

    def __init__(self, sched: Scheduler, handle, p):
        self.s, self.h, self.p = sched, handle, p
        self.stats = None

    def run(self, mode="exact"):
        """qs_stream_run: mode "exact" (spec S7/S8) or "batched" (spec S11)."""
        st = QsStats()
        self.s._chk(self.s.lib.qs_stream_run(self.s.ctx, self.h, MODES[mode], ctypes.byref(st)))
        self.stats = st.as_dict()
        # windows of identical pods the resident launch was given (0: none, or another engine)
        uw = ctypes.c_uint32(0)
        self.s._chk(self.s.lib.qs_stream_uniform_windows(self.s.ctx, self.h, ctypes.byref(uw)))
        self.stats["uniform_windows"] = int(uw.value)
        return self.stats

    def results(self):
        placement = np.empty(self.p, np.int32)
        keys = np.empty(self.p, np.uint64)
        self.s._chk(self.s.lib.qs_stream_results(self.s.ctx, self.h, _ptr(placement), _ptr(keys)))
        return placement, keys

    def stamps(self):
        out = np.empty(self.p, np.uint64)
        self.s._chk(self.s.lib.qs_stream_stamps(self.s.ctx, self.h, _ptr(out)))
        return out

    def fit_errors(self, pods=None, by_taint=False):
        """qs_stream_fit_errors: per requested pod (arrival indices; default: every unschedulable
        pod) the count of nodes per FitError reason column (FIT_REASONS), against the table at that
        pod's turn.  Returns (indices, counts[m, 7]); with by_taint (qs_stream_fit_taints) also
        taint_counts[m, 64], the untolerated-taint column split by the node's first untolerated taint
        bit (upstream names that taint in the reason string)."""
        if pods is None:
            pl, _ = self.results()
            pods = np.nonzero(pl < 0)[0]
        idx = np.ascontiguousarray(pods, dtype=np.uint32)
        counts = np.zeros((len(idx), len(FIT_REASONS)), np.uint32)
        if not by_taint:
            self.s._chk(self.s.lib.qs_stream_fit_errors(self.s.ctx, self.h, _ptr(idx), len(idx), _ptr(counts)))
            return idx, counts
        tcounts = np.zeros((len(idx), 64), np.uint32)
        self.s._chk(self.s.lib.qs_stream_fit_taints(self.s.ctx, self.h, _ptr(idx), len(idx), _ptr(counts),
                                                     _ptr(tcounts)))
        return idx, counts, tcounts

    def free(self):
        if self.h:
            self.s._chk(self.s.lib.qs_stream_free(self.s.ctx, self.h))
            self.h = None


def dist_unique_id() -> bytes:
    """128-byte RCCL unique id (qs_dist_unique_id) for qs_open_shard; create on rank 0 only."""
    lib = load()
    buf = (ctypes.c_uint8 * 128)()
    st = lib.qs_dist_unique_id(buf)
    if st != QS_OK:
        raise QschedError(st, "qs_dist_unique_id failed")
    return bytes(buf)


def shape_table(shape):
    """qs_shape_table: the 101-entry table raw(0..100) (scores scaled to 0..100) of a
    RequestedToCapacityRatio shape [(utilization, score), ...]; raises QschedError for a bad shape."""
    lib = load()
    shape = list(shape)
    pts = ((ctypes.c_int32 * 2) * max(1, len(shape)))()
    for i, (u, sc) in enumerate(shape):
        pts[i][0], pts[i][1] = int(u), int(sc)
    out = np.zeros(101, np.uint8)
    st = lib.qs_shape_table(pts, len(shape), _ptr(out))
    if st != QS_OK:
        raise QschedError(st, "qs_shape_table: bad shape")
    return out


def synth_generate(config: int, n: int, p: int, seed=None):
    """spec/synth.md cluster (host C++ generator in libqsched).  Returns (nodes dict, pods array)."""
    lib = load()
    nodes = empty_nodes(n)
    s, _ = _soa(nodes, lib_out=True)
    pods = np.zeros(p, POD_DTYPE)
    seed = 0x5EED0000 + config if seed is None else seed
    st = lib.qs_synth_generate(config, seed, n, p, ctypes.byref(s), _ptr(pods))
    if st != QS_OK:
        raise QschedError(st, "qs_synth_generate failed")
    return nodes, pods


def _containers(containers):
    arr = (QsContainer * max(1, len(containers)))()
    for i, c in enumerate(containers):
        for k, v in c.items():
            if k == "req_ext":
                for e, x in enumerate(v):
                    arr[i].req_ext[e] = int(x)
            elif k == "kind":
                arr[i].kind = {"regular": 0, "init": 1, "sidecar": 2}.get(v, v)
            elif k in ("req_cpu", "req_mem", "lim_cpu", "lim_mem"):
                setattr(arr[i], k, int(v))
                setattr(arr[i], "has_" + k, 1)
    return arr


def fit_error_message(counts, n_nodes, ext_names=("ext0", "ext1"), taint_counts=None, taint_names=None):
    """UP framework/types.go#FitError.Error() from one pod's reason counts: "0/N nodes are available:
    <count> <reason>, ..." with the "count reason" strings sorted as Go's sort.Strings does.

    Upstream's TaintToleration reason names the node's first untolerated taint ("node(s) had
    untolerated taint {key: value}", taint_toleration.go#Filter), so each distinct taint is its own
    reason.  Pass taint_counts (this pod's row of ``fit_errors(by_taint=True)``) and taint_names
    (interned bit -> "key: value", e.g. from qsched.workload's taint dictionary) to get that text;
    without them the untolerated-taint nodes are one reason and a bit without a name renders as
    "taint-<bit>"."""
    names = [r.format(ext0=ext_names[0], ext1=ext_names[1], taint="{taint}") for r in FIT_REASONS]
    parts = []
    for k, c in enumerate(counts):
        if not c:
            continue
        if k == QS_FIT_TAINT and taint_counts is not None:
            tc = np.asarray(taint_counts)
            assert int(tc.sum()) == int(c), "taint_counts must split this pod's untolerated-taint count"
            for b in np.nonzero(tc)[0]:
                nm = (taint_names or {}).get(int(b), f"taint-{int(b)}")
                parts.append(f"{int(tc[b])} " + names[k].replace("{taint}", nm))
        elif k == QS_FIT_TAINT:
            parts.append(f"{int(c)} node(s) had untolerated taint")
        else:
            parts.append(f"{int(c)} {names[k]}")
    parts.sort()
    msg = f"0/{n_nodes} nodes are available:"
    return msg + (f" {', '.join(parts)}." if parts else "")


def pod_from_containers(containers, overhead=None):
    """spec S2/S3 for a pod spec given as a list of container dicts (missing keys = missing)."""
    lib = load()
    arr = _containers(containers)
    out = np.zeros(1, POD_DTYPE)
    ov = None if overhead is None else (ctypes.c_int64 * 2)(*overhead)
    st = lib.qs_pod_from_containers(arr, len(containers), ov, _ptr(out))
    if st != QS_OK:
        raise QschedError(st, "qs_pod_from_containers failed")
    return out[0]


def compute_qos(containers) -> int:
    lib = load()
    return int(lib.qs_compute_qos(_containers(containers), len(containers)))
