// cpu_plugins.cpp — the CPU reference plugins of cpu_plugins.hpp (upstream citations there).  Each
// Filter / Score call evaluates one (pod, node) pair from the k8s objects; the framework runtime
// (framework.cpp) runs them over the nodes with its Parallelizer.
#include "cpu_plugins.hpp"

#include <algorithm>
#include <cmath>

#include "intern.hpp"

namespace qsfw {
namespace {

constexpr int64_t kMaxNodeScore = MaxNodeScore;

const PodResources &resources_of(CycleState &s, const Pod &pod, const Handle *h, PodResources *tmp) {
    if (auto *pr = s.Read<PodResourcesState>(kPodResourcesKey)) return pr->res;
    *tmp = ComputePodResources(pod, h->ExtendedResourceNames());
    return *tmp;
}

const NodeInfo *node_of(const Handle *h, const std::string &name) {
    const int i = h->NodeIndex(name);
    return i < 0 ? nullptr : &h->NodeInfos()[(size_t)i];
}

// UP noderesources/least_allocated.go#leastRequestedScore
int64_t least_requested_score(int64_t requested, int64_t capacity) {
    if (capacity == 0) return 0;
    if (requested > capacity) return 0;
    return ((capacity - requested) * kMaxNodeScore) / capacity;
}

// UP noderesources/most_allocated.go#mostRequestedScore (v1.32 clips an over-committed resource to
// its capacity; it does not score it 0)
int64_t most_requested_score(int64_t requested, int64_t capacity) {
    if (capacity == 0) return 0;
    if (requested > capacity) requested = capacity;
    return (requested * kMaxNodeScore) / capacity;
}

// UP helper/shape_score.go#BuildBrokenLinearFunction over the shape's scores scaled by
// MaxNodeScore / MaxCustomPriorityScore = 10 (requested_to_capacity_ratio.go); int64 division
// truncates toward zero, as Go's
int64_t broken_linear(const qs_scoring_strategy &st, int64_t p) {
    const int n = st.n_shape;
    for (int i = 0; i < n; ++i) {
        if (p > st.shape[i].utilization) continue;
        const int64_t s1 = (int64_t)st.shape[i].score * 10;
        if (i == 0) return s1;
        const int64_t s0 = (int64_t)st.shape[i - 1].score * 10;
        const int64_t u0 = st.shape[i - 1].utilization, u1 = st.shape[i].utilization;
        return s0 + (s1 - s0) * (p - u0) / (u1 - u0);
    }
    return n > 0 ? (int64_t)st.shape[n - 1].score * 10 : 0;
}

// UP helper/normalize_score.go#DefaultNormalizeScore
void default_normalize(NodeScoreList &scores, bool reverse) {
    int64_t mx = 0;
    for (const auto &s : scores) mx = std::max(mx, s.score);
    if (mx == 0) {
        if (reverse)
            for (auto &s : scores) s.score = kMaxNodeScore;
        return;
    }
    for (auto &s : scores) {
        int64_t v = kMaxNodeScore * s.score / mx;
        s.score = reverse ? kMaxNodeScore - v : v;
    }
}

bool hard_effect(const std::string &e) { return e == kNoSchedule || e == kNoExecute; }

// NodeResourcesFitArgs.ScoringStrategy.Resources / NodeResourcesBalancedAllocationArgs.Resources as
// (qs_resource, weight) in list order; the defaults [cpu: fit_weight_cpu, memory: fit_weight_mem] and
// [cpu, memory] (UP apis/config/v1/defaults.go)
using ResList = std::vector<std::pair<int32_t, int64_t>>;
ResList fit_list(const qs_config &c) {
    if (c.n_fit_resources == 0) return {{QS_RES_CPU, c.fit_weight_cpu}, {QS_RES_MEMORY, c.fit_weight_mem}};
    ResList r;
    for (int i = 0; i < c.n_fit_resources; ++i) r.push_back({c.fit_resources[i].resource, c.fit_resources[i].weight});
    return r;
}
ResList balanced_list(const qs_config &c) {
    if (c.n_balanced_resources == 0) return {{QS_RES_CPU, 1}, {QS_RES_MEMORY, 1}};
    ResList r;
    for (int i = 0; i < c.n_balanced_resources; ++i) r.push_back({c.balanced_resources[i], 1});
    return r;
}

int64_t lookup(const std::map<std::string, int64_t> &m, const std::string &k) {
    auto it = m.find(k);
    return it == m.end() ? 0 : it->second;
}

// UP noderesources/resource_allocation.go#calculateResourceAllocatableRequest: (allocatable,
// requested + the pod's request) of one scoring resource; cpu / memory from NonZeroRequested and the
// pod's non-zero requests (useRequested = false, LeastAllocated) or Requested and the plain requests
// (true, BalancedAllocation); an extended (scalar) resource the pod does not request is (0, 0), and
// so is one the node does not have (Allocatable.ScalarResources lookup).
std::pair<int64_t, int64_t> alloc_request(const NodeInfo &ni, const PodResources &r, int32_t res,
                                          bool use_requested, const std::vector<std::string> &ext_names) {
    switch (res) {
        case QS_RES_CPU:
            return {ni.allocatable.milli_cpu,
                    use_requested ? ni.requested.milli_cpu + r.cpu : ni.non_zero_requested.milli_cpu + r.nz_cpu};
        case QS_RES_MEMORY:
            return {ni.allocatable.memory,
                    use_requested ? ni.requested.memory + r.mem : ni.non_zero_requested.memory + r.nz_mem};
        default: {
            const size_t k = (size_t)(res - QS_RES_EXT0);
            if (k >= ext_names.size()) return {0, 0};
            const std::string &name = ext_names[k];
            const int64_t q = lookup(r.scalar, name);
            if (q == 0 || !ni.allocatable.scalar.count(name)) return {0, 0};
            return {ni.allocatable.scalar.at(name), lookup(ni.requested.scalar, name) + q};
        }
    }
}

}  // namespace

// The three scorers of NodeResourcesFit over (allocatable, requested, weight) entries, int64 / double
// as upstream: LeastAllocated (UP least_allocated.go#leastResourceScorer), MostAllocated (UP
// most_allocated.go#mostResourceScorer), RequestedToCapacityRatio (UP requested_to_capacity_ratio.go#
// buildRequestedToCapacityRatioScorerFunction: a resource whose shape score is 0 does not count
// towards the weight sum; math.Round of the float64 quotient).  Entries with allocatable 0 are skipped.
int64_t FitStrategyScore(const qs_scoring_strategy &st, const int64_t *alloc, const int64_t *reqd,
                         const int64_t *weight, int n) {
    int64_t score = 0, wsum = 0;
    for (int i = 0; i < n; ++i) {
        if (alloc[i] == 0) continue;
        if (st.type == QS_STRATEGY_REQUESTED_TO_CAPACITY_RATIO) {
            const int64_t s = reqd[i] > alloc[i] ? broken_linear(st, 100)
                                                 : broken_linear(st, reqd[i] * kMaxNodeScore / alloc[i]);
            if (s > 0) {
                score += s * weight[i];
                wsum += weight[i];
            }
            continue;
        }
        score += (st.type == QS_STRATEGY_MOST_ALLOCATED ? most_requested_score(reqd[i], alloc[i])
                                                        : least_requested_score(reqd[i], alloc[i])) * weight[i];
        wsum += weight[i];
    }
    if (wsum == 0) return 0;
    if (st.type == QS_STRATEGY_REQUESTED_TO_CAPACITY_RATIO) return (int64_t)std::round((double)score / (double)wsum);
    return score / wsum;
}

namespace {

// ---- NodeResourcesFit ------------------------------------------------------------------------
class NodeResourcesFit final : public PreFilterPlugin, public FilterPlugin, public ScorePlugin {
   public:
    NodeResourcesFit(const qs_config &cfg, const qs_scoring_strategy &st, Handle *h)
        : res_(fit_list(cfg)), st_(st), h_(h) {}
    std::string Name() const override { return kNodeResourcesFit; }

    // UP fit.go#PreFilter computes the pod's requests once per cycle (preFilterState)
    std::pair<PreFilterResult, Status> PreFilter(CycleState &s, const Pod &pod) override {
        if (!s.Read<PodResourcesState>(kPodResourcesKey))
            s.Write(kPodResourcesKey, std::make_shared<PodResourcesState>(ComputePodResources(pod, h_->ExtendedResourceNames())));
        return {PreFilterResult{}, Status::OK()};
    }

    // UP fit.go#fitsRequest: every insufficient resource is a reason
    Status Filter(CycleState &s, const Pod &pod, const NodeInfo &ni) override {
        PodResources tmp;
        const PodResources &r = resources_of(s, pod, h_, &tmp);
        std::vector<std::string> why;
        if (ni.pods + 1 > ni.allocatable.allowed_pod_number) why.push_back("Too many pods");
        bool any_scalar = false;
        for (const auto &kv : r.scalar) any_scalar |= kv.second != 0;
        if (r.cpu == 0 && r.mem == 0 && !any_scalar) {
            return why.empty() ? Status::OK() : Status(Code::Unschedulable, why);
        }
        if (r.cpu > 0 && r.cpu > ni.allocatable.milli_cpu - ni.requested.milli_cpu) why.push_back("Insufficient cpu");
        if (r.mem > 0 && r.mem > ni.allocatable.memory - ni.requested.memory) why.push_back("Insufficient memory");
        for (const auto &kv : r.scalar) {
            if (kv.second == 0) continue;
            auto a = ni.allocatable.scalar.find(kv.first);
            auto u = ni.requested.scalar.find(kv.first);
            const int64_t alloc = a == ni.allocatable.scalar.end() ? 0 : a->second;
            const int64_t used = u == ni.requested.scalar.end() ? 0 : u->second;
            if (kv.second > alloc - used) why.push_back("Insufficient " + kv.first);
        }
        return why.empty() ? Status::OK() : Status(Code::Unschedulable, why);
    }

    // The configured strategy (LeastAllocated by default) over the scoring resources (UP
    // least_allocated.go / most_allocated.go / requested_to_capacity_ratio.go, resource_allocation.go#
    // score): requested = NonZeroRequested + the pod's non-zero requests for
    // cpu / memory, Requested + the request for extended resources; resources with allocatable 0 are
    // skipped (their weight not counted)
    std::pair<int64_t, Status> Score(CycleState &s, const Pod &pod, const std::string &node) override {
        const NodeInfo *ni = node_of(h_, node);
        if (!ni) return {0, Status::AsError("node " + node + " not found")};
        PodResources tmp;
        const PodResources &r = resources_of(s, pod, h_, &tmp);
        int64_t alloc[QS_MAX_SCORE_RES], reqd[QS_MAX_SCORE_RES], weight[QS_MAX_SCORE_RES];
        int n = 0;
        for (const auto &rw : res_) {
            if (n == QS_MAX_SCORE_RES) break;
            const auto ar = alloc_request(*ni, r, rw.first, false, h_->ExtendedResourceNames());
            alloc[n] = ar.first;
            reqd[n] = ar.second;
            weight[n++] = rw.second;
        }
        return {FitStrategyScore(st_, alloc, reqd, weight, n), Status::OK()};
    }

   private:
    ResList res_;
    qs_scoring_strategy st_;
    Handle *h_;
};

// ---- NodeResourcesBalancedAllocation ---------------------------------------------------------
class BalancedAllocation final : public ScorePlugin {
   public:
    BalancedAllocation(const qs_config &cfg, Handle *h)
        : res_(balanced_list(cfg)), skip_be_(cfg.balanced_skip_besteffort != 0), h_(h) {}
    std::string Name() const override { return kNodeResourcesBalancedAllocation; }

    // UP balanced_allocation.go#balancedResourceScorer over the configured resources, float64:
    // fractions of Requested + the pod's requests (capped at 1) in list order, std = |f0 - f1| / 2 for
    // two, the population standard deviation (mean, sum of squared deviations, sqrt) for more,
    // int64((1 - std) * MaxNodeScore)
    std::pair<int64_t, Status> Score(CycleState &s, const Pod &pod, const std::string &node) override {
        const NodeInfo *ni = node_of(h_, node);
        if (!ni) return {0, Status::AsError("node " + node + " not found")};
        PodResources tmp;
        const PodResources &r = resources_of(s, pod, h_, &tmp);
        if (skip_be_ && r.qos == QS_QOS_BESTEFFORT) return {0, Status::OK()};
        double fr[QS_MAX_SCORE_RES], total = 0.0;
        int cnt = 0;
        for (const auto &rw : res_) {
            const auto ar = alloc_request(*ni, r, rw.first, true, h_->ExtendedResourceNames());
            if (ar.first == 0) continue;
            const double f = (double)ar.second / (double)ar.first;
            fr[cnt] = f > 1 ? 1 : f;
            total += fr[cnt++];
        }
        double sd = 0.0;
        if (cnt == 2) {
            sd = std::fabs((fr[0] - fr[1]) / 2);
        } else if (cnt > 2) {
            const double mean = total / (double)cnt;
            double sum = 0.0;
            for (int i = 0; i < cnt; ++i) sum = sum + (fr[i] - mean) * (fr[i] - mean);
            sd = std::sqrt(sum / (double)cnt);
        }
        const double scaled = (1 - sd) * (double)kMaxNodeScore;
        return {(int64_t)scaled, Status::OK()};
    }

   private:
    ResList res_;
    bool skip_be_;
    Handle *h_;
};

// ---- TaintToleration -------------------------------------------------------------------------
class TaintToleration final : public FilterPlugin, public ScorePlugin {
   public:
    explicit TaintToleration(Handle *h) : h_(h) {}
    std::string Name() const override { return kTaintToleration; }

    // UP taint_toleration.go#Filter: an untolerated NoSchedule / NoExecute taint rejects the node
    Status Filter(CycleState &, const Pod &pod, const NodeInfo &ni) override {
        for (const auto &t : ni.node.taints) {
            if (!hard_effect(t.effect)) continue;
            bool tol = false;
            for (const auto &x : pod.tolerations) tol = tol || tolerates(x, t);
            if (!tol)
                return Status(Code::UnschedulableAndUnresolvable,
                              {"node(s) had untolerated taint {" + t.key + ": " + t.value + "}"});
        }
        return Status::OK();
    }
    // UP taint_toleration.go#Score: intolerable PreferNoSchedule taints, counted against the
    // tolerations with effect "" or PreferNoSchedule (getAllTolerationPreferNoSchedule)
    std::pair<int64_t, Status> Score(CycleState &, const Pod &pod, const std::string &node) override {
        const NodeInfo *ni = node_of(h_, node);
        if (!ni) return {0, Status::AsError("node " + node + " not found")};
        int64_t n = 0;
        for (const auto &t : ni->node.taints) {
            if (t.effect != kPreferNoSchedule) continue;
            bool tol = false;
            for (const auto &x : pod.tolerations)
                tol = tol || ((x.effect.empty() || x.effect == kPreferNoSchedule) && tolerates(x, t));
            n += tol ? 0 : 1;
        }
        return {n, Status::OK()};
    }
    bool HasScoreExtensions() const override { return true; }
    Status NormalizeScore(CycleState &, const Pod &, NodeScoreList &scores) override {
        default_normalize(scores, /*reverse=*/true);
        return Status::OK();
    }

   private:
    Handle *h_;
};

// ---- NodeAffinity ----------------------------------------------------------------------------
bool term_matches(const NodeSelectorTerm &t, const std::map<std::string, std::string> &labels) {
    if (t.match_expressions.empty()) return false;  // UP nodeaffinity#NewNodeSelector: matches nothing
    for (const auto &r : t.match_expressions)
        if (!requirement_matches(r, labels)) return false;
    return true;
}

class NodeAffinity final : public FilterPlugin, public ScorePlugin {
   public:
    explicit NodeAffinity(Handle *h) : h_(h) {}
    std::string Name() const override { return kNodeAffinity; }

    // UP node_affinity.go#Filter: nodeSelector, then the required terms (OR of ANDs)
    Status Filter(CycleState &, const Pod &pod, const NodeInfo &ni) override {
        bool ok = true;
        for (const auto &kv : pod.node_selector) {
            auto it = ni.node.labels.find(kv.first);
            ok = ok && it != ni.node.labels.end() && it->second == kv.second;
        }
        if (ok && !pod.required_terms.empty()) {
            bool any = false;
            for (const auto &t : pod.required_terms) any = any || term_matches(t, ni.node.labels);
            ok = any;
        }
        return ok ? Status::OK()
                  : Status(Code::UnschedulableAndUnresolvable, {"node(s) didn't match Pod's node affinity/selector"});
    }
    // UP node_affinity.go#Score: sum of the weights of the matching preferred terms (weight 0 skipped)
    std::pair<int64_t, Status> Score(CycleState &, const Pod &pod, const std::string &node) override {
        const NodeInfo *ni = node_of(h_, node);
        if (!ni) return {0, Status::AsError("node " + node + " not found")};
        int64_t s = 0;
        for (const auto &pt : pod.preferred_terms)
            if (pt.weight > 0 && term_matches(pt.preference, ni->node.labels)) s += pt.weight;
        return {s, Status::OK()};
    }
    bool HasScoreExtensions() const override { return true; }
    Status NormalizeScore(CycleState &, const Pod &, NodeScoreList &scores) override {
        default_normalize(scores, /*reverse=*/false);
        return Status::OK();
    }

   private:
    Handle *h_;
};

// spec S8 (shape of UP queuesort/priority_sort.go#Less): QoS class, then priority, then FIFO
class QoSSort final : public QueueSortPlugin {
   public:
    std::string Name() const override { return kCPUQoSSort; }
    bool Less(const QueuedPodInfo &a, const QueuedPodInfo &b) const override {
        if (a.res.qos != b.res.qos) return a.res.qos > b.res.qos;
        if (a.pod.priority != b.pod.priority) return a.pod.priority > b.pod.priority;
        return a.arrival < b.arrival;
    }
};

const char *kProfileName[3] = {"besteffort", "burstable", "guaranteed"};

}  // namespace

Registry CPURegistry(const qs_config &cfg) { return CPURegistry(cfg, qs_scoring_strategy{}); }

Registry CPURegistry(const qs_config &cfg, const qs_scoring_strategy &st) {
    Registry r;
    r[kNodeResourcesFit] = [cfg, st](Handle *h) { return std::make_shared<NodeResourcesFit>(cfg, st, h); };
    r[kNodeResourcesBalancedAllocation] = [cfg](Handle *h) { return std::make_shared<BalancedAllocation>(cfg, h); };
    r[kTaintToleration] = [](Handle *h) { return std::make_shared<TaintToleration>(h); };
    r[kNodeAffinity] = [](Handle *h) { return std::make_shared<NodeAffinity>(h); };
    r[kCPUQoSSort] = [](Handle *) { return std::make_shared<QoSSort>(); };
    return r;
}

// One NodeResourcesFit per QoS class.  Upstream's factory receives the profile's PluginConfig args;
// PluginFactory here takes none, so the class's instance is registered under a key of its own
// (CPUFitKey) that the class's profile names.  Name() stays NodeResourcesFit.
std::string CPUFitKey(int qos) { return std::string(kNodeResourcesFit) + "/" + kProfileName[std::clamp(qos, 0, 2)]; }

Registry CPURegistry(const qs_config &cfg, const qs_scoring_strategy (&st)[3]) {
    Registry r = CPURegistry(cfg);
    for (int q = 0; q < 3; ++q) {
        const qs_scoring_strategy sq = st[q];
        r[CPUFitKey(q)] = [cfg, sq](Handle *h) { return std::make_shared<NodeResourcesFit>(cfg, sq, h); };
    }
    return r;
}

std::vector<Profile> CPUProfiles(const qs_config &cfg) { return CPUProfiles(cfg, false); }

std::vector<Profile> CPUProfiles(const qs_config &cfg, bool per_class_fit) {
    std::vector<Profile> out;
    for (int q = 0; q < 3; ++q) {
        const std::string fit = per_class_fit ? CPUFitKey(q) : std::string(kNodeResourcesFit);
        Profile p;
        p.scheduler_name = kProfileName[q];
        p.queue_sort = kCPUQoSSort;
        p.pre_filter = {{fit}};
        // upstream's default filter order: TaintToleration, NodeAffinity, ..., NodeResourcesFit
        if (cfg.enable_taint) p.filter.push_back({kTaintToleration});
        if (cfg.enable_affinity) p.filter.push_back({kNodeAffinity});
        p.filter.push_back({fit});
        auto add = [&](const std::string &n, int32_t w) { if (w > 0) p.score.push_back({n, w}); };
        add(fit, cfg.w_fit[q]);
        add(kNodeResourcesBalancedAllocation, cfg.w_bal[q]);
        if (cfg.enable_taint) add(kTaintToleration, cfg.w_taint);
        if (cfg.enable_affinity) add(kNodeAffinity, cfg.w_affinity);
        out.push_back(p);
    }
    return out;
}

std::string CPUProfileOf(const Pod &, const PodResources &r) { return kProfileName[std::clamp(r.qos, 0, 2)]; }

}  // namespace qsfw
