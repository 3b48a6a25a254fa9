// qos_strategy_driver.cpp — the CPU reference plugins with one NodeResourcesFit scoring strategy per
// QoS class (spec S9 "Strategy per QoS class": one profile per class, each with its own
// NodeResourcesFit instance), driven from tests/test_qos_strategy_cpu.py.  No GPU.
//
// A strategy is written <type> <n_shape> {<utilization> <score>}; three of them follow in class order
// (BestEffort, Burstable, Guaranteed).
//
//   qos_strategy_driver kat <qos> <3 strategies> <n> {<alloc> <reqd> <weight>}
//       -> the NodeResourcesFit score of a pod of class qos over the n entries
//          (host/cpu_plugins.hpp#FitStrategyScore with the class's strategy)
//   qos_strategy_driver loop <seed> <nodes> <pods> <zero_mod> <3 strategies>
//       -> spec/synth.md's config-4 cluster as k8s objects (tools/synth_objects.hpp), node i with
//          i % zero_mod == 3 given allocatable cpu 0, through the framework runtime (per-QoS profiles,
//          QoSSort, Filter / Score / NormalizeScore, selectHost, assume) with the CPU plugins of
//          CPURegistry(cfg, strategies) / CPUProfiles(cfg, true), scoring [cpu:1, memory:1,
//          amd.com/gpu:5] and Balanced over [cpu, memory, amd.com/gpu]: one line with every pod's node
//          index in arrival order, one with the chosen nodes' weighted totals (-1: unschedulable, or a
//          single feasible node, for which the runtime skips the score pass), and one with every
//          pod's QoS class
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../custom-k8s-scheduler_amd/host/cpu_plugins.hpp"
#include "../../tools/synth_objects.hpp"

using namespace qsfw;

static int read_strategy(char **argv, int at, int argc, qs_scoring_strategy *st) {
    if (at < 0 || at + 2 > argc) return -1;
    *st = qs_scoring_strategy{};
    st->type = atoi(argv[at++]);
    st->n_shape = atoi(argv[at++]);
    if (st->n_shape < 0 || st->n_shape > QS_MAX_SHAPE || at + 2 * st->n_shape > argc) return -1;
    for (int i = 0; i < st->n_shape; ++i) {
        st->shape[i].utilization = atoi(argv[at++]);
        st->shape[i].score = atoi(argv[at++]);
    }
    return at;
}

static int read_three(char **argv, int at, int argc, qs_scoring_strategy (&st)[3]) {
    for (int q = 0; q < 3; ++q) at = read_strategy(argv, at, argc, &st[q]);
    return at;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    qs_scoring_strategy st[3];
    if (std::strcmp(argv[1], "kat") == 0) {
        const int qos = atoi(argv[2]);
        if (qos < 0 || qos > 2) return 2;
        int at = read_three(argv, 3, argc, st);
        if (at < 0 || at >= argc) return 2;
        const int n = atoi(argv[at++]);
        if (n < 0 || n > QS_MAX_SCORE_RES || at + 3 * n > argc) return 2;
        int64_t a[QS_MAX_SCORE_RES], r[QS_MAX_SCORE_RES], w[QS_MAX_SCORE_RES];
        for (int i = 0; i < n; ++i) {
            a[i] = atoll(argv[at++]);
            r[i] = atoll(argv[at++]);
            w[i] = atoll(argv[at++]);
        }
        std::printf("%lld\n", (long long)FitStrategyScore(st[qos], a, r, w, n));
        return 0;
    }
    if (std::strcmp(argv[1], "loop") == 0 && argc >= 12) {
        const uint64_t seed = strtoull(argv[2], nullptr, 0);
        const uint32_t n = (uint32_t)atoi(argv[3]), p = (uint32_t)atoi(argv[4]);
        const uint32_t zero_mod = (uint32_t)atoi(argv[5]);
        if (read_three(argv, 6, argc, st) < 0) return 2;
        std::vector<Node> nodes;
        std::vector<Pod> pods;
        synth_objects(4, seed, n, p, &nodes, &pods);
        for (uint32_t i = 0; i < n; ++i)
            if (zero_mod && i % zero_mod == 3) nodes[i].allocatable[kCPU] = "0";
        qs_config cfg;
        qs_config_default(&cfg);
        cfg.enable_taint = cfg.enable_affinity = 1;
        cfg.n_fit_resources = 3;
        cfg.fit_resources[0] = {QS_RES_CPU, 1};
        cfg.fit_resources[1] = {QS_RES_MEMORY, 1};
        cfg.fit_resources[2] = {QS_RES_EXT0, 5};
        cfg.n_balanced_resources = 3;
        cfg.balanced_resources[0] = QS_RES_CPU;
        cfg.balanced_resources[1] = QS_RES_MEMORY;
        cfg.balanced_resources[2] = QS_RES_EXT0;
        Scheduler sched(CPURegistry(cfg, st), CPUProfiles(cfg, true), CPUProfileOf, 4);
        for (const auto &x : nodes) sched.AddNode(x);
        for (const auto &x : pods) sched.AddPod(x);
        std::vector<int> out(p, -2), qos(p, -1);
        std::vector<long long> tot(p, -1);
        for (const auto &r : sched.Run()) {
            if (r.status.code() == Code::Error) return 3;
            out[(size_t)r.arrival] = r.node_index;
            tot[(size_t)r.arrival] = (long long)r.total_score;
        }
        for (uint32_t j = 0; j < p; ++j) qos[j] = ComputePodResources(pods[j]).qos;
        for (uint32_t j = 0; j < p; ++j) std::printf(j ? " %d" : "%d", out[j]);
        std::printf("\n");
        for (uint32_t j = 0; j < p; ++j) std::printf(j ? " %lld" : "%lld", tot[j]);
        std::printf("\n");
        for (uint32_t j = 0; j < p; ++j) std::printf(j ? " %d" : "%d", qos[j]);
        std::printf("\n");
        return 0;
    }
    return 2;
}
