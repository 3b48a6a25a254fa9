// preempt_bench.cpp — time of the preemption dry run (spec S18) over the C ABI, on a table
// whose every node is filled to its pod limit (110 pods of 100m / 64Mi on 11,000m nodes, placed by exact
// streams with the registry on), next to a single-thread CPU walk of the same registry (read back with
// qs_node_pods / qs_nodes_read; the walk restates S18 under QS_PREEMPT_BY_PRIORITY and must give the
// device's node and victims per node).
//
//   preempt_bench [nodes] [calls] [rounds]   ->  one JSON line
//   per call: qs_preempt_pod alone (without / with the per-node array); per round: qs_preempt_pod, qs_evict
//   of every victim, qs_reserve of the pod.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/qsched.h"

using clk = std::chrono::steady_clock;
static double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }
#define OK(x)                                                                          \
    do {                                                                               \
        if ((x) != QS_OK) {                                                            \
            fprintf(stderr, "%s failed: %s\n", #x, qs_last_error(ctx));                \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

int main(int argc, char **argv) {
    const uint32_t n = argc > 1 ? (uint32_t)atoi(argv[1]) : 5000;
    const int calls = argc > 2 ? atoi(argv[2]) : 50, rounds = argc > 3 ? atoi(argv[3]) : 20;
    const uint32_t per_node = 110;
    const int64_t MI = 1 << 20;
    std::vector<int64_t> ac(n, 100 * per_node), am(n, 8192 * MI), mp(n, per_node);
    qs_node_soa in{};
    in.alloc_cpu = ac.data(); in.alloc_mem = am.data(); in.max_pods = mp.data();
    qs_config cfg;
    qs_config_default(&cfg);
    qs_ctx *ctx = nullptr;
    if (qs_open(&cfg, 0, &ctx) != QS_OK) { fprintf(stderr, "qs_open: %s\n", qs_last_error(nullptr)); return 1; }
    OK(qs_set_preemption(ctx, 1));
    OK(qs_nodes_load(ctx, &in, n));
    // fill: streams of at most 550,000 pods until every node holds its 110
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&] { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    const uint64_t total = (uint64_t)n * per_node;
    const auto f0 = clk::now();
    for (uint64_t done = 0; done < total;) {
        const uint32_t p = (uint32_t)std::min<uint64_t>(550000, total - done);
        std::vector<qs_pod> pods(p);
        std::memset(pods.data(), 0, sizeof(qs_pod) * p);
        for (auto &q : pods) {
            q.req_cpu = q.nz_cpu = 100; q.req_mem = q.nz_mem = 64 * MI;
            q.qos = (int32_t)(next() % 3); q.priority = (int32_t)(next() % 1000);
            q.tol_hard = q.tol_soft = ~0ull;
        }
        std::vector<int32_t> pl(p);
        OK(qs_schedule_stream(ctx, pods.data(), p, QS_MODE_EXACT, pl.data(), nullptr));
        for (int32_t v : pl) if (v < 0) { fprintf(stderr, "fill: a pod found no node\n"); return 1; }
        done += p;
    }
    const double fill_s = secs(f0, clk::now());
    qs_pod pod;
    std::memset(&pod, 0, sizeof pod);
    pod.req_cpu = pod.nz_cpu = 1000; pod.req_mem = pod.nz_mem = 640 * MI;
    pod.qos = QS_QOS_GUARANTEED; pod.priority = 10000; pod.tol_hard = pod.tol_soft = ~0ull;
    std::vector<qs_victim> vic(QS_MAX_VICTIMS);
    std::vector<int32_t> nv(n), nv_cpu(n);
    int32_t node = -2;
    uint32_t nvic = 0;
    auto t0 = clk::now();
    OK(qs_preempt_pod(ctx, &pod, &node, vic.data(), &nvic, nv.data()));  // (uploads the registry's device copy)
    const double first_s = secs(t0, clk::now());
    t0 = clk::now();
    for (int k = 0; k < calls; k++) OK(qs_preempt_pod(ctx, &pod, &node, vic.data(), &nvic, nullptr));
    const double call_s = secs(t0, clk::now()) / calls;
    t0 = clk::now();
    for (int k = 0; k < calls; k++) OK(qs_preempt_pod(ctx, &pod, &node, vic.data(), &nvic, nv.data()));
    const double call_nv_s = secs(t0, clk::now()) / calls;

    // ---- the CPU walk: registry and rows read back (untimed), then S18 in one thread ----
    std::vector<int64_t> rc(n), rm(n), np(n);
    qs_node_soa_out out{};
    out.req_cpu = rc.data(); out.req_mem = rm.data(); out.pods = np.data();
    OK(qs_nodes_read(ctx, &out, n));
    std::vector<uint32_t> off(n + 1, 0);
    std::vector<qs_victim> reg;
    reg.reserve(total);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t m = 0;
        OK(qs_node_pods(ctx, i, vic.data(), QS_MAX_VICTIMS, &m));
        reg.insert(reg.end(), vic.begin(), vic.begin() + m);
        off[i + 1] = off[i] + m;
    }
    auto imp = [](int32_t prio) { return (uint64_t)((int64_t)prio + (1LL << 31)); };
    const uint64_t P = imp(pod.priority);
    int32_t cpu_node = -1;
    double cpu_s = 1e30;
    for (int rep = 0; rep < 3; rep++) {
        t0 = clk::now();
        uint64_t best[5] = {~0ull, 0, 0, 0, 0};
        cpu_node = -1;
        for (uint32_t i = 0; i < n; i++) {
            const qs_victim *l = reg.data() + off[i];
            const uint32_t len = off[i + 1] - off[i];
            uint32_t first = len;
            while (first > 0 && imp(l[first - 1].priority) < P) --first;  // the suffix below the pod
            nv_cpu[i] = -1;
            if (first == len) continue;
            int64_t c = rc[i], m = rm[i], k = np[i];
            for (uint32_t s = first; s < len; s++) { c -= l[s].req_cpu; m -= l[s].req_mem; --k; }
            auto fits = [&](int64_t cc, int64_t mm, int64_t kk) {
                return kk < mp[i] && pod.req_cpu <= ac[i] - cc && pod.req_mem <= am[i] - mm;
            };
            if (!fits(c, m, k)) continue;
            uint64_t hi = 0, sum = 0, start = 0, cnt = 0;
            for (uint32_t s = first; s < len; s++) {
                if (fits(c + l[s].req_cpu, m + l[s].req_mem, k + 1)) { c += l[s].req_cpu; m += l[s].req_mem; ++k; continue; }
                if (!cnt) { hi = imp(l[s].priority); start = l[s].seq; }
                sum += imp(l[s].priority);
                ++cnt;
            }
            nv_cpu[i] = (int32_t)cnt;
            const uint64_t key[5] = {cnt ? 1u : 0u, hi, sum, cnt, ~start};
            if (cpu_node < 0 || std::lexicographical_compare(key, key + 5, best, best + 5)) {
                std::copy(key, key + 5, best);
                cpu_node = (int32_t)i;
            }
        }
        cpu_s = std::min(cpu_s, secs(t0, clk::now()));
    }
    const bool match = cpu_node == node && nv_cpu == nv;

    // ---- full rounds ----
    t0 = clk::now();
    uint64_t evicted = 0;
    for (int k = 0; k < rounds; k++) {
        OK(qs_preempt_pod(ctx, &pod, &node, vic.data(), &nvic, nullptr));
        if (node < 0) { fprintf(stderr, "round %d: no candidate\n", k); return 1; }
        for (uint32_t v = 0; v < nvic; v++) OK(qs_evict(ctx, (uint32_t)node, vic[v].seq));
        OK(qs_reserve(ctx, (uint32_t)node, &pod));
        evicted += nvic;
    }
    const double round_s = secs(t0, clk::now()) / rounds;
    printf("{\"nodes\": %u, \"pods_per_node\": %u, \"fill_s\": %.3f, \"first_call_ms\": %.3f, \"call_us\": %.1f, "
           "\"call_with_per_node_us\": %.1f, \"round_us\": %.1f, \"victims_per_round\": %.1f, "
           "\"cpu_walk_1thread_us\": %.1f, \"cpu_walk_matches_device\": %s}\n",
           n, per_node, fill_s, first_s * 1e3, call_s * 1e6, call_nv_s * 1e6, round_s * 1e6, (double)evicted / rounds,
           cpu_s * 1e6, match ? "true" : "false");
    qs_close(ctx);
    return match ? 0 : 1;
}
