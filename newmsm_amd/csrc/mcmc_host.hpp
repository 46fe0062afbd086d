// mcmc_host.hpp -- the two pieces of the Monte Carlo optimiser's GPU sweeps that are plain host C++ (no HIP header: tests/cpp/mcmc_host_check.cpp builds
// them alone under the sanitizers): the proposal stream both optimisers consume and the level schedule the workgroup walks.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <random>
#include <vector>

namespace msm {

// The proposals of MCMC::optimise (M/mcmc_opt.h:31-134) in visit order: one draw of std::geometric_distribution<>(mcparam) from std::mt19937(seed) per
// visited triplet, drawn again while it is not a label.  The host sweeps (regtools.cpp) and the GPU sweeps take their labels from here and nowhere else.
struct McmcProposals {
    std::mt19937 gen;
    std::geometric_distribution<> distribution;
    int L;
    McmcProposals(uint64_t seed, double mcparam, int L_) : gen((std::mt19937::result_type)seed), distribution(mcparam), L(L_) {}
    int next() {
        int label;
        do { label = distribution(gen); } while (label >= L);
        return label;
    }
    void fill(uint16_t *out, size_t n) {  // L <= 65535 (checked by the callers)
        for (size_t i = 0; i < n; ++i) out[i] = (uint16_t)next();
    }
};

// Triplet t depends on the earlier triplets that share a node with it: level(t) = 1 + the highest level among them (0-based here: a triplet nothing
// precedes has level 0).  Triplets of one level touch disjoint nodes, so walking the levels in order, the triplets of a level in any order, gives the
// serial sweep's labelling.  Holds for any list: a triplet that names a node twice depends on nothing because of it, two triplets with the same nodes
// fall into consecutive levels.
struct McmcSchedule {
    std::vector<int32_t> level;      // T
    std::vector<int32_t> order;      // T: the triplets by level, ascending index within a level
    std::vector<int32_t> level_off;  // levels + 1 offsets into order
    int levels() const { return (int)level_off.size() - 1; }
    int widest() const {
        int w = 0;
        for (int l = 0; l < levels(); ++l) w = std::max(w, level_off[(size_t)l + 1] - level_off[(size_t)l]);
        return w;
    }
};

inline void mcmc_build_schedule(const int32_t *triplets /* T x 3, nodes in [0, N) */, int N, int T, McmcSchedule &s) {
    s.level.assign((size_t)T, 0);
    s.order.assign((size_t)T, 0);
    std::vector<int32_t> last((size_t)N, -1);  // per node: the level of the latest triplet so far that touches it
    int levels = 0;
    for (int t = 0; t < T; ++t) {
        const int32_t a = triplets[3 * (size_t)t], b = triplets[3 * (size_t)t + 1], c = triplets[3 * (size_t)t + 2];
        const int32_t lv = 1 + std::max(last[(size_t)a], std::max(last[(size_t)b], last[(size_t)c]));
        s.level[(size_t)t] = lv;
        last[(size_t)a] = last[(size_t)b] = last[(size_t)c] = lv;
        levels = std::max(levels, lv + 1);
    }
    s.level_off.assign((size_t)levels + 1, 0);
    for (int t = 0; t < T; ++t) ++s.level_off[(size_t)s.level[(size_t)t] + 1];
    for (int l = 0; l < levels; ++l) s.level_off[(size_t)l + 1] += s.level_off[(size_t)l];
    std::vector<int32_t> fill(s.level_off.begin(), s.level_off.end() - 1);
    for (int t = 0; t < T; ++t) s.order[(size_t)fill[(size_t)s.level[(size_t)t]]++] = t;  // ascending index within a level
}

}  // namespace msm
