// mcmc_host.hpp -- the two pieces of the Monte Carlo optimiser's GPU sweeps that are plain host C++ (no HIP header: tests/cpp/mcmc_host_check.cpp builds
// them alone under the sanitizers): the proposal stream both optimisers consume and the level schedule the workgroup walks; for several
// chains (tests/cpp/mcmc_chains_host_check.cpp) the threaded drawing of their streams, the energy of a labelling and the choice of the best chain.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <random>
#include <vector>

#include "host_parallel.hpp"

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

// ---------------------------------------------------------------- several chains ("Chains")

// The proposals of K chains, chunk by chunk, in the layout k_mcmc_chains reads: sweep s of the chunk of chain k at ((size_t)k * stride + s) * T, the label
// of triplet t at pos[t] within it (its place in the schedule).  A chain's stream is advanced by one task of a parallel_for, so what is drawn depends
// neither on the number of threads nor on which thread takes which chain.
struct McmcChainStreams {
    std::vector<McmcProposals> streams;  // one per chain seed
    McmcChainStreams(const uint64_t *seeds, int K, double mcparam, int L) {
        streams.reserve((size_t)K);
        for (int k = 0; k < K; ++k) streams.emplace_back(seeds[k], mcparam, L);
    }
    int chains() const { return (int)streams.size(); }
    // the next `sweeps` sweeps of every chain into out (chains x stride x T, stride >= sweeps)
    void draw(uint16_t *out, int stride, int sweeps, int T, const int32_t *pos, int threads) {
        parallel_for(chains(), threads, [&](int k) {
            McmcProposals &p = streams[(size_t)k];
            for (int sw = 0; sw < sweeps; ++sw) {
                uint16_t *row = out + ((size_t)k * stride + sw) * T;
                for (int t = 0; t < T; ++t) row[(size_t)pos[(size_t)t]] = (uint16_t)p.next();
            }
        });
    }
};

// host threads that draw K chains: the workers of host_parallel.hpp, never more than 16, never more than there are chains
inline int mcmc_draw_threads(int K) { return std::max(1, std::min(std::min(host_workers(), 16), K)); }

// sweeps per chunk and chain: `asked` (MSMHIP_MCMC_CHUNK_SWEEPS; <= 0: as many as make half a million proposals per chain), reduced so that one chunk
// over all chains holds at most 2^23 proposals (16 MB) by default and 2^30 whatever was asked for; at least 1, at most iters
inline int mcmc_chunk_sweeps(long asked, int T, int iters, int K) {
    const long per_sweep = (long)std::max(T, 1) * std::max(K, 1);
    long n = asked;
    if (n <= 0) n = std::min(((long)1 << 19) / std::max(T, 1), ((long)1 << 23) / per_sweep);
    n = std::min(n, ((long)1 << 30) / per_sweep);
    return (int)std::max(1L, std::min(n, (long)iters));
}

// The table form of evaluateTotalCostSum (M/DiscreteCostFunction.cpp:55-77) over N + T terms: the unary terms summed in ascending order from 0.0, the
// (absent) pairwise sum 0.0, the triplet terms summed in ascending order from 0.0; the three added left to right.
inline double mcmc_energy_of_terms(const double *terms, int N, int T) {
    double u = 0.0, pw = 0.0, tc = 0.0;
    for (int i = 0; i < N; ++i) u += terms[i];
    for (int t = 0; t < T; ++t) tc += terms[(size_t)N + t];
    return u + pw + tc;
}

// the terms of a labelling over host tables (unary: L x N, tcosts: T x L^3), in the order k_mcmc_chain_terms writes them
inline void mcmc_energy_terms(const double *unary, const double *tcosts, const int32_t *triplets, int N, int L, int T, const int32_t *labeling, double *terms) {
    const size_t L1 = (size_t)L, L2 = L1 * L1, L3 = L2 * L1;
    for (int i = 0; i < N; ++i) terms[i] = unary[(size_t)labeling[i] * N + i];
    for (int t = 0; t < T; ++t) {
        const size_t la = (size_t)labeling[triplets[3 * (size_t)t]], lb = (size_t)labeling[triplets[3 * (size_t)t + 1]], lc = (size_t)labeling[triplets[3 * (size_t)t + 2]];
        terms[(size_t)N + t] = tcosts[(size_t)t * L3 + la * L2 + lb * L1 + lc];
    }
}

// std::min_element's rule, as MCMC::optimise itself picks among its eight costs: the first chain no later chain's energy is strictly smaller than.  Ties
// go to the lower index, a NaN never beats anything, nothing beats a NaN in slot 0.
inline int mcmc_best_chain(const double *energies, int K) {
    int best = 0;
    for (int k = 1; k < K; ++k)
        if (energies[k] < energies[best]) best = k;
    return best;
}

}  // namespace msm
