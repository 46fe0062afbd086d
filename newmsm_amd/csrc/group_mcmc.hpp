// group_mcmc.hpp -- gMSM with the Monte Carlo optimiser, subject by subject (group_mcmc.cpp, group_mcmc_kernels.hip).  The group energy
// restricted to one subject, the other subjects' labels held fixed, is a unary table (the node's pair costs against its partners' current labels) plus
// the subject's strain triplets: the form MCMC::optimise reads (M/mcmc_opt.h:31-134).  The first part of this header is plain host C++ without a HIP
// header -- the incidence of the pair list, the seed rule and the acceptance rule; tests/cpp/group_mcmc_host_check.cpp builds it alone under the
// sanitizers.  The kernels' arguments follow behind GROUP_MCMC_HOST_ONLY.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace msm {

// The incidence of a pair list over `nodes` nodes as CSR: for node n the pair indices p with pairs[2p] == n or pairs[2p + 1] == n, ascending -- a pair
// that names a node twice is listed once.  O(P): a count, a prefix sum, a fill in ascending p.  Returns false when a pair names a node outside [0, nodes).
inline bool group_mcmc_incidence(const int32_t *pairs, int64_t P, int nodes, std::vector<int32_t> &ptr, std::vector<int32_t> &idx) {
    ptr.assign((size_t)nodes + 1, 0);
    for (int64_t p = 0; p < P; ++p) {
        const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || a >= nodes || b < 0 || b >= nodes) return false;
        ++ptr[(size_t)a + 1];
        if (b != a) ++ptr[(size_t)b + 1];
    }
    for (int n = 0; n < nodes; ++n) ptr[(size_t)n + 1] += ptr[(size_t)n];
    idx.assign((size_t)ptr[(size_t)nodes], 0);
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int64_t p = 0; p < P; ++p) {
        const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        idx[(size_t)fill[(size_t)a]++] = (int32_t)p;
        if (b != a) idx[(size_t)fill[(size_t)b]++] = (int32_t)p;
    }
    return true;
}

// Chain k of subject s in pass p of iteration `it` of a run over S subjects: seed + it + 1000003 k + 15485863 (p S + s), modulo 2^64.  Chain 0 of
// subject 0 in pass 0 is the pairwise loops' seed + it; the chains of a block are theirs (seed + it + 1000003 k).
inline uint64_t group_mcmc_seed(uint64_t seed, int it, int k, int pass, int S, int s) {
    return seed + (uint64_t)(int64_t)it + (uint64_t)1000003 * (uint64_t)k + (uint64_t)15485863 * ((uint64_t)pass * (uint64_t)S + (uint64_t)s);
}

// The best chain's labelling replaces the subject's only when its energy is strictly below the start's; a NaN on either side compares false.
inline bool group_mcmc_accept(double start, double best) { return best < start; }

}  // namespace msm

#ifndef GROUP_MCMC_HOST_ONLY
#include "internal.hpp"

namespace msm {

// Subject s of a group: entries [e0, e0 + E) of the incidence CSR belong to its N nodes.  The queries of the segment (v, l) -- the incident pairs of
// node s N + v, ascending, the node's own slot taking l and the partner's its current label -- start at seg(v, l) = (inc_ptr[s N + v] - e0) L + l deg(v).
struct GroupCondArgs {
    const int32_t *pairs;    // P x 2
    const int32_t *inc_ptr;  // S N + 1
    const int32_t *inc_idx;  // inc_ptr[S N]
    const int32_t *lab;      // S N
    int S, N, L, s;
    int64_t P;
    int32_t e0, E;                // the subject's entries
    int32_t *qp, *qa, *qb;        // E x L queries
    int32_t *seg_off;             // N L + 1
    int *status;
};
int launch_group_cond_queries(msm_ctx *ctx, const GroupCondArgs &a);
// U[l N + v] = the segment's values added in order from 0.0, one lane per (v, l)
int launch_group_cond_sum(msm_ctx *ctx, const int32_t *seg_off, const double *vals, int N, int L, int64_t nvals, double *U, int *status);
// the queries of the subject's triplets [t0, t1) (local numbers) over all L^3 label triples: entry ((t - t0) L + a) L^2 + b L + c asks (s Tc + t, a, b, c)
int launch_group_triplet_queries(msm_ctx *ctx, int s, int Tc, int L, int t0, int t1, int32_t *qt, int32_t *qa, int32_t *qb, int32_t *qc);

}  // namespace msm
#endif
