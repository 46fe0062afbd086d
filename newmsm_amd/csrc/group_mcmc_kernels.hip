// group_mcmc_kernels.hip -- the device side of a gMSM block (group_mcmc.hpp): the queries of a subject's conditional unary table, the
// sums of their answers, and the queries of its triplet table.  The pair and triplet costs themselves are k_group_pairwise / k_group_triplet through
// their launchers, unchanged; the sweeps are k_mcmc_chains.  Every loop here is bounded by counts the host computed (the incidence CSR, L), nothing
// spins or waits for another workgroup, the only global atomic is the status word's atomicMin on an error path, and whatever is out of range indexes
// nothing: the host zeroes the query arrays before k_group_cond_queries, so a slot an erring lane leaves out asks the valid query (0, 0, 0).
#include "group_mcmc.hpp"

namespace msm {

namespace {

__device__ __forceinline__ void raise_status(int *status, int code) { atomicMin(status, code); }

// One lane per incidence entry of the subject (the queries of that pair for all L labels of the node; consecutive lanes write consecutive slots of a
// segment), and one lane per segment offset.
__global__ __launch_bounds__(256) void k_group_cond_queries(GroupCondArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nodes = (int64_t)a.S * a.N, segs = (int64_t)a.N * a.L;
    const int first = a.s * a.N;
    if (i <= segs) {
        if (i == segs) {
            a.seg_off[i] = (int32_t)((int64_t)a.E * a.L);
        } else {
            const int v = (int)(i / a.L), l = (int)(i - (int64_t)v * a.L);
            const int base = a.inc_ptr[first + v], deg = a.inc_ptr[first + v + 1] - base;
            if (base < a.e0 || deg < 0 || (int64_t)base + deg > (int64_t)a.e0 + a.E) {
                raise_status(a.status, MSM_ERR_INVALID);
                a.seg_off[i] = 0;
            } else {
                a.seg_off[i] = (int32_t)((int64_t)(base - a.e0) * a.L + (int64_t)l * deg);
            }
        }
    }
    if (i >= a.E) return;
    const int e = a.e0 + (int)i;
    const int p = a.inc_idx[e];
    if (p < 0 || p >= a.P) return raise_status(a.status, MSM_ERR_INVALID);
    const int na = a.pairs[2 * (size_t)p], nb = a.pairs[2 * (size_t)p + 1];
    if (na < 0 || na >= nodes || nb < 0 || nb >= nodes) return raise_status(a.status, MSM_ERR_INVALID);
    const bool a_in = na >= first && na < first + a.N, b_in = nb >= first && nb < first + a.N;
    if (a_in == b_in) return raise_status(a.status, MSM_ERR_INVALID);  // a pair joins two different subjects (estimate_pairs)
    const int own = a_in ? na : nb, partner = a_in ? nb : na;
    const int lp = a.lab[partner];
    const int base = a.inc_ptr[own], deg = a.inc_ptr[own + 1] - base, j = e - base;
    if (lp < 0 || lp >= a.L || base < a.e0 || j < 0 || j >= deg || (int64_t)base + deg > (int64_t)a.e0 + a.E) return raise_status(a.status, MSM_ERR_INVALID);
    const size_t seg0 = (size_t)(base - a.e0) * (size_t)a.L + (size_t)j;
    for (int l = 0; l < a.L; ++l) {
        const size_t q = seg0 + (size_t)l * (size_t)deg;  // < E L: base - e0 + deg <= E
        a.qp[q] = p;
        a.qa[q] = a_in ? l : lp;
        a.qb[q] = a_in ? lp : l;
    }
}

// One lane per (v, l): its segment added in order from 0.0, each addition rounded (-ffp-contract=off, and there is nothing to contract).  No atomic and
// no cross-lane sum: the order is the definition.  A node without incident pairs has an empty segment and gets exactly 0.0.
__global__ __launch_bounds__(256) void k_group_cond_sum(const int32_t *__restrict__ seg_off, const double *__restrict__ vals, int N, int L, int64_t nvals,
                                                        double *__restrict__ U, int *status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * L) return;
    const int v = (int)(i / L), l = (int)(i - (int64_t)v * L);
    const int64_t b = seg_off[i], e = seg_off[i + 1];
    double sum = 0.0;
    if (b < 0 || e < b || e > nvals) raise_status(status, MSM_ERR_INVALID);
    else
        for (int64_t k = b; k < e; ++k) sum += vals[k];
    U[(size_t)l * N + v] = sum;
}

__global__ __launch_bounds__(256) void k_group_triplet_queries(int s, int Tc, int L, int t0, int64_t n, int32_t *__restrict__ qt, int32_t *__restrict__ qa,
                                                               int32_t *__restrict__ qb, int32_t *__restrict__ qc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t L2 = (int64_t)L * L, L3 = L2 * L;
    const int64_t t = i / L3, r = i - t * L3;
    const int la = (int)(r / L2), lb = (int)((r - la * L2) / L), lc = (int)(r - la * L2 - (int64_t)lb * L);
    qt[i] = s * Tc + t0 + (int)t;
    qa[i] = la;
    qb[i] = lb;
    qc[i] = lc;
}

}  // namespace

int launch_group_cond_queries(msm_ctx *ctx, const GroupCondArgs &a) {
    const int64_t segs = (int64_t)a.N * a.L, lanes = std::max<int64_t>(segs + 1, a.E);
    if (a.S < 1 || a.N < 1 || a.L < 1 || a.s < 0 || a.s >= a.S || a.E < 0 || a.e0 < 0 || (int64_t)a.E * a.L > INT32_MAX || (lanes + 255) / 256 > INT32_MAX)
        return fail(MSM_ERR_INVALID, "msm_group_conditional_unary: bad launch (subject %d of %d, %d incidence entries, %d labels)", a.s, a.S, a.E, a.L);
    hipLaunchKernelGGL(k_group_cond_queries, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, a);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_group_cond_sum(msm_ctx *ctx, const int32_t *seg_off, const double *vals, int N, int L, int64_t nvals, double *U, int *status) {
    const int64_t segs = (int64_t)N * L;
    if (N < 1 || L < 1 || nvals < 0 || (segs + 255) / 256 > INT32_MAX) return fail(MSM_ERR_INVALID, "msm_group_conditional_unary: bad launch (%d nodes, %d labels)", N, L);
    hipLaunchKernelGGL(k_group_cond_sum, dim3((unsigned)((segs + 255) / 256)), dim3(256), 0, ctx->stream, seg_off, vals, N, L, nvals, U, status);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_group_triplet_queries(msm_ctx *ctx, int s, int Tc, int L, int t0, int t1, int32_t *qt, int32_t *qa, int32_t *qb, int32_t *qc) {
    const int64_t n = (int64_t)(t1 - t0) * L * L * L;
    if (n <= 0) return MSM_OK;
    if (s < 0 || t0 < 0 || t1 > Tc || n > INT32_MAX) return fail(MSM_ERR_INVALID, "msm_group_subject_triplet_table: bad launch (triplets [%d, %d) of %d)", t0, t1, Tc);
    hipLaunchKernelGGL(k_group_triplet_queries, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, s, Tc, L, t0, n, qt, qa, qb, qc);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
