// mcmc_kernels.hip -- the sweeps of MCMC::optimise (M/mcmc_opt.h:31-134) on one workgroup, level by level (mcmc.hpp).
//
// The serial sweep visits the triplets in order, and a visit reads and writes the labels of its three nodes only.  The host has sorted the triplets into
// levels whose members touch disjoint nodes (mcmc_build_schedule): the workgroup walks the levels in order with a barrier between them, one triplet
// per thread, the labelling in LDS.  Whatever the threads of a level do among themselves, every visit sees the labels the serial sweep would show it.
// Per visit the arithmetic is the host function's (regtools.cpp: msm_mcmc_optimise) and nothing else; the file is built with -ffp-contract=off like the
// rest of the library, and the double division is the correctly rounded one.
//
// A level is a chain of dependent latencies and nothing else: barrier, schedule record and proposal (L2), three labels (LDS), fourteen table values (L2 /
// HBM), the labels written back.  (Fetching the next level's record and proposal ahead of the barrier was tried and measured: 2.02 against 2.04 us per
// level at ico4, not told apart; the plain loop stays.)
//
// Several chains (k_mcmc_chains, k_mcmc_chain_terms; DESIGN.md 5.16 "Chains"): K workgroups, each the loop above on a labelling and a proposal stream of
// its own over the shared schedule and tables; they exchange nothing.  The terms of every chain's energy are written out and summed on the host.
#include "mcmc.hpp"

namespace msm {

namespace {

__device__ __forceinline__ void raise_status(int *status, int code) { atomicMin(status, code); }

// one visit: r = {triplet, node A, node B, node C}, label = the proposal
__device__ __forceinline__ void mcmc_visit(const McmcArgs &a, uint16_t *s_lab, const int4 r, const unsigned label) {
    const unsigned N = (unsigned)a.N, L = (unsigned)a.L;
    const unsigned A = (unsigned)r.y, B = (unsigned)r.z, C = (unsigned)r.w;
    if (A >= N || B >= N || C >= N || label >= L || (unsigned)r.x >= (unsigned)a.T) {  // (the host has checked: what is out of range indexes nothing)
        raise_status(a.status, MSM_ERR_INVALID);
        return;
    }
    const size_t L1 = (size_t)L, L2 = L1 * L1, L3 = L2 * L1, Ns = (size_t)N;
    const unsigned ca = s_lab[A], cb = s_lab[B], cc = s_lab[C];
    const double *__restrict__ tc = a.tc + (size_t)r.x * L3;
    const double *__restrict__ U = a.U;
    // the eight table values and the six unary values are independent of one another: all loads are issued before the first use
    const size_t a0 = (size_t)ca * L2, a1 = (size_t)label * L2, b0 = (size_t)cb * L1, b1 = (size_t)label * L1;
    const double t0 = tc[a0 + b0 + cc], t1 = tc[a0 + b0 + label], t2 = tc[a0 + b1 + cc], t3 = tc[a0 + b1 + label];
    const double t4 = tc[a1 + b0 + cc], t5 = tc[a1 + b0 + label], t6 = tc[a1 + b1 + cc], t7 = tc[a1 + b1 + label];
    const double ua0 = U[(size_t)ca * Ns + A], ua1 = U[(size_t)label * Ns + A];
    const double ub0 = U[(size_t)cb * Ns + B], ub1 = U[(size_t)label * Ns + B];
    const double uc0 = U[(size_t)cc * Ns + C], uc1 = U[(size_t)label * Ns + C];
    // costs[4a + 2b + c]: a/b/c = 1 takes the proposed label for node A/B/C; the sum of three left to right, one division, one addition
    double costs[8];
    costs[0] = t0 + (ua0 + ub0 + uc0) / 3.0;
    costs[1] = t1 + (ua0 + ub0 + uc1) / 3.0;
    costs[2] = t2 + (ua0 + ub1 + uc0) / 3.0;
    costs[3] = t3 + (ua0 + ub1 + uc1) / 3.0;
    costs[4] = t4 + (ua1 + ub0 + uc0) / 3.0;
    costs[5] = t5 + (ua1 + ub0 + uc1) / 3.0;
    costs[6] = t6 + (ua1 + ub1 + uc0) / 3.0;
    costs[7] = t7 + (ua1 + ub1 + uc1) / 3.0;
    // std::min_element: the first index no later cost is strictly smaller than (a NaN is never smaller, nothing is smaller than a NaN)
    int best = 0;
    double lowest = costs[0];
#pragma unroll
    for (int k = 1; k < 8; ++k)
        if (costs[k] < lowest) {
            lowest = costs[k];
            best = k;
        }
    if (best & 4) s_lab[A] = (uint16_t)label;
    if (best & 2) s_lab[B] = (uint16_t)label;
    if (best & 1) s_lab[C] = (uint16_t)label;
}

// K chains (a single chain is K = 1): workgroup k walks the levels on chain k's labelling and proposals, over the shared schedule and tables, a level
// wider than the workgroup in strides.  The workgroups never meet: no atomic but the status word's on the error path, every loop bounded by the host's counts.
__global__ __launch_bounds__(kMcmcThreads) void k_mcmc_chains(McmcChainArgs c) {
    extern __shared__ __align__(16) uint16_t s_lab[];  // N labels of this chain
    const McmcArgs &a = c.a;
    const int tid = (int)threadIdx.x, k = (int)blockIdx.x;
    if (k >= c.chains) return;  // (the whole workgroup)
    int32_t *__restrict__ labeling = a.labeling + (size_t)k * a.N;
    for (int i = tid; i < a.N; i += kMcmcThreads) {
        int l = labeling[i];
        if ((unsigned)l >= (unsigned)a.L) {
            raise_status(a.status, MSM_ERR_INVALID);
            l = 0;
        }
        s_lab[i] = (uint16_t)l;
    }
    __syncthreads();
    for (int s = 0; s < a.sweeps; ++s) {
        const uint16_t *__restrict__ prop = a.prop + ((size_t)k * c.chunk_sweeps + s) * a.T;  // this chain's proposals for sweep s of the chunk
        for (int lv = 0; lv < a.levels; ++lv) {
            const int begin = a.level_off[lv], end = a.level_off[lv + 1];
            for (int i = begin + tid; i < end; i += kMcmcThreads) mcmc_visit(a, s_lab, a.sched[i], prop[i]);
            __syncthreads();
        }
    }
    for (int i = tid; i < a.N; i += kMcmcThreads) labeling[i] = (int)s_lab[i];
}

// the N + T terms of every chain's energy, a term per thread; they are summed on the host in the reference's order
__global__ __launch_bounds__(256) void k_mcmc_chain_terms(McmcChainArgs c, double *__restrict__ terms) {
    const McmcArgs &a = c.a;
    const int k = (int)blockIdx.y;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= c.chains || j >= (long)a.N + a.T) return;
    const unsigned N = (unsigned)a.N, L = (unsigned)a.L;
    const int32_t *__restrict__ lab = a.labeling + (size_t)k * a.N;
    double *__restrict__ out = terms + (size_t)k * ((size_t)a.N + a.T);
    if (j < (long)a.N) {
        const unsigned l = (unsigned)lab[j];
        if (l >= L) {
            raise_status(a.status, MSM_ERR_INVALID);
            out[j] = 0.0;
            return;
        }
        out[j] = a.U[(size_t)l * N + (size_t)j];
        return;
    }
    const int4 r = a.sched[j - a.N];  // {triplet, node A, node B, node C}: the term goes to the triplet's place in list order
    if ((unsigned)r.x >= (unsigned)a.T) {
        raise_status(a.status, MSM_ERR_INVALID);
        return;
    }
    if ((unsigned)r.y >= N || (unsigned)r.z >= N || (unsigned)r.w >= N) {
        raise_status(a.status, MSM_ERR_INVALID);
        out[(size_t)a.N + r.x] = 0.0;
        return;
    }
    const unsigned la = (unsigned)lab[r.y], lb = (unsigned)lab[r.z], lc = (unsigned)lab[r.w];
    if (la >= L || lb >= L || lc >= L) {
        raise_status(a.status, MSM_ERR_INVALID);
        out[(size_t)a.N + r.x] = 0.0;
        return;
    }
    const size_t L1 = (size_t)L, L2 = L1 * L1, L3 = L2 * L1;
    out[(size_t)a.N + r.x] = a.tc[(size_t)r.x * L3 + (size_t)la * L2 + (size_t)lb * L1 + lc];
}

}  // namespace

int launch_mcmc_chains(msm_ctx *ctx, const McmcChainArgs &c) {
    const McmcArgs &a = c.a;
    if (a.sweeps <= 0 || a.T <= 0 || a.levels <= 0) return MSM_OK;
    if (c.chains < 1 || c.chains > kMcmcMaxChains || a.sweeps > c.chunk_sweeps) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise_chains_gpu: bad launch (%d chains, %d sweeps of %d)", c.chains, a.sweeps, c.chunk_sweeps);
    MSM_TRY(mcmc_check_node_count("msm_mcmc_optimise_gpu", a.N));
    const size_t lds = (sizeof(uint16_t) * (size_t)a.N + 15) & ~(size_t)15;
    if (lds > 64 * 1024) MSM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mcmc_chains), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_mcmc_chains, dim3((unsigned)c.chains), dim3(kMcmcThreads), lds, ctx->stream, c);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_mcmc_chain_terms(msm_ctx *ctx, const McmcChainArgs &c, double *terms) {
    const McmcArgs &a = c.a;
    if (c.chains < 1 || c.chains > kMcmcMaxChains || a.N <= 0 || a.T < 0) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise_chains_gpu: bad launch (%d chains)", c.chains);
    const long n = (long)a.N + a.T;
    hipLaunchKernelGGL(k_mcmc_chain_terms, dim3((unsigned)((n + 255) / 256), (unsigned)c.chains), dim3(256), 0, ctx->stream, c, terms);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
