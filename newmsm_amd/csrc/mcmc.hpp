// mcmc.hpp -- the Monte Carlo optimiser's sweeps (MCMC::optimise, M/mcmc_opt.h:31-134) on the GPU: the kernel's arguments and the host loop around it
// (mcmc.cpp, mcmc_kernels.hip).  The proposal stream and the level schedule are plain host code: mcmc_host.hpp.
#pragma once

#include "internal.hpp"
#include "mcmc_draw.hpp"
#include "mcmc_host.hpp"

namespace msm {

constexpr int kMcmcThreads = 512;     // one workgroup; a wider level is walked in strides
constexpr int kMcmcMaxNodes = 80000;  // uint16 labels of all nodes in the workgroup's 160 KB of LDS

struct McmcArgs {
    const double *U;           // L x N
    const double *tc;          // T x L^3
    const int4 *sched;         // T records in schedule order: {triplet, node A, node B, node C}
    const int32_t *level_off;  // levels + 1
    const uint16_t *prop;      // sweeps x T proposals, each sweep's in schedule order
    int32_t *labeling;         // N, read at the start and written at the end
    int N, L, T, levels, sweeps;
    int *status;
};

// K chains side by side, workgroup k walks chain k: a.labeling holds K x N labels, a.prop the chunk of every chain, sweep s of chain k at
// ((size_t)k * chunk_sweeps + s) * T; the schedule and both tables are shared.  A single chain is K = 1: there is no other sweeps kernel.
constexpr int kMcmcMaxChains = 256;
struct McmcChainArgs {
    McmcArgs a;
    int chains, chunk_sweeps;
};
int launch_mcmc_chains(msm_ctx *ctx, const McmcChainArgs &c);
// the terms of every chain's energy, terms[k * (N + T) + ...]: U[lab[i] * N + i] for i < N, then tc[t][la][lb][lc] for t < T (a.sweeps, a.prop unused)
int launch_mcmc_chain_terms(msm_ctx *ctx, const McmcChainArgs &c, double *terms);

// The proposals drawn on the device (mcmc_draw.hpp, mcmc_draw_kernels.hip; DESIGN.md 5.16 "Proposals on the device"): workgroup k continues chain k's
// stream from rec[k] by `need` accepted proposals and stores them where McmcChainStreams::draw puts them: number j at
// prop[((size_t)k * chunk_sweeps + j / T) * T + pos[j % T]] (pos null: j % T itself).
constexpr int kMcmcDrawThreads = 320;      // five wavefronts: a candidate of the 312 per thread
constexpr int kMcmcDrawLdsLabels = 4096;   // thresholds of up to this many labels (32 KB) are copied to LDS, more are read from global memory
struct McmcDrawRecord {
    uint32_t state[kMtWords];  // the engine's words; the current block's once the first block has been generated
    uint32_t consumed;         // candidates of that block already taken (312: none left, as in a seeded engine)
    uint32_t pad;
    unsigned long long candidates, accepted;  // counted over the launches since the record was written by the host
};
struct McmcDrawArgs {
    McmcDrawRecord *rec;   // chains
    const uint64_t *thr;   // L thresholds (mcmc_draw_thresholds)
    const int32_t *pos;    // T, or null
    uint16_t *prop;        // chains x chunk_sweeps x T
    int chains, L, T, chunk_sweeps;
    uint32_t need;         // proposals per chain in this launch: sweeps x T <= chunk_sweeps x T
    long max_blocks;       // 312-candidate blocks a chain may generate in this launch (mcmc_draw_block_bound)
    int *status;           // raised (atomicMin) to MSM_ERR_CAPACITY by a chain that reaches max_blocks first
};
int launch_mcmc_draw(msm_ctx *ctx, const McmcDrawArgs &d, hipStream_t stream);

// `iters` sweeps of K chains from one start (chain k: seeds[k]) on the device over tables that lie there (d_U: L x N, d_tc: T x L^3).  labeling (host, N)
// is the start and receives chain *best's labelling (best may be null); labelings (host, K x N) and energies (host, K) may be null.  The energies are
// computed when K > 1 or they are asked for.  The arguments have been checked by the caller (mcmc_check_arguments; 1 <= K <= kMcmcMaxChains:
// mcmc_check_chains).  Complete on return; labeling is written only when the call succeeds.  `what` names the call in what the kernels' status reports.
int mcmc_run_device_chains(msm_ctx *ctx, const double *d_U, const double *d_tc, const int32_t *triplets, int N, int L, int T, double mcparam, int iters,
                           const uint64_t *seeds, int K, int32_t *labeling, int32_t *labelings, double *energies, int32_t *best,
                           const char *what = "msm_mcmc_optimise_chains_gpu");
// A single chain: mcmc_run_device_chains with K = 1, reported as msm_mcmc_optimise_gpu.  Without sweeps or triplets it returns at once (the context's
// stats stay the previous call's).
int mcmc_run_device(msm_ctx *ctx, const double *d_U, const double *d_tc, const int32_t *triplets, int N, int L, int T, double mcparam, int iters, uint64_t seed,
                    int32_t *labeling);
int upload_in_pieces(msm_ctx *ctx, void *dst, const void *src, size_t bytes);  // host -> device through the staging blocks, 16 MB at a time (mcmc.cpp)
int mcmc_check_chains(const uint64_t *seeds, int K);  // 1 <= K <= kMcmcMaxChains and seeds given, or MSM_ERR_INVALID
int mcmc_check_node_count(const char *what, int N);   // N <= kMcmcMaxNodes, or MSM_ERR_CAPACITY reported under the name `what`
// the sweeps of msm_mcmc_optimise over checked arguments (regtools.cpp)
void mcmc_sweeps_host(const double *unary, const double *tcosts, const int32_t *triplets, int N, int L, int T, double mcparam, int iters, uint64_t seed,
                      int32_t *labeling);
// the checks of msm_mcmc_optimise on mcparam, the labeling and the triplets, with its messages
int mcmc_check_arguments(const int32_t *triplets, int N, int L, int T, double mcparam, const int32_t *labeling);

}  // namespace msm
