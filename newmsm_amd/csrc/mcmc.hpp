// mcmc.hpp -- the Monte Carlo optimiser's sweeps (MCMC::optimise, M/mcmc_opt.h:31-134) on the GPU: the kernel's arguments and the host loop around it
// (mcmc.cpp, mcmc_kernels.hip).  The proposal stream and the level schedule are plain host code: mcmc_host.hpp.
#pragma once

#include "internal.hpp"
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
int launch_mcmc_sweeps(msm_ctx *ctx, const McmcArgs &a);

// `iters` sweeps on the device over tables that lie there (d_U: L x N, d_tc: T x L^3); labeling (host, N) is read and updated.  The arguments have been
// checked by the caller (mcmc_check_arguments).  Complete on return.
int mcmc_run_device(msm_ctx *ctx, const double *d_U, const double *d_tc, const int32_t *triplets, int N, int L, int T, double mcparam, int iters, uint64_t seed,
                    int32_t *labeling);
// the checks of msm_mcmc_optimise on mcparam, the labeling and the triplets, with its messages
int mcmc_check_arguments(const int32_t *triplets, int N, int L, int T, double mcparam, const int32_t *labeling);

}  // namespace msm
