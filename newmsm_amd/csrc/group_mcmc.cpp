// group_mcmc.cpp -- gMSM with the Monte Carlo optimiser, block-coordinate descent over the subjects (include/msmhip.h, "groupwise MCMC").
// A block: the conditional unary table of subject s (its nodes' pair costs against the partners' current labels: queries built by a kernel from the
// incidence of the pair list, evaluated by launch_group_pairwise as msm_group_pairwise_batch evaluates them, summed per (node, label) in ascending pair
// order), its triplet table (launch_group_triplet over all label triples), then mcmc_run_device_chains on the two device tables.  No cost table leaves
// the device; what travels is the labelling, the proposals (host draw) and the chains' labellings and energy terms.
#include "group_internal.hpp"
#include "group_mcmc.hpp"
#include "mcmc.hpp"

namespace {

constexpr int kBlockRecord = 8;  // doubles per block of msm_group_mcmc_pass's per_block

// what every device entry point refuses before anything is queued
int mcmc_group_refusal(msm_group *g, const char *what) {
    if (!g) return fail(MSM_ERR_INVALID, "%s: null group", what);
    if (!g->ready) return fail(MSM_ERR_STATE, "%s: msm_group_finalize() must be called first", what);
    for (int s = 0; s < g->S; ++s)
        if (g->have_subject[s] == 2)
            return fail(MSM_ERR_STATE, "%s: subject %d was imported from another rank; the groupwise Monte Carlo optimiser runs on one rank only", what, s);
    if (g->L > 65535) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise_gpu: %d labels; the proposals travel as 16-bit values (at most 65535)", g->L);
    if (g->N > kMcmcMaxNodes)
        return fail(MSM_ERR_CAPACITY, "msm_mcmc_optimise_gpu: the labels of %d nodes do not fit the LDS of one workgroup (at most %d)", g->N, kMcmcMaxNodes);
    return pair_refusal(g);
}

int check_subject(const msm_group *g, int s, const char *what) {
    if (s < 0 || s >= g->S) return fail(MSM_ERR_INVALID, "%s: subject %d out of range (%d subjects)", what, s, g->S);
    return MSM_OK;
}

int check_labeling(const msm_group *g, const int32_t *labeling, const char *what) {
    if (!labeling) return fail(MSM_ERR_INVALID, "%s: null labeling", what);
    const int64_t nodes = (int64_t)g->S * g->N;
    for (int64_t i = 0; i < nodes; ++i)
        if (labeling[i] < 0 || labeling[i] >= g->L) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise: label of node %lld out of range", (long long)i);
    return MSM_OK;
}

// the incidence of the group's current pair list, on the host and on the device: built once per set-up
int ensure_incidence(msm_group *g) {
    if (g->mc_inc_gen == g->pairs_gen && g->mc_inc_ptr.size() == (size_t)g->S * g->N + 1) return MSM_OK;
    std::vector<int32_t> pairs(2 * (size_t)std::max<int64_t>(g->npairs, 1));
    if (g->npairs > 0) MSM_TRY(msm_group_get_pairs(g, pairs.data()));
    const int nodes = g->S * g->N;
    if (!group_mcmc_incidence(pairs.data(), g->npairs, nodes, g->mc_inc_ptr, g->mc_inc_idx)) return fail(MSM_ERR_INVALID, "msm_group_mcmc: a pair names a node out of range");
    for (int64_t p = 0; p < g->npairs; ++p)  // estimate_pairs, M/DiscreteGroupModel.cpp:37-55
        if (pairs[2 * p] / g->N == pairs[2 * p + 1] / g->N) return fail(MSM_ERR_INVALID, "msm_group_mcmc: pair %lld joins two nodes of one subject", (long long)p);
    MSM_TRY(g->d_mc_inc_ptr.upload_vec(g->mc_inc_ptr, g->ctx));
    MSM_TRY(g->d_mc_inc_idx.upload_vec(g->mc_inc_idx, g->ctx));
    g->mc_inc_gen = g->pairs_gen;
    return MSM_OK;
}

// room for n queries in the group's query columns and answers
int ensure_queries(msm_group *g, size_t n, int ncols) {
    for (int k = 0; k < ncols; ++k)
        if (g->d_query[k].ensure(std::max<size_t>(n, 1)) != hipSuccess) return stage_alloc_failed(sizeof(int) * n);
    return MSM_OK;
}

int record(msm_group *g, int k) {
    if (!g->mc_ev[k]) MSM_HIP(hipEventCreate(&g->mc_ev[k]));
    MSM_HIP(hipEventRecord(g->mc_ev[k], g->ctx->stream));
    return MSM_OK;
}

// U_s of the checked labelling into g->d_mc_U (queued; events 0 .. 2 around the two phases)
int queue_conditional_unary(msm_group *g, const GroupArgs &ga, int s, const int32_t *labeling) {
    msm_ctx *ctx = g->ctx;
    MSM_TRY(ensure_incidence(g));
    const int N = g->N, L = g->L;
    const int32_t e0 = g->mc_inc_ptr[(size_t)s * N], E = g->mc_inc_ptr[(size_t)(s + 1) * N] - e0;
    const int64_t Q = (int64_t)E * L;
    if (Q > ((int64_t)1 << 30)) return fail(MSM_ERR_CAPACITY, "msm_group_conditional_unary: %lld pair-cost queries for subject %d (at most 2^30)", (long long)Q, s);
    MSM_TRY(g->d_mc_lab.upload(labeling, (size_t)g->S * N, ctx));
    MSM_TRY(ensure_queries(g, (size_t)Q, 3));
    if (g->d_answer.ensure(std::max<size_t>((size_t)Q, 1)) != hipSuccess) return stage_alloc_failed(sizeof(double) * (size_t)Q);
    if (g->d_mc_seg.ensure((size_t)N * L + 1) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * ((size_t)N * L + 1));
    if (g->d_mc_U.ensure((size_t)N * L) != hipSuccess) return stage_alloc_failed(sizeof(double) * (size_t)N * L);
    MSM_TRY(record(g, 0));
    for (int k = 0; k < 3 && Q > 0; ++k) MSM_HIP(hipMemsetAsync(g->d_query[k].p, 0, sizeof(int) * (size_t)Q, ctx->stream));  // a slot left out asks (0, 0, 0)
    GroupCondArgs c;
    c.pairs = g->d_pairs.p;
    c.inc_ptr = g->d_mc_inc_ptr.p;
    c.inc_idx = g->d_mc_inc_idx.p;
    c.lab = g->d_mc_lab.p;
    c.S = g->S, c.N = N, c.L = L, c.s = s;
    c.P = g->npairs;
    c.e0 = e0, c.E = E;
    c.qp = g->d_query[0].p, c.qa = g->d_query[1].p, c.qb = g->d_query[2].p;
    c.seg_off = g->d_mc_seg.p;
    c.status = ctx->d_status;
    MSM_TRY(launch_group_cond_queries(ctx, c));
    MSM_TRY(launch_group_pairwise(ctx, ga, g->d_query[0].p, g->d_query[1].p, g->d_query[2].p, (int)Q, g->d_answer.p));
    MSM_TRY(record(g, 1));
    MSM_TRY(launch_group_cond_sum(ctx, g->d_mc_seg.p, g->d_answer.p, N, L, Q, g->d_mc_U.p, ctx->d_status));
    MSM_TRY(record(g, 2));
    return MSM_OK;
}

// tc_s into g->d_mc_tc (queued; event 3 behind it): the triplets in ranges of at most kBatchChunk queries -- a table beyond 2^31 values is filled
// range by range like any other, the offsets are 64-bit
int queue_triplet_table(msm_group *g, const GroupArgs &ga, int s) {
    msm_ctx *ctx = g->ctx;
    const int Tc = g->Tc, L = g->L;
    const size_t per = (size_t)L * L * L, total = (size_t)Tc * per;
    if (per > (size_t)INT32_MAX) return fail(MSM_ERR_CAPACITY, "msm_group_subject_triplet_table: %d labels make %zu label triples per triplet (at most 2^31 - 1)", L, per);
    if (g->d_mc_tc.ensure(std::max<size_t>(total, 1)) != hipSuccess) return stage_alloc_failed(sizeof(double) * total);
    const int step = (int)std::max<size_t>(1, std::min<size_t>((size_t)Tc, (size_t)kBatchChunk / per));
    MSM_TRY(ensure_queries(g, (size_t)step * per, 4));
    for (int t0 = 0; t0 < Tc; t0 += step) {
        const int t1 = std::min(Tc, t0 + step);
        MSM_TRY(launch_group_triplet_queries(ctx, s, Tc, L, t0, t1, g->d_query[0].p, g->d_query[1].p, g->d_query[2].p, g->d_query[3].p));
        MSM_TRY(launch_group_triplet(ctx, ga, g->d_query[0].p, g->d_query[1].p, g->d_query[2].p, g->d_query[3].p, (int)((size_t)(t1 - t0) * per),
                                     g->d_mc_tc.p + (size_t)t0 * per));
    }
    MSM_TRY(record(g, 3));
    return MSM_OK;
}

void local_triplets(const msm_group *g, int s, std::vector<int32_t> &tri) {
    tri.resize(3 * (size_t)g->Tc);
    for (size_t i = 0; i < tri.size(); ++i) tri[i] = g->triplets[3 * (size_t)s * g->Tc + i] - s * g->N;
}

// One block over checked arguments.  rec (kBlockRecord doubles, may be null): start energy, kept energy, accepted, best chain, then the milliseconds of
// the query build plus pair costs, the sums, the triplet table (HIP events) and the sweeps' kernels (msm_mcmc_gpu_stats).
int run_block(msm_group *g, int s, int32_t *labeling, double mcparam, int iters, const uint64_t *seeds, int K, double *rec) {
    msm_ctx *ctx = g->ctx;
    GroupArgs ga;
    MSM_TRY(group_args(g, ga));
    MSM_TRY(queue_conditional_unary(g, ga, s, labeling));
    MSM_TRY(queue_triplet_table(g, ga, s));
    MSM_TRY(check_status(ctx, "msm_group_mcmc_subject"));  // what the table kernels raised, before the sweeps
    float ms[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) MSM_HIP(hipEventElapsedTime(&ms[k], g->mc_ev[k], g->mc_ev[k + 1]));
    const int N = g->N, L = g->L, Tc = g->Tc;
    std::vector<int32_t> tri;
    local_triplets(g, s, tri);
    std::vector<int32_t> start(labeling + (size_t)s * N, labeling + (size_t)(s + 1) * N), lab(start);
    // the start's energy in the chains' own table arithmetic: a run of no sweeps is the start (mcmc_run_device_chains computes the energies alone)
    double e0 = 0.0;
    const uint64_t none = 0;
    MSM_TRY(mcmc_run_device_chains(ctx, g->d_mc_U.p, g->d_mc_tc.p, tri.data(), N, L, Tc, mcparam, 0, &none, 1, lab.data(), nullptr, &e0, nullptr));
    std::vector<double> E((size_t)K);
    int32_t best = 0;
    MSM_TRY(mcmc_run_device_chains(ctx, g->d_mc_U.p, g->d_mc_tc.p, tri.data(), N, L, Tc, mcparam, iters, seeds, K, lab.data(), nullptr, E.data(), &best));
    const bool take = group_mcmc_accept(e0, E[(size_t)best]);
    if (take) std::copy(lab.begin(), lab.end(), labeling + (size_t)s * N);
    if (rec) {
        double st[6] = {0, 0, 0, 0, 0, 0};
        MSM_TRY(msm_mcmc_gpu_stats(ctx, st));
        rec[0] = e0;
        rec[1] = take ? E[(size_t)best] : e0;
        rec[2] = take ? 1.0 : 0.0;
        rec[3] = (double)best;
        rec[4] = ms[0], rec[5] = ms[1], rec[6] = ms[2], rec[7] = st[0];
    }
    return MSM_OK;
}

int check_block_arguments(msm_group *g, const int32_t *labeling, double mcparam, int iters, const char *what) {
    if (iters < 0) return fail(MSM_ERR_INVALID, "%s: %d iterations", what, iters);
    MSM_TRY(check_labeling(g, labeling, what));
    if (!(mcparam > 0.0 && mcparam <= 1.0)) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise: the geometric distribution parameter must be in (0, 1]");
    return MSM_OK;
}

}  // namespace

extern "C" {

int msm_group_mcmc_incidence(const int32_t *pairs, int32_t P, int32_t nodes, int32_t *ptr, int32_t *idx) {
    if (P < 0 || nodes <= 0 || !ptr || (P > 0 && (!pairs || !idx))) return fail(MSM_ERR_INVALID, "msm_group_mcmc_incidence: bad arguments");
    std::vector<int32_t> p, i;
    if (!group_mcmc_incidence(pairs, P, nodes, p, i)) return fail(MSM_ERR_INVALID, "msm_group_mcmc_incidence: a pair names a node out of range");
    std::copy(p.begin(), p.end(), ptr);
    std::copy(i.begin(), i.end(), idx);
    return MSM_OK;
}

int msm_group_mcmc_seeds(uint64_t seed, int32_t it, int32_t pass, int32_t S, int32_t subject, int32_t K, uint64_t *seeds) {
    if (!seeds || S < 1 || subject < 0 || subject >= S || pass < 0 || it < 0) return fail(MSM_ERR_INVALID, "msm_group_mcmc_seeds: bad arguments");
    if (K < 1 || K > kMcmcMaxChains) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise_chains: %d chains (1 to %d)", K, kMcmcMaxChains);
    for (int k = 0; k < K; ++k) seeds[k] = group_mcmc_seed(seed, it, k, pass, S, subject);
    return MSM_OK;
}

int msm_group_mcmc_accept(double start, double best, int32_t *accepted) {
    if (!accepted) return fail(MSM_ERR_INVALID, "msm_group_mcmc_accept: null argument");
    *accepted = group_mcmc_accept(start, best) ? 1 : 0;
    return MSM_OK;
}

int msm_group_conditional_unary(msm_group *g, int32_t subject, const int32_t *labeling, double *U) {
    MSM_TRY(mcmc_group_refusal(g, "msm_group_conditional_unary"));
    MSM_TRY(check_subject(g, subject, "msm_group_conditional_unary"));
    MSM_TRY(check_labeling(g, labeling, "msm_group_conditional_unary"));
    msm_ctx *ctx = g->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    GroupArgs ga;
    MSM_TRY(group_args(g, ga));
    MSM_TRY(queue_conditional_unary(g, ga, subject, labeling));
    std::vector<double> host(U ? (size_t)g->N * g->L : 0);  // the caller's array stays as it is when the call fails
    if (U) MSM_TRY(g->d_mc_U.download(host.data(), host.size(), ctx));
    MSM_TRY(check_status(ctx, "msm_group_conditional_unary"));
    if (U) std::copy(host.begin(), host.end(), U);
    return MSM_OK;
}

int msm_group_subject_triplet_table(msm_group *g, int32_t subject, double *tc) {
    MSM_TRY(mcmc_group_refusal(g, "msm_group_subject_triplet_table"));
    MSM_TRY(check_subject(g, subject, "msm_group_subject_triplet_table"));
    msm_ctx *ctx = g->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    GroupArgs ga;
    MSM_TRY(group_args(g, ga));
    MSM_TRY(queue_triplet_table(g, ga, subject));
    const size_t total = (size_t)g->Tc * g->L * g->L * g->L, piece = (size_t)1 << 21;
    if (!tc) return check_status(ctx, "msm_group_subject_triplet_table");
    for (size_t off = 0; off < total; off += piece) {  // through the staging blocks in pieces of 16 MB
        MSM_TRY(stage_d2h(ctx, tc + off, g->d_mc_tc.p + off, sizeof(double) * std::min(piece, total - off)));
        MSM_TRY(check_status(ctx, "msm_group_subject_triplet_table"));
    }
    return MSM_OK;
}

int msm_group_mcmc_subject(msm_group *g, int32_t subject, int32_t *labeling, double mcparam, int32_t iters, const uint64_t *seeds, int32_t K, double energies[2],
                           int32_t *accepted) {
    MSM_TRY(mcmc_group_refusal(g, "msm_group_mcmc_subject"));
    MSM_TRY(check_subject(g, subject, "msm_group_mcmc_subject"));
    MSM_TRY(mcmc_check_chains(seeds, K));
    MSM_TRY(check_block_arguments(g, labeling, mcparam, iters, "msm_group_mcmc_subject"));
    MSM_HIP(hipSetDevice(g->ctx->device));
    MSM_TRY(drop_ctx_pending(g->ctx));
    std::vector<int32_t> lab(labeling, labeling + (size_t)g->S * g->N);  // the caller's labelling stays as it is when the call fails
    double rec[kBlockRecord];
    MSM_TRY(run_block(g, subject, lab.data(), mcparam, iters, seeds, K, rec));
    std::copy(lab.begin(), lab.end(), labeling);
    if (energies) energies[0] = rec[0], energies[1] = rec[1];
    if (accepted) *accepted = (int32_t)rec[2];
    return MSM_OK;
}

int msm_group_mcmc_pass(msm_group *g, int32_t *labeling, double mcparam, int32_t iters, uint64_t seed, int32_t it, int32_t K, int32_t passes, double *per_block) {
    MSM_TRY(mcmc_group_refusal(g, "msm_group_mcmc_pass"));
    if (K < 1 || K > kMcmcMaxChains) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise_chains: %d chains (1 to %d)", K, kMcmcMaxChains);
    if (passes < 1 || it < 0) return fail(MSM_ERR_INVALID, "msm_group_mcmc_pass: %d passes, iteration %d", passes, it);
    MSM_TRY(check_block_arguments(g, labeling, mcparam, iters, "msm_group_mcmc_pass"));
    MSM_HIP(hipSetDevice(g->ctx->device));
    MSM_TRY(drop_ctx_pending(g->ctx));
    std::vector<int32_t> lab(labeling, labeling + (size_t)g->S * g->N);
    std::vector<double> recs((size_t)passes * g->S * kBlockRecord);
    std::vector<uint64_t> seeds((size_t)K);
    for (int p = 0; p < passes; ++p)
        for (int s = 0; s < g->S; ++s) {  // ascending: a block sees the labels the earlier blocks wrote
            for (int k = 0; k < K; ++k) seeds[(size_t)k] = group_mcmc_seed(seed, it, k, p, g->S, s);
            MSM_TRY(run_block(g, s, lab.data(), mcparam, iters, seeds.data(), K, recs.data() + ((size_t)p * g->S + s) * kBlockRecord));
        }
    std::copy(lab.begin(), lab.end(), labeling);
    if (per_block) std::copy(recs.begin(), recs.end(), per_block);
    return MSM_OK;
}

}  // extern "C"
