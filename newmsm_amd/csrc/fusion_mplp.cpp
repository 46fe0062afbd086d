// fusion_mplp.cpp -- the host side of MPLP over one label step's binary problem (fusion_mplp.hpp; the kernel: fusion_mplp_kernels.hip):
// the plan of a triplet list, the literal msm_fusion_mplp_step (mplp_run_host and mplp_round_host of mplp_host.hpp at L = 2), the one launch with the
// copy of its output block behind it, and what reads that block after the caller's synchronisation: the sums are the device's, in the literal's
// order; the winners are picked here, by the literal's rule.
#include <cstdlib>
#include <cstring>

#include "fusion_mplp.hpp"
#include "mplp.hpp"

using namespace msm;

namespace {

struct FusionScratch {
    DevBuf<double> u2, octets;  // the host tables of msm_fusion_mplp_step_gpu
    FusionMplpPlan plan;        // and the plan of its triplet list
    DevBuf<double> u2w, m, eterms, bterms;
    DevBuf<char> block;
    std::vector<char> host;     // the block, downloaded
    int N = 0, S = 0, P = 0;    // of the solve in flight
    hipEvent_t ev[2] = {nullptr, nullptr};
    double stats[4] = {0, 0, 0, 0};
    int launches = 0, levels = 0;
    ~FusionScratch() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

FusionScratch &scratch(msm_ctx *ctx) {
    if (!ctx->fusion_mplp_scratch) ctx->fusion_mplp_scratch = std::shared_ptr<void>(new FusionScratch(), [](void *p) { delete static_cast<FusionScratch *>(p); });
    return *static_cast<FusionScratch *>(ctx->fusion_mplp_scratch.get());
}

size_t block_doubles(int S, int P) { return 2 * fusion_slots(S, P) + (size_t)std::max(S, 1); }
size_t block_bytes(int N, int S, int P) { return sizeof(double) * block_doubles(S, P) + sizeof(int32_t) * 8 + fusion_slots(S, P) * (size_t)N; }

// the judgement of the step's tables (and, mc non-null, of its messages) under the plain reading: mplp_judge's refusals, the factor table called by its name
int judge(const char *what, int64_t bad_unary, int64_t bad_octets, const int64_t *mc) {
    MplpReading r(false);
    r.table = "octet";
    r.counts[0] = bad_unary;
    r.counts[1] = bad_octets;
    bool F = false;
    return mplp_judge(what, r, mc, &F);
}

// the candidates' energies in order and the winner so far (mplp_run_host's and mplp_round_host's rule: the first lowest)
struct Winner {
    size_t slot = 0;
    double energy = 0.0;
    void offer(size_t s, double e) {
        if (e < energy) energy = e, slot = s;
    }
};

}  // namespace

namespace msm {

int fusion_mplp_check(const char *what, const int32_t *triplets, int N, int T, int sweeps, int polish) {
    if (N <= 0 || T < 0 || (T > 0 && !triplets)) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    if (sweeps < 0 || sweeps > kFusionMaxSweeps) return fail(MSM_ERR_INVALID, "%s: %d sweeps (0 to %d)", what, sweeps, kFusionMaxSweeps);
    if (polish < 0 || polish > kMplpMaxPolish) return fail(MSM_ERR_INVALID, "%s: %d polish passes (0 to %d)", what, polish, kMplpMaxPolish);
    const std::vector<int32_t> zeros((size_t)N, 0);
    return mplp_check_arguments(what, triplets, N, 2, T, sweeps, zeros.data());
}

int fusion_mplp_build_plan(msm_ctx *ctx, const int32_t *triplets, int N, int T, FusionMplpPlan &plan) {
    McmcSchedule sch;
    mcmc_build_schedule(triplets, N, T, sch);
    std::vector<int4> rec((size_t)T);
    for (int i = 0; i < T; ++i) {
        const int t = sch.order[(size_t)i];
        rec[(size_t)i] = make_int4(t, triplets[3 * (size_t)t], triplets[3 * (size_t)t + 1], triplets[3 * (size_t)t + 2]);
    }
    MplpIncidence inc;
    mplp_build_incidence(triplets, N, T, inc);
    MplpColouring col;
    mplp_build_colouring(triplets, N, inc, col);
    std::vector<int4> nbr(6 * (size_t)T);
    for (int i = 0; i < T; ++i)
        for (int s = 0; s < 3; ++s) {
            const int t = sch.order[(size_t)i], node = triplets[3 * (size_t)t + s];
            int q[kFusionNbr] = {0, 0, 0, 0, 0, 0, 0}, n = 0;
            for (int32_t k = inc.ptr[(size_t)node]; k < inc.ptr[(size_t)node + 1]; ++k) {
                if (inc.slot[(size_t)k] == 3 * t + s) continue;
                if (n < kFusionNbr) q[n] = inc.slot[(size_t)k];
                ++n;
            }
            nbr[6 * (size_t)i + 2 * s] = make_int4(n <= kFusionNbr ? n : -1, q[0], q[1], q[2]);
            nbr[6 * (size_t)i + 2 * s + 1] = make_int4(q[3], q[4], q[5], q[6]);
        }
    MSM_TRY(plan.sched.upload_vec(rec, ctx));
    MSM_TRY(plan.nbr.upload_vec(nbr, ctx));
    MSM_TRY(plan.level_off.upload_vec(sch.level_off, ctx));
    MSM_TRY(plan.inc_ptr.upload_vec(inc.ptr, ctx));
    MSM_TRY(plan.inc_slot.upload_vec(inc.slot, ctx));
    MSM_TRY(plan.triplets.upload(triplets, 3 * (size_t)T, ctx));
    MSM_TRY(plan.colour.upload_vec(col.colour, ctx));
    MSM_TRY(plan.cls_node.upload_vec(col.node, ctx));
    MSM_TRY(plan.class_off.upload_vec(col.class_off, ctx));
    plan.N = N;
    plan.T = T;
    plan.levels = sch.levels();
    plan.classes = col.classes();
    return MSM_OK;
}

int fusion_mplp_queue(msm_ctx *ctx, const char *what, const FusionMplpPlan &plan, const double *d_u2, const double *d_U, const int32_t *d_labeling, int label, int L,
                      const double *d_octets, int sweeps, int polish, bool again) {
    FusionScratch &s = scratch(ctx);
    const int N = plan.N, T = plan.T;
    const size_t C = fusion_slots(sweeps, polish), SB = (size_t)std::max(sweeps, 1), nterms = (size_t)N + T, nm = 6 * (size_t)T;
    // where the messages live: LDS where they fit; MSMHIP_FUSION_MSG=lds|global forces one (read per call: the tests run both in one process)
    bool lds = sizeof(double) * nm <= kFusionLdsBudget;
    if (const char *env = std::getenv("MSMHIP_FUSION_MSG")) {
        if (std::strcmp(env, "global") == 0)
            lds = false;
        else if (std::strcmp(env, "lds") == 0) {
            if (!lds) return fail(MSM_ERR_CAPACITY, "%s: MSMHIP_FUSION_MSG=lds, but the messages of %d triplets (%zu bytes) do not fit in LDS", what, T, sizeof(double) * nm);
        } else if (*env)
            return fail(MSM_ERR_INVALID, "%s: MSMHIP_FUSION_MSG=%s (lds or global)", what, env);
    }
    const size_t bytes = block_bytes(N, sweeps, polish);
    if (s.eterms.ensure(fusion_term_count(nterms, C)) != hipSuccess) return stage_alloc_failed(sizeof(double) * fusion_term_count(nterms, C));
    if (s.bterms.ensure(fusion_term_count(nterms, SB)) != hipSuccess) return stage_alloc_failed(sizeof(double) * fusion_term_count(nterms, SB));
    if (s.block.ensure(bytes) != hipSuccess) return stage_alloc_failed(bytes);
    if (!lds && s.m.ensure(std::max<size_t>(nm, 1)) != hipSuccess) return stage_alloc_failed(sizeof(double) * nm);
    if (d_U && s.u2w.ensure(2 * (size_t)N) != hipSuccess) return stage_alloc_failed(sizeof(double) * 2 * (size_t)N);
    for (hipEvent_t &e : s.ev)
        if (!e) MSM_HIP(hipEventCreate(&e));

    FusionMplpArgs a;
    a.u2 = d_u2;
    a.octets = d_octets;
    a.sched = plan.sched.p;
    a.nbr = plan.nbr.p;
    a.level_off = plan.level_off.p;
    a.inc_ptr = plan.inc_ptr.p;
    a.inc_slot = plan.inc_slot.p;
    a.triplets = plan.triplets.p;
    a.colour = plan.colour.p;
    a.cls_node = plan.cls_node.p;
    a.class_off = plan.class_off.p;
    a.m = lds ? nullptr : s.m.p;
    a.eterms = s.eterms.p;
    a.bterms = s.bterms.p;
    a.sums = reinterpret_cast<double *>(s.block.p);
    a.head = reinterpret_cast<int32_t *>(s.block.p + sizeof(double) * block_doubles(sweeps, polish));
    a.cand = reinterpret_cast<uint8_t *>(a.head + 8);
    a.U = d_U;
    a.labeling = d_labeling;
    a.u2w = d_U ? s.u2w.p : nullptr;
    a.label = label;
    a.L = L;
    a.N = N;
    a.T = T;
    a.S = sweeps;
    a.P = polish;
    a.levels = plan.levels;
    a.classes = plan.classes;
    a.status = ctx->d_status;
    MSM_HIP(hipEventRecord(s.ev[0], ctx->stream));
    MSM_TRY(launch_fusion_mplp(ctx, a, lds));
    MSM_HIP(hipEventRecord(s.ev[1], ctx->stream));
    s.host.resize(bytes);
    MSM_TRY(stage_d2h(ctx, s.host.data(), s.block.p, bytes));
    s.N = N, s.S = sweeps, s.P = polish;
    s.levels = plan.levels;
    s.launches = again ? s.launches + 1 : 1;
    return MSM_OK;
}

int fusion_mplp_collect(msm_ctx *ctx, const char *what, const FusionMplpOutputs &o) {
    FusionScratch &s = scratch(ctx);
    const int N = s.N, S = s.S, P = s.P;
    const size_t C = fusion_slots(S, P);
    const double *usum = reinterpret_cast<const double *>(s.host.data()), *tsum = usum + C, *bsum = tsum + C;
    const int32_t *head = reinterpret_cast<const int32_t *>(s.host.data() + sizeof(double) * block_doubles(S, P));
    const uint8_t *cand = reinterpret_cast<const uint8_t *>(head + 8);
    float ms = 0.f;
    MSM_HIP(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
    const int run = head[0], passes = head[1];
    s.stats[0] = ms;
    s.stats[1] = s.levels;
    s.stats[2] = run;
    s.stats[3] = s.launches;
    if (run < 0 || run > S || passes < 0 || passes > P) return fail(MSM_ERR_HIP,"%s: the solve reported %d sweeps and %d passes", what, run, passes);
    const int64_t mc[4] = {0, head[2], 0, 0};
    MSM_TRY(judge(what, head[3], head[4], P > 0 ? mc : nullptr));
    auto energy_of = [&](size_t slot) { return usum[slot] + 0.0 + tsum[slot]; };  // mcmc_energy_of_terms: u + pw + tc
    // the sweeps: candidate 0 is x = 0, candidate k the decode after sweep k
    Winner w;
    w.energy = energy_of(0);
    double e_last = w.energy;
    for (int k = 1; k <= run; ++k) w.offer((size_t)k, e_last = energy_of((size_t)k));
    const double bound = bsum[run > 0 ? run - 1 : 0];
    if (o.energies) {
        o.energies[0] = energy_of(0);
        for (int k = 1; k <= S; ++k) o.energies[k] = k <= run ? energy_of((size_t)k) : e_last;
    }
    if (o.bounds)
        for (int k = 0; k < S; ++k) o.bounds[k] = k < run ? bsum[k] : bound;
    // the rounding: candidate 0 is that winner, then the conditioned decode, then the polish passes
    if (P > 0) {
        w.offer((size_t)S + 1, e_last = energy_of((size_t)S + 1));
        if (o.energies) o.energies[S + 1] = e_last;
        for (int p = 0; p < P; ++p) {
            if (p < passes) w.offer((size_t)S + 2 + p, e_last = energy_of((size_t)S + 2 + p));
            if (o.energies) o.energies[S + 2 + p] = e_last;
        }
    }
    const uint8_t *x = cand + w.slot * (size_t)N;
    for (int i = 0; i < N; ++i) o.x[i] = x[i];
    if (o.sweeps_run) *o.sweeps_run = run;
    if (o.passes_run) *o.passes_run = passes;
    if (o.energy) *o.energy = w.energy;
    if (o.bound) *o.bound = bound;
    return MSM_OK;
}

}  // namespace msm

namespace {

// the literal
int step_host(const char *what, const double *unary2, const double *octets, const int32_t *triplets, int T, int N, int sweeps, int polish, const FusionMplpOutputs &o) {
    if (!o.x || (T > 0 && !octets)) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    MSM_TRY(fusion_mplp_check(what, triplets, N, T, sweeps, polish));
    std::vector<double> U(2 * (size_t)N, 0.0);  // 5.19's layout: theta_i(x) at U[x N + i]
    if (unary2)
        for (int i = 0; i < N; ++i) U[(size_t)i] = unary2[2 * (size_t)i], U[(size_t)N + i] = unary2[2 * (size_t)i + 1];
    int64_t counts[4];
    mplp_classify(U.data(), U.size(), octets, 8 * (size_t)T, counts);
    MSM_TRY(judge(what, counts[0], counts[1] + counts[2] + counts[3], nullptr));
    std::vector<int32_t> lab((size_t)N, 0);
    std::vector<double> en((size_t)sweeps), bn((size_t)sweeps), m(6 * (size_t)T), terms((size_t)N + T), ren((size_t)polish + 2);
    mcmc_energy_terms(U.data(), octets, triplets, N, 2, T, lab.data(), terms.data());
    const double e0 = mcmc_energy_of_terms(terms.data(), N, T);
    int32_t run = 0, passes = 0;
    double e = 0.0, b = 0.0;
    mplp_run_host(U.data(), octets, triplets, N, 2, T, sweeps, {lab.data(), &run, &e, &b, sweeps ? en.data() : nullptr, sweeps ? bn.data() : nullptr, T ? m.data() : nullptr});
    if (run == 0) std::fill(en.begin(), en.end(), e0), std::fill(bn.begin(), bn.end(), b);  // no sweep ran: the start's energy, the bound of zero messages
    if (polish > 0) {
        int64_t mc[4];
        mplp_classify(nullptr, 0, m.data(), m.size(), mc);
        const int64_t bad[4] = {0, mc[1] + mc[2] + mc[3], 0, 0};
        MSM_TRY(judge(what, 0, 0, bad));
        mplp_round_host(U.data(), octets, triplets, N, 2, T, T ? m.data() : nullptr, 0, polish, {lab.data(), &passes, &e, ren.data()});
    }
    std::copy(lab.begin(), lab.end(), o.x);
    if (o.sweeps_run) *o.sweeps_run = run;
    if (o.passes_run) *o.passes_run = passes;
    if (o.energy) *o.energy = e;
    if (o.bound) *o.bound = b;
    if (o.energies) {
        o.energies[0] = e0;
        std::copy(en.begin(), en.end(), o.energies + 1);
        if (polish > 0) std::copy(ren.begin() + 1, ren.end(), o.energies + 1 + sweeps);
    }
    if (o.bounds) std::copy(bn.begin(), bn.end(), o.bounds);
    return MSM_OK;
}

}  // namespace

extern "C" {

int msm_fusion_mplp_step(const double *unary2, const double *octets, const int32_t *triplets, int32_t T, int32_t N, int32_t sweeps, int32_t polish, int32_t *x,
                         int32_t *sweeps_run, int32_t *passes_run, double *energy, double *bound, double *energies, double *bounds) {
    return step_host("msm_fusion_mplp_step", unary2, octets, triplets, T, N, sweeps, polish, {x, sweeps_run, passes_run, energy, bound, energies, bounds});
}

int msm_fusion_mplp_step_gpu(msm_ctx *ctx, const double *unary2, const double *octets, const int32_t *triplets, int32_t T, int32_t N, int32_t sweeps,
                             int32_t polish, int32_t *x, int32_t *sweeps_run, int32_t *passes_run, double *energy, double *bound, double *energies,
                             double *bounds) {
    const char *what = "msm_fusion_mplp_step";
    if (!ctx) return fail(MSM_ERR_INVALID, "msm_fusion_mplp_step_gpu: null context");
    if (!x || (T > 0 && !octets)) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    MSM_TRY(fusion_mplp_check(what, triplets, N, T, sweeps, polish));
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    FusionScratch &s = scratch(ctx);
    MSM_TRY(fusion_mplp_build_plan(ctx, triplets, N, T, s.plan));
    const std::vector<double> zeros(unary2 ? 0 : 2 * (size_t)N, 0.0);
    MSM_TRY(s.u2.upload(unary2 ? unary2 : zeros.data(), 2 * (size_t)N, ctx));
    MSM_TRY(s.octets.upload(octets, 8 * (size_t)T, ctx));
    MSM_TRY(fusion_mplp_queue(ctx, what, s.plan, s.u2.p, nullptr, nullptr, 0, 2, s.octets.p, sweeps, polish, false));
    MSM_TRY(check_status(ctx, what));  // the one synchronisation
    return fusion_mplp_collect(ctx, what, {x, sweeps_run, passes_run, energy, bound, energies, bounds});
}

int msm_fusion_mplp_gpu_stats(msm_ctx *ctx, double stats[4]) {
    if (!ctx || !stats) return fail(MSM_ERR_INVALID, "msm_fusion_mplp_gpu_stats: null argument");
    std::memcpy(stats, scratch(ctx).stats, sizeof(double) * 4);
    return MSM_OK;
}

}  // extern "C"
