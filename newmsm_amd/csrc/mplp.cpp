// mplp.cpp -- the host side of the MPLP optimiser (mplp.hpp; kernels: mplp_kernels.hip; the serial literal: mplp_host.hpp): the checks
// both sides share, the loop that queues a chunk of sweeps -- a launch per level, the decode, the energy terms, the bound terms -- and sums what comes
// back in the literal's order, and the entry points over host tables.  The rounding of the messages (mplp_round_device) has the same shape: a launch
// per colour class and pass, a copy of the labelling and its energy terms per pass, one synchronisation per chunk of passes.
#include <cstring>

#include "mplp.hpp"

using namespace msm;

namespace {

struct MplpScratch {
    DevBuf<double> U, tc;  // the host tables of msm_mplp_optimise_gpu
    DevBuf<int4> sched;
    DevBuf<int32_t> inc_ptr, inc_slot, start, labs, changed, flags;
    DevBuf<unsigned long long> counts;  // k_mplp_classify: four of the tables, four of the rounding's messages
    DevBuf<double> m, eterms, bterms;
    // the rounding's own (mplp_round_device): it leaves m alone
    DevBuf<int4> tri;
    DevBuf<int32_t> colour, cls_node, cur, rlabs, rchanged;
    DevBuf<double> rm, rterms;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double stats[4] = {0, 0, 0, 0}, round_stats[4] = {0, 0, 0, 0};
    ~MplpScratch() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

MplpScratch &mplp_scratch(msm_ctx *ctx) {
    if (!ctx->mplp_scratch) ctx->mplp_scratch = std::shared_ptr<void>(new MplpScratch(), [](void *p) { delete static_cast<MplpScratch *>(p); });
    return *static_cast<MplpScratch *>(ctx->mplp_scratch.get());
}

int refuse_non_finite(const char *what, const char *table) {
    return fail(MSM_ERR_INVALID,
                "%s: the %s table holds a non-finite value (NaN or infinity); clean the input data first (--fixnan), and mind that a label set which lets "
                "two control points meet collapses a triangle and makes the regulariser non-finite (the unscaled sampling grid does: use --rescaleL)",
                what, table);
}

// the refusals of the forbidden-entry reading (DESIGN.md 5.19 "Forbidden entries"): each names the table and the class of value
int refuse_minus_infinity(const char *what) {
    return fail(MSM_ERR_INVALID,
                "%s: the triplet table holds -infinity; the forbidden-entry reading takes NaN and +infinity as forbidden label combinations and nothing "
                "else",
                what);
}

int refuse_messages(const char *what, const int64_t mc[4]) {
    return fail(MSM_ERR_INVALID, "%s: the messages hold %s; under the forbidden-entry reading a message is finite or +infinity", what, mc[1] ? "a NaN" : "-infinity");
}

// the forbid route's refusals over counted tables; MSM_OK leaves *forbidden = whether the triplet table holds a forbidden entry
int check_counts(const char *what, const int64_t counts[4], bool *forbidden) {
    if (counts[0]) return refuse_non_finite(what, "unary");
    if (counts[3]) return refuse_minus_infinity(what);
    *forbidden = counts[1] + counts[2] > 0;
    return MSM_OK;
}

int refuse_label_count(const char *what, int L) {
    return fail(MSM_ERR_CAPACITY, "%s: %d labels; a factor's cavities and minima (6 L doubles) live in the LDS of one workgroup (at most %d labels)", what, L,
                kMplpMaxLabels);
}

int check_pointers(const char *what, const double *unary, const double *tcosts, const int32_t *triplets, int N, int L, int T, int sweeps, const int32_t *labeling) {
    if (!unary || !labeling || N <= 0 || L <= 0 || T < 0 || sweeps < 0 || (T > 0 && (!tcosts || !triplets))) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    return MSM_OK;
}

}  // namespace

namespace msm {

int mplp_check_arguments(const char *what, const int32_t *triplets, int N, int L, int T, int sweeps, const int32_t *labeling) {
    if (sweeps < 0) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    MSM_TRY(mcmc_check_arguments(triplets, N, L, T, 1.0, labeling));
    const int t = mplp_first_repeated_node(triplets, T);
    if (t >= 0) return fail(MSM_ERR_INVALID, "%s: triplet %d names a node twice", what, t);
    return MSM_OK;
}

int mplp_round_check(const char *what, int L, int mode, int polish) {
    if (mode != 0 && mode != 1) return fail(MSM_ERR_INVALID, "%s: mode %d (0: conditioned decode and polish, 1: polish alone)", what, mode);
    if (polish < 0 || polish > kMplpMaxPolish) return fail(MSM_ERR_INVALID, "%s: %d polish passes (0 to %d)", what, polish, kMplpMaxPolish);
    if (L > kMplpMaxLabels) return refuse_label_count(what, L);
    return MSM_OK;
}

int mplp_round_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_tc, const double *d_m, bool use_scratch_m, bool check_tables,
                      const int32_t *triplets, int N, int L, int T, int mode, int polish, const MplpRoundOutputs &o, bool forbid, int64_t *counts) {
    MplpScratch &s = mplp_scratch(ctx);
    const size_t nU = (size_t)L * N, ntc = (size_t)T * L * L * L, nm = 3 * (size_t)T * L, nterms = (size_t)N + T;
    if (use_scratch_m) d_m = s.m.p;
    if (mode != 0 || nm == 0) d_m = nullptr;  // mode 1 reads no messages
    bool F = false;  // the forbidden-aware kernels: taken where the tables or the messages call for them, the plain ones otherwise
    if (forbid) {
        // one pass over both tables and one over the messages; check_tables false: counts holds what the caller's pass over these tables counted
        int64_t got[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are downloaded as they are");
        if (s.counts.zero(8, ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int64_t) * 8);
        if (check_tables) MSM_TRY(launch_mplp_classify(ctx, d_U, nU, d_tc, ntc, s.counts.p));
        if (d_m) MSM_TRY(launch_mplp_classify(ctx, nullptr, 0, d_m, nm, s.counts.p + 4));
        MSM_TRY(s.counts.download(reinterpret_cast<unsigned long long *>(got), 8, ctx));
        MSM_TRY(check_status(ctx, what));
        if (!check_tables && counts) std::copy(counts, counts + 4, got);
        MSM_TRY(check_counts(what, got, &F));
        if (got[5] || got[7]) return refuse_messages(what, got + 4);
        F |= got[6] > 0;  // a message of +infinity
        if (counts) std::copy(got, got + 4, counts);
    } else {
        int32_t bad[4] = {0, 0, 0, 0};
        if (s.flags.zero(4, ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * 4);
        if (check_tables) MSM_TRY(launch_mplp_finite(ctx, d_U, nU, d_tc, ntc, s.flags.p));
        if (d_m) MSM_TRY(launch_mplp_finite(ctx, d_m, nm, nullptr, 0, s.flags.p + 2));
        MSM_TRY(s.flags.download(bad, 4, ctx));
        MSM_TRY(check_status(ctx, what));
        if (bad[0]) return refuse_non_finite(what, "unary");
        if (bad[1]) return refuse_non_finite(what, "triplet");
        if (bad[2]) return fail(MSM_ERR_INVALID, "%s: the messages hold a non-finite value (NaN or infinity)", what);
    }
    MSM_TRY(mplp_round_check(what, L, mode, polish));

    MplpIncidence inc;
    mplp_build_incidence(triplets, N, T, inc);
    MplpColouring col;
    mplp_build_colouring(triplets, N, inc, col);
    std::vector<int4> rec((size_t)T);
    for (int t = 0; t < T; ++t) rec[(size_t)t] = make_int4(t, triplets[3 * (size_t)t], triplets[3 * (size_t)t + 1], triplets[3 * (size_t)t + 2]);
    // passes per chunk: a chunk's labellings and terms stay below 32 MB, as the sweeps' do
    const int first = mode == 0 ? 2 : 1;  // candidates ahead of the polish passes
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(polish, 256), ((size_t)1 << 22) / nterms));
    const size_t held = (size_t)std::max(chunk, first);
    MSM_TRY(s.tri.upload_vec(rec, ctx));
    MSM_TRY(s.inc_ptr.upload_vec(inc.ptr, ctx));
    MSM_TRY(s.inc_slot.upload_vec(inc.slot, ctx));
    MSM_TRY(s.colour.upload_vec(col.colour, ctx));
    MSM_TRY(s.cls_node.upload_vec(col.node, ctx));
    MSM_TRY(s.cur.upload(o.labeling, (size_t)N, ctx));
    if (s.rchanged.zero((size_t)std::max(polish, 1), ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * (size_t)polish);
    if (s.rlabs.ensure(held * N) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * held * N);
    if (s.rterms.ensure(held * nterms) != hipSuccess) return stage_alloc_failed(sizeof(double) * held * nterms);
    for (hipEvent_t &e : s.ev)
        if (!e) MSM_HIP(hipEventCreate(&e));

    MplpRoundArgs a;
    a.U = d_U;
    a.tc = d_tc;
    a.m = d_m;
    a.tri = s.tri.p;
    a.inc_ptr = s.inc_ptr.p;
    a.inc_slot = s.inc_slot.p;
    a.colour = s.colour.p;
    a.cls_node = s.cls_node.p;
    a.lab = s.cur.p;
    a.changed = s.rchanged.p;
    a.N = N;
    a.L = L;
    a.T = T;
    a.status = ctx->d_status;
    McmcChainArgs c;  // the energy terms of the labelling being walked: k_mcmc_chain_terms with K = 1 (the records may come in any order)
    c.a.U = d_U;
    c.a.tc = d_tc;
    c.a.sched = s.tri.p;
    c.a.level_off = nullptr;
    c.a.prop = nullptr;
    c.a.labeling = s.cur.p;
    c.a.N = N;
    c.a.L = L;
    c.a.T = T;
    c.a.levels = 0;
    c.a.sweeps = 0;
    c.a.status = ctx->d_status;
    c.chains = 1;
    c.chunk_sweeps = 0;
    const int classes = col.classes();
    auto snapshot = [&](size_t j) -> int {  // the labelling as it stands and its energy terms, to place j of the chunk
        MSM_HIP(hipMemcpyAsync(s.rlabs.p + j * N, s.cur.p, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
        return launch_mcmc_chain_terms(ctx, c, s.rterms.p + j * nterms);
    };

    // candidate 0 and, in mode 0, the conditioned decode
    std::vector<double> terms(held * nterms), energies((size_t)first + polish);
    std::vector<int32_t> labs(held * N), changed((size_t)polish, 0);
    float ms = 0.f;
    double decode_ms = 0.0, polish_ms = 0.0;
    MSM_TRY(snapshot(0));
    if (mode == 0) {
        MSM_HIP(hipEventRecord(s.ev[0], ctx->stream));
        for (int k = 0; k < classes; ++k) MSM_TRY(launch_mplp_round(ctx, a, col.class_off[(size_t)k], col.class_off[(size_t)k + 1] - col.class_off[(size_t)k], k, F));
        MSM_HIP(hipEventRecord(s.ev[1], ctx->stream));
        MSM_TRY(snapshot(1));
    }
    MSM_TRY(s.rterms.download(terms.data(), (size_t)first * nterms, ctx));
    MSM_TRY(s.rlabs.download(labs.data(), (size_t)first * N, ctx));
    MSM_TRY(check_status(ctx, what));
    if (mode == 0) {
        MSM_HIP(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
        decode_ms = ms;
    }
    double e_last = mplp_energy_of_terms(terms.data(), N, T, F);
    MplpWinner win(o.labeling, N, e_last);
    energies[0] = e_last;
    if (mode == 0) {
        energies[1] = e_last = mplp_energy_of_terms(terms.data() + nterms, N, T, F);
        win.offer(labs.data() + N, N, e_last);
    }

    int run = 0;
    bool fixed = false;
    for (int p0 = 0; p0 < polish && !fixed; p0 += chunk) {
        const int n = std::min(chunk, polish - p0);
        MSM_HIP(hipEventRecord(s.ev[0], ctx->stream));
        for (int j = 0; j < n; ++j) {
            for (int k = 0; k < classes; ++k)
                MSM_TRY(launch_mplp_polish(ctx, a, col.class_off[(size_t)k], col.class_off[(size_t)k + 1] - col.class_off[(size_t)k], p0 + j, F));
            MSM_TRY(snapshot((size_t)j));
        }
        MSM_HIP(hipEventRecord(s.ev[1], ctx->stream));
        MSM_TRY(s.rlabs.download(labs.data(), (size_t)n * N, ctx));
        MSM_TRY(s.rterms.download(terms.data(), (size_t)n * nterms, ctx));
        MSM_TRY(stage_d2h(ctx, changed.data() + p0, s.rchanged.p + p0, sizeof(int32_t) * (size_t)n));
        MSM_TRY(check_status(ctx, what));
        MSM_HIP(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
        polish_ms += ms;
        for (int j = 0; j < n; ++j) {
            const int p = p0 + j;
            if (p > 0 && changed[(size_t)p - 1] == 0) {  // pass p - 1 changed no label: pass p and the rest did not run
                fixed = true;
                break;
            }
            run = p + 1;
            energies[(size_t)first + p] = e_last = mplp_energy_of_terms(terms.data() + (size_t)j * nterms, N, T, F);
            win.offer(labs.data() + (size_t)j * N, N, e_last);
        }
    }
    for (int p = run; p < polish; ++p) energies[(size_t)first + p] = e_last;
    std::copy(win.lab.begin(), win.lab.end(), o.labeling);
    if (o.passes_run) *o.passes_run = run;
    if (o.energy) *o.energy = win.energy;
    if (o.energies) std::copy(energies.begin(), energies.end(), o.energies);
    s.round_stats[0] = decode_ms;
    s.round_stats[1] = polish_ms;
    s.round_stats[2] = classes;
    s.round_stats[3] = run;
    return MSM_OK;
}

int mplp_run_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_tc, const int32_t *triplets, int N, int L, int T, int sweeps,
                    const MplpOutputs &o, bool forbid, int64_t *counts) {
    MplpScratch &s = mplp_scratch(ctx);
    const size_t nU = (size_t)L * N, ntc = (size_t)T * L * L * L, nm = 3 * (size_t)T * L, nterms = (size_t)N + T;
    // the refusals that need the tables: one pass over both, before anything else is launched
    bool F = false;  // the forbidden-aware kernels: only where the table holds a forbidden entry, so a finite table runs the plain ones
    if (forbid) {
        int64_t got[4] = {0, 0, 0, 0};
        if (s.counts.zero(4, ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int64_t) * 4);
        MSM_TRY(launch_mplp_classify(ctx, d_U, nU, d_tc, ntc, s.counts.p));
        MSM_TRY(s.counts.download(reinterpret_cast<unsigned long long *>(got), 4, ctx));
        MSM_TRY(check_status(ctx, what));
        MSM_TRY(check_counts(what, got, &F));
        if (counts) std::copy(got, got + 4, counts);
    } else {
        int32_t bad[2] = {0, 0};
        if (s.flags.zero(2, ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * 2);
        MSM_TRY(launch_mplp_finite(ctx, d_U, nU, d_tc, ntc, s.flags.p));
        MSM_TRY(s.flags.download(bad, 2, ctx));
        MSM_TRY(check_status(ctx, what));
        if (bad[0]) return refuse_non_finite(what, "unary");
        if (bad[1]) return refuse_non_finite(what, "triplet");
    }
    if (L > kMplpMaxLabels) return refuse_label_count(what, L);

    McmcSchedule sch;
    mcmc_build_schedule(triplets, N, T, sch);
    std::vector<int4> rec((size_t)T);
    for (int i = 0; i < T; ++i) {
        const int t = sch.order[(size_t)i];
        rec[(size_t)i] = make_int4(t, triplets[3 * (size_t)t], triplets[3 * (size_t)t + 1], triplets[3 * (size_t)t + 2]);
    }
    MplpIncidence inc;
    mplp_build_incidence(triplets, N, T, inc);
    // sweeps per chunk: the terms of a chunk (two arrays of N + T doubles per sweep) stay below 32 MB each, and a run that reaches its fixed point
    // early in a chunk has at most 255 idle sweeps' launches behind it
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min(sweeps, 256), ((size_t)1 << 22) / nterms));
    MSM_TRY(s.sched.upload_vec(rec, ctx));
    MSM_TRY(s.inc_ptr.upload_vec(inc.ptr, ctx));
    MSM_TRY(s.inc_slot.upload_vec(inc.slot, ctx));
    MSM_TRY(s.start.upload(o.labeling, (size_t)N, ctx));
    if (s.m.zero(std::max<size_t>(nm, 1), ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(double) * nm);
    if (s.changed.zero((size_t)std::max(sweeps, 1), ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * (size_t)sweeps);
    if (s.labs.ensure((size_t)chunk * N) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * (size_t)chunk * N);
    if (s.eterms.ensure((size_t)chunk * nterms) != hipSuccess || s.bterms.ensure((size_t)chunk * nterms) != hipSuccess)
        return stage_alloc_failed(sizeof(double) * (size_t)chunk * nterms);
    for (hipEvent_t &e : s.ev)
        if (!e) MSM_HIP(hipEventCreate(&e));

    MplpArgs a;
    a.U = d_U;
    a.tc = d_tc;
    a.sched = s.sched.p;
    a.inc_ptr = s.inc_ptr.p;
    a.inc_slot = s.inc_slot.p;
    a.m = s.m.p;
    a.changed = s.changed.p;
    a.N = N;
    a.L = L;
    a.T = T;
    a.status = ctx->d_status;
    McmcChainArgs c;  // the energy terms of one labelling: k_mcmc_chain_terms with K = 1
    c.a.U = d_U;
    c.a.tc = d_tc;
    c.a.sched = s.sched.p;
    c.a.level_off = nullptr;
    c.a.prop = nullptr;
    c.a.labeling = s.start.p;
    c.a.N = N;
    c.a.L = L;
    c.a.T = T;
    c.a.levels = sch.levels();
    c.a.sweeps = 0;
    c.a.status = ctx->d_status;
    c.chains = 1;
    c.chunk_sweeps = 0;

    // candidate 0: the start
    std::vector<double> eterms((size_t)chunk * nterms), bterms((size_t)chunk * nterms);
    MSM_TRY(launch_mcmc_chain_terms(ctx, c, s.eterms.p));
    MSM_TRY(s.eterms.download(eterms.data(), nterms, ctx));
    MSM_TRY(check_status(ctx, what));
    MplpWinner win(o.labeling, N, mplp_energy_of_terms(eterms.data(), N, T, F));

    std::vector<int32_t> labs((size_t)chunk * N), changed((size_t)sweeps, 0);
    std::vector<double> energies((size_t)sweeps), bounds(o.bounds ? (size_t)sweeps : 0);
    int run = 0;
    double kernel_ms = 0.0, e_last = 0.0, b_last = 0.0;
    bool fixed = false;
    for (int k0 = 0; k0 < sweeps && T > 0 && !fixed; k0 += chunk) {
        const int n = std::min(chunk, sweeps - k0);
        MSM_HIP(hipEventRecord(s.ev[0], ctx->stream));
        for (int j = 0; j < n; ++j) {
            for (int lv = 0; lv < sch.levels(); ++lv)
                MSM_TRY(launch_mplp_update(ctx, a, sch.level_off[(size_t)lv], sch.level_off[(size_t)lv + 1] - sch.level_off[(size_t)lv], k0 + j, F));
            MSM_TRY(launch_mplp_decode(ctx, a, s.labs.p + (size_t)j * N, s.bterms.p + (size_t)j * nterms));
            c.a.labeling = s.labs.p + (size_t)j * N;
            MSM_TRY(launch_mcmc_chain_terms(ctx, c, s.eterms.p + (size_t)j * nterms));
            if (o.bounds) MSM_TRY(launch_mplp_factor_terms(ctx, a, s.bterms.p + (size_t)j * nterms + N, k0 + j, F));
        }
        MSM_HIP(hipEventRecord(s.ev[1], ctx->stream));
        MSM_TRY(s.labs.download(labs.data(), (size_t)n * N, ctx));
        MSM_TRY(s.eterms.download(eterms.data(), (size_t)n * nterms, ctx));
        if (o.bounds) MSM_TRY(s.bterms.download(bterms.data(), (size_t)n * nterms, ctx));
        MSM_TRY(stage_d2h(ctx, changed.data() + k0, s.changed.p + k0, sizeof(int32_t) * (size_t)n));
        MSM_TRY(check_status(ctx, what));
        float ms = 0.f;
        MSM_HIP(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
        kernel_ms += ms;
        for (int j = 0; j < n; ++j) {
            const int k = k0 + j;
            if (k > 0 && changed[(size_t)k - 1] == 0) {  // sweep k - 1 moved nothing: sweep k and the rest did not run
                fixed = true;
                break;
            }
            run = k + 1;
            energies[(size_t)k] = e_last = mplp_energy_of_terms(eterms.data() + (size_t)j * nterms, N, T, F);
            win.offer(labs.data() + (size_t)j * N, N, e_last);
            if (o.bounds) bounds[(size_t)k] = b_last = mplp_bound_of_terms(bterms.data() + (size_t)j * nterms, N, T);
        }
    }
    for (int k = run; k < sweeps && run > 0; ++k) {
        energies[(size_t)k] = e_last;
        if (o.bounds) bounds[(size_t)k] = b_last;
    }
    double bound = b_last;
    if (o.bound && !(o.bounds && run > 0)) {  // one pass over the table for the bound of the last messages
        MSM_TRY(launch_mplp_decode(ctx, a, nullptr, s.bterms.p));
        MSM_TRY(launch_mplp_factor_terms(ctx, a, s.bterms.p + N, -1, F));
        MSM_TRY(s.bterms.download(bterms.data(), nterms, ctx));
        MSM_TRY(check_status(ctx, what));
        bound = mplp_bound_of_terms(bterms.data(), N, T);
    }
    if (o.messages && nm) {
        std::vector<double> m(nm);  // the caller's array stays as it is when the call fails
        MSM_TRY(s.m.download(m.data(), nm, ctx));
        MSM_TRY(check_status(ctx, what));
        std::copy(m.begin(), m.end(), o.messages);
    }
    std::copy(win.lab.begin(), win.lab.end(), o.labeling);
    if (o.sweeps_run) *o.sweeps_run = run;
    if (o.energy) *o.energy = win.energy;
    if (o.bound) *o.bound = bound;
    if (run > 0) {
        if (o.energies) std::copy(energies.begin(), energies.end(), o.energies);
        if (o.bounds) std::copy(bounds.begin(), bounds.end(), o.bounds);
    }
    s.stats[0] = kernel_ms;
    s.stats[1] = sch.levels();
    s.stats[2] = run;
    s.stats[3] = sch.widest();
    return MSM_OK;
}

}  // namespace msm

namespace {

// msm_mplp_optimise and msm_mplp_optimise_forbid (forbid; counts may be null)
int optimise_host(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, int32_t sweeps, const MplpOutputs &o,
                  bool forbid, int64_t *counts) {
    const char *what = "msm_mplp_optimise";
    MSM_TRY(check_pointers(what, unary, tcosts, triplets, N, L, T, sweeps, o.labeling));
    MSM_TRY(mplp_check_arguments(what, triplets, N, L, T, sweeps, o.labeling));
    bool F = false;  // the plain literal where the table holds no forbidden entry
    if (forbid) {
        int64_t got[4];
        mplp_classify(unary, (size_t)L * N, tcosts, (size_t)T * L * L * L, got);
        MSM_TRY(check_counts(what, got, &F));
        if (counts) std::copy(got, got + 4, counts);
    } else {
        if (!mplp_all_finite(unary, (size_t)L * N)) return refuse_non_finite(what, "unary");
        if (!mplp_all_finite(tcosts, (size_t)T * L * L * L)) return refuse_non_finite(what, "triplet");
    }
    if (L > kMplpMaxLabels) return refuse_label_count(what, L);
    mplp_run_host(unary, tcosts, triplets, N, L, T, sweeps, o, F);
    return MSM_OK;
}

int optimise_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, int32_t sweeps,
                 const MplpOutputs &o, bool forbid, int64_t *counts) {
    if (!ctx) return fail(MSM_ERR_INVALID, "msm_mplp_optimise_gpu: null context");
    MSM_TRY(check_pointers("msm_mplp_optimise", unary, tcosts, triplets, N, L, T, sweeps, o.labeling));
    MSM_TRY(mplp_check_arguments("msm_mplp_optimise", triplets, N, L, T, sweeps, o.labeling));
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MplpScratch &s = mplp_scratch(ctx);
    const size_t nU = (size_t)L * N, ntc = (size_t)T * L * L * L;
    if (s.U.ensure(nU) != hipSuccess) return stage_alloc_failed(sizeof(double) * nU);
    if (s.tc.ensure(ntc ? ntc : 1) != hipSuccess) return stage_alloc_failed(sizeof(double) * ntc);
    MSM_TRY(upload_in_pieces(ctx, s.U.p, unary, sizeof(double) * nU));
    MSM_TRY(upload_in_pieces(ctx, s.tc.p, tcosts, sizeof(double) * ntc));
    return mplp_run_device(ctx, "msm_mplp_optimise", s.U.p, s.tc.p, triplets, N, L, T, sweeps, o, forbid, counts);
}

int round_host(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const double *messages, int32_t mode,
               int32_t polish, const MplpRoundOutputs &o, bool forbid, int64_t *counts) {
    const char *what = "msm_mplp_round";
    MSM_TRY(check_pointers(what, unary, tcosts, triplets, N, L, T, 0, o.labeling));
    MSM_TRY(mplp_check_arguments(what, triplets, N, L, T, 0, o.labeling));
    bool F = false;
    if (forbid) {
        int64_t got[4], mc[4] = {0, 0, 0, 0};
        mplp_classify(unary, (size_t)L * N, tcosts, (size_t)T * L * L * L, got);
        MSM_TRY(check_counts(what, got, &F));
        if (mode == 0 && messages) mplp_classify(nullptr, 0, messages, 3 * (size_t)T * L, mc);
        if (mc[1] || mc[3]) return refuse_messages(what, mc);
        F |= mc[2] > 0;  // a message of +infinity
        if (counts) std::copy(got, got + 4, counts);
    } else {
        if (!mplp_all_finite(unary, (size_t)L * N)) return refuse_non_finite(what, "unary");
        if (!mplp_all_finite(tcosts, (size_t)T * L * L * L)) return refuse_non_finite(what, "triplet");
        if (mode == 0 && messages && !mplp_all_finite(messages, 3 * (size_t)T * L))
            return fail(MSM_ERR_INVALID, "%s: the messages hold a non-finite value (NaN or infinity)", what);
    }
    MSM_TRY(mplp_round_check(what, L, mode, polish));
    mplp_round_host(unary, tcosts, triplets, N, L, T, mode == 0 ? messages : nullptr, mode, polish, o, F);
    return MSM_OK;
}

int round_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const double *messages,
              int32_t mode, int32_t polish, const MplpRoundOutputs &o, bool forbid, int64_t *counts) {
    const char *what = "msm_mplp_round";
    if (!ctx) return fail(MSM_ERR_INVALID, "msm_mplp_round_gpu: null context");
    MSM_TRY(check_pointers(what, unary, tcosts, triplets, N, L, T, 0, o.labeling));
    MSM_TRY(mplp_check_arguments(what, triplets, N, L, T, 0, o.labeling));
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MplpScratch &s = mplp_scratch(ctx);
    const size_t nU = (size_t)L * N, ntc = (size_t)T * L * L * L, nm = 3 * (size_t)T * L;
    const bool with_m = mode == 0 && messages && nm;
    if (s.U.ensure(nU) != hipSuccess) return stage_alloc_failed(sizeof(double) * nU);
    if (s.tc.ensure(ntc ? ntc : 1) != hipSuccess) return stage_alloc_failed(sizeof(double) * ntc);
    if (with_m && s.rm.ensure(nm) != hipSuccess) return stage_alloc_failed(sizeof(double) * nm);
    MSM_TRY(upload_in_pieces(ctx, s.U.p, unary, sizeof(double) * nU));
    MSM_TRY(upload_in_pieces(ctx, s.tc.p, tcosts, sizeof(double) * ntc));
    if (with_m) MSM_TRY(upload_in_pieces(ctx, s.rm.p, messages, sizeof(double) * nm));
    return mplp_round_device(ctx, what, s.U.p, s.tc.p, with_m ? s.rm.p : nullptr, false, true, triplets, N, L, T, mode, polish, o, forbid, counts);
}

}  // namespace

extern "C" {

int msm_mplp_optimise(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, int32_t sweeps, int32_t *labeling,
                      int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds, double *messages) {
    return optimise_host(unary, tcosts, triplets, N, L, T, sweeps, {labeling, sweeps_run, energy, bound, energies, bounds, messages}, false, nullptr);
}

int msm_mplp_optimise_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, int32_t sweeps,
                          int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds, double *messages) {
    return optimise_gpu(ctx, unary, tcosts, triplets, N, L, T, sweeps, {labeling, sweeps_run, energy, bound, energies, bounds, messages}, false, nullptr);
}

int msm_mplp_classify(const double *unary, const double *tcosts, int32_t N, int32_t L, int32_t T, int64_t counts[4]) {
    if (!unary || !counts || N <= 0 || L <= 0 || T < 0 || (T > 0 && !tcosts)) return fail(MSM_ERR_INVALID, "msm_mplp_classify: bad arguments");
    mplp_classify(unary, (size_t)L * N, tcosts, (size_t)T * L * L * L, counts);
    return MSM_OK;
}

int msm_mplp_optimise_forbid(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, int32_t sweeps,
                             int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds, double *messages,
                             int64_t counts[4]) {
    return optimise_host(unary, tcosts, triplets, N, L, T, sweeps, {labeling, sweeps_run, energy, bound, energies, bounds, messages}, true, counts);
}

int msm_mplp_optimise_forbid_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T,
                                 int32_t sweeps, int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds,
                                 double *messages, int64_t counts[4]) {
    return optimise_gpu(ctx, unary, tcosts, triplets, N, L, T, sweeps, {labeling, sweeps_run, energy, bound, energies, bounds, messages}, true, counts);
}

int msm_mplp_colouring(const int32_t *triplets, int32_t N, int32_t T, int32_t *colour, int32_t *classes) {
    const char *what = "msm_mplp_colouring";
    if (!colour || N <= 0 || T < 0 || (T > 0 && !triplets)) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    const std::vector<int32_t> zeros((size_t)N, 0);
    MSM_TRY(mplp_check_arguments(what, triplets, N, 1, T, 0, zeros.data()));
    MplpIncidence inc;
    mplp_build_incidence(triplets, N, T, inc);
    MplpColouring col;
    mplp_build_colouring(triplets, N, inc, col);
    std::copy(col.colour.begin(), col.colour.end(), colour);
    if (classes) *classes = col.classes();
    return MSM_OK;
}

int msm_mplp_round(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const double *messages, int32_t mode,
                   int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies) {
    return round_host(unary, tcosts, triplets, N, L, T, messages, mode, polish, {labeling, passes_run, energy, energies}, false, nullptr);
}

int msm_mplp_round_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const double *messages,
                       int32_t mode, int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies) {
    return round_gpu(ctx, unary, tcosts, triplets, N, L, T, messages, mode, polish, {labeling, passes_run, energy, energies}, false, nullptr);
}

int msm_mplp_round_forbid(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const double *messages,
                          int32_t mode, int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies, int64_t counts[4]) {
    return round_host(unary, tcosts, triplets, N, L, T, messages, mode, polish, {labeling, passes_run, energy, energies}, true, counts);
}

int msm_mplp_round_forbid_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T,
                              const double *messages, int32_t mode, int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies,
                              int64_t counts[4]) {
    return round_gpu(ctx, unary, tcosts, triplets, N, L, T, messages, mode, polish, {labeling, passes_run, energy, energies}, true, counts);
}

int msm_mplp_round_gpu_stats(msm_ctx *ctx, double stats[4]) {
    if (!ctx || !stats) return fail(MSM_ERR_INVALID, "msm_mplp_round_gpu_stats: null argument");
    std::memcpy(stats, mplp_scratch(ctx).round_stats, sizeof(double) * 4);
    return MSM_OK;
}

int msm_mplp_gpu_stats(msm_ctx *ctx, double stats[4]) {
    if (!ctx || !stats) return fail(MSM_ERR_INVALID, "msm_mplp_gpu_stats: null argument");
    std::memcpy(stats, mplp_scratch(ctx).stats, sizeof(double) * 4);
    return MSM_OK;
}

}  // extern "C"
