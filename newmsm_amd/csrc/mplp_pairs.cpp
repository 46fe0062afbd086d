// mplp_pairs.cpp -- the host side of MPLP over the pair tables (mplp_pairs.hpp; kernels: mplp_pairs_kernels.hip; the serial literal:
// mplp_pairs_host.hpp), shaped like mplp.cpp: the checks both sides share, the tables counted by one classification (mplp_classify /
// k_mplp_classify) and judged by mplp_judge under the plain reading, the loop that queues a chunk of sweeps -- a launch per pair class, the decode, the
// energy terms, the bound terms -- and sums what comes back in the literal's order, the polish with a launch per node class and pass, and the entry
// points over host tables.
#include <cstring>

#include "mplp_pairs.hpp"

using namespace msm;

namespace {

struct MplpPairScratch {
    DevBuf<double> U, pc;  // the host tables of the *_gpu entry points
    DevBuf<int32_t> pairs, sched, inc_ptr, inc_slot, start, labs, changed;
    DevBuf<unsigned long long> counts;  // k_mplp_classify's four
    DevBuf<double> m, eterms, bterms;
    DevBuf<int32_t> cls_node, cur, rlabs, rchanged;  // the polish's own
    DevBuf<double> rterms;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double stats[6] = {0, 0, 0, 0, 0, 0};
    ~MplpPairScratch() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

MplpPairScratch &scratch_of(msm_ctx *ctx) {
    if (!ctx->mplp_pairs_scratch)
        ctx->mplp_pairs_scratch = std::shared_ptr<void>(new MplpPairScratch(), [](void *p) { delete static_cast<MplpPairScratch *>(p); });
    return *static_cast<MplpPairScratch *>(ctx->mplp_pairs_scratch.get());
}

int refuse_label_count(const char *what, int L) {
    return fail(MSM_ERR_CAPACITY, "%s: %d labels; a pair's cavities and minima live in the LDS of one workgroup (at most %d labels)", what, L, kMplpMaxLabels);
}

int check_pointers(const char *what, const double *unary, const double *paircosts, const int32_t *pairs, int N, int L, int P, int sweeps, const int32_t *labeling) {
    if (!unary || !labeling || N <= 0 || L <= 0 || P < 0 || sweeps < 0 || (P > 0 && (!paircosts || !pairs))) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    return MSM_OK;
}

int check_polish(const char *what, int polish) {
    if (polish < 0 || polish > kMplpMaxPolish) return fail(MSM_ERR_INVALID, "%s: %d polish passes (0 to %d)", what, polish, kMplpMaxPolish);
    return MSM_OK;
}

// the plain reading over counted tables; the refusal names the unary table first, then the pair table
int judge(const char *what, const int64_t counts[4]) {
    MplpReading r(false);
    r.table = "pair";
    std::copy(counts, counts + 4, r.counts);
    bool F = false;
    return mplp_judge(what, r, nullptr, &F);
}

// one device pass over both tables unless they have passed already
int inspect_device(msm_ctx *ctx, const char *what, MplpPairScratch &s, const double *d_U, size_t nU, const double *d_pc, size_t npc, bool *inspected) {
    if (inspected && *inspected) return MSM_OK;
    int64_t got[4] = {0, 0, 0, 0};
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are downloaded as they are");
    if (s.counts.zero(4, ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int64_t) * 4);
    MSM_TRY(launch_mplp_classify(ctx, d_U, nU, d_pc, npc, s.counts.p));
    MSM_TRY(s.counts.download(reinterpret_cast<unsigned long long *>(got), 4, ctx));
    MSM_TRY(check_status(ctx, what));
    MSM_TRY(judge(what, got));
    if (inspected) *inspected = true;
    return MSM_OK;
}

// sweeps or passes per chunk of n: what a chunk brings back (N + P doubles per sweep) stays below 32 MB, and a run that reaches its fixed point early
// in a chunk has at most 255 idle sweeps' launches behind it
int chunk_size(int n, size_t nterms) { return (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(n, 256), ((size_t)1 << 22) / nterms)); }

int ensure_events(MplpPairScratch &s) {
    for (hipEvent_t &e : s.ev)
        if (!e) MSM_HIP(hipEventCreate(&e));
    return MSM_OK;
}

int widest(const MplpColouring &col) {
    int w = 0;
    for (int k = 0; k < col.classes(); ++k) w = std::max(w, (int)(col.class_off[(size_t)k + 1] - col.class_off[(size_t)k]));
    return w;
}

}  // namespace

namespace msm {

int mplp_pairs_check_arguments(const char *what, const int32_t *pairs, int N, int L, int P, int sweeps, const int32_t *labeling) {
    if (sweeps < 0) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    MSM_TRY(mcmc_check_arguments(nullptr, N, L, 0, 1.0, labeling));  // the labels, with msm_mcmc_optimise's wording
    for (int64_t q = 0; q < 2 * (int64_t)P; ++q)
        if (pairs[q] < 0 || pairs[q] >= N) return fail(MSM_ERR_INVALID, "%s: pair node out of range", what);
    const int p = mplp_pairs_first_loop(pairs, P);
    if (p >= 0) return fail(MSM_ERR_INVALID, "%s: pair %d names a node twice", what, p);
    return MSM_OK;
}

int mplp_pairs_run_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_pc, const int32_t *pairs, int N, int L, int P, int sweeps,
                          const MplpOutputs &o, bool *inspected) {
    MplpPairScratch &s = scratch_of(ctx);
    const size_t nU = (size_t)L * N, npc = (size_t)P * L * L, nm = 2 * (size_t)P * L, nterms = (size_t)N + P;
    MSM_TRY(inspect_device(ctx, what, s, d_U, nU, d_pc, npc, inspected));
    if (L > kMplpMaxLabels) return refuse_label_count(what, L);

    MplpIncidence inc;
    mplp_pairs_build_incidence(pairs, N, P, inc);
    MplpColouring col;
    mplp_pairs_colour_pairs(pairs, P, inc, col);
    const int chunk = chunk_size(sweeps, nterms), classes = col.classes();
    MSM_TRY(s.pairs.upload(pairs, 2 * (size_t)P, ctx));
    MSM_TRY(s.sched.upload_vec(col.node, ctx));
    MSM_TRY(s.inc_ptr.upload_vec(inc.ptr, ctx));
    MSM_TRY(s.inc_slot.upload_vec(inc.slot, ctx));
    MSM_TRY(s.start.upload(o.labeling, (size_t)N, ctx));
    if (s.m.zero(std::max<size_t>(nm, 1), ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(double) * nm);
    if (s.changed.zero((size_t)std::max(sweeps, 1), ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * (size_t)sweeps);
    if (s.labs.ensure((size_t)chunk * N) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * (size_t)chunk * N);
    if (s.eterms.ensure((size_t)chunk * nterms) != hipSuccess || s.bterms.ensure((size_t)chunk * nterms) != hipSuccess)
        return stage_alloc_failed(sizeof(double) * (size_t)chunk * nterms);
    MSM_TRY(ensure_events(s));

    const MplpPairArgs a = {d_U, d_pc, s.pairs.p, s.sched.p, s.inc_ptr.p, s.inc_slot.p, s.m.p, s.changed.p, N, L, P, ctx->d_status};

    // candidate 0: the start
    std::vector<double> eterms((size_t)chunk * nterms), bterms((size_t)chunk * nterms);
    MSM_TRY(launch_mplp_pair_energy_terms(ctx, a, s.start.p, s.eterms.p));
    MSM_TRY(s.eterms.download(eterms.data(), nterms, ctx));
    MSM_TRY(check_status(ctx, what));
    MplpWinner win(o.labeling, N, mcmc_energy_of_terms(eterms.data(), N, P));

    std::vector<int32_t> labs((size_t)chunk * N), changed((size_t)sweeps, 0);
    std::vector<double> energies((size_t)sweeps), bounds(o.bounds ? (size_t)sweeps : 0);
    int run = 0;
    double kernel_ms = 0.0, e_last = 0.0, b_last = 0.0;
    bool fixed = false;
    for (int k0 = 0; k0 < sweeps && P > 0 && !fixed; k0 += chunk) {
        const int n = std::min(chunk, sweeps - k0);
        MSM_HIP(hipEventRecord(s.ev[0], ctx->stream));
        for (int j = 0; j < n; ++j) {
            for (int c = 0; c < classes; ++c)
                MSM_TRY(launch_mplp_pair_update(ctx, a, col.class_off[(size_t)c], col.class_off[(size_t)c + 1] - col.class_off[(size_t)c], k0 + j));
            MSM_TRY(launch_mplp_pair_decode(ctx, a, s.labs.p + (size_t)j * N, s.bterms.p + (size_t)j * nterms));
            MSM_TRY(launch_mplp_pair_energy_terms(ctx, a, s.labs.p + (size_t)j * N, s.eterms.p + (size_t)j * nterms));
            if (o.bounds) MSM_TRY(launch_mplp_pair_factor_terms(ctx, a, s.bterms.p + (size_t)j * nterms + N, k0 + j));
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
            energies[(size_t)k] = e_last = mcmc_energy_of_terms(eterms.data() + (size_t)j * nterms, N, P);
            win.offer(labs.data() + (size_t)j * N, N, e_last);
            if (o.bounds) bounds[(size_t)k] = b_last = mplp_bound_of_terms(bterms.data() + (size_t)j * nterms, N, P);
        }
    }
    for (int k = run; k < sweeps && run > 0; ++k) {
        energies[(size_t)k] = e_last;
        if (o.bounds) bounds[(size_t)k] = b_last;
    }
    double bound = b_last;
    if (o.bound && !(o.bounds && run > 0)) {  // one pass over the table for the bound of the last messages
        MSM_TRY(launch_mplp_pair_decode(ctx, a, nullptr, s.bterms.p));
        MSM_TRY(launch_mplp_pair_factor_terms(ctx, a, s.bterms.p + N, -1));
        MSM_TRY(s.bterms.download(bterms.data(), nterms, ctx));
        MSM_TRY(check_status(ctx, what));
        bound = mplp_bound_of_terms(bterms.data(), N, P);
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
    s.stats[1] = classes;
    s.stats[2] = run;
    s.stats[3] = widest(col);
    s.stats[4] = s.stats[5] = 0.0;
    return MSM_OK;
}

int mplp_pairs_polish_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_pc, const int32_t *pairs, int N, int L, int P, int polish,
                             const MplpRoundOutputs &o, bool *inspected) {
    MplpPairScratch &s = scratch_of(ctx);
    const size_t nU = (size_t)L * N, npc = (size_t)P * L * L, nterms = (size_t)N + P;
    MSM_TRY(inspect_device(ctx, what, s, d_U, nU, d_pc, npc, inspected));
    MSM_TRY(check_polish(what, polish));
    if (L > kMplpMaxLabels) return refuse_label_count(what, L);

    MplpIncidence inc;
    mplp_pairs_build_incidence(pairs, N, P, inc);
    MplpColouring col;
    mplp_pairs_colour_nodes(pairs, N, inc, col);
    const int chunk = chunk_size(polish, nterms), classes = col.classes();
    MSM_TRY(s.pairs.upload(pairs, 2 * (size_t)P, ctx));
    MSM_TRY(s.inc_ptr.upload_vec(inc.ptr, ctx));
    MSM_TRY(s.inc_slot.upload_vec(inc.slot, ctx));
    MSM_TRY(s.cls_node.upload_vec(col.node, ctx));
    MSM_TRY(s.cur.upload(o.labeling, (size_t)N, ctx));
    if (s.rchanged.zero((size_t)std::max(polish, 1), ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * (size_t)polish);
    if (s.rlabs.ensure((size_t)chunk * N) != hipSuccess) return stage_alloc_failed(sizeof(int32_t) * (size_t)chunk * N);
    if (s.rterms.ensure((size_t)chunk * nterms) != hipSuccess) return stage_alloc_failed(sizeof(double) * (size_t)chunk * nterms);
    MSM_TRY(ensure_events(s));

    const MplpPairPolishArgs a = {d_U, d_pc, s.pairs.p, s.inc_ptr.p, s.inc_slot.p, s.cls_node.p, s.cur.p, s.rchanged.p, N, L, P, ctx->d_status};
    const MplpPairArgs t = {d_U, d_pc, s.pairs.p, nullptr, s.inc_ptr.p, s.inc_slot.p, nullptr, nullptr, N, L, P, ctx->d_status};  // of the energy terms
    auto snapshot = [&](size_t j) -> int {  // the labelling as it stands and its energy terms, to place j of the chunk
        MSM_HIP(hipMemcpyAsync(s.rlabs.p + j * N, s.cur.p, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
        return launch_mplp_pair_energy_terms(ctx, t, s.cur.p, s.rterms.p + j * nterms);
    };

    // candidate 0: the labelling handed in
    std::vector<double> terms((size_t)chunk * nterms), energies((size_t)1 + polish);
    std::vector<int32_t> labs((size_t)chunk * N), changed((size_t)polish, 0);
    MSM_TRY(launch_mplp_pair_energy_terms(ctx, t, s.cur.p, s.rterms.p));
    MSM_TRY(s.rterms.download(terms.data(), nterms, ctx));
    MSM_TRY(check_status(ctx, what));
    double e_last = mcmc_energy_of_terms(terms.data(), N, P), polish_ms = 0.0;
    MplpWinner win(o.labeling, N, e_last);
    energies[0] = e_last;

    int run = 0;
    bool fixed = false;
    for (int p0 = 0; p0 < polish && !fixed; p0 += chunk) {
        const int n = std::min(chunk, polish - p0);
        MSM_HIP(hipEventRecord(s.ev[0], ctx->stream));
        for (int j = 0; j < n; ++j) {
            for (int k = 0; k < classes; ++k)
                MSM_TRY(launch_mplp_pair_polish(ctx, a, col.class_off[(size_t)k], col.class_off[(size_t)k + 1] - col.class_off[(size_t)k], p0 + j));
            MSM_TRY(snapshot((size_t)j));
        }
        MSM_HIP(hipEventRecord(s.ev[1], ctx->stream));
        MSM_TRY(s.rlabs.download(labs.data(), (size_t)n * N, ctx));
        MSM_TRY(s.rterms.download(terms.data(), (size_t)n * nterms, ctx));
        MSM_TRY(stage_d2h(ctx, changed.data() + p0, s.rchanged.p + p0, sizeof(int32_t) * (size_t)n));
        MSM_TRY(check_status(ctx, what));
        float ms = 0.f;
        MSM_HIP(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
        polish_ms += ms;
        for (int j = 0; j < n; ++j) {
            const int p = p0 + j;
            if (p > 0 && changed[(size_t)p - 1] == 0) {  // pass p - 1 changed no label: pass p and the rest did not run
                fixed = true;
                break;
            }
            run = p + 1;
            energies[(size_t)1 + p] = e_last = mcmc_energy_of_terms(terms.data() + (size_t)j * nterms, N, P);
            win.offer(labs.data() + (size_t)j * N, N, e_last);
        }
    }
    for (int p = run; p < polish; ++p) energies[(size_t)1 + p] = e_last;
    std::copy(win.lab.begin(), win.lab.end(), o.labeling);
    if (o.passes_run) *o.passes_run = run;
    if (o.energy) *o.energy = win.energy;
    if (o.energies) std::copy(energies.begin(), energies.end(), o.energies);
    s.stats[4] = polish_ms;
    s.stats[5] = run;
    return MSM_OK;
}

}  // namespace msm

namespace {

int inspect_host(const char *what, const double *unary, const double *paircosts, int N, int L, int P) {
    int64_t counts[4];
    mplp_classify(unary, (size_t)L * N, paircosts, (size_t)P * L * L, counts);
    return judge(what, counts);
}

// uploads both host tables into the scratch of the context
int upload_tables(msm_ctx *ctx, MplpPairScratch &s, const double *unary, const double *paircosts, int N, int L, int P) {
    const size_t nU = (size_t)L * N, npc = (size_t)P * L * L;
    if (s.U.ensure(nU) != hipSuccess) return stage_alloc_failed(sizeof(double) * nU);
    if (s.pc.ensure(npc ? npc : 1) != hipSuccess) return stage_alloc_failed(sizeof(double) * npc);
    MSM_TRY(upload_in_pieces(ctx, s.U.p, unary, sizeof(double) * nU));
    return upload_in_pieces(ctx, s.pc.p, paircosts, sizeof(double) * npc);
}

}  // namespace

extern "C" {

int msm_mplp_pairs_colouring(const int32_t *pairs, int32_t N, int32_t P, int32_t *pair_colour, int32_t *pair_classes, int32_t *node_colour,
                             int32_t *node_classes) {
    const char *what = "msm_mplp_pairs_colouring";
    if (N <= 0 || P < 0 || (P > 0 && !pairs)) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    const std::vector<int32_t> zeros((size_t)N, 0);
    MSM_TRY(mplp_pairs_check_arguments(what, pairs, N, 1, P, 0, zeros.data()));
    MplpIncidence inc;
    mplp_pairs_build_incidence(pairs, N, P, inc);
    MplpColouring pc, nc;
    mplp_pairs_colour_pairs(pairs, P, inc, pc);
    mplp_pairs_colour_nodes(pairs, N, inc, nc);
    if (pair_colour) std::copy(pc.colour.begin(), pc.colour.end(), pair_colour);
    if (pair_classes) *pair_classes = pc.classes();
    if (node_colour) std::copy(nc.colour.begin(), nc.colour.end(), node_colour);
    if (node_classes) *node_classes = nc.classes();
    return MSM_OK;
}

int msm_mplp_pairs_energy(const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P, const int32_t *labeling,
                          double *energy) {
    const char *what = "msm_mplp_pairs_energy";
    if (!energy) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    MSM_TRY(check_pointers(what, unary, paircosts, pairs, N, L, P, 0, labeling));
    MSM_TRY(mplp_pairs_check_arguments(what, pairs, N, L, P, 0, labeling));
    std::vector<double> terms((size_t)N + P);
    mplp_pairs_energy_terms(unary, paircosts, pairs, N, L, P, labeling, terms.data());
    *energy = mcmc_energy_of_terms(terms.data(), N, P);
    return MSM_OK;
}

int msm_mplp_pairs_optimise(const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P, int32_t sweeps,
                            int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds, double *messages) {
    const char *what = "msm_mplp_pairs_optimise";
    MSM_TRY(check_pointers(what, unary, paircosts, pairs, N, L, P, sweeps, labeling));
    MSM_TRY(mplp_pairs_check_arguments(what, pairs, N, L, P, sweeps, labeling));
    MSM_TRY(inspect_host(what, unary, paircosts, N, L, P));
    if (L > kMplpMaxLabels) return refuse_label_count(what, L);
    mplp_pairs_run_host(unary, paircosts, pairs, N, L, P, sweeps, {labeling, sweeps_run, energy, bound, energies, bounds, messages});
    return MSM_OK;
}

int msm_mplp_pairs_optimise_gpu(msm_ctx *ctx, const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P,
                                int32_t sweeps, int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds,
                                double *messages) {
    const char *what = "msm_mplp_pairs_optimise";
    if (!ctx) return fail(MSM_ERR_INVALID, "msm_mplp_pairs_optimise_gpu: null context");
    MSM_TRY(check_pointers(what, unary, paircosts, pairs, N, L, P, sweeps, labeling));
    MSM_TRY(mplp_pairs_check_arguments(what, pairs, N, L, P, sweeps, labeling));
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MplpPairScratch &s = scratch_of(ctx);
    MSM_TRY(upload_tables(ctx, s, unary, paircosts, N, L, P));
    return mplp_pairs_run_device(ctx, what, s.U.p, s.pc.p, pairs, N, L, P, sweeps, {labeling, sweeps_run, energy, bound, energies, bounds, messages}, nullptr);
}

int msm_mplp_pairs_polish(const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P, int32_t polish,
                          int32_t *labeling, int32_t *passes_run, double *energy, double *energies) {
    const char *what = "msm_mplp_pairs_polish";
    MSM_TRY(check_pointers(what, unary, paircosts, pairs, N, L, P, 0, labeling));
    MSM_TRY(mplp_pairs_check_arguments(what, pairs, N, L, P, 0, labeling));
    MSM_TRY(inspect_host(what, unary, paircosts, N, L, P));
    MSM_TRY(check_polish(what, polish));
    if (L > kMplpMaxLabels) return refuse_label_count(what, L);
    mplp_pairs_polish_host(unary, paircosts, pairs, N, L, P, polish, {labeling, passes_run, energy, energies});
    return MSM_OK;
}

int msm_mplp_pairs_polish_gpu(msm_ctx *ctx, const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P,
                              int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies) {
    const char *what = "msm_mplp_pairs_polish";
    if (!ctx) return fail(MSM_ERR_INVALID, "msm_mplp_pairs_polish_gpu: null context");
    MSM_TRY(check_pointers(what, unary, paircosts, pairs, N, L, P, 0, labeling));
    MSM_TRY(mplp_pairs_check_arguments(what, pairs, N, L, P, 0, labeling));
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MplpPairScratch &s = scratch_of(ctx);
    MSM_TRY(upload_tables(ctx, s, unary, paircosts, N, L, P));
    return mplp_pairs_polish_device(ctx, what, s.U.p, s.pc.p, pairs, N, L, P, polish, {labeling, passes_run, energy, energies}, nullptr);
}

int msm_mplp_pairs_gpu_stats(msm_ctx *ctx, double stats[6]) {
    if (!ctx || !stats) return fail(MSM_ERR_INVALID, "msm_mplp_pairs_gpu_stats: null argument");
    std::memcpy(stats, scratch_of(ctx).stats, sizeof(double) * 6);
    return MSM_OK;
}

}  // extern "C"
