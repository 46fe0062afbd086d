// cost_cliques.cpp -- C ABI of the pairwise / triplet clique costs and of evaluateTotalCostSum
// (include/msmhip.h), except the label step (label_step.cpp).  Kernels: clique_kernels.hip.
#include <algorithm>

#include "cost_internal.hpp"
#include "label_step.hpp"
#include "mcmc.hpp"
#include "mplp.hpp"
#include "mplp_pairs.hpp"

using namespace msm;

namespace msm {

// everything the clique kernels read; uploads the control grid's connectivity on first use
int clique_args(msm_cost *c, bool need_triplets, bool need_pairs, CliqueArgs &a) {
    if (int st = drop_pending_move(c)) return st;
    if (int st = drop_ctx_pending(c->ctx)) return st;  // (another cost function's, on the same context)
    if (!c->cpgrid || !c->source || !c->target) return fail(MSM_ERR_STATE, "msm_cost: meshes must be set first");
    if (need_triplets && c->triplets.empty()) return fail(MSM_ERR_STATE, "msm_cost: triplets must be set first");
    if (need_pairs && c->pairs.empty()) return fail(MSM_ERR_STATE, "msm_cost: pairs must be set first");
    int st = ensure_label_rotations(c);
    if (st) return st;
    msm_ctx *ctx = c->ctx;
    msm_mesh *g = c->cpgrid;
    if (!c->cp_conn_valid) {
        const Adjacency &adj = mesh_adjacency(g);
        MSM_TRY(c->d_cp_tri.upload(g->tri.data(), g->tri.size(), ctx));
        MSM_TRY(c->d_cp_tid_ptr.upload(adj.tid_ptr.data(), adj.tid_ptr.size(), ctx));
        MSM_TRY(c->d_cp_tid.upload(adj.tid.data(), adj.tid.size(), ctx));
        MSM_TRY(ctx_sync(ctx));
        c->cp_conn_valid = true;
    }
    a.kind = c->p.kind;
    a.simmeasure = c->p.simmeasure;
    a.N = g->V;
    a.L = c->L;
    a.T = (int)(c->triplets.size() / 3);
    a.P = (int)(c->pairs.size() / 2);
    a.triplets = c->d_triplets.p;
    a.pairs = c->d_pairs.p;
    a.cp = g->d_xyz.p;
    a.ocp = c->d_ocp.p;
    a.orig = c->d_orig.p;
    a.Norig = (int)(c->orig_xyz.size() / 3);
    a.moved = c->d_moved.p;
    a.rnl = c->d_rnl.p;
    a.cp_tri = c->d_cp_tri.p;
    a.Tc = g->T;
    a.cp_tid_ptr = c->d_cp_tid_ptr.p;
    a.cp_tid = c->d_cp_tid.p;
    a.lambda = c->p.lambda;
    a.mu = c->p.mu;
    a.kappa = c->p.kappa;
    a.k_exp = c->p.k_exp;
    a.rexp = c->p.rexp;
    a.mvdmax = c->mvdmax;
    a.percentile = c->p.percentile;
    a.tfeat = c->target->d_feat.p;
    a.D = c->D;
    a.src = c->source->d_xyz.p;
    a.Nsrc = c->source->V;
    a.sfeat = c->d_sfeat.p;
    a.cfw = c->cfw.empty() ? nullptr : c->d_cfw.p;
    a.cfw_rows = c->cfw_rows;
    a.sfeat_vm = a.cfw_vm = nullptr;
    a.bin_ptr = c->d_pptr.p;
    a.bin_idx = c->d_pidx.p;
    a.bin_cap = std::max(c->pmax, 1);
    a.ho_vals = nullptr;
    a.ho_big = nullptr;
    a.ho_pending = nullptr;
    a.ho_count = nullptr;
    a.absw = c->d_absw.p;
    a.status = ctx->d_status;
    if (need_triplets && cost_is_ho(c)) {
        if (!c->have_source) return fail(MSM_ERR_STATE, "msm_cost: get_source_data() must be called first");
        if (!c->target->d_feat.p || c->target->D != c->D) return fail(MSM_ERR_STATE, "msm_cost: target features must match the source features");
        // the triclique likelihood is evaluated by hundreds of fusion moves per level and its two kernel families sum in
        // different orders, so this path waits for the direction table instead of switching to it mid-run
        st = ensure_rays(c->target, true);  // includes the sub-cell masks the group search uses
        if (st) return st;
        if (c->p.kind == MSM_COST_HO_MULTIVARIATE) {
            st = ensure_vertex_major(c);
            if (st) return st;
            a.sfeat_vm = c->d_sfeat_vm.p;
            a.cfw_vm = c->cfw.empty() ? nullptr : c->d_cfw_vm.p;
        }
        if (c->target->tree.rays.G > 0 && c->pmax <= 1024 && a.T < (1 << 18)) {  // fusion moves: sample -> fix up -> reduce
            const size_t nv = 8 * c->pidx.size();
            MSM_HIP(c->d_ho_vals.ensure(std::max<size_t>(nv, 1)));
            MSM_HIP(c->d_ho_pending.ensure(std::max<size_t>(nv, 1)));
            if (!c->d_ho_count.p) MSM_HIP(c->d_ho_count.zero(1, ctx->stream));
            a.ho_vals = c->d_ho_vals.p;
            a.ho_pending = c->d_ho_pending.p;
            a.ho_count = c->d_ho_count.p;
        }
        if (c->pmax > kHoBinMax) {
            // a bin that outgrows a workgroup's LDS (an ico7 data mesh under an ico0 control grid; the reference pushes into a std::vector,
            // M/DiscreteCostFunction.cpp:468-485, and has no limit): the sampled values of an evaluation live in HBM, a slice per workgroup
            MSM_HIP(c->d_ho_big.ensure((size_t)kHoBigBlocks * (size_t)c->pmax));
            a.ho_big = c->d_ho_big.p;
        }
    }
    a.tree = dev_tree(c->target);
    a.rmode = c->p.rmode;
    a.atree = DevTree{};
    a.atarget = a.asrc = a.aw_val = nullptr;
    a.asrc_tri = a.aw_ptr = a.aw_cp = a.af_ptr = a.af_idx = nullptr;
    a.Va = a.Vs = a.Ts = 0;
    if (need_triplets && (c->p.rmode == 4 || c->p.rmode == 5)) {
        if (!c->have_anat) return fail(MSM_ERR_STATE, "MeshREG ERROR:: regoption 5 requires anatomical meshes (msm_cost_set_anatomical)");  // M/mesh_registration.cpp:103
        st = ensure_tree(c->asphere);
        if (st) return st;
        a.atree = dev_tree(c->asphere);
        a.atarget = c->d_atarget.p;
        a.Va = c->asphere->V;
        a.asrc = c->d_asrc.p;
        a.Vs = c->aVs;
        a.asrc_tri = c->d_asrc_tri.p;
        a.Ts = c->aTs;
        a.aw_ptr = c->d_aw_ptr.p;
        a.aw_cp = c->d_aw_cp.p;
        a.aw_val = c->d_aw_val.p;
        a.af_ptr = c->d_af_ptr.p;
        a.af_idx = c->d_af_idx.p;
    } else if (need_triplets && c->p.rmode != 2 && c->p.rmode != 3) {
        return fail(MSM_ERR_INVALID, "DiscreteModel computeTripletCost regoption does not exist");  // M/DiscreteCostFunction.cpp:184
    }
    return MSM_OK;
}

}  // namespace msm

static int upload_ints(msm_ctx *ctx, DevBuf<int> &buf, const int32_t *host, size_t n) {
    MSM_TRY(buf.upload(host, n, ctx));
    return MSM_OK;
}

extern "C" {

int msm_cost_set_anatomical(msm_cost *c, msm_mesh *sphere, const double *atarget_xyz, const double *asource_xyz, int32_t Vs,
                            const int32_t *asource_tri, int32_t Ts, const int32_t *w_ptr, const int32_t *w_cp, const double *w_val,
                            const int32_t *face_ptr, const int32_t *face_idx) {
    if (!c || !sphere || !atarget_xyz || !asource_xyz || !asource_tri || !w_ptr || !w_cp || !w_val || !face_ptr || !face_idx || Vs <= 0 || Ts <= 0)
        return fail(MSM_ERR_INVALID, "msm_cost_set_anatomical: bad arguments");
    const int T = (int)(c->triplets.size() / 3);
    if (T == 0 || !c->cpgrid) return fail(MSM_ERR_STATE, "msm_cost_set_anatomical: set_meshes and set_triplets first");
    const int N = c->cpgrid->V;
    if (w_ptr[0] != 0 || face_ptr[0] != 0) return fail(MSM_ERR_INVALID, "msm_cost_set_anatomical: CSR rows must start at 0");
    for (int v = 0; v < Vs; ++v)
        if (w_ptr[v + 1] < w_ptr[v]) return fail(MSM_ERR_INVALID, "msm_cost_set_anatomical: weight rows are not monotone");
    for (int j = 0; j < w_ptr[Vs]; ++j)
        if (w_cp[j] < 0 || w_cp[j] >= N) return fail(MSM_ERR_INVALID, "msm_cost_set_anatomical: control point id %d out of range", w_cp[j]);
    for (int v = 0; v < Vs; ++v)
        for (int j = w_ptr[v] + 1; j < w_ptr[v + 1]; ++j)
            if (w_cp[j] <= w_cp[j - 1]) return fail(MSM_ERR_INVALID, "msm_cost_set_anatomical: control point ids must ascend within a row (std::map order)");
    for (int t = 0; t < T; ++t)
        if (face_ptr[t + 1] < face_ptr[t]) return fail(MSM_ERR_INVALID, "msm_cost_set_anatomical: face rows are not monotone");
    for (int j = 0; j < face_ptr[T]; ++j)
        if (face_idx[j] < 0 || face_idx[j] >= Ts) return fail(MSM_ERR_INVALID, "msm_cost_set_anatomical: face id %d out of range", face_idx[j]);
    for (int j = 0; j < 3 * Ts; ++j)
        if (asource_tri[j] < 0 || asource_tri[j] >= Vs) return fail(MSM_ERR_INVALID, "msm_cost_set_anatomical: vertex id %d out of range", asource_tri[j]);
    msm_ctx *ctx = c->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(c->d_atarget.upload(atarget_xyz, 3 * (size_t)sphere->V, ctx));
    MSM_TRY(c->d_asrc.upload(asource_xyz, 3 * (size_t)Vs, ctx));
    MSM_TRY(c->d_asrc_tri.upload(asource_tri, 3 * (size_t)Ts, ctx));
    MSM_TRY(c->d_aw_ptr.upload(w_ptr, (size_t)Vs + 1, ctx));
    MSM_TRY(c->d_aw_cp.upload(w_cp, std::max<size_t>(w_ptr[Vs], 1), ctx));
    MSM_TRY(c->d_aw_val.upload(w_val, std::max<size_t>(w_ptr[Vs], 1), ctx));
    MSM_TRY(c->d_af_ptr.upload(face_ptr, (size_t)T + 1, ctx));
    MSM_TRY(c->d_af_idx.upload(face_idx, std::max<size_t>(face_ptr[T], 1), ctx));
    MSM_TRY(ctx_sync(ctx));  // the caller's arrays may go away
    c->asphere = sphere;
    c->aVs = Vs;
    c->aTs = Ts;
    c->have_anat = true;
    return MSM_OK;
}

int msm_cost_triplet_batch(msm_cost *c, const int32_t *triplet, const int32_t *la, const int32_t *lb, const int32_t *lc, int32_t n, double *out) {
    if (!c || !triplet || !la || !lb || !lc || !out || n < 0) return fail(MSM_ERR_INVALID, "msm_cost_triplet_batch: bad arguments");
    if (n == 0) return MSM_OK;
    CliqueArgs a;
    int st = clique_args(c, true, false, a);
    if (st) return st;
    for (int i = 0; i < n; ++i)
        if (triplet[i] < 0 || triplet[i] >= a.T || la[i] < 0 || la[i] >= a.L || lb[i] < 0 || lb[i] >= a.L || lc[i] < 0 || lc[i] >= a.L)
            return fail(MSM_ERR_INVALID, "triplet query %d out of range", i);
    msm_ctx *ctx = c->ctx;
    DevBuf<int> qt, qa, qb, qc;
    DevBuf<double> dout;
    if ((st = upload_ints(ctx, qt, triplet, n)) || (st = upload_ints(ctx, qa, la, n)) || (st = upload_ints(ctx, qb, lb, n)) ||
        (st = upload_ints(ctx, qc, lc, n)))
        return st;
    MSM_HIP(dout.ensure(n));
    st = launch_triplet_batch(ctx, a, qt.p, qa.p, qb.p, qc.p, n, dout.p);
    if (st) return st;
    MSM_TRY(dout.download(out, n, ctx));
    c->counters[2] += n;
    return check_status(ctx, "computeTripletCost");
}

int msm_cost_pairwise_batch(msm_cost *c, const int32_t *pair, const int32_t *la, const int32_t *lb, int32_t n, double *out) {
    if (!c || !pair || !la || !lb || !out || n < 0) return fail(MSM_ERR_INVALID, "msm_cost_pairwise_batch: bad arguments");
    if (n == 0) return MSM_OK;
    CliqueArgs a;
    int st = clique_args(c, false, true, a);
    if (st) return st;
    for (int i = 0; i < n; ++i)
        if (pair[i] < 0 || pair[i] >= a.P || la[i] < 0 || la[i] >= a.L || lb[i] < 0 || lb[i] >= a.L) return fail(MSM_ERR_INVALID, "pairwise query %d out of range", i);
    msm_ctx *ctx = c->ctx;
    DevBuf<int> qp, qa, qb;
    DevBuf<double> dout;
    if ((st = upload_ints(ctx, qp, pair, n)) || (st = upload_ints(ctx, qa, la, n)) || (st = upload_ints(ctx, qb, lb, n))) return st;
    MSM_HIP(dout.ensure(n));
    st = launch_pairwise_batch(ctx, a, qp.p, qa.p, qb.p, n, dout.p);
    if (st) return st;
    MSM_TRY(dout.download(out, n, ctx));
    c->counters[3] += n;
    return check_status(ctx, "computePairwiseCost");
}

int msm_cost_pairwise_table(msm_cost *c, double *paircosts) {
    if (!c || !paircosts) return fail(MSM_ERR_INVALID, "msm_cost_pairwise_table: null argument");
    CliqueArgs a;
    int st = clique_args(c, false, true, a);
    if (st) return st;
    msm_ctx *ctx = c->ctx;
    const size_t total = (size_t)a.P * a.L * a.L;
    MSM_HIP(c->d_clique_out.ensure(total));
    st = launch_pairwise_table(ctx, a, c->d_clique_out.p);
    if (st) return st;
    MSM_TRY(c->d_clique_out.download(paircosts, total, ctx));
    c->counters[3] += (int64_t)total;
    return check_status(ctx, "computePairwiseCosts");
}

int msm_cost_triplet_table(msm_cost *c, int32_t t0, int32_t t1, double *tcosts) {
    if (!c || !tcosts) return fail(MSM_ERR_INVALID, "msm_cost_triplet_table: null argument");
    CliqueArgs a;
    int st = clique_args(c, true, false, a);
    if (st) return st;
    if (t0 < 0 || t1 < t0 || t1 > a.T) return fail(MSM_ERR_INVALID, "msm_cost_triplet_table: triplet range [%d, %d) out of [0, %d)", t0, t1, a.T);
    msm_ctx *ctx = c->ctx;
    const size_t total = (size_t)(t1 - t0) * a.L * a.L * a.L;
    if (total == 0) return MSM_OK;
    if (total > ((size_t)1 << 31)) return fail(MSM_ERR_CAPACITY, "msm_cost_triplet_table: %zu values in one call; ask for a smaller triplet range", total);
    MSM_HIP(c->d_clique_out.ensure(total));
    st = launch_triplet_table(ctx, a, t0, t1, c->d_clique_out.p);
    if (st) return st;
    MSM_TRY(c->d_clique_out.download(tcosts, total, ctx));
    c->counters[2] += (int64_t)total;
    return check_status(ctx, "computeTripletCosts");
}

// computeUnaryCosts + computeTripletCosts with both tables staying where their kernels wrote them (c->d_U, c->d_clique_out), once the caller's checks have
// passed (msm_cost_mcmc_optimise*, msm_cost_mplp_optimise)
static int fill_tables_on_device(msm_cost *c, int *N, int *L, int *T) {
    MSM_TRY(msm_cost_unary_table_async(c));  // (drops a label step queued ahead on the context first)
    MSM_TRY(check_status(c->ctx, "computeUnaryCosts"));  // what the table's kernels raised is reported as msm_cost_unary_table reports it
    CliqueArgs a;
    MSM_TRY(clique_args(c, true, false, a));
    const size_t per = (size_t)a.L * a.L * a.L, total = (size_t)a.T * per;
    if (c->d_clique_out.ensure(total ? total : 1) != hipSuccess) return stage_alloc_failed(sizeof(double) * total);
    // the table kernel indexes one launch with 32 bits of workgroups: a table beyond 2^31 values is filled in triplet ranges
    const int step = (int)std::max<size_t>(1, std::min<size_t>((size_t)a.T, ((size_t)1 << 31) / per));
    for (int t0 = 0; t0 < a.T; t0 += step) MSM_TRY(launch_triplet_table(c->ctx, a, t0, std::min(a.T, t0 + step), c->d_clique_out.p + (size_t)t0 * per));
    c->counters[2] += (int64_t)total;
    *N = a.N, *L = a.L, *T = a.T;
    return check_status(c->ctx, "computeTripletCosts");  // before the sweeps, as msm_cost_triplet_table reports it
}

// what both msm_cost_mcmc_optimise* do ahead of the sweeps (mcmc.cpp runs those): the host optimiser's checks first, before anything is launched, then
// the two tables on the device
static int mcmc_tables_on_device(msm_cost *c, double mcparam, int32_t iters, const uint64_t *seeds, int32_t K, const int32_t *labeling, int *N, int *L, int *T) {
    if (!c || !labeling || iters < 0) return fail(MSM_ERR_INVALID, "msm_cost_mcmc_optimise: bad arguments");
    if (!c->cpgrid || c->L <= 0 || c->triplets.empty()) return fail(MSM_ERR_STATE, "msm_cost_mcmc_optimise: meshes, labels and triplets must be set first");
    MSM_TRY(mcmc_check_chains(seeds, K));
    MSM_TRY(mcmc_check_arguments(c->triplets.data(), c->cpgrid->V, c->L, (int)(c->triplets.size() / 3), mcparam, labeling));
    return fill_tables_on_device(c, N, L, T);
}

int msm_cost_mcmc_optimise(msm_cost *c, double mcparam, int32_t iters, uint64_t seed, int32_t *labeling) {
    int N, L, T;
    MSM_TRY(mcmc_tables_on_device(c, mcparam, iters, &seed, 1, labeling, &N, &L, &T));
    return mcmc_run_device(c->ctx, c->d_U.p, c->d_clique_out.p, c->triplets.data(), N, L, T, mcparam, iters, seed, labeling);
}

// the same for K chains from one start; the tables are built once and shared
int msm_cost_mcmc_optimise_chains(msm_cost *c, double mcparam, int32_t iters, const uint64_t *seeds, int32_t K, int32_t *labeling, int32_t *labelings,
                                  double *energies, int32_t *best) {
    int N, L, T;
    MSM_TRY(mcmc_tables_on_device(c, mcparam, iters, seeds, K, labeling, &N, &L, &T));
    return mcmc_run_device_chains(c->ctx, c->d_U.p, c->d_clique_out.p, c->triplets.data(), N, L, T, mcparam, iters, seeds, K, labeling, labelings, energies, best);
}

// what msm_cost_mplp_forbidden reports after the three calls below: the tables' counts under the forbidden-entry reading, once the tables have passed
// (st: the call's status, handed through)
static int keep_counts(msm_cost *c, const MplpReading &r, int st) {
    if (r.forbid && r.inspected) std::copy(r.counts, r.counts + 4, c->mplp_counts);
    return st;
}

// MPLP over the same two device tables (mplp.cpp runs the sweeps): the Monte Carlo argument checks do not apply, the MPLP ones do
int msm_cost_mplp_optimise(msm_cost *c, int32_t sweeps, int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies,
                           double *bounds, double *messages) {
    if (!c || !labeling || sweeps < 0) return fail(MSM_ERR_INVALID, "msm_cost_mplp_optimise: bad arguments");
    if (!c->cpgrid || c->L <= 0 || c->triplets.empty()) return fail(MSM_ERR_STATE, "msm_cost_mplp_optimise: meshes, labels and triplets must be set first");
    MSM_TRY(mplp_check_arguments("msm_mplp_optimise", c->triplets.data(), c->cpgrid->V, c->L, (int)(c->triplets.size() / 3), sweeps, labeling));
    int N, L, T;
    MSM_TRY(fill_tables_on_device(c, &N, &L, &T));
    const MplpOutputs o = {labeling, sweeps_run, energy, bound, energies, bounds, messages};
    MplpReading r(c->mplp_forbid);
    return keep_counts(c, r, mplp_run_device(c->ctx, "msm_mplp_optimise", c->d_U.p, c->d_clique_out.p, c->triplets.data(), N, L, T, sweeps, o, r));
}

// the switch to the forbidden-entry reading of the triplet table (DESIGN.md 5.19 "Forbidden entries") for the three calls here, and what the last
// of them counted
int msm_cost_set_mplp_forbid(msm_cost *c, int32_t on) {
    if (!c) return fail(MSM_ERR_INVALID, "msm_cost_set_mplp_forbid: null argument");
    c->mplp_forbid = on != 0;
    return MSM_OK;
}

int msm_cost_mplp_forbidden(msm_cost *c, int64_t counts[4]) {
    if (!c || !counts) return fail(MSM_ERR_INVALID, "msm_cost_mplp_forbidden: null argument");
    std::copy(c->mplp_counts, c->mplp_counts + 4, counts);
    return MSM_OK;
}

// MPLP's sweeps, then the rounding of mode 0 on the messages they left on the device, the sweeps' winner handed in (DESIGN.md 5.19 "Rounding").
// then_polish: a mode-1 call on that result follows over the same tables (what a level's iteration does); passes_run and energies stay mode 0's.
int msm_cost_mplp_round(msm_cost *c, int32_t sweeps, int32_t polish, int32_t then_polish, int32_t *labeling, int32_t *sweeps_run, int32_t *passes_run,
                        double *energy, double *bound, double *energies) {
    if (!c || !labeling || sweeps < 0) return fail(MSM_ERR_INVALID, "msm_cost_mplp_round: bad arguments");
    if (!c->cpgrid || c->L <= 0 || c->triplets.empty()) return fail(MSM_ERR_STATE, "msm_cost_mplp_round: meshes, labels and triplets must be set first");
    MSM_TRY(mplp_check_arguments("msm_mplp_round", c->triplets.data(), c->cpgrid->V, c->L, (int)(c->triplets.size() / 3), sweeps, labeling));
    MSM_TRY(mplp_round_check("msm_mplp_round", c->L, 0, polish));
    int N, L, T;
    MSM_TRY(fill_tables_on_device(c, &N, &L, &T));
    std::vector<int32_t> lab(labeling, labeling + N);  // the caller's labelling stays as it is when the rounding fails
    int32_t run = 0;
    double b = 0.0;
    const MplpOutputs o = {lab.data(), &run, nullptr, bound ? &b : nullptr, nullptr, nullptr, nullptr};
    // run, round on the run's messages with the run's reading, polish with the same reading
    const char *what = "msm_mplp_round";
    const double *d_U = c->d_U.p, *d_tc = c->d_clique_out.p;
    MplpReading r(c->mplp_forbid);
    MSM_TRY(keep_counts(c, r, mplp_run_device(c->ctx, what, d_U, d_tc, c->triplets.data(), N, L, T, sweeps, o, r)));
    const MplpRoundOutputs r0 = {lab.data(), passes_run, energy, energies}, r1 = {lab.data(), nullptr, energy, nullptr};
    MSM_TRY(mplp_round_device(c->ctx, what, d_U, d_tc, mplp_last_messages(c->ctx), c->triplets.data(), N, L, T, 0, polish, r0, r));
    if (then_polish) MSM_TRY(mplp_round_device(c->ctx, what, d_U, d_tc, nullptr, c->triplets.data(), N, L, T, 1, polish, r1, r));
    std::copy(lab.begin(), lab.end(), labeling);
    if (sweeps_run) *sweeps_run = run;
    if (bound) *bound = b;
    return MSM_OK;
}

// the rounding of mode 1 (polish passes of the labelling handed in; no messages) over the device tables
int msm_cost_mplp_polish(msm_cost *c, int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies) {
    if (!c || !labeling) return fail(MSM_ERR_INVALID, "msm_cost_mplp_polish: bad arguments");
    if (!c->cpgrid || c->L <= 0 || c->triplets.empty()) return fail(MSM_ERR_STATE, "msm_cost_mplp_polish: meshes, labels and triplets must be set first");
    MSM_TRY(mplp_check_arguments("msm_mplp_round", c->triplets.data(), c->cpgrid->V, c->L, (int)(c->triplets.size() / 3), 0, labeling));
    MSM_TRY(mplp_round_check("msm_mplp_round", c->L, 1, polish));
    int N, L, T;
    MSM_TRY(fill_tables_on_device(c, &N, &L, &T));
    const MplpRoundOutputs r = {labeling, passes_run, energy, energies};
    MplpReading rd(c->mplp_forbid);
    return keep_counts(c, rd, mplp_round_device(c->ctx, "msm_mplp_round", c->d_U.p, c->d_clique_out.p, nullptr, c->triplets.data(), N, L, T, 1, polish, r, rd));
}

// MPLP over the pair tables (mplp_pairs.cpp runs the sweeps and the polish): computeUnaryCosts + computePairwiseCosts with both tables
// staying where their kernels wrote them (c->d_U, c->d_clique_out), the sweeps from `labeling`, then `polish` passes of the sweeps' winner over the
// same tables, inspected once.  The forbidden-entry switch does not apply: computePairwiseCost returns a finite cost or the folding value.
int msm_cost_mplp_pairs_optimise(msm_cost *c, int32_t sweeps, int32_t polish, int32_t *labeling, int32_t *sweeps_run, int32_t *passes_run, double *energy,
                                 double *bound, double *energies, double *bounds, double *polish_energies) {
    const char *what = "msm_cost_mplp_pairs_optimise";  // every refusal and failure of this call, the sweeps' and the polish's included, names it
    if (!c || !labeling || sweeps < 0) return fail(MSM_ERR_INVALID, "%s: bad arguments", what);
    if (!c->cpgrid || c->L <= 0) return fail(MSM_ERR_STATE, "%s: meshes and labels must be set first", what);
    if (c->pairs.empty()) return fail(MSM_ERR_STATE, "%s: pairs must be set first (msm_cost_set_pairs)", what);
    if (polish < 0 || polish > kMplpMaxPolish) return fail(MSM_ERR_INVALID, "%s: %d polish passes (0 to %d)", what, polish, kMplpMaxPolish);
    MSM_TRY(mplp_pairs_check_arguments(what, c->pairs.data(), c->cpgrid->V, c->L, (int)(c->pairs.size() / 2), sweeps, labeling));
    MSM_TRY(msm_cost_unary_table_async(c));  // (drops a label step queued ahead on the context first)
    MSM_TRY(check_status(c->ctx, "computeUnaryCosts"));
    CliqueArgs a;
    MSM_TRY(clique_args(c, false, true, a));
    const size_t total = (size_t)a.P * a.L * a.L;
    if (c->d_clique_out.ensure(total) != hipSuccess) return stage_alloc_failed(sizeof(double) * total);
    MSM_TRY(launch_pairwise_table(c->ctx, a, c->d_clique_out.p));
    c->counters[3] += (int64_t)total;
    MSM_TRY(check_status(c->ctx, "computePairwiseCosts"));
    std::vector<int32_t> lab(labeling, labeling + a.N);  // the caller's labelling stays as it is when the polish fails
    int32_t run = 0, passes = 0;
    double e = 0.0, b = 0.0;
    std::vector<double> es((size_t)sweeps), bs(bounds ? (size_t)sweeps : 0);
    bool inspected = false;
    const MplpOutputs o = {lab.data(), &run, &e, bound ? &b : nullptr, es.data(), bounds ? bs.data() : nullptr, nullptr};
    MSM_TRY(mplp_pairs_run_device(c->ctx, what, c->d_U.p, c->d_clique_out.p, c->pairs.data(), a.N, a.L, a.P, sweeps, o, &inspected));
    if (polish > 0) {
        const MplpRoundOutputs r = {lab.data(), &passes, &e, polish_energies};
        MSM_TRY(mplp_pairs_polish_device(c->ctx, what, c->d_U.p, c->d_clique_out.p, c->pairs.data(), a.N, a.L, a.P, polish, r, &inspected));
    }
    std::copy(lab.begin(), lab.end(), labeling);
    if (sweeps_run) *sweeps_run = run;
    if (passes_run) *passes_run = passes;
    if (energy) *energy = e;
    if (bound) *bound = b;
    if (run > 0) {
        if (energies) std::copy(es.begin(), es.end(), energies);
        if (bounds) std::copy(bs.begin(), bs.end(), bounds);
    }
    return MSM_OK;
}

// evaluateTotalCostSum, M/DiscreteCostFunction.cpp:55-77: the three sums run in the reference's serial order on
// the host over device-evaluated terms (N + P + T values), because the order defines the reported energy
int msm_cost_total(msm_cost *c, const int32_t *labeling, double *total, double parts[3]) {
    if (!c || !labeling || !total) return fail(MSM_ERR_INVALID, "msm_cost_total: null argument");
    if (!c->cpgrid) return fail(MSM_ERR_STATE, "msm_cost: meshes must be set first");
    const int N = c->cpgrid->V;
    double u = 0.0, pw = 0.0, tc = 0.0;
    if (!cost_is_ho(c)) {  // the HO classes' computeUnaryCost returns 0 (M/DiscreteCostFunction.h:249,258): a sum of N zeros
        std::vector<int32_t> nodes(N);
        std::vector<double> vals(N);
        for (int i = 0; i < N; ++i) nodes[i] = i;
        int st = msm_cost_unary_batch(c, nodes.data(), labeling, N, vals.data());
        if (st) return st;
        for (int i = 0; i < N; ++i) u += vals[i];
    }
    const int P = (int)(c->pairs.size() / 2), T = (int)(c->triplets.size() / 3);
    if (P > 0) {
        std::vector<int32_t> id(P), la(P), lb(P);
        std::vector<double> vals(P);
        for (int p = 0; p < P; ++p) {
            id[p] = p;
            la[p] = labeling[c->pairs[2 * p]];
            lb[p] = labeling[c->pairs[2 * p + 1]];
        }
        int st = msm_cost_pairwise_batch(c, id.data(), la.data(), lb.data(), P, vals.data());
        if (st) return st;
        for (int p = 0; p < P; ++p) pw += vals[p];
    }
    bool triplets_done = false;
    if (T > 0 && cost_is_ho(c)) {
        std::vector<double> vals(T);
        int st = fused_single_costs(c, labeling, vals.data(), &triplets_done);  // the fused move with one combination per control triangle, where it applies
        if (st) return st;
        if (triplets_done)
            for (int t = 0; t < T; ++t) tc += vals[t];  // serial, in triplet order (:70-75)
    }
    if (T > 0 && !triplets_done) {
        std::vector<int32_t> id(T), la(T), lb(T), lc(T);
        std::vector<double> vals(T);
        for (int t = 0; t < T; ++t) {
            id[t] = t;
            la[t] = labeling[c->triplets[3 * t]];
            lb[t] = labeling[c->triplets[3 * t + 1]];
            lc[t] = labeling[c->triplets[3 * t + 2]];
        }
        int st = msm_cost_triplet_batch(c, id.data(), la.data(), lb.data(), lc.data(), T, vals.data());
        if (st) return st;
        for (int t = 0; t < T; ++t) tc += vals[t];
    }
    if (parts) {
        parts[0] = u;
        parts[1] = pw;
        parts[2] = tc;
    }
    *total = u + pw + tc;
    return MSM_OK;
}

}  // extern "C"
