// group.cpp -- C ABI of the groupwise (gMSM) path (include/msmhip.h, "groupwise registration").
//
// DiscreteGroupModel::setupCostFunction (M/DiscreteGroupModel.cpp:163-196) is per-iteration set-up: closest
// control points between subjects, and for every (subject, label) a rigid rotation of the data mesh followed by
// an adaptive-barycentric resample of its features to the template.  All of it runs on the GPU (trees as a forest,
// queries, weight-list surgery, weighted sums, patch lists: DESIGN.md section 5.6); the resampled feature maps
// F[subject][label] (D x V_template) and the patch lists stay in HBM, where the pairwise kernel reads them
// (group_kernels.hip).  Here: the handle and its setters, msm_group_finalize, the queries and the batch evaluators; the set-up is in group_setup.cpp,
// the exchange of subjects between groups in group_exchange.cpp, the label step in group_move.cpp.
#include "group_internal.hpp"

namespace msm {

// F[s][0..L) as windows of `per` doubles each into the subject's slab
int subject_feature_slab(msm_group *g, int s, size_t per) {
    auto &slab = g->Fslab[s];
    if (!slab) slab.reset(new DevBuf<double>());
    const double *before = slab->p;
    MSM_HIP(slab->ensure(per * g->L));
    for (int l = 0; l < g->L; ++l) {
        auto &buf = g->F[(size_t)s * g->L + l];
        if (!buf) buf.reset(new DevBuf<double>());
        if (buf->p != slab->p + per * l || slab->p != before || buf->cap != per) buf->view(slab->p + per * l, per);
    }
    return MSM_OK;
}

int group_args(msm_group *g, GroupArgs &a) {
    if (!g->ready) return fail(MSM_ERR_STATE, "msm_group: msm_group_setup() must be called first");
    a.S = g->S;
    a.N = g->N;
    a.L = g->L;
    a.D = g->D;
    a.Tc = g->Tc;
    a.Vt = g->tmpl->V;
    a.simmeasure = g->p.simmeasure;
    a.fixnan = g->p.fixnan;
    a.pairs = g->d_pairs.p;
    a.triplets = g->d_triplets.p;
    a.pptr = g->d_pptrp.p;
    a.pidx = g->d_pidxp.p;
    a.F = g->d_Fp.p;
    const bool pval_all = g->pval_serves_all();  // (a slice's copies serve that slice's label steps only: group_move_compute)
    a.pval = pval_all ? const_cast<const double *const *>(g->d_pvalp.p) : nullptr;
    a.dir = pval_all ? g->d_patch_dir.p : nullptr;
    a.mask = g->mask.empty() ? nullptr : g->d_mask.p;
    a.moved = g->d_moved.p;
    a.cp = g->d_cp.p;
    a.orig = g->d_orig.p;
    a.lambda = g->p.lambda;
    a.mu = g->p.mu;
    a.kappa = g->p.kappa;
    a.k_exp = g->p.k_exp;
    a.rexp = g->p.rexp;
    a.subcorr = 0.1 * g->S;  // set_meshes, M/DiscreteGroupCostFunction.h:45
    a.percentile = g->p.percentile;
    a.move_labeling = nullptr;
    a.move_label = a.move_offset = 0;
    a.move_order = nullptr;
    a.move_order4 = nullptr;
    a.move_first = a.move_count = 0;
    a.move_base = 0;
    a.move_combos = 0;
    a.move_prev = nullptr;
    a.move_e00 = nullptr;
    a.move_e11 = nullptr;
    a.patch_cap = g->patch_max;
    a.pair_lanes = g->pair_lanes;
    a.status = g->ctx->d_status;
    return MSM_OK;
}

// a DICE group whose largest patch does not fit the pair kernel's LDS: said before a pair evaluation queues anything (launch_group_pairwise would say it too)
int pair_refusal(const msm_group *g) {
    if ((g->p.simmeasure == 4 || g->p.simmeasure == 5) && group_dice_lds(g->patch_max, nullptr, nullptr) == 2)
        return fail(MSM_ERR_CAPACITY, "group patch of %d entries does not fit in LDS", g->patch_max);
    return MSM_OK;
}

// the host copy of a subject's row offsets, fetched when first asked for (the lists live on the device, whoever brought them)
int fetch_host_pptr(msm_group *g, int s) {
    if (!g->h_pptr[s].empty()) return MSM_OK;
    if (!g->have_subject[s]) return fail(MSM_ERR_STATE, "msm_group: subject %d is neither set up nor imported", s);
    g->h_pptr[s].resize((size_t)g->N * g->L + 1);
    MSM_TRY(g->pptr[s]->download(g->h_pptr[s].data(), g->h_pptr[s].size(), g->ctx));
    MSM_TRY(ctx_sync(g->ctx));
    return MSM_OK;
}

// ... and of its index list
int fetch_host_pidx(msm_group *g, int s) {
    if (!g->h_pidx[s].empty() || g->patch_stat[s].npidx <= 0) return MSM_OK;
    g->h_pidx[s].resize((size_t)g->patch_stat[s].npidx);
    MSM_TRY(g->pidx[s]->download(g->h_pidx[s].data(), g->h_pidx[s].size(), g->ctx));
    MSM_TRY(ctx_sync(g->ctx));
    return MSM_OK;
}

}  // namespace msm

namespace {

// A batch of n evaluations in chunks of bounded pinned staging, whatever the batch: the chunk's index columns go through the context's pinned
// block into buffers kept on the handle (no allocation and no pageable copy per call), launch(m) evaluates them from g->d_query into
// g->d_answer, and the answers come back through the same block.
int run_batch(msm_group *g, const int32_t *const *cols, int ncols, int n, double *out, const char *what, const std::function<int(int)> &launch) {
    msm_ctx *ctx = g->ctx;
    for (int off = 0; off < n; off += kBatchChunk) {
        const int m = std::min(kBatchChunk, n - off);
        const size_t bi = (sizeof(int32_t) * (size_t)m + 255) & ~(size_t)255, bo = sizeof(double) * (size_t)m;
        void *pin = nullptr;
        int st = ctx_io_pinned(ctx, bi * ncols + bo, &pin);
        if (st) return st;
        for (int k = 0; k < ncols; ++k) {
            MSM_HIP(g->d_query[k].ensure(m));
            std::memcpy((char *)pin + bi * k, cols[k] + off, sizeof(int32_t) * (size_t)m);
            MSM_HIP(hipMemcpyAsync(g->d_query[k].p, (char *)pin + bi * k, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        }
        MSM_HIP(g->d_answer.ensure(m));
        double *pinned_out = reinterpret_cast<double *>((char *)pin + bi * ncols);
        st = launch(m);
        if (st) return st;
        MSM_HIP(hipMemcpyAsync(pinned_out, g->d_answer.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        st = check_status(ctx, what);
        std::memcpy(out + off, pinned_out, sizeof(double) * (size_t)m);
        if (st) return st;
    }
    return MSM_OK;
}

}  // namespace

extern "C" {

msm_group *msm_group_create(msm_ctx *ctx, const msm_group_params *params, int32_t S) {
    if (!ctx || !params || S < 1) {
        fail(MSM_ERR_INVALID, "msm_group_create: bad arguments");
        return nullptr;
    }
    if (params->simmeasure != 1 && params->simmeasure != 2 && params->simmeasure != 4 && params->simmeasure != 5) {
        fail(MSM_ERR_INVALID, "Unknown similarity metric");  // get_sim_for_min, M/similarities.h:57
        return nullptr;
    }
    const double percentile = params->percentile == 0.0 ? 0.75 : params->percentile;  // sparsesimkernel's default, M/similarities.h:68
    if ((params->simmeasure == 4 || params->simmeasure == 5) && !(percentile > 0.0 + 1e-8 && percentile < 1.0 - 1e-8)) {
        fail(MSM_ERR_INVALID, "Percentile must be between 0 and 1.");  // M/mesh_registration.cpp:782-783
        return nullptr;
    }
    msm_group *g = new msm_group();
    g->ctx = ctx;
    g->p = *params;
    g->p.percentile = percentile;
    g->S = S;
    g->cpmesh.assign(S, nullptr);
    g->data.assign(S, nullptr);
    g->feat.resize(S);
    g->orig.resize(S);
    g->have_orig.assign(S, 0);
    g->spacing.resize(S);
    g->h_pptr.resize(S);
    g->h_pidx.resize(S);
    g->patch_stat.resize(S);
    for (int s = 0; s < S; ++s) {
        g->pptr.emplace_back(new DevBuf<int32_t>());
        g->pidx.emplace_back(new DevBuf<int32_t>());
    }
    return g;
}

void msm_group_destroy(msm_group *g) {
    if (!g) return;
    (void)hipStreamSynchronize(g->ctx->stream);
    for (msm_mesh *m : g->cpmesh) msm_mesh_destroy(m);
    for (auto &pp : g->pipe) {
        if (pp.batch.ctx) {
            (void)hipStreamSynchronize(pp.batch.ctx->stream);
            msm_mesh_destroy(pp.fallback);
            msm_ctx_destroy(pp.batch.ctx);
            pp.batch.ctx = nullptr;
        }
        if (pp.own_main && pp.main) {
            (void)hipStreamSynchronize(pp.main->stream);
            msm_ctx_destroy(pp.main);
        }
        pp.main = nullptr;
    }
    if (g->copy_stream) {
        (void)hipStreamSynchronize(g->copy_stream);
        (void)hipStreamDestroy(g->copy_stream);
    }
    for (hipEvent_t e : g->copy_events) (void)hipEventDestroy(e);
    if (g->t_ev0) (void)hipEventDestroy(g->t_ev0);
    if (g->t_ev1) (void)hipEventDestroy(g->t_ev1);
    for (hipEvent_t e : g->mc_ev)
        if (e) (void)hipEventDestroy(e);
    delete g;
}

int msm_group_set_template(msm_group *g, msm_mesh *t, const double *mask) {
    if (!g || !t) return fail(MSM_ERR_INVALID, "msm_group_set_template: null argument");
    g->tmpl = t;
    g->mask.clear();
    if (mask) {
        g->mask.assign(mask, mask + t->V);
        MSM_TRY(g->d_mask.upload(g->mask.data(), g->mask.size(), g->ctx));
        MSM_TRY(ctx_sync(g->ctx));
    }
    g->ready = false;
    g->common_ready = false;
    g->drop_kept();
    return MSM_OK;
}

int msm_group_set_controlgrid(msm_group *g, const double *xyz, const int32_t *tri, int32_t N, int32_t Tc) {
    if (!g || !xyz || !tri || N <= 0 || Tc <= 0) return fail(MSM_ERR_INVALID, "msm_group_set_controlgrid: bad arguments");
    g->N = N;
    g->Tc = Tc;
    g->cp_tri.assign(tri, tri + 3 * (size_t)Tc);
    for (int s = 0; s < g->S; ++s) {
        msm_mesh_destroy(g->cpmesh[s]);
        g->cpmesh[s] = msm_mesh_create(g->ctx, xyz, N, tri, Tc);
        if (!g->cpmesh[s]) return MSM_ERR_HIP;
    }
    // estimate_triplets, M/DiscreteGroupModel.cpp:57-75
    g->triplets.resize(3 * (size_t)g->S * Tc);
    for (int s = 0; s < g->S; ++s)
        for (int t = 0; t < Tc; ++t) {
            int32_t v[3] = {tri[t] + s * N, tri[Tc + t] + s * N, tri[2 * Tc + t] + s * N};
            std::sort(v, v + 3);
            std::copy(v, v + 3, &g->triplets[3 * ((size_t)s * Tc + t)]);
        }
    MSM_TRY(g->d_triplets.upload(g->triplets.data(), g->triplets.size(), g->ctx));
    MSM_TRY(ctx_sync(g->ctx));
    g->ready = false;
    g->common_ready = false;
    g->drop_kept();
    return MSM_OK;
}

int msm_group_set_subject(msm_group *g, int32_t s, msm_mesh *data, const double *feat, int32_t D) {
    if (!g || !data || !feat || s < 0 || s >= g->S || D <= 0) return fail(MSM_ERR_INVALID, "msm_group_set_subject: bad arguments");
    if (g->N <= 0) return fail(MSM_ERR_STATE, "msm_group: the control grid must be set first");
    if (data->V < g->N) return fail(MSM_ERR_INVALID, "data mesh has fewer vertices than the control grid");
    for (int o = 0; o < g->S; ++o)
        if (o != s && g->data[o] && g->D != D) return fail(MSM_ERR_INVALID, "all subjects must have the same number of feature dimensions");
    g->D = D;
    g->data[s] = data;
    g->feat[s].assign(feat, feat + (size_t)D * data->V);
    if (!g->have_orig[s]) {
        g->orig[s].resize(3 * (size_t)g->N);
        for (int v = 0; v < g->N; ++v) {
            g->orig[s][v] = data->xyz[v];
            g->orig[s][g->N + v] = data->xyz[data->V + v];
            g->orig[s][2 * (size_t)g->N + v] = data->xyz[2 * (size_t)data->V + v];
        }
        g->have_orig[s] = 1;
    }
    g->ready = false;
    g->common_ready = false;
    g->drop_kept();
    return MSM_OK;
}

int msm_group_reset_cpgrid(msm_group *g, int32_t s, const double *xyz) {
    if (!g || !xyz || s < 0 || s >= g->S || !g->cpmesh[s]) return fail(MSM_ERR_INVALID, "msm_group_reset_cpgrid: bad arguments");
    g->ready = false;
    g->common_ready = false;
    g->drop_kept();
    return msm_mesh_update_coords(g->cpmesh[s], xyz);
}

int msm_group_set_labels(msm_group *g, const double *labels, int32_t L) {
    if (!g || !labels || L <= 0) return fail(MSM_ERR_INVALID, "msm_group_set_labels: bad arguments");
    g->L = L;
    g->labels.assign(labels, labels + 3 * (size_t)L);
    g->ready = false;
    g->common_ready = false;
    g->drop_kept();
    return MSM_OK;
}

// The order of the pair list (what msm_group_get_pairs returns and every pair index of this interface refers to).  0 (default): the reference's,
// estimate_pairs' loops -- subject A, control point, subject B (M/DiscreteGroupModel.cpp:37-55).  1: control point by control point along a space-
// filling curve, all subject pairs of one control point together: a contiguous slice of THAT list is a region of the sphere, so a rank evaluating
// an eighth of it touches an eighth of every resampled map instead of all of eight subjects' and most of everyone else's (an eighth of a label
// step at S = 64, ico6 / ico4: 1.59 -> 1.42 ms of kernels).  The optimiser takes the list as it comes (I/Fusion/Fusion.h:157-196 reads pairs[i]
// beside the i-th costs); the same set of pairs either way.  Takes effect at the next msm_group_setup / msm_group_setup_subjects.
msm_ctx *msm_group_context(msm_group *g) { return g ? g->ctx : nullptr; }

int msm_group_set_pair_layout(msm_group *g, int32_t layout) {
    if (!g || (layout != 0 && layout != 1)) return fail(MSM_ERR_INVALID, "msm_group_set_pair_layout: layout must be 0 (reference order) or 1 (control-point major)");
    if (g->pair_layout == layout) return MSM_OK;
    g->pair_layout = layout;
    g->pair_order.clear();  // rebuilt (and with it the slices and pieces) by the next set-up
    g->order_S = g->order_N = 0;
    g->order_p0 = g->order_p1 = -1;
    g->pairs.clear();
    g->ready = false;
    g->common_ready = false;
    g->drop_kept();
    return MSM_OK;
}

// Who computes estimate_rotation_matrix(centre, vertex) (R/point.cpp:97-152) for the vertices of the data meshes in get_patch_data (M/DiscreteGroupModel.cpp:
// 97-105).  1 (default): the host's libm -- acos / sincos as the reference calls them -- with the matrices applied on the device in the reference's operation
// order: the rotated meshes are then the reference's to the bit.  That matters when a label carries data vertices EXACTLY onto template vertices (a regular
// icosphere as the template under regular data grids, as gMSM's own scripts set a run up): which triangle around such a vertex "contains" it is decided by the
// last bits of the rotation.  V x 0.15 us of host time per subject and set-up, on the host workers beside the GPU's work on other subjects
// (S = 64 at ico6: 145 against 144 ms per set-up).  0: the device computes them (its own acos / sincos).  Takes effect at the next set-up.
int msm_group_set_rotation_mode(msm_group *g, int32_t mode) {
    if (!g || (mode != 0 && mode != 1)) return fail(MSM_ERR_INVALID, "msm_group_set_rotation_mode: mode must be 0 (device) or 1 (the host's libm)");
    if (g->rotation_mode != mode) {
        g->rotation_mode = mode;
        g->ready = false;
        g->drop_kept();
    }
    return MSM_OK;
}

int msm_group_finalize(msm_group *g) {
    if (!g) return fail(MSM_ERR_INVALID, "null group");
    if (!g->common_ready) return fail(MSM_ERR_STATE, "msm_group: nothing has been set up");
    for (int s = 0; s < g->S; ++s)
        if (!g->have_subject[s]) return fail(MSM_ERR_STATE, "msm_group: subject %d is neither set up nor imported", s);
    msm_ctx *ctx = g->ctx;
    const int S = g->S, L = g->L;
    std::vector<const double *> Fp((size_t)S * L);
    for (size_t k = 0; k < Fp.size(); ++k) Fp[k] = g->F[k]->p;
    std::vector<const int *> pp(S), pi(S);
    for (int s = 0; s < S; ++s) {
        pp[s] = g->pptr[s]->p;
        pi[s] = g->pidx[s]->p;
    }
    MSM_TRY(g->d_Fp.upload(Fp.data(), Fp.size(), ctx));
    MSM_TRY(g->d_pptrp.upload(pp.data(), pp.size(), ctx));
    MSM_TRY(g->d_pidxp.upload(pi.data(), pi.size(), ctx));
    MSM_TRY(ctx_sync(ctx));
    g->drop_kept();  // new patches: nothing kept from earlier label steps applies
    g->patch_max = 0;
    int64_t npatch = 0, nsmall = 0;
    for (int s = 0; s < S; ++s) {  // whoever gave the subject its lists counted
        g->patch_max = std::max(g->patch_max, g->patch_stat[s].largest);
        npatch += (int64_t)g->N * L;
        nsmall += g->patch_stat[s].small;
    }
    // a quarter wavefront per pair cost when (nearly) all patches fit its registers: four queries share a wavefront's instruction stream and latency
    // instead of two (label step 12.5 -> 9.5 ms at ico6 / ico4, patches of ~65 entries); the others take the general path, at half the lanes
    g->pair_lanes = (npatch > 0 && 10 * nsmall >= 9 * npatch) ? 16 : 32;
    g->npatch = npatch, g->nsmall = nsmall;
    if (const char *e = std::getenv("MSMHIP_GROUP_PAIR_LANES")) g->pair_lanes = std::atoi(e) == 16 ? 16 : 32;
    // The patch entries' values beside their ids (GroupArgs::pval), for the register path of k_group_pairwise (D <= 2): one launch over all subjects, whether
    // they were set up here or imported -- 3.2 GB written at S = 64, ico6 / ico4 (0.5 ms), and the label steps' value gathers by vertex id become a coalesced
    // read of patch A and reads of one 1 KB window of patch B.
    g->pval_ready = g->pval_deferred = false;
    g->pval_p0 = g->pval_p1 = -1;
    if (g->D <= 2) {
        g->pval.resize(S);
        std::vector<double *> pv(S);
        bool imported = false;
        for (int s = 0; s < S; ++s) {
            if (!g->pval[s]) g->pval[s].reset(new DevBuf<double>());
            MSM_HIP(ensure_patch_entries(*g->pval[s], (size_t)g->patch_stat[s].npidx, (size_t)g->D));
            pv[s] = g->pval[s]->p;
            imported = imported || g->have_subject[s] == 2;
        }
        MSM_TRY(g->d_pvalp.upload(pv.data(), pv.size(), ctx));
        if (g->d_patch_dir.ensure((size_t)S * g->N * L) != hipSuccess) return fail(MSM_ERR_HIP, "device allocation of the patch directory failed");
        g->ready = true;  // (group_args checks it)
        if (imported) {
            g->pval_deferred = true;  // a rank of a sharded run: written for the nodes of its slice when the slice is first evaluated
            MSM_TRY(ctx_sync(ctx));
        } else {
            const int st = ensure_patch_values(g, 0, g->npairs);
            if (st) {
                g->ready = false;
                return st;
            }
        }
    }
    if (std::getenv("MSMHIP_TIMING"))
        fprintf(stderr, "  group patches: %lld, %.1f %% of them with at most %d entries, largest %d -> %d lanes per pair cost\n", (long long)npatch,
                npatch ? 100.0 * (double)nsmall / (double)npatch : 0.0, kPairSmallPatch, g->patch_max, g->pair_lanes);
    g->ready = true;
    return MSM_OK;
}

int msm_group_pair_route(int32_t cntA, int32_t cntB, int32_t D, int32_t simmeasure, int32_t lanes, int32_t route[4]) {
    if (!route || cntA < 0 || cntB < 0 || D < 1 || (lanes != 16 && lanes != 32 && lanes != 64) || (simmeasure != 1 && simmeasure != 2 && simmeasure != 4 && simmeasure != 5) ||
        ((simmeasure == 4 || simmeasure == 5) != (lanes == 64)))
        return fail(MSM_ERR_INVALID, "msm_group_pair_route: bad arguments");
    const GroupPairRoute r = group_pair_route(cntA, cntB, D, simmeasure, lanes);
    route[MSM_PAIR_ROUTE_FAST] = r.fast, route[MSM_PAIR_ROUTE_PADDED] = r.padded, route[MSM_PAIR_ROUTE_STAGED] = r.staged, route[MSM_PAIR_ROUTE_BEYOND] = r.beyond;
    return MSM_OK;
}

int msm_group_pair_launch(msm_group *g, int64_t out[8]) {
    if (!g || !out) return fail(MSM_ERR_INVALID, "msm_group_pair_launch: null argument");
    if (!g->ready) return fail(MSM_ERR_STATE, "msm_group: msm_group_finalize() must be called first");
    const bool dice = g->p.simmeasure == 4 || g->p.simmeasure == 5;
    size_t total = 0;
    const int fit = dice ? group_dice_lds(g->patch_max, &total, nullptr) : 0;
    const bool pval_all = g->pval_serves_all();  // what group_args hands the kernel
    out[MSM_PAIR_LAUNCH_LANES] = dice ? 64 : g->pair_lanes;
    out[MSM_PAIR_LAUNCH_PATCH_MAX] = g->patch_max;
    out[MSM_PAIR_LAUNCH_NPATCH] = g->npatch;
    out[MSM_PAIR_LAUNCH_NSMALL] = g->nsmall;
    out[MSM_PAIR_LAUNCH_DICE_LDS] = (int64_t)total;
    out[MSM_PAIR_LAUNCH_DICE_FIT] = fit;
    out[MSM_PAIR_LAUNCH_PVAL] = pval_all;
    out[MSM_PAIR_LAUNCH_DIR] = pval_all;
    return MSM_OK;
}

int msm_group_setup(msm_group *g) {
    if (!g) return fail(MSM_ERR_INVALID, "null group");
    std::vector<int32_t> all(g->S);
    for (int s = 0; s < g->S; ++s) all[s] = s;
    int st = msm_group_setup_subjects(g, all.data(), g->S);
    if (st) return st;
    return msm_group_finalize(g);
}

int msm_group_sizes(msm_group *g, int32_t *nodes, int32_t *pairs, int32_t *triplets) {
    if (!g) return fail(MSM_ERR_INVALID, "null group");
    if (nodes) *nodes = g->S * g->N;
    if (pairs) *pairs = g->N * g->S * (g->S - 1) / 2;
    if (triplets) *triplets = g->S * g->Tc;
    return MSM_OK;
}

int msm_group_dims(msm_group *g, int32_t *S, int32_t *N, int32_t *L, int32_t *D, int32_t *Vt) {
    if (!g) return fail(MSM_ERR_INVALID, "null group");
    if (S) *S = g->S;
    if (N) *N = g->N;
    if (L) *L = g->L;
    if (D) *D = g->D;
    if (Vt) *Vt = g->tmpl ? g->tmpl->V : 0;
    return MSM_OK;
}

int msm_group_get_pairs(msm_group *g, int32_t *pairs) {
    if (!g || !pairs) return fail(MSM_ERR_INVALID, "msm_group_get_pairs: null argument");
    if (!g->ready) return fail(MSM_ERR_STATE, "msm_group: msm_group_setup() must be called first");
    if (g->pairs.size() != 2 * (size_t)g->npairs) {  // the list was written on the device: fetched when first asked for
        g->pairs.resize(2 * (size_t)g->npairs);
        if (g->npairs > 0) MSM_TRY(g->d_pairs.download(g->pairs.data(), g->pairs.size(), g->ctx));
        MSM_TRY(ctx_sync(g->ctx));
    }
    std::copy(g->pairs.begin(), g->pairs.end(), pairs);
    return MSM_OK;
}

int msm_group_get_triplets(msm_group *g, int32_t *triplets) {
    if (!g || !triplets) return fail(MSM_ERR_INVALID, "msm_group_get_triplets: null argument");
    std::copy(g->triplets.begin(), g->triplets.end(), triplets);
    return MSM_OK;
}

int msm_group_patch(msm_group *g, int32_t s, int32_t v, int32_t l, int32_t *ids, double *data, int32_t cap, int32_t *n) {
    if (!g || !n) return fail(MSM_ERR_INVALID, "msm_group_patch: null argument");
    if (!g->ready) return fail(MSM_ERR_STATE, "msm_group: msm_group_setup() must be called first");
    if (s < 0 || s >= g->S || v < 0 || v >= g->N || l < 0 || l >= g->L) return fail(MSM_ERR_INVALID, "msm_group_patch: index out of range");
    {
        int st = fetch_host_pptr(g, s);
        if (st) return st;
    }
    const int beg = g->h_pptr[s][v * g->L + l], cnt = g->h_pptr[s][v * g->L + l + 1] - beg;
    *n = cnt;
    MSM_TRY(fetch_host_pidx(g, s));
    if (!ids && !data) return MSM_OK;
    const int Vt = g->tmpl->V;
    std::vector<double> F;
    if (data) {
        F.resize((size_t)g->D * Vt);
        MSM_TRY(g->F[(size_t)s * g->L + l]->download(F.data(), F.size(), g->ctx));
        MSM_TRY(ctx_sync(g->ctx));
    }
    for (int i = 0; i < cnt && i < cap; ++i) {
        const int id = g->h_pidx[s][beg + i];
        if (ids) ids[i] = id;
        if (data)
            for (int d = 0; d < g->D; ++d) data[(size_t)i * g->D + d] = F[(size_t)d * Vt + id];
    }
    return MSM_OK;
}

int msm_group_pairwise_batch(msm_group *g, const int32_t *pair, const int32_t *la, const int32_t *lb, int32_t n, double *out) {
    if (!g || !pair || !la || !lb || !out || n < 0) return fail(MSM_ERR_INVALID, "msm_group_pairwise_batch: bad arguments");
    if (n == 0) return MSM_OK;
    GroupArgs a;
    int st = group_args(g, a);
    if (!st) st = pair_refusal(g);
    if (st) return st;
    const int P = (int)g->npairs;
    for (int i = 0; i < n; ++i)
        if (pair[i] < 0 || pair[i] >= P || la[i] < 0 || la[i] >= g->L || lb[i] < 0 || lb[i] >= g->L) return fail(MSM_ERR_INVALID, "group pairwise query %d out of range", i);
    const int32_t *cols[3] = {pair, la, lb};
    return run_batch(g, cols, 3, n, out, "DiscreteGroupCostFunction::computePairwiseCost",
                     [&](int m) { return launch_group_pairwise(g->ctx, a, g->d_query[0].p, g->d_query[1].p, g->d_query[2].p, m, g->d_answer.p); });
}

int msm_group_triplet_batch(msm_group *g, const int32_t *t, const int32_t *la, const int32_t *lb, const int32_t *lc, int32_t n, double *out) {
    if (!g || !t || !la || !lb || !lc || !out || n < 0) return fail(MSM_ERR_INVALID, "msm_group_triplet_batch: bad arguments");
    if (n == 0) return MSM_OK;
    GroupArgs a;
    int st = group_args(g, a);
    if (st) return st;
    const int T = g->S * g->Tc;
    for (int i = 0; i < n; ++i)
        if (t[i] < 0 || t[i] >= T || la[i] < 0 || la[i] >= g->L || lb[i] < 0 || lb[i] >= g->L || lc[i] < 0 || lc[i] >= g->L)
            return fail(MSM_ERR_INVALID, "group triplet query %d out of range", i);
    const int32_t *cols[4] = {t, la, lb, lc};
    return run_batch(g, cols, 4, n, out, "DiscreteGroupCostFunction::computeTripletCost",
                     [&](int m) { return launch_group_triplet(g->ctx, a, g->d_query[0].p, g->d_query[1].p, g->d_query[2].p, g->d_query[3].p, m, g->d_answer.p); });
}

}  // extern "C"
