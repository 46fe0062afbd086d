// dedrift.cpp -- the post-processing of a finished groupwise run behind the C ABI (msm_dedrift_*): what the reference's tutorial pipeline does with
// wb_command and nibabel after gMSM (gMSM_scripts/gMSM_tutorial/gw_MSM.sh:65-128, compare_stats.py).  Validation, the order of the launches and the
// copies are here; the searches are the library's own (kernels.hip, resample_kernels.hip), everything else per vertex, per map and per pair is in
// dedrift_kernels.hip.  Between "the subject's arrays are on the device" and "the results leave for the host" nothing crosses the link: the running
// sum, the warp, every subject's resampled maps and the masks stay in HBM.
#include <cmath>
#include <vector>

#include "dedrift.hpp"
#include "kernels.hpp"
#include "resample.hpp"

using namespace msm;

struct msm_dedrift {
    msm_ctx *ctx = nullptr;
    msm_mesh *tmpl = nullptr;
    int S = 0, Vt = 0, D = 0;
    int accumulated = 0;
    bool finished = false;
    bool warp_set = false;  // the warp came from msm_dedrift_set_warp
    std::vector<char> have;  // per subject: its maps are resident
    DevBuf<double> sum, drift, warp;       // 3 x Vt each
    DevBuf<double> m_xyz, inverse, w;      // the subject in hand: its input sphere (3 x Vs), its inverse (3 x Vt), search weights (3 x max(Vt, Vs))
    DevBuf<int32_t> tri, vid, open;        // search results and the direction table's open list
    DevBuf<double> data, dist;             // the subject's data (D x Vs) and distortion maps (2 x Vs)
    DevBuf<double> maps;                   // S x D x Vt: every subject's resampled data
    DevBuf<double> mean, sd, stats, thr, cc, dice;
    DevBuf<unsigned long long> bits;
    DevBuf<int32_t> count;
    DevBuf<int32_t> list, kept;            // group statistics: the listed subjects, the kept vertices (ascending)
    DevBuf<double> pair_mean;              // 2 x D: cc, then dice
};

namespace {

int check_subject_mesh(const msm_dedrift *d, const msm_mesh *reg, int32_t V, const char *what) {
    if (reg->ctx != d->ctx) return fail(MSM_ERR_INVALID, "%s: the registered sphere belongs to another context", what);
    if (reg == d->tmpl) return fail(MSM_ERR_INVALID, "%s: the registered sphere is the template's own handle", what);
    if (V != reg->V) return fail(MSM_ERR_INVALID, "%s: the input sphere has %d vertices, the registered sphere %d", what, V, reg->V);
    return MSM_OK;
}

int accumulate(msm_dedrift *d, msm_mesh *reg, const double *orig_xyz, int32_t *tri_id, double *w, double *inverse) {
    msm_ctx *ctx = d->ctx;
    const int Vt = d->Vt, Vs = reg->V;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MSM_TRY(ensure_tree(reg));
    MSM_TRY(d->m_xyz.upload(orig_xyz, 3 * (size_t)Vs, ctx));
    if (d->tri.ensure(std::max(Vt, Vs)) || d->vid.ensure(3 * (size_t)Vt) || d->w.ensure(3 * (size_t)std::max(Vt, Vs)) || d->open.ensure((size_t)Vt + 1) ||
        (inverse && d->inverse.ensure(3 * (size_t)Vt)))
        return stage_alloc_failed(sizeof(double) * 9 * (size_t)std::max(Vt, Vs));
    // the template's vertices in the registered sphere: its direction table where it has one, the complete search otherwise (same triangles, same weights)
    MSM_TRY(launch_query_rays(ctx, dev_tree(reg), d->tmpl->d_xyz.p, Vt, d->tri.p, d->vid.p, d->w.p, MSM_WEIGHTS_PROJECTED, reg->rays_valid ? d->open.p : nullptr));
    MSM_TRY(launch_dedrift_accumulate(ctx, d->vid.p, d->w.p, Vt, d->m_xyz.p, Vs, d->sum.p, inverse ? d->inverse.p : nullptr));
    ++d->accumulated;
    if (!tri_id && !w && !inverse) return MSM_OK;  // nothing to fetch: the launch is queued, msm_dedrift_finish looks at the status word
    if (tri_id) MSM_TRY(d->tri.download(tri_id, Vt, ctx));
    if (w) MSM_TRY(d->w.download(w, 3 * (size_t)Vt, ctx));
    if (inverse) MSM_TRY(d->inverse.download(inverse, 3 * (size_t)Vt, ctx));
    return check_status(ctx, "msm_dedrift_accumulate");
}

int correct(msm_dedrift *d, int subject, msm_mesh *reg, const double *orig_xyz, const double *data, int D, double *corrected, double *resampled,
            double *distortion, int32_t *tri_id, double *w) {
    msm_ctx *ctx = d->ctx;
    msm_mesh *tmpl = d->tmpl;
    const int Vt = d->Vt, Vs = reg->V;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MSM_TRY(ensure_tree(tmpl));
    MSM_TRY(ensure_adjacency_dev(reg));
    const size_t nmap = (size_t)D * Vt;
    if (d->maps.ensure((size_t)d->S * nmap, true) || d->data.ensure((size_t)D * Vs) || d->dist.ensure(2 * (size_t)Vs) ||
        d->tri.ensure(std::max(Vt, Vs)) || d->w.ensure(3 * (size_t)std::max(Vt, Vs)))
        return stage_alloc_failed(sizeof(double) * d->S * nmap);
    ++ctx->epoch;  // the mesh's coordinates change
    if (tri_id || w) {  // the second search's decisions, for a caller that wants to compare them (the warp kernel below searches again, identically)
        MSM_TRY(launch_query(ctx, dev_tree(tmpl), reg->d_xyz.p, Vs, d->tri.p, nullptr, d->w.p, MSM_WEIGHTS_PROJECTED));
        if (tri_id) MSM_TRY(d->tri.download(tri_id, Vs, ctx));
        if (w) MSM_TRY(d->w.download(w, 3 * (size_t)Vs, ctx));
    }
    // sphere_project_warp(R_s, T, W) in place on the device (R/resampler.cpp:311-328); the host copy of the handle follows
    MSM_TRY(launch_warp(ctx, dev_tree(tmpl), reg->d_xyz.p, Vs, d->warp.p, Vt, true, reg->d_xyz.p));
    reg->tree_valid = false;
    MSM_TRY(reg->d_xyz.download(reg->xyz.data(), 3 * (size_t)Vs, ctx));
    const int st = check_status(ctx, "msm_dedrift_correct (warp)");  // on a failed search the unmoved points stay
    reg->host_xyz_stale = false;
    if (st) return st;
    if (corrected) std::copy(reg->xyz.begin(), reg->xyz.end(), corrected);
    // metric_resample(corrected_s -> T), adaptive barycentric: searches, list surgery and the weighted sums on the device, into the subject's resident slot
    AdaptiveDev aw;
    MSM_TRY(adaptive_weights_dev(reg, tmpl, aw));
    MSM_TRY(upload_staged(ctx, d->data.p, data, sizeof(double) * (size_t)D * Vs));
    double *slot = d->maps.p + (size_t)subject * nmap;
    MSM_TRY(apply_weights_dev(ctx, aw, d->data.p, D, slot));
    // distortion of corrected_s against the input sphere
    MSM_TRY(d->m_xyz.upload(orig_xyz, 3 * (size_t)Vs, ctx));
    MSM_TRY(launch_vertex_distortion(ctx, d->m_xyz.p, reg->d_xyz.p, Vs, reg->d_tri.p, reg->T, reg->d_tid_ptr.p, reg->d_tid.p, d->dist.p));
    if (resampled) MSM_TRY(stage_d2h(ctx, resampled, slot, sizeof(double) * nmap));
    if (distortion) MSM_TRY(d->dist.download(distortion, 2 * (size_t)Vs, ctx));
    MSM_TRY(check_status(ctx, "msm_dedrift_correct"));
    d->have[subject] = 1;
    return MSM_OK;
}

// The whole set without a mask goes through the per-pair kernels up to this many subjects, through the tile kernels above it (the same bits either way).
// Measured on an MI355X at ico6, D = 2, medians of 30 (profiles/hierarchy_time_parent.json): the whole call with the per-pair kernels
// against the tile kernels 0.36 / 0.48 ms at S = 2, 0.39 / 0.53 at 8 and 9, 0.39 / 0.55 at 16, 0.68 / 0.74 at 64 and 3.76 / 2.03 at 256, the same call
// twice differing by 1 %: one to three tiles per feature are a latency chain on one to three CUs.  64 is the largest measured size at which the tiles lose.
constexpr int kPerPairMax = 64;

// the group statistics over n listed subjects (subjects == nullptr: the subjects 0 .. n - 1, no list is uploaded) and the kept vertices (!masked: all of
// them).  Matrices and per-map arrays are indexed by list position.  `what` names the entry point for check_status.
int group_stats(msm_dedrift *d, const char *what, const int32_t *subjects, int n, const std::vector<int32_t> &kept, bool masked, double percentile,
                double *mean, double *stdev, double *cc, double *dice, double *cc_mean, double *dice_mean) {
    msm_ctx *ctx = d->ctx;
    const int D = d->D, Vt = d->Vt, nmaps = n * D, K = masked ? (int)kept.size() : Vt, words = (K + 63) / 64;
    const size_t nmap = (size_t)D * Vt, nmat = (size_t)D * n * n;
    const bool want_cc = cc || cc_mean, want_dice = dice || dice_mean;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    if (d->mean.ensure(nmap) || d->sd.ensure(nmap) || d->stats.ensure(2 * (size_t)nmaps) || d->thr.ensure(nmaps) || d->cc.ensure(nmat) ||
        d->dice.ensure(nmat) || d->bits.ensure((size_t)nmaps * words) || d->count.ensure(nmaps) || d->pair_mean.ensure(2 * (size_t)D))
        return stage_alloc_failed(sizeof(double) * (2 * nmap + 2 * nmat));
    if (subjects) MSM_TRY(d->list.upload(subjects, n, ctx));
    if (masked) MSM_TRY(d->kept.upload_vec(kept, ctx));
    const int32_t *d_list = subjects ? d->list.p : nullptr, *d_kept = masked ? d->kept.p : nullptr;
    if (mean || stdev) MSM_TRY(launch_dedrift_moments(ctx, d->maps.p, d_list, n, nmap, d->mean.p, d->sd.p));
    const bool per_pair = !subjects && !masked && n <= kPerPairMax;
    if (want_cc) {
        MSM_TRY(launch_dedrift_map_stats(ctx, d->maps.p, d_list, n, D, Vt, d_kept, K, d->stats.p));
        if (per_pair)
            MSM_TRY(launch_dedrift_pair_cc(ctx, d->maps.p, n, D, Vt, d->stats.p, d->cc.p));
        else
            MSM_TRY(launch_dedrift_tile_cc(ctx, d->maps.p, d_list, n, D, Vt, d_kept, K, d->stats.p, d->cc.p));
        if (cc_mean) MSM_TRY(launch_dedrift_pair_mean(ctx, d->cc.p, D, n, d->pair_mean.p));
    }
    if (want_dice) {
        const double vidx = (K - 1) * (percentile / 100.0);  // numpy.percentile over the K kept values
        const double fl = std::floor(vidx);
        MSM_TRY(launch_dedrift_masks(ctx, d->maps.p, d_list, n, D, Vt, d_kept, K, (int)fl, vidx - fl, d->thr.p, d->bits.p, words, d->count.p));
        if (per_pair)
            MSM_TRY(launch_dedrift_pair_dice(ctx, d->bits.p, d->count.p, n, D, words, d->dice.p));
        else
            MSM_TRY(launch_dedrift_tile_dice(ctx, d->bits.p, d->count.p, n, D, words, d->dice.p));
        if (dice_mean) MSM_TRY(launch_dedrift_pair_mean(ctx, d->dice.p, D, n, d->pair_mean.p + D));
    }
    if (mean) MSM_TRY(d->mean.download(mean, nmap, ctx));
    if (stdev) MSM_TRY(d->sd.download(stdev, nmap, ctx));
    if (cc) MSM_TRY(d->cc.download(cc, nmat, ctx));
    if (dice) MSM_TRY(d->dice.download(dice, nmat, ctx));
    if (cc_mean) MSM_TRY(stage_d2h(ctx, cc_mean, d->pair_mean.p, sizeof(double) * D));
    if (dice_mean) MSM_TRY(stage_d2h(ctx, dice_mean, d->pair_mean.p + D, sizeof(double) * D));
    return check_status(ctx, what);
}

}  // namespace

extern "C" {

msm_dedrift *msm_dedrift_create(msm_ctx *ctx, msm_mesh *template_mesh, int32_t num_subjects) {
    if (!ctx || !template_mesh || num_subjects < 1) {
        fail(MSM_ERR_INVALID, "msm_dedrift_create: bad arguments");
        return nullptr;
    }
    if (template_mesh->ctx != ctx) {
        fail(MSM_ERR_INVALID, "msm_dedrift_create: the template belongs to another context");
        return nullptr;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) {
        fail(MSM_ERR_HIP, "msm_dedrift_create: hipSetDevice failed");
        return nullptr;
    }
    msm_dedrift *d = new msm_dedrift();
    d->ctx = ctx;
    d->tmpl = template_mesh;
    d->S = num_subjects;
    d->Vt = template_mesh->V;
    d->have.assign(num_subjects, 0);
    const size_t n = 3 * (size_t)d->Vt;
    if (d->sum.ensure(n, true) || d->drift.ensure(n, true) || d->warp.ensure(n, true) || msm_dedrift_reset(d) != MSM_OK) {
        stage_alloc_failed(3 * n * sizeof(double));
        delete d;
        return nullptr;
    }
    return d;
}

void msm_dedrift_destroy(msm_dedrift *d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    delete d;  // the device arrays go back to the pool with their DevBuf members
}

int msm_dedrift_reset(msm_dedrift *d) {
    if (!d) return fail(MSM_ERR_INVALID, "msm_dedrift_reset: null handle");
    MSM_HIP(hipSetDevice(d->ctx->device));
    MSM_HIP(hipMemsetAsync(d->sum.p, 0, sizeof(double) * 3 * (size_t)d->Vt, d->ctx->stream));
    d->accumulated = 0;
    d->finished = false;
    d->warp_set = false;
    d->D = 0;
    d->have.assign(d->S, 0);
    return MSM_OK;
}

int msm_dedrift_accumulate(msm_dedrift *d, msm_mesh *reg, const double *orig_xyz, int32_t V, int32_t *tri_id, double *w, double *inverse_xyz) {
    if (!d || !reg || !orig_xyz) return fail(MSM_ERR_INVALID, "msm_dedrift_accumulate: null argument");
    MSM_TRY(check_subject_mesh(d, reg, V, "msm_dedrift_accumulate"));
    if (d->finished) return fail(MSM_ERR_STATE, "msm_dedrift_accumulate: the warp has been finished (msm_dedrift_reset starts a new group)");
    if (d->accumulated >= d->S) return fail(MSM_ERR_STATE, "msm_dedrift_accumulate: all %d subjects have been accumulated", d->S);
    return accumulate(d, reg, orig_xyz, tri_id, w, inverse_xyz);
}

int msm_dedrift_finish(msm_dedrift *d, double *warp_xyz, double *drift_xyz) {
    if (!d) return fail(MSM_ERR_INVALID, "msm_dedrift_finish: null handle");
    if (d->accumulated != d->S) return fail(MSM_ERR_STATE, "msm_dedrift_finish: %d of %d subjects accumulated", d->accumulated, d->S);
    msm_ctx *ctx = d->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MSM_TRY(launch_dedrift_finish(ctx, d->sum.p, d->Vt, d->S, d->drift.p, d->warp.p));
    if (warp_xyz) MSM_TRY(d->warp.download(warp_xyz, 3 * (size_t)d->Vt, ctx));
    if (drift_xyz) MSM_TRY(d->drift.download(drift_xyz, 3 * (size_t)d->Vt, ctx));
    MSM_TRY(check_status(ctx, "msm_dedrift_finish"));  // + the searches of the accumulate calls that fetched nothing
    d->finished = true;
    return MSM_OK;
}

int msm_dedrift_correct(msm_dedrift *d, int32_t subject, msm_mesh *reg, const double *orig_xyz, int32_t V, const double *data, int32_t D,
                        double *corrected_xyz, double *resampled, double *distortion, int32_t *tri_id, double *w) {
    if (!d || !reg || !orig_xyz || !data) return fail(MSM_ERR_INVALID, "msm_dedrift_correct: null argument");
    MSM_TRY(check_subject_mesh(d, reg, V, "msm_dedrift_correct"));
    if (!d->finished && !d->warp_set) return fail(MSM_ERR_STATE, "msm_dedrift_correct: msm_dedrift_finish has not been called");
    if (subject < 0 || subject >= d->S) return fail(MSM_ERR_INVALID, "msm_dedrift_correct: subject %d of %d", subject, d->S);
    if (D < 1 || (d->D && D != d->D)) return fail(MSM_ERR_INVALID, "msm_dedrift_correct: %d data rows, the group has %d", D, d->D);
    d->D = D;
    return correct(d, subject, reg, orig_xyz, data, D, corrected_xyz, resampled, distortion, tri_id, w);
}

int msm_dedrift_set_map(msm_dedrift *d, int32_t subject, const double *map, int32_t D) {
    if (!d || !map) return fail(MSM_ERR_INVALID, "msm_dedrift_set_map: null argument");
    if (subject < 0 || subject >= d->S) return fail(MSM_ERR_INVALID, "msm_dedrift_set_map: subject %d of %d", subject, d->S);
    if (D < 1 || (d->D && D != d->D)) return fail(MSM_ERR_INVALID, "msm_dedrift_set_map: %d data rows, the group has %d", D, d->D);
    msm_ctx *ctx = d->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    const size_t nmap = (size_t)D * d->Vt;
    if (d->maps.ensure((size_t)d->S * nmap, true)) return stage_alloc_failed(sizeof(double) * d->S * nmap);
    d->D = D;
    MSM_TRY(upload_staged(ctx, d->maps.p + (size_t)subject * nmap, map, sizeof(double) * nmap));
    d->have[subject] = 1;
    return MSM_OK;
}

int msm_dedrift_group_stats(msm_dedrift *d, double percentile, double *mean, double *stdev, double *cc, double *dice) {
    if (!d) return fail(MSM_ERR_INVALID, "msm_dedrift_group_stats: null handle");
    if (!(percentile >= 0.0 && percentile <= 100.0)) return fail(MSM_ERR_INVALID, "msm_dedrift_group_stats: percentile %g (0 .. 100)", percentile);
    for (int s = 0; s < d->S; ++s)
        if (!d->have[s]) return fail(MSM_ERR_STATE, "msm_dedrift_group_stats: subject %d has no resampled maps yet", s);
    return group_stats(d, "msm_dedrift_group_stats", nullptr, d->S, {}, false, percentile, mean, stdev, cc, dice, nullptr, nullptr);
}

int msm_dedrift_set_warp(msm_dedrift *d, const double *warp_xyz) {
    if (!d || !warp_xyz) return fail(MSM_ERR_INVALID, "msm_dedrift_set_warp: null argument");
    msm_ctx *ctx = d->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(d->warp.upload(warp_xyz, 3 * (size_t)d->Vt, ctx));  // on the context's stream: behind a correct that still reads the previous warp
    d->warp_set = true;
    return MSM_OK;
}

int msm_dedrift_group_stats_select(msm_dedrift *d, const int32_t *subjects, int32_t n, const double *mask, double percentile, double *mean, double *stdev,
                                   double *cc, double *dice, double *cc_mean, double *dice_mean) {
    if (!d || !subjects) return fail(MSM_ERR_INVALID, "msm_dedrift_group_stats_select: null argument");
    if (!(percentile >= 0.0 && percentile <= 100.0)) return fail(MSM_ERR_INVALID, "msm_dedrift_group_stats_select: percentile %g (0 .. 100)", percentile);
    if (n < 1 || n > d->S) return fail(MSM_ERR_INVALID, "msm_dedrift_group_stats_select: %d subjects listed, the group has %d", n, d->S);
    std::vector<char> seen(d->S, 0);
    for (int a = 0; a < n; ++a) {
        const int s = subjects[a];
        if (s < 0 || s >= d->S) return fail(MSM_ERR_INVALID, "msm_dedrift_group_stats_select: subject %d of %d", s, d->S);
        if (seen[s]) return fail(MSM_ERR_INVALID, "msm_dedrift_group_stats_select: subject %d is listed twice", s);
        seen[s] = 1;
    }
    for (int a = 0; a < n; ++a)
        if (!d->have[subjects[a]]) return fail(MSM_ERR_STATE, "msm_dedrift_group_stats_select: subject %d has no resampled maps yet", subjects[a]);
    std::vector<int32_t> kept;
    if (mask) {
        for (int v = 0; v < d->Vt; ++v)
            if (mask[v] > 0) kept.push_back(v);  // a NaN is not kept
        if (kept.empty()) return fail(MSM_ERR_INVALID, "msm_dedrift_group_stats_select: the mask keeps no vertex");
    }
    return group_stats(d, "msm_dedrift_group_stats_select", subjects, n, kept, mask != nullptr, percentile, mean, stdev, cc, dice, cc_mean, dice_mean);
}

}  // extern "C"
