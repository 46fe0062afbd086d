// features.cpp -- msm_level_features behind the C ABI: featurespace::initialise (M/featurespace.cpp:39-86) for n data sets on one level grid.  Per data
// set the matrix goes up once; its mask (create_exclusion), the resampling onto the grid (queries, list surgery -- masked or not -- and the weighted sums)
// and the smoothing are queued on the context's stream behind it, then the histogram matching of data sets 1 .. n-1 against data set 0 over the resident
// matrices.  Nothing is waited for in between: one status check and one download at the end.  The variance normalisation follows on the host, one
// parallel section over the n x D rows (its recurrence is serial per row: varnorm.hpp).  Every kernel is the one the separate entry points launch, or
// its masked form (resample_kernels.hip: row_active, k_apply_rows_masked; features_kernels.hip: k_create_exclusion), so the bytes are theirs.
#include <algorithm>
#include <cmath>

#include "features.hpp"
#include "histmatch.hpp"
#include "host_parallel.hpp"
#include "kernels.hpp"
#include "resample.hpp"
#include "varnorm.hpp"

using namespace msm;

namespace {

struct FeaturesScratch {
    DevBuf<double> in, excl;        // a data set's matrix and mask on its native mesh
    DevBuf<double> res, res_mask;   // resampled, before the smoothing
    DevBuf<double> feat, mask;      // the level's matrices (n x D x V) and masks (n x V) on the grid
    DevBuf<double> unit;            // launch_smooth's scratch
    DevBuf<int> cv;                 // the grid vertex closest to every grid vertex (smooth_data's centres)
};

FeaturesScratch &features_scratch(msm_ctx *ctx) {
    if (!ctx->features_scratch) ctx->features_scratch = std::shared_ptr<void>(new FeaturesScratch(), [](void *p) { delete static_cast<FeaturesScratch *>(p); });
    return *static_cast<FeaturesScratch *>(ctx->features_scratch.get());
}

}  // namespace

namespace msm {

// msm_level_features' argument checks (no handle is dereferenced beyond its context and sizes): MSM_OK or MSM_ERR_INVALID with a message
int level_features_check(const msm_mesh *grid, int n, msm_mesh *const *in_mesh, const double *const *data, int D, const double *sigma,
                         const msm_level_features_params *p, const double *feat, const double *mask) {
    if (!grid || !in_mesh || !data || !sigma || !p || !feat) return fail(MSM_ERR_INVALID, "msm_level_features: null argument");
    if (n <= 0) return fail(MSM_ERR_INVALID, "msm_level_features: %d data sets", n);
    if (D <= 0) return fail(MSM_ERR_INVALID, "msm_level_features: %d feature rows", D);
    if (p->exclude && !mask) return fail(MSM_ERR_INVALID, "msm_level_features: exclusion masks are asked for and there is no room for them (mask is NULL)");
    for (int i = 0; i < n; ++i) {
        if (!in_mesh[i]) return fail(MSM_ERR_INVALID, "msm_level_features: the mesh of data set %d is NULL", i);
        if (!data[i]) return fail(MSM_ERR_INVALID, "msm_level_features: the data of data set %d is NULL", i);
        if (in_mesh[i]->ctx != grid->ctx) return fail(MSM_ERR_INVALID, "msm_level_features: the mesh of data set %d and the grid belong to different contexts", i);
    }
    return MSM_OK;
}

}  // namespace msm

extern "C" int msm_level_features(msm_mesh *grid, int32_t n, msm_mesh *const *in_mesh, const double *const *data, int32_t D, const double *sigma,
                                  const msm_level_features_params *p, double *feat, double *mask) {
    MSM_TRY(level_features_check(grid, n, in_mesh, data, D, sigma, p, feat, mask));
    msm_ctx *ctx = grid->ctx;
    const int N = grid->V;
    const bool exclude = p->exclude != 0, match = p->intensity != 0 && n > 1;
    if (N <= 0) return fail(MSM_ERR_INVALID, "msm_level_features: the grid has no vertices");
    if ((int64_t)n * D > (1 << 24)) return fail(MSM_ERR_CAPACITY, "msm_level_features: %lld rows exceed one call", (long long)n * D);
    if (match) MSM_TRY(hist_rows_check("msm_level_features", n - 1, D, N, N));
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));

    // ---- everything that may wait (tree builds, adjacency uploads, allocations) first, so that the queue below runs through
    int maxV = 0, maxT = 0;
    bool smooth = false;
    for (int i = 0; i < n; ++i) {
        if (in_mesh[i]->V <= 0) return fail(MSM_ERR_INVALID, "msm_level_features: the mesh of data set %d has no vertices", i);
        maxV = std::max(maxV, in_mesh[i]->V), maxT = std::max(maxT, in_mesh[i]->T);
        smooth = smooth || sigma[i] > 0;
        MSM_TRY(ensure_tree_pair(in_mesh[i], grid));
        MSM_TRY(ensure_adjacency_dev(in_mesh[i]));
    }
    MSM_TRY(ensure_adjacency_dev(grid));
    MSM_TRY(reserve_surgery_scratch(ctx, maxV, N, maxT, grid->T));
    FeaturesScratch &s = features_scratch(ctx);
    const size_t DN = (size_t)D * N, total = (size_t)n * DN;
    if (s.in.ensure((size_t)D * maxV) || s.feat.ensure(total) || (exclude && (s.excl.ensure(maxV) || s.mask.ensure((size_t)n * N))) ||
        (smooth && (s.res.ensure(DN) || s.unit.ensure(smooth_scratch_doubles(N)) || s.cv.ensure(N) || (exclude && s.res_mask.ensure(N)))))
        return stage_alloc_failed(sizeof(double) * (total + (size_t)D * maxV + DN));

    // ---- the queue
    if (smooth) MSM_TRY(launch_closest_vertex(ctx, dev_tree(grid), grid->d_xyz.p, N, s.cv.p));  // Octree(orig).get_closest_vertex_ID(ci), R/resampler.cpp:182
    const double lo = p->thrl - kEps, hi = p->thru + kEps;
    for (int i = 0; i < n; ++i) {
        msm_mesh *m = in_mesh[i];
        const bool sm = sigma[i] > 0;
        double *f_i = s.feat.p + (size_t)i * DN, *m_i = exclude ? s.mask.p + (size_t)i * N : nullptr;
        double *r_out = sm ? s.res.p : f_i, *rm_out = !exclude ? nullptr : (sm ? s.res_mask.p : m_i);
        MSM_TRY(upload_staged(ctx, s.in.p, data[i], sizeof(double) * (size_t)D * m->V));
        AdaptiveDev w;
        if (exclude) {
            MSM_TRY(launch_create_exclusion(ctx, s.in.p, D, m->V, lo, hi, s.excl.p));
            MSM_TRY(adaptive_weights_dev_masked(m, grid, s.excl.p, w));
            MSM_TRY(launch_apply_rows_masked(ctx, w.nNew, w.nOld, D, w.row_ptr, w.col, w.val, s.in.p, s.excl.p, r_out, rm_out));
        } else {
            MSM_TRY(adaptive_weights_dev(m, grid, w, false));
            MSM_TRY(apply_weights_dev(ctx, w, s.in.p, D, r_out));
        }
        if (sm) {
            const double ang = 4 * asin(sigma[i] / (2 * kRad));  // R/resampler.cpp:175, with the host's libm like msm_smooth_data
            MSM_TRY(launch_smooth(ctx, grid->d_xyz.p, N, s.unit.p, s.cv.p, s.res.p, N, D, sigma[i], cos(ang), exclude ? s.res_mask.p : nullptr, f_i, m_i));
        }
    }
    if (match) {  // data sets 1 .. n-1 against data set 0, in place (every lane reads and writes its own value)
        HistRows rows;
        rows.src = s.feat.p + DN, rows.ref = s.feat.p;
        rows.src_excl = exclude ? s.mask.p + N : nullptr, rows.ref_excl = exclude ? s.mask.p : nullptr;
        rows.n_src = n - 1, rows.D = D, rows.Vs = N, rows.Vt = N;
        rows.src_rows = exclude ? 1 : 0, rows.ref_rows = exclude ? 1 : 0;
        MSM_TRY(hist_match_dev(ctx, rows, s.feat.p + DN));
    }
    MSM_TRY(s.feat.download(feat, total, ctx));
    if (exclude) MSM_TRY(s.mask.download(mask, (size_t)n * N, ctx));
    MSM_TRY(check_status(ctx, "msm_level_features"));  // a failed search of any data set (synchronises)
    if (p->varnorm) variance_normalise_rows(feat, n, D, N, exclude ? mask : nullptr);
    return MSM_OK;
}
