// cohort.cpp -- msm_surface_distortion and msm_abs_summary behind the C ABI: the distortion maps and the distortion summary of a cohort registered to
// one template (gMSM_scripts/newMSM_HCP_to_template_v2.sh: wb_command -surface-distortion -local-affine-method -log2 per subject; get_group_stats.py /
// compare_stats.py: mean, max and percentiles of the absolute maps).  Validation, the copies and the order of the launches are here; everything per
// triangle, per vertex and per value is in cohort_kernels.hip.  The arrays go up through the stager and the results come back through it; per-triangle
// values, counters and partial sums never leave HBM.
#include <algorithm>
#include <cmath>
#include <vector>

#include "cohort.hpp"

using namespace msm;

namespace {

struct CohortScratch {
    DevBuf<double> orig, fin, tl, out;     // distortion: 3 x V, S x 3 x V, 2 x S x T, S x 2 x V
    DevBuf<int32_t> tri, tid_ptr, tid;
    DevBuf<double> x, partial, gamma, res;  // summary: the values, one partial sum per workgroup, the interpolation fractions, mean / max / values
    DevBuf<long long> k;
    DevBuf<unsigned long long> counters;
};

CohortScratch &cohort_scratch(msm_ctx *ctx) {
    if (!ctx->cohort_scratch) ctx->cohort_scratch = std::shared_ptr<void>(new CohortScratch(), [](void *p) { delete static_cast<CohortScratch *>(p); });
    return *static_cast<CohortScratch *>(ctx->cohort_scratch.get());
}

}  // namespace

extern "C" int msm_surface_distortion(msm_ctx *ctx, const double *orig_xyz, const int32_t *tri, int32_t V, int32_t T, const double *final_xyz, int32_t S,
                                      double *out) {
    if (!ctx || !orig_xyz || !final_xyz || !out || (T > 0 && !tri)) return fail(MSM_ERR_INVALID, "msm_surface_distortion: null argument");
    if (S <= 0 || V <= 0 || T < 0) return fail(MSM_ERR_INVALID, "msm_surface_distortion: %d deformed copies of %d vertices and %d triangles", S, V, T);
    if (S > 65535) return fail(MSM_ERR_CAPACITY, "msm_surface_distortion: %d deformed copies exceed one launch (65535)", S);
    for (size_t i = 0; i < 3 * (size_t)T; ++i)
        if (tri[i] < 0 || tri[i] >= V) return fail(MSM_ERR_INVALID, "msm_surface_distortion: triangle %zu names vertex %d of %d", i % (size_t)T, tri[i], V);
    if (T == 0) {  // no triangle anywhere: every vertex's value is 0
        std::fill(out, out + (size_t)S * 2 * V, 0.0);
        return MSM_OK;
    }
    Adjacency adj;  // Mpoint::trID lists: per vertex its triangles in ascending id
    build_adjacency(tri, V, T, adj);
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    CohortScratch &s = cohort_scratch(ctx);
    const size_t nfin = (size_t)S * 3 * V, nout = (size_t)S * 2 * V, ntl = 2 * (size_t)S * T;
    if (s.orig.ensure(3 * (size_t)V) || s.fin.ensure(nfin) || s.tl.ensure(ntl ? ntl : 1) || s.out.ensure(nout))
        return stage_alloc_failed(sizeof(double) * (3 * (size_t)V + nfin + ntl + nout));
    MSM_TRY(upload_staged(ctx, s.orig.p, orig_xyz, sizeof(double) * 3 * (size_t)V));
    MSM_TRY(upload_staged(ctx, s.fin.p, final_xyz, sizeof(double) * nfin));
    MSM_TRY(s.tri.upload(tri, 3 * (size_t)T, ctx));
    MSM_TRY(s.tid_ptr.upload_vec(adj.tid_ptr, ctx));
    MSM_TRY(s.tid.upload_vec(adj.tid, ctx));
    MSM_TRY(launch_triangle_distortion(ctx, s.orig.p, s.fin.p, V, s.tri.p, T, S, s.tl.p));
    MSM_TRY(launch_vertex_gather(ctx, s.tl.p, V, T, S, s.tid_ptr.p, s.tid.p, s.out.p));
    MSM_TRY(s.out.download(out, nout, ctx));
    return check_status(ctx, "msm_surface_distortion");
}

extern "C" int msm_abs_summary(msm_ctx *ctx, const double *x, int64_t n, const double *percentiles, int32_t np, double *mean, double *max, double *values) {
    if (!ctx || !x || (np > 0 && (!percentiles || !values))) return fail(MSM_ERR_INVALID, "msm_abs_summary: null argument");
    if (n <= 0 || np < 0) return fail(MSM_ERR_INVALID, "msm_abs_summary: %lld values, %d percentiles", (long long)n, np);
    if (np > kSummaryMaxPercentiles) return fail(MSM_ERR_CAPACITY, "msm_abs_summary: %d percentiles exceed one call (%d)", np, kSummaryMaxPercentiles);
    // numpy.percentile, method "linear": the virtual index (n - 1) q with q = percentile / 100, between the order statistics floor and floor + 1
    std::vector<long long> k((size_t)np + 1, 0);
    std::vector<double> gamma((size_t)np + 1, 0.0);
    for (int q = 0; q < np; ++q) {
        if (!(percentiles[q] >= 0.0 && percentiles[q] <= 100.0)) return fail(MSM_ERR_INVALID, "msm_abs_summary: percentile %g (0 .. 100)", percentiles[q]);
        const double vidx = (double)(n - 1) * (percentiles[q] / 100.0);
        const double fl = std::floor(vidx);
        k[(size_t)q] = (long long)fl, gamma[(size_t)q] = vidx - fl;
    }
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    CohortScratch &s = cohort_scratch(ctx);
    const int blocks = summary_blocks(n);
    const size_t words = summary_counter_words(np);
    if (s.x.ensure((size_t)n) || s.partial.ensure(kSummaryMaxBlocks) || s.res.ensure(2 + (size_t)kSummaryMaxPercentiles) || s.counters.ensure(words))
        return stage_alloc_failed(sizeof(double) * (size_t)n);
    MSM_TRY(upload_staged(ctx, s.x.p, x, sizeof(double) * (size_t)n));
    MSM_TRY(s.k.upload_vec(k, ctx));
    MSM_TRY(s.gamma.upload_vec(gamma, ctx));
    MSM_HIP(hipMemsetAsync(s.counters.p, 0, sizeof(unsigned long long) * words, ctx->stream));
    const SummaryCounters c = summary_counters(s.counters.p, np);
    MSM_TRY(launch_abs_partials(ctx, s.x.p, n, blocks, s.partial.p, c, s.k.p, np));
    for (int pass = 0; pass < 8; ++pass) MSM_TRY(launch_abs_select_pass(ctx, s.x.p, n, blocks, c, np, pass));
    MSM_TRY(launch_abs_next(ctx, s.x.p, n, blocks, c, np));
    MSM_TRY(launch_abs_finish(ctx, s.partial.p, blocks, n, c, s.k.p, s.gamma.p, np, s.res.p));
    std::vector<double> res(2 + (size_t)np);
    MSM_TRY(s.res.download(res.data(), res.size(), ctx));
    MSM_TRY(check_status(ctx, "msm_abs_summary"));
    if (mean) *mean = res[0];
    if (max) *max = res[1];
    for (int q = 0; q < np; ++q) values[q] = res[2 + (size_t)q];
    return MSM_OK;
}
