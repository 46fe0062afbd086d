// histmatch.cpp -- msm_histogram_match behind the C ABI: --IN / --INc, multivariate_histogram_normalization (M/reg_tools.cpp:745-802) for n_src source
// matrices against one target.  Validation, the copies and the order of the four launches are here; everything per value, per bin and per row is in
// histmatch_kernels.hip.  The matrices and masks go up through the stager, the matched rows come back through it; ranges, counters, tables and flags
// never leave HBM.
#include <algorithm>

#include "histmatch.hpp"

using namespace msm;

namespace {

struct HistScratch {
    DevBuf<double> src, ref, src_excl, ref_excl, table;
    DevBuf<unsigned long long> stats;  // per row two range words, then per row 256 32-bit counters: zeroed together
    DevBuf<int32_t> flag;
};

HistScratch &hist_scratch(msm_ctx *ctx) {
    if (!ctx->histmatch_scratch) ctx->histmatch_scratch = std::shared_ptr<void>(new HistScratch(), [](void *p) { delete static_cast<HistScratch *>(p); });
    return *static_cast<HistScratch *>(ctx->histmatch_scratch.get());
}

}  // namespace

namespace msm {

int hist_rows_check(const char *who, int n_src, int D, int Vs, int Vt) {
    const int64_t rows64 = ((int64_t)n_src + 1) * D;
    if (rows64 > (1 << 24) || (std::max(Vs, Vt) + kHistChunk - 1) / kHistChunk > 65535)
        return fail(MSM_ERR_CAPACITY, "%s: %lld rows of up to %d values exceed one launch", who, (long long)rows64, std::max(Vs, Vt));
    return MSM_OK;
}

int hist_match_dev(msm_ctx *ctx, const HistRows &rows, double *d_out) {
    HistScratch &s = hist_scratch(ctx);
    const int R = (rows.n_src + 1) * rows.D, nsrc_rows = rows.n_src * rows.D;
    const size_t nstat = 2 * (size_t)R + (size_t)R * kHistBins / 2;  // 64-bit words: the counters are 32-bit
    if (s.table.ensure((size_t)nsrc_rows * kHistBins) || s.stats.ensure(nstat) || s.flag.ensure(nsrc_rows)) return stage_alloc_failed(sizeof(double) * nstat);
    MSM_HIP(hipMemsetAsync(s.stats.p, 0, sizeof(unsigned long long) * nstat, ctx->stream));
    unsigned long long *range = s.stats.p;
    unsigned int *counts = reinterpret_cast<unsigned int *>(s.stats.p + 2 * (size_t)R);
    MSM_TRY(launch_hist_range(ctx, rows, range));
    MSM_TRY(launch_hist_counts(ctx, rows, range, counts));
    MSM_TRY(launch_hist_table(ctx, rows, range, counts, s.table.p, s.flag.p));
    return launch_hist_apply(ctx, rows, range, s.table.p, s.flag.p, d_out);
}

}  // namespace msm

extern "C" int msm_histogram_match(msm_ctx *ctx, int32_t n_src, int32_t D, int32_t Vs, const double *src, const double *src_excl, int32_t src_excl_rows,
                                   int32_t Vt, const double *ref, const double *ref_excl, int32_t ref_excl_rows, double *out) {
    if (!ctx || !src || !ref || !out) return fail(MSM_ERR_INVALID, "msm_histogram_match: null argument");
    if (n_src < 1 || D < 1 || Vs < 1 || Vt < 1) return fail(MSM_ERR_INVALID, "msm_histogram_match: %d source matrices of %d x %d against %d x %d", n_src, D, Vs, D, Vt);
    if ((src_excl && src_excl_rows < 1) || (ref_excl && ref_excl_rows < 1)) return fail(MSM_ERR_INVALID, "msm_histogram_match: a mask needs at least one row");
    MSM_TRY(hist_rows_check("msm_histogram_match", n_src, D, Vs, Vt));
    const int nsrc_rows = n_src * D;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    HistScratch &s = hist_scratch(ctx);
    const size_t nsrc = (size_t)nsrc_rows * Vs, nref = (size_t)D * Vt;
    const size_t nsrc_excl = src_excl ? (size_t)n_src * src_excl_rows * Vs : 0, nref_excl = ref_excl ? (size_t)ref_excl_rows * Vt : 0;
    if (s.src.ensure(nsrc) || s.ref.ensure(nref) ||
        (src_excl && s.src_excl.ensure(nsrc_excl)) || (ref_excl && s.ref_excl.ensure(nref_excl)))
        return stage_alloc_failed(sizeof(double) * (nsrc + nref + nsrc_excl + nref_excl));
    // (a matrix in pinned memory of the context goes up from where it lies, anything else through the staging blocks)
    MSM_TRY(upload_staged(ctx, s.src.p, src, sizeof(double) * nsrc));
    MSM_TRY(upload_staged(ctx, s.ref.p, ref, sizeof(double) * nref));
    if (src_excl) MSM_TRY(upload_staged(ctx, s.src_excl.p, src_excl, sizeof(double) * nsrc_excl));
    if (ref_excl) MSM_TRY(upload_staged(ctx, s.ref_excl.p, ref_excl, sizeof(double) * nref_excl));
    HistRows rows;
    rows.src = s.src.p, rows.ref = s.ref.p;
    rows.src_excl = src_excl ? s.src_excl.p : nullptr, rows.ref_excl = ref_excl ? s.ref_excl.p : nullptr;
    rows.n_src = n_src, rows.D = D, rows.Vs = Vs, rows.Vt = Vt;
    rows.src_rows = src_excl ? src_excl_rows : 0, rows.ref_rows = ref_excl ? ref_excl_rows : 0;
    MSM_TRY(hist_match_dev(ctx, rows, s.src.p));  // in place: every lane reads and writes its own value
    MSM_TRY(s.src.download(out, nsrc, ctx));
    return check_status(ctx, "msm_histogram_match");
}
