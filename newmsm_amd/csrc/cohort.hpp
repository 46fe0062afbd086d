// cohort.hpp -- launch wrappers of cohort_kernels.hip (device pointers only), used by cohort.cpp: what a cohort registered to one template needs after
// its registrations (gMSM_scripts/newMSM_HCP_to_template_v2.sh, get_group_stats.py, compare_stats.py): the distortion maps of many deformed copies of
// one sphere in one launch, and the mean / maximum / percentiles of |x| over all of them.
#pragma once

#include "internal.hpp"

namespace msm {

constexpr int kSummaryMaxPercentiles = 16;  // one 256-bin LDS histogram each
constexpr int kSummaryMaxBlocks = 1024;

// workgroups of the summary's passes over n values: a function of n alone, so the shape of the mean's sum is too
inline int summary_blocks(int64_t n) {
    const int64_t b = (n + 256 * 16 - 1) / (256 * 16);
    return (int)(b < 1 ? 1 : b > kSummaryMaxBlocks ? kSummaryMaxBlocks : b);
}

// tl (2 x S x T): log2 J and log2 R of every triangle of orig (3 x V) against the same triangle of each of the S deformed copies (fin: S x 3 x V)
int launch_triangle_distortion(msm_ctx *ctx, const double *d_orig, const double *d_fin, int V, const int32_t *d_tri, int T, int S, double *d_tl);
// out (S x 2 x V): per vertex the plain mean of its triangles' two values in tid order, 0 without a triangle
int launch_vertex_gather(msm_ctx *ctx, const double *d_tl, int V, int T, int S, const int32_t *d_tid_ptr, const int32_t *d_tid, double *d_out);

// The counters of one msm_abs_summary call, zeroed together before it: hist (np x 256), prefix / krem / cnt (np each), mn (np, preset to all ones by
// launch_abs_partials) and maxkey (1).  All integers.
struct SummaryCounters {
    unsigned long long *hist, *prefix, *krem, *cnt, *mn, *maxkey;
};
inline size_t summary_counter_words(int np) { return (size_t)np * 256 + 4 * (size_t)np + 1; }
inline SummaryCounters summary_counters(unsigned long long *base, int np) {
    SummaryCounters c;
    c.hist = base;
    c.prefix = c.hist + (size_t)np * 256;
    c.krem = c.prefix + np;
    c.cnt = c.krem + np;
    c.mn = c.cnt + np;
    c.maxkey = c.mn + np;
    return c;
}
// partial[b]: workgroup b's sum of |x| over its strided share (a fixed tree); maxkey: the largest key; krem[q] = k[q]; mn[q] = all ones
int launch_abs_partials(msm_ctx *ctx, const double *d_x, int64_t n, int blocks, double *d_partial, SummaryCounters c, const long long *d_k, int np);
// one of the eight passes of the radix select (pass 0: the top eight bits), for all np order statistics together: counts, then the choice of the bin
int launch_abs_select_pass(msm_ctx *ctx, const double *d_x, int64_t n, int blocks, SummaryCounters c, int np, int pass);
// cnt[q] = how many keys are <= the selected one, mn[q] = the smallest larger key
int launch_abs_next(msm_ctx *ctx, const double *d_x, int64_t n, int blocks, SummaryCounters c, int np);
// out[0] = mean, out[1] = max, out[2 + q] = the interpolated percentile (numpy's _lerp with gamma[q]); all NaN when a NaN was met
int launch_abs_finish(msm_ctx *ctx, const double *d_partial, int blocks, int64_t n, SummaryCounters c, const long long *d_k, const double *d_gamma, int np,
                      double *d_out);

}  // namespace msm
