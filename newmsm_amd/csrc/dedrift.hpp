// dedrift.hpp -- launch wrappers of dedrift_kernels.hip (device pointers only), used by dedrift.cpp: the post-processing of a groupwise run
// (the dedrift warp, the corrected spheres' distortion maps and the group statistics; gMSM_scripts/gMSM_tutorial/gw_MSM.sh:65-128, compare_stats.py).
#pragma once

#include "internal.hpp"

namespace msm {

// inverse (optional, 3 x Vt) = the weights w (3 x Vt) of every template vertex in its triangle vid (3 x Vt) of the registered sphere applied to the
// subject's input sphere m (3 x Vs), summed in ascending vertex id (project_anatomical_mesh, R/resampler.cpp:260-282); sum += inverse
int launch_dedrift_accumulate(msm_ctx *ctx, const int32_t *d_vid, const double *d_w, int Vt, const double *d_m, int Vs, double *d_sum, double *d_inverse);
// drift = sum / S; warp = (drift - midpoint of its bounding box) scaled to length 100.  One workgroup; box: 6 doubles of scratch
int launch_dedrift_finish(msm_ctx *ctx, const double *d_sum, int Vt, int S, double *d_drift, double *d_warp);
// out (2 x V): per vertex the mean over its triangles (tid order) of log2 J and of log2 R, original m against deformed c (both 3 x V, triangles 3 x T)
int launch_vertex_distortion(msm_ctx *ctx, const double *d_m, const double *d_c, int V, const int32_t *d_tri, int T, const int32_t *d_tid_ptr,
                             const int32_t *d_tid, double *d_out);
// mean and population standard deviation over the S maps (S x n), two passes in subject order
int launch_dedrift_moments(msm_ctx *ctx, const double *d_maps, int S, size_t n, double *d_mean, double *d_sd);
// stats[2 m] = mean of map m, stats[2 m + 1] = sqrt(sum (x - mean)^2); nmaps maps of Vt values
int launch_dedrift_map_stats(msm_ctx *ctx, const double *d_maps, int nmaps, int Vt, double *d_stats);
// cc[d][i][j] for the S x D maps (map (s, d) at maps[(s * D + d) * Vt ..]); the diagonal is 1
int launch_dedrift_pair_cc(msm_ctx *ctx, const double *d_maps, int S, int D, int Vt, const double *d_stats, double *d_cc);
// per map: the threshold numpy.percentile's linear interpolation gives from the order statistics k and k + 1 with fraction gamma, the mask x > threshold
// as bits (words 64-bit words per map) and its population count
int launch_dedrift_masks(msm_ctx *ctx, const double *d_maps, int nmaps, int Vt, int k, double gamma, double *d_thr, unsigned long long *d_bits, int words,
                         int32_t *d_count);
// dice[d][i][j] = 2 |A and B| / (|A| + |B|)
int launch_dedrift_pair_dice(msm_ctx *ctx, const unsigned long long *d_bits, const int32_t *d_count, int S, int D, int words, double *d_dice);

// --- the same figures over a list of the resident subjects (d_list: n positions -> subject) and the kept vertices (d_kept: K ascending vertex ids, or
// nullptr with K = Vt); stats, thr, bits and count are indexed by list position (a * D + d), the matrices are D x n x n
int launch_dedrift_moments_list(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, size_t nmap, double *d_mean, double *d_sd);
int launch_dedrift_map_stats_sel(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, int D, int Vt, const int32_t *d_kept, int K,
                                 double *d_stats);
// order statistics k, k + 1 and fraction gamma of K values; words = ceil(K / 64), bit j of a map's mask is its j-th kept vertex
int launch_dedrift_masks_sel(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, int D, int Vt, const int32_t *d_kept, int K, int k,
                             double gamma, double *d_thr, unsigned long long *d_bits, int words, int32_t *d_count);
// one workgroup per tile of 8 x 8 listed subjects and feature: every map row (mask row) is read once per tile
int launch_dedrift_tile_cc(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, int D, int Vt, const int32_t *d_kept, int K,
                           const double *d_stats, double *d_cc);
int launch_dedrift_tile_dice(msm_ctx *ctx, const unsigned long long *d_bits, const int32_t *d_count, int n, int D, int words, double *d_dice);
// out[m] = the mean over the pairs a < b of matrix m (n x n) of d_mat, one fixed tree per matrix; NaN when n = 1
int launch_dedrift_pair_mean(msm_ctx *ctx, const double *d_mat, int nmat, int n, double *d_out);

}  // namespace msm
