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

// --- the group statistics over a list of the resident subjects (d_list: n positions -> subject, or nullptr: the subjects 0 .. n - 1 themselves) and the
// kept vertices (d_kept: K ascending vertex ids, or nullptr with K = Vt); map (s, d) is at maps[(s * D + d) * Vt ..]; stats, thr, bits and count are
// indexed by list position (a * D + d), the matrices are D x n x n
// mean and population standard deviation over the n listed maps (nmap = D * Vt values each), two passes in list order
int launch_dedrift_moments(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, size_t nmap, double *d_mean, double *d_sd);
// stats[2 m] = mean of map m over its kept values, stats[2 m + 1] = sqrt(sum (x - mean)^2)
int launch_dedrift_map_stats(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, int D, int Vt, const int32_t *d_kept, int K, double *d_stats);
// per map: the threshold numpy.percentile's linear interpolation gives from the order statistics k and k + 1 of its K kept values with fraction gamma, the
// mask x > threshold as bits (words = ceil(K / 64) 64-bit words per map, bit j is the j-th kept vertex) and its population count
int launch_dedrift_masks(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, int D, int Vt, const int32_t *d_kept, int K, int k, double gamma,
                         double *d_thr, unsigned long long *d_bits, int words, int32_t *d_count);
// cc[d][a][b], diagonal 1, and dice[d][a][b] = 2 |A and B| / (|A| + |B|), diagonal by the formula.  One workgroup per tile of 8 x 8 listed subjects and
// feature: every map row (mask row) is read once per tile
int launch_dedrift_tile_cc(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, int D, int Vt, const int32_t *d_kept, int K,
                           const double *d_stats, double *d_cc);
int launch_dedrift_tile_dice(msm_ctx *ctx, const unsigned long long *d_bits, const int32_t *d_count, int n, int D, int words, double *d_dice);
// the same two matrices of the whole set (no list) without a mask by one workgroup (cc) / one wavefront (dice) per pair and feature: the same bits, and
// sooner done where the pairs are few
int launch_dedrift_pair_cc(msm_ctx *ctx, const double *d_maps, int S, int D, int Vt, const double *d_stats, double *d_cc);
int launch_dedrift_pair_dice(msm_ctx *ctx, const unsigned long long *d_bits, const int32_t *d_count, int S, int D, int words, double *d_dice);
// out[m] = the mean over the pairs a < b of matrix m (n x n) of d_mat, one fixed tree per matrix; NaN when n = 1
int launch_dedrift_pair_mean(msm_ctx *ctx, const double *d_mat, int nmat, int n, double *d_out);

}  // namespace msm
