// histmatch.hpp -- launch wrappers of histmatch_kernels.hip (device pointers only), used by histmatch.cpp: --IN / --INc, the histogram matching of
// multivariate_histogram_normalization (M/reg_tools.cpp:745-802) by the definition of DESIGN.md section 5.11.
#pragma once

#include "internal.hpp"

namespace msm {

constexpr int kHistBins = 256;   // numbins, M/reg_tools.cpp:756
constexpr int kHistChunk = 4096;  // values of a row per workgroup of the range, count and apply kernels

// The rows of one call: n_src * D source rows of Vs values, then D target rows of Vt values (row r >= n_src * D is target row r - n_src * D).
// Masks: src_excl n_src x src_rows x Vs, ref_excl ref_rows x Vt, either may be null.
struct HistRows {
    const double *src, *ref, *src_excl, *ref_excl;
    int n_src, D, Vs, Vt, src_rows, ref_rows;
};

// range[2 r], range[2 r + 1] (zeroed by the caller): the largest inverted key and the largest key over the finite values of row r -- its minimum and
// maximum under an order-preserving map of doubles to unsigned integers; both stay 0 for a row without a finite value
int launch_hist_range(msm_ctx *ctx, const HistRows &rows, unsigned long long *d_range);
// counts[r * 256 + b - 1] (zeroed by the caller) += the counted values of row r in bin b; rows without a range are left at zero
int launch_hist_counts(msm_ctx *ctx, const HistRows &rows, const unsigned long long *d_range, unsigned int *d_counts);
// per source row: table[row * 256 + b - 1] = the target value of source bin b, flag[row] = 1 -- or flag[row] = 0: the row is left unchanged
int launch_hist_table(msm_ctx *ctx, const HistRows &rows, const unsigned long long *d_range, const unsigned int *d_counts, double *d_table, int32_t *d_flag);
// out (n_src x D x Vs) = src with every counted value of a flagged row replaced by its bin's table entry
int launch_hist_apply(msm_ctx *ctx, const HistRows &rows, const unsigned long long *d_range, const double *d_table, const int32_t *d_flag, double *d_out);

// histmatch.cpp, the device part of msm_histogram_match: the four launches over rows that lie in HBM, with the context's range words, counters, tables and
// flags (zeroed here); d_out may be rows.src.  Nothing is waited for.  hist_rows_check: the limits of one launch (MSM_ERR_CAPACITY with `who` in the message).
int hist_rows_check(const char *who, int n_src, int D, int Vs, int Vt);
int hist_match_dev(msm_ctx *ctx, const HistRows &rows, double *d_out);

}  // namespace msm
