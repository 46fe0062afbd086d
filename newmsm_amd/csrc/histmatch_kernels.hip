// histmatch_kernels.hip -- --IN / --INc on gfx950: every feature row of the source matrices matched to the same row of one target matrix through
// 256-bin histograms (multivariate_histogram_normalization, M/reg_tools.cpp:745-802; the matching itself by the definition of DESIGN.md section 5.11,
// restated in tests/histmatch_literal.py -- the reference hands it to FSL's MISCMATHS::Histogram, which is not in its tree).
//
//   k_hist_range   workgroups over chunks of a row: minimum and maximum of its finite values.  Doubles are mapped to unsigned integers that order as they
//                  do, a chunk is reduced over a fixed LDS tree and joins the row's two words by integer atomicMax (the minimum as the maximum of the
//                  inverted key, so that both words start from zero).  Order independent.
//   k_hist_counts  workgroups over chunks of a row: 256 integer counters in LDS, added to the row's global counters by integer atomics, one 1 KB segment
//                  per workgroup.  A wavefront first settles the bins most of its lanes may share with one add of the lane count (twice: a zero-valued
//                  medial wall puts whole wavefronts into one counter, and 64 adds to one LDS address are served one after the other); what is left
//                  adds for itself.
//   k_hist_table   one workgroup of 256 lanes per (source, row): integer prefix sums of both histograms, both CDFs (an exact integer sum, one division)
//                  in LDS, lane b finds the target bin of source bin b + 1 by binary search and writes its target value; decides the "row left
//                  unchanged" cases and flags them.
//   k_hist_apply   one lane per value: its bin again, the table's entry where the value is counted.
//
// Integer atomics only, no floating-point sum anywhere: two runs give the same bits.  Built with -ffp-contract=off: the divisions, products and sums below
// are the ones the definition writes, one rounding each.
#include "histmatch.hpp"

namespace msm {

namespace {

constexpr int kBlock = 256;
static_assert(kBlock == kHistBins, "lane b of a workgroup owns bin b + 1");

typedef unsigned long long u64;

__device__ __forceinline__ bool is_finite(double v) { return ((u64)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
// finite doubles -> unsigned integers in the same order, never 0
__device__ __forceinline__ u64 order_key(double v) {
    const u64 u = (u64)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(u64 k) { return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k)); }

struct RowView {
    const double *x, *m;  // the values and their mask (or null)
    int V;
};

__device__ __forceinline__ RowView row_view(const HistRows &r, int row) {
    const int nsrc = r.n_src * r.D;
    RowView v;
    if (row < nsrc) {
        const int s = row / r.D, d = row - s * r.D;
        v.x = r.src + (size_t)row * r.Vs;
        v.m = r.src_excl ? r.src_excl + ((size_t)s * r.src_rows + (d < r.src_rows ? d : 0)) * r.Vs : nullptr;  // M/reg_tools.cpp:764-767
        v.V = r.Vs;
    } else {
        const int d = row - nsrc;
        v.x = r.ref + (size_t)d * r.Vt;
        v.m = r.ref_excl ? r.ref_excl + (size_t)(d < r.ref_rows ? d : 0) * r.Vt : nullptr;
        v.V = r.Vt;
    }
    return v;
}

// a row's range from its two words; false: no finite value, or minimum == maximum
__device__ __forceinline__ bool row_range(const u64 *__restrict__ range, int row, double &lo, double &hi) {
    const u64 klo = range[2 * (size_t)row], khi = range[2 * (size_t)row + 1];
    if (khi == 0) return false;
    lo = key_value(~klo), hi = key_value(khi);
    return hi != lo;
}

__device__ __forceinline__ int hist_bin(double v, double lo, double w) {
    const int b = (int)((v - lo) / w) + 1;
    return b < 1 ? 1 : (b > kHistBins ? kHistBins : b);
}

__device__ __forceinline__ bool counted(double v, double m) { return is_finite(v) && m > 0.0; }

// kLoads values of a row per lane and sweep, loaded together so that their latencies overlap (a sweep of one load each is a chain of kHistChunk / kBlock
// memory latencies: 12 us for a row of 40 962 values); a lane beyond `end` gets a NaN, which nothing counts
constexpr int kLoads = 4;
static_assert(kHistChunk % (kLoads * kBlock) == 0, "a chunk is a whole number of sweeps");

__device__ __forceinline__ void load_values(const RowView &rv, int base, int end, double (&v)[kLoads]) {
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int i = base + k * kBlock + (int)threadIdx.x;
        v[k] = i < end ? rv.x[i] : __longlong_as_double(0x7ff8000000000000ll);
    }
}
// their masks: 1 without a mask
__device__ __forceinline__ void load_masks(const RowView &rv, int base, int end, double (&m)[kLoads]) {
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int i = base + k * kBlock + (int)threadIdx.x;
        m[k] = (rv.m && i < end) ? rv.m[i] : 1.0;
    }
}

__global__ __launch_bounds__(kBlock) void k_hist_range(HistRows r, u64 *__restrict__ range) {
    __shared__ u64 s_lo[kBlock], s_hi[kBlock];
    const int row = blockIdx.x, t = threadIdx.x;
    const RowView rv = row_view(r, row);
    const int begin = blockIdx.y * kHistChunk, end = min(begin + kHistChunk, rv.V);
    u64 lo = 0, hi = 0;  // the largest inverted key, the largest key
    for (int base = begin; base < end; base += kLoads * kBlock) {
        double v[kLoads];
        load_values(rv, base, end, v);
#pragma unroll
        for (int k = 0; k < kLoads; ++k) {
            if (!is_finite(v[k])) continue;
            const u64 key = order_key(v[k]);
            lo = max(lo, ~key), hi = max(hi, key);
        }
    }
    s_lo[t] = lo, s_hi[t] = hi;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) s_lo[t] = max(s_lo[t], s_lo[t + s]), s_hi[t] = max(s_hi[t], s_hi[t + s]);
        __syncthreads();
    }
    if (t == 0 && s_hi[0] != 0) {
        atomicMax(&range[2 * (size_t)row], s_lo[0]);
        atomicMax(&range[2 * (size_t)row + 1], s_hi[0]);
    }
}

__global__ __launch_bounds__(kBlock) void k_hist_counts(HistRows r, const u64 *__restrict__ range, unsigned int *__restrict__ counts) {
    __shared__ unsigned int h[kHistBins];
    const int row = blockIdx.x, t = threadIdx.x, lane = t & 63;
    double lo, hi;
    if (!row_range(range, row, lo, hi)) return;  // the whole workgroup: the row's counters stay zero and the table kernel leaves the row unchanged
    const double w = (hi - lo) / (double)kHistBins;
    const RowView rv = row_view(r, row);
    const int begin = blockIdx.y * kHistChunk, end = min(begin + kHistChunk, rv.V);
    h[t] = 0;
    __syncthreads();
    for (int base = begin; base < end; base += kLoads * kBlock) {  // the same trip count for every lane: the ballots below see whole wavefronts
        double v[kLoads], m[kLoads];
        load_values(rv, base, end, v);
        load_masks(rv, base, end, m);
#pragma unroll
        for (int k = 0; k < kLoads; ++k) {
            int bin = counted(v[k], m[k]) ? hist_bin(v[k], lo, w) - 1 : -1;
            for (int round = 0; round < 2; ++round) {
                const u64 live = __ballot(bin >= 0);
                if (!live) break;
                const int leader = __ffsll((long long)live) - 1;
                const int lead = __shfl(bin, leader);
                const u64 same = __ballot(bin == lead);
                if (lane == leader) atomicAdd(&h[lead], (unsigned int)__popcll(same));
                if (bin == lead) bin = -1;
            }
            if (bin >= 0) atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    if (h[t]) atomicAdd(&counts[(size_t)row * kHistBins + t], h[t]);
}

// inclusive prefix sums of the 256 counters in LDS (every lane one counter)
__device__ __forceinline__ void scan_counts(unsigned int *c) {
    const int t = threadIdx.x;
    for (int off = 1; off < kHistBins; off <<= 1) {
        const unsigned int a = t >= off ? c[t - off] : 0u;
        __syncthreads();
        c[t] += a;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void k_hist_table(HistRows r, const u64 *__restrict__ range, const unsigned int *__restrict__ counts,
                                                       double *__restrict__ table, int32_t *__restrict__ flag) {
    __shared__ unsigned int cx[kHistBins], cy[kHistBins];
    __shared__ double cdf_y[kHistBins];
    const int row = blockIdx.x, t = threadIdx.x;
    const int yrow = r.n_src * r.D + row % r.D;
    cx[t] = counts[(size_t)row * kHistBins + t];
    cy[t] = counts[(size_t)yrow * kHistBins + t];
    __syncthreads();
    scan_counts(cx);
    scan_counts(cy);
    const unsigned int nx = cx[kHistBins - 1], ny = cy[kHistBins - 1];
    double lo_x, hi_x, lo_y = 0.0, hi_y = 0.0;
    const bool rx = row_range(range, row, lo_x, hi_x), ry = row_range(range, yrow, lo_y, hi_y);
    if (!rx || !ry || nx == 0 || ny == 0) {  // the same for every lane
        table[(size_t)row * kHistBins + t] = 0.0;
        if (t == 0) flag[row] = 0;
        return;
    }
    const double w_y = (hi_y - lo_y) / (double)kHistBins;
    cdf_y[t] = (double)cy[t] / (double)ny;
    __syncthreads();
    const double c = (double)cx[t] / (double)nx;
    int newbin = kHistBins;
    double dist = 0.0;
    if (t < kHistBins - 1) {
        int a = 0, b = kHistBins - 1;  // the smallest j with cdf_y[j] >= c lies in [a, b]: cdf_y[255] is exactly 1 >= c
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (cdf_y[mid] >= c) b = mid;
            else a = mid + 1;
        }
        newbin = a + 1;
        if (newbin > 1) dist = (c - cdf_y[a - 1]) / (cdf_y[a] - cdf_y[a - 1]);
    }
    double v = lo_y + (double)(newbin - 1) * w_y + dist * w_y;
    v = v < lo_y ? lo_y : (v > hi_y ? hi_y : v);
    table[(size_t)row * kHistBins + t] = v;
    if (t == 0) flag[row] = 1;
}

__global__ __launch_bounds__(kBlock) void k_hist_apply(HistRows r, const u64 *__restrict__ range, const double *__restrict__ table,
                                                       const int32_t *__restrict__ flag, double *out) {  // out may be the source rows themselves
    __shared__ double tab[kHistBins];
    const int row = blockIdx.x, t = threadIdx.x;
    const RowView rv = row_view(r, row);  // a source row: the grid has n_src * D of them
    const int begin = blockIdx.y * kHistChunk, end = min(begin + kHistChunk, rv.V);
    double *o = out + (size_t)row * r.Vs;
    double lo, hi;
    if (!flag[row] || !row_range(range, row, lo, hi)) {  // left unchanged
        if (o != rv.x)
            for (int i = begin + t; i < end; i += kBlock) o[i] = rv.x[i];
        return;
    }
    const double w = (hi - lo) / (double)kHistBins;
    tab[t] = table[(size_t)row * kHistBins + t];
    __syncthreads();
    for (int base = begin; base < end; base += kLoads * kBlock) {
        double v[kLoads], m[kLoads];
        load_values(rv, base, end, v);
        load_masks(rv, base, end, m);
#pragma unroll
        for (int k = 0; k < kLoads; ++k) {
            const int i = base + k * kBlock + t;
            if (i < end && counted(v[k], m[k])) o[i] = tab[hist_bin(v[k], lo, w) - 1];
            else if (i < end && o != rv.x) o[i] = v[k];
        }
    }
}

dim3 row_grid(int rows, int V) { return dim3((unsigned)rows, (unsigned)((V + kHistChunk - 1) / kHistChunk)); }

}  // namespace

int launch_hist_range(msm_ctx *ctx, const HistRows &rows, unsigned long long *d_range) {
    const int R = rows.n_src * rows.D + rows.D;
    hipLaunchKernelGGL(k_hist_range, row_grid(R, std::max(rows.Vs, rows.Vt)), dim3(kBlock), 0, ctx->stream, rows, d_range);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_hist_counts(msm_ctx *ctx, const HistRows &rows, const unsigned long long *d_range, unsigned int *d_counts) {
    const int R = rows.n_src * rows.D + rows.D;
    hipLaunchKernelGGL(k_hist_counts, row_grid(R, std::max(rows.Vs, rows.Vt)), dim3(kBlock), 0, ctx->stream, rows, d_range, d_counts);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_hist_table(msm_ctx *ctx, const HistRows &rows, const unsigned long long *d_range, const unsigned int *d_counts, double *d_table, int32_t *d_flag) {
    hipLaunchKernelGGL(k_hist_table, dim3((unsigned)(rows.n_src * rows.D)), dim3(kBlock), 0, ctx->stream, rows, d_range, d_counts, d_table, d_flag);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_hist_apply(msm_ctx *ctx, const HistRows &rows, const unsigned long long *d_range, const double *d_table, const int32_t *d_flag, double *d_out) {
    hipLaunchKernelGGL(k_hist_apply, row_grid(rows.n_src * rows.D, rows.Vs), dim3(kBlock), 0, ctx->stream, rows, d_range, d_table, d_flag, d_out);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
