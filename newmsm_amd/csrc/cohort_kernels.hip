// cohort_kernels.hip -- the post-processing of a cohort registered to one template on gfx950 (gMSM_scripts/newMSM_HCP_to_template_v2.sh runs
// wb_command -surface-distortion per subject, get_group_stats.py / compare_stats.py summarise the maps with numpy).
//
//   k_triangle_distortion  one lane per (triangle, subject): J and R of triangle_strain (strain_device.hpp) of the original triangle against the
//                          subject's deformed one, their log2.  Every triangle is evaluated once.
//   k_vertex_gather        one lane per (vertex, subject): the plain mean of its incident triangles' two values in trID order -- the sum
//                          k_vertex_distortion (dedrift_kernels.hip) forms, from the same values in the same order: the same bits.
//   k_abs_partials         workgroup b: the sum of |x| over its strided share as a fixed tree; the largest key (integer atomicMax).
//   k_abs_hist / k_abs_pick  one pass of a radix select over an order-preserving integer key, eight bits at a time from the top, across workgroups:
//                          256-bin integer histograms in LDS, flushed to integer counters in HBM; then one workgroup picks each order statistic's bin.
//   k_abs_next             the next order statistic: how many keys are <= the selected one, and the smallest larger key.
//   k_abs_finish           one workgroup: the partial sums in a fixed tree, the interpolation numpy.percentile does (k_dedrift_masks' arithmetic).
//
// No floating-point atomics anywhere: every floating-point sum has a fixed shape, two runs give the same bits.
#include "cohort.hpp"
#include "reduce_device.hpp"
#include "strain_device.hpp"

namespace msm {

namespace {

constexpr int kBlock = kSumBlock;

__global__ __launch_bounds__(kBlock) void k_triangle_distortion(const double *__restrict__ m, const double *__restrict__ fin, int V,
                                                                const int32_t *__restrict__ tri, int T, int S, double *__restrict__ tl) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (t >= T) return;
    const double *c = fin + (size_t)s * 3 * V;
    V3 o[3], f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int id = tri[(size_t)k * T + t];
        o[k] = mk(m[id], m[(size_t)V + id], m[2 * (size_t)V + id]);
        f[k] = mk(c[id], c[(size_t)V + id], c[2 * (size_t)V + id]);
    }
    double J, R;
    triangular_strain_JR(strain_frame(o), f, J, R);
    tl[(size_t)s * T + t] = log2(J);
    tl[((size_t)S + s) * T + t] = log2(R);
}

__global__ __launch_bounds__(kBlock) void k_vertex_gather(const double *__restrict__ tl, int V, int T, int S, const int32_t *__restrict__ tid_ptr,
                                                          const int32_t *__restrict__ tid, double *__restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (v >= V) return;
    const double *lj = tl + (size_t)s * T, *lr = tl + ((size_t)S + s) * T;
    const int e0 = tid_ptr[v], e1 = tid_ptr[v + 1];
    double sj = 0.0, sr = 0.0;
    for (int e = e0; e < e1; ++e) {
        const int t = tid[e];
        sj += lj[t];
        sr += lr[t];
    }
    const int n = e1 - e0;
    double *o = out + (size_t)s * 2 * V;
    o[v] = n > 0 ? sj / n : 0.0;
    o[(size_t)V + v] = n > 0 ? sr / n : 0.0;
}

// |x| as an integer with the order of the values: the bits without the sign.  Every NaN lies above the key of infinity.
__device__ __forceinline__ unsigned long long abs_key(double x) { return (unsigned long long)__double_as_longlong(x) & 0x7fffffffffffffffull; }
__device__ __forceinline__ double key_value(unsigned long long k) { return __longlong_as_double((long long)k); }
constexpr unsigned long long kInfKey = 0x7ff0000000000000ull;

__global__ __launch_bounds__(kBlock) void k_abs_partials(const double *__restrict__ x, size_t n, double *__restrict__ partial, SummaryCounters c,
                                                         const long long *__restrict__ k, int np) {
    __shared__ double lds[kBlock];
    __shared__ unsigned long long s_max;
    const int t = threadIdx.x;
    if (t == 0) s_max = 0;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * kBlock;
    double a = 0.0;
    unsigned long long mx = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + t; i < n; i += stride) {
        const unsigned long long key = abs_key(x[i]);
        a += key_value(key);
        mx = key > mx ? key : mx;
    }
    const double sum = block_sum(a, lds);
    atomicMax(&s_max, mx);
    __syncthreads();
    if (t == 0) {
        partial[blockIdx.x] = sum;
        atomicMax(c.maxkey, s_max);
    }
    if (blockIdx.x == 0 && t < np) c.krem[t] = (unsigned long long)k[t], c.mn[t] = ~0ull;
}

__global__ __launch_bounds__(kBlock) void k_abs_hist(const double *__restrict__ x, size_t n, SummaryCounters c, int np, int pass) {
    __shared__ unsigned int hist[kSummaryMaxPercentiles * 256];
    __shared__ unsigned long long prefix[kSummaryMaxPercentiles];
    const int t = threadIdx.x, shift = 56 - 8 * pass;
    for (int i = t; i < np * 256; i += kBlock) hist[i] = 0;
    if (t < np) prefix[t] = c.prefix[t];
    __syncthreads();
    const unsigned long long himask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + t; i < n; i += stride) {  // (a workgroup's share is under 2^32 values: 32-bit LDS counters suffice below 2^50 values)
        const unsigned long long key = abs_key(x[i]);
        const int bin = (int)((key >> shift) & 255);
        for (int q = 0; q < np; ++q)
            if ((key & himask) == prefix[q]) atomicAdd(&hist[q * 256 + bin], 1u);
    }
    __syncthreads();
    for (int i = t; i < np * 256; i += kBlock)
        if (hist[i]) atomicAdd(&c.hist[i], (unsigned long long)hist[i]);
}

// order statistic q: the bin that holds the krem[q]-th key (0-based) among those that share its prefix; the counters are zeroed for the next pass
__global__ __launch_bounds__(kBlock) void k_abs_pick(SummaryCounters c, int np, int pass) {
    const int t = threadIdx.x, shift = 56 - 8 * pass;
    if (t < np) {
        unsigned long long cum = 0;
        const unsigned long long kk = c.krem[t];
        for (int b = 0; b < 256; ++b) {
            const unsigned long long h = c.hist[t * 256 + b];
            if (cum + h > kk) {
                c.prefix[t] |= (unsigned long long)b << shift;
                c.krem[t] = kk - cum;
                break;
            }
            cum += h;
        }
    }
    __syncthreads();
    for (int i = t; i < np * 256; i += kBlock) c.hist[i] = 0;
}

__global__ __launch_bounds__(kBlock) void k_abs_next(const double *__restrict__ x, size_t n, SummaryCounters c, int np) {
    __shared__ unsigned long long lo[kSummaryMaxPercentiles], s_cnt[kSummaryMaxPercentiles], s_min[kSummaryMaxPercentiles];
    const int t = threadIdx.x;
    if (t < np) lo[t] = c.prefix[t], s_cnt[t] = 0, s_min[t] = ~0ull;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (int q = 0; q < np; ++q) {
        const unsigned long long lo_key = lo[q];
        unsigned long long cnt = 0, mn = ~0ull;
        for (size_t i = (size_t)blockIdx.x * kBlock + t; i < n; i += stride) {
            const unsigned long long key = abs_key(x[i]);
            if (key <= lo_key)
                ++cnt;
            else if (key < mn)
                mn = key;
        }
        if (cnt) atomicAdd(&s_cnt[q], cnt);
        atomicMin(&s_min[q], mn);
    }
    __syncthreads();
    if (t < np) {
        atomicAdd(&c.cnt[t], s_cnt[t]);
        atomicMin(&c.mn[t], s_min[t]);
    }
}

__global__ __launch_bounds__(kBlock) void k_abs_finish(const double *__restrict__ partial, int blocks, size_t n, SummaryCounters c,
                                                       const long long *__restrict__ k, const double *__restrict__ gamma, int np, double *__restrict__ out) {
    __shared__ double lds[kBlock];
    const int t = threadIdx.x;
    double a = 0.0;
    for (int b = t; b < blocks; b += kBlock) a += partial[b];
    const double sum = block_sum(a, lds);
    const unsigned long long maxkey = *c.maxkey;
    const bool nan = maxkey > kInfKey;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (t == 0) out[0] = nan ? qnan : sum / (double)n, out[1] = nan ? qnan : key_value(maxkey);
    if (t < np) {
        const unsigned long long kk = (unsigned long long)k[t], lo_key = c.prefix[t];
        // the next order statistic: the same value when more than k + 1 values are <= it, the smallest larger value otherwise
        const unsigned long long hi_key = (kk + 1 >= n || c.cnt[t] > kk + 1) ? lo_key : c.mn[t];
        // numpy's _lerp: a + (b - a) t, and b - (b - a) (1 - t) from t = 0.5 on
        const double lo = key_value(lo_key), hi = key_value(hi_key), diff = hi - lo, g = gamma[t];
        out[2 + t] = nan ? qnan : (g >= 0.5 ? hi - diff * (1 - g) : lo + diff * g);
    }
}

}  // namespace

int launch_triangle_distortion(msm_ctx *ctx, const double *d_orig, const double *d_fin, int V, const int32_t *d_tri, int T, int S, double *d_tl) {
    if (T <= 0 || S <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_triangle_distortion, dim3((T + kBlock - 1) / kBlock, S), dim3(kBlock), 0, ctx->stream, d_orig, d_fin, V, d_tri, T, S, d_tl);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_vertex_gather(msm_ctx *ctx, const double *d_tl, int V, int T, int S, const int32_t *d_tid_ptr, const int32_t *d_tid, double *d_out) {
    if (V <= 0 || S <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_vertex_gather, dim3((V + kBlock - 1) / kBlock, S), dim3(kBlock), 0, ctx->stream, d_tl, V, T, S, d_tid_ptr, d_tid, d_out);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_abs_partials(msm_ctx *ctx, const double *d_x, int64_t n, int blocks, double *d_partial, SummaryCounters c, const long long *d_k, int np) {
    hipLaunchKernelGGL(k_abs_partials, dim3(blocks), dim3(kBlock), 0, ctx->stream, d_x, (size_t)n, d_partial, c, d_k, np);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_abs_select_pass(msm_ctx *ctx, const double *d_x, int64_t n, int blocks, SummaryCounters c, int np, int pass) {
    if (np <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_abs_hist, dim3(blocks), dim3(kBlock), 0, ctx->stream, d_x, (size_t)n, c, np, pass);
    MSM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_abs_pick, dim3(1), dim3(kBlock), 0, ctx->stream, c, np, pass);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_abs_next(msm_ctx *ctx, const double *d_x, int64_t n, int blocks, SummaryCounters c, int np) {
    if (np <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_abs_next, dim3(blocks), dim3(kBlock), 0, ctx->stream, d_x, (size_t)n, c, np);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_abs_finish(msm_ctx *ctx, const double *d_partial, int blocks, int64_t n, SummaryCounters c, const long long *d_k, const double *d_gamma, int np,
                      double *d_out) {
    hipLaunchKernelGGL(k_abs_finish, dim3(1), dim3(kBlock), 0, ctx->stream, d_partial, blocks, (size_t)n, c, d_k, d_gamma, np, d_out);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
