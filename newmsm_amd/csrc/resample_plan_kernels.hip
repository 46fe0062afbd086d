// resample_plan_kernels.hip -- applying the rows of a resampling plan (resample_plan.cpp) to many maps, and the label vote.
//
// An apply is a sparse-times-dense product: 3 to about 15 entries per row (hundreds going fine to coarse), up to thousands of maps.  k_apply_rows
// (resample_kernels.hip) gives every (map, vertex) a thread, so the row is read again for every map and every entry is a scattered 8-byte look-up.
// Here the maps are taken kPlanTile at a time:
//   k_plan_tile_in    the tile, nd x nOld map-major, becomes nOld x kPlanTile vertex-major through an LDS tile (both sides coalesced)
//   k_plan_rows       a wavefront per output row, lane j owns map j: the row's (col, val) are wave-uniform (read once per tile), every entry costs the
//                     wavefront ONE contiguous line of kPlanTile elements, and no value crosses lanes -- the stored order of the sum is kept for free
//   k_plan_tile_out   the result, nNew x kPlanTile, goes back to nd x nNew map-major
// The alternative -- a lane group per row with kPlanTile accumulators in registers reading data[(d0 + j) * nOld + col] from the map-major tile -- saves the
// two transposes and turns every entry into kPlanTile scattered look-ups again.
// Arithmetic (msmhip.h): acc = 0.0, acc += (double)x * val per kept entry in stored order, product and sum rounded separately (-ffp-contract=off), the
// result stored as T.  A smoothing plan's rows (smooth_plan_kernels.hip) divide the sum by the row's divisor first.  No atomics: two runs give the same bits.
#include "resample_plan.hpp"

namespace msm {
namespace {

constexpr int TD = kPlanTile;
static_assert(TD == 64, "a wavefront's lanes are the maps of a tile");

// src: nd rows of V values (row stride V) -> dst: V rows of TD values, columns [0, nd) written
template <typename T>
__global__ __launch_bounds__(256) void k_plan_tile_in(const T *__restrict__ src, int nd, int V, T *__restrict__ dst) {
    __shared__ T tile[TD][TD + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int v0 = blockIdx.x * TD;
    for (int r = ty; r < TD; r += 4) {  // row r of the tile = map r, along the vertices
        const int v = v0 + tx;
        if (r < nd && v < V) tile[r][tx] = src[(size_t)r * V + v];
    }
    __syncthreads();
    for (int r = ty; r < TD; r += 4) {  // vertex v0 + r, along the maps
        const int v = v0 + r;
        if (tx < nd && v < V) dst[(size_t)v * TD + tx] = tile[tx][r];
    }
}

// src: V rows of TD values -> dst: nd rows of V values
template <typename T>
__global__ __launch_bounds__(256) void k_plan_tile_out(const T *__restrict__ src, int nd, int V, T *__restrict__ dst) {
    __shared__ T tile[TD][TD + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int v0 = blockIdx.x * TD;
    for (int r = ty; r < TD; r += 4) {
        const int v = v0 + r;
        if (tx < nd && v < V) tile[r][tx] = src[(size_t)v * TD + tx];
    }
    __syncthreads();
    for (int r = ty; r < TD; r += 4) {
        const int v = v0 + tx;
        if (r < nd && v < V) dst[(size_t)r * V + v] = tile[tx][r];
    }
}

// one wavefront per output row; tin: nOld x TD, tout: nNew x TD.  Div: a smoothing plan's rows, whose sum is divided by the row's divisor where that is
// not 0.0 (one FP64 division, k_smooth's; kernels.hip) -- a compile-time variant, so the other methods run the code they ran before there was one
template <typename T, bool Div>
__global__ __launch_bounds__(256) void k_plan_rows(PlanRows p, int nd, const T *__restrict__ tin, T *__restrict__ tout) {
    const int lane = threadIdx.x & 63;
    const int k = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (k >= p.nNew) return;
    const int b = p.row_ptr[k], end = p.row_ptr[k + 1];
    const bool live = lane < nd;
    double acc = 0.0;
    int e = b;
    // four entries at a time: their lines are requested together, the sum still runs in stored order
    for (; e + 4 <= end; e += 4) {
        int c[4];
        double w[4], x[4];
        bool keep[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            c[u] = p.col[e + u];
            w[u] = p.val[e + u];
            keep[u] = c[u] >= 0 && c[u] < p.nOld && (!p.excl || p.excl[c[u]] != 0.0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = (keep[u] && live) ? (double)tin[(size_t)c[u] * TD + lane] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (keep[u]) acc += x[u] * w[u];
    }
    for (; e < end; ++e) {
        const int c = p.col[e];
        const double w = p.val[e];
        if (!(c >= 0 && c < p.nOld && (!p.excl || p.excl[c] != 0.0))) continue;
        const double x = live ? (double)tin[(size_t)c * TD + lane] : 0.0;
        acc += x * w;
    }
    if constexpr (Div) {
        const double dv = p.row_div[k];
        if (dv != 0.0) acc = acc / dv;
    }
    if (live) tout[(size_t)k * TD + lane] = (T)acc;
}

// The vote: a group of 16 lanes per (row of keys, output vertex).  A lane takes every 16th entry as a candidate; a candidate that is the first kept
// entry with its key sums the weights of that key over the rest of the row in stored order (the entries before it do not hold the key: the same sum as
// over the whole row).  Quadratic in the row length, which is a few to a few hundred entries; correct for any length.
constexpr int kVoteLanes = 16;
__global__ __launch_bounds__(256) void k_plan_labels(PlanRows p, const int32_t *__restrict__ labels, long long items, int32_t unassigned, int32_t *__restrict__ out) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, item = gid / kVoteLanes;
    const int sub = (int)(gid % kVoteLanes);
    const bool live = item < items;
    const long long d = live ? item / p.nNew : 0;
    const int k = live ? (int)(item - d * p.nNew) : 0;
    const int32_t *lab = labels + (size_t)d * p.nOld;
    const int b = live ? p.row_ptr[k] : 0, end = live ? p.row_ptr[k + 1] : 0;
    auto kept = [&](int c) { return c >= 0 && c < p.nOld && (!p.excl || p.excl[c] != 0.0); };
    bool have = false;
    double best = 0.0;
    int32_t best_key = 0;
    for (int i = b + sub; i < end; i += kVoteLanes) {
        const int c = p.col[i];
        if (!kept(c)) continue;
        const int32_t key = lab[c];
        bool seen = false;
        for (int j = b; j < i && !seen; ++j) {
            const int cj = p.col[j];
            seen = kept(cj) && lab[cj] == key;
        }
        if (seen) continue;
        double s = 0.0;
        for (int j = i; j < end; ++j) {
            const int cj = p.col[j];
            if (kept(cj) && lab[cj] == key) s += p.val[j];
        }
        if (!have || s > best || (s == best && key < best_key)) have = true, best = s, best_key = key;
    }
    // every lane of the wavefront arrives here; the groups are aligned runs of 16 lanes
    for (int m = kVoteLanes / 2; m >= 1; m >>= 1) {
        const int o_have = __shfl_xor((int)have, m);
        const double o_best = __shfl_xor(best, m);
        const int32_t o_key = __shfl_xor(best_key, m);
        if (o_have && (!have || o_best > best || (o_best == best && o_key < best_key))) have = true, best = o_best, best_key = o_key;
    }
    if (live && sub == 0) out[(size_t)d * p.nNew + k] = have ? best_key : unassigned;
}

}  // namespace

template <typename T>
int launch_plan_tile(msm_ctx *ctx, const PlanRows &r, const T *d_data, int nd, T *d_tin, T *d_tout, T *d_out) {
    if (nd <= 0 || r.nNew <= 0) return MSM_OK;
    if (nd > TD) return fail(MSM_ERR_INVALID, "resampling plan: a tile holds %d maps, %d asked for", TD, nd);
    if (r.nOld > 0) hipLaunchKernelGGL(k_plan_tile_in<T>, dim3((unsigned)((r.nOld + TD - 1) / TD)), dim3(256), 0, ctx->stream, d_data, nd, r.nOld, d_tin);
    if (r.row_div) hipLaunchKernelGGL((k_plan_rows<T, true>), dim3((unsigned)((r.nNew + 3) / 4)), dim3(256), 0, ctx->stream, r, nd, (const T *)d_tin, d_tout);
    else hipLaunchKernelGGL((k_plan_rows<T, false>), dim3((unsigned)((r.nNew + 3) / 4)), dim3(256), 0, ctx->stream, r, nd, (const T *)d_tin, d_tout);
    hipLaunchKernelGGL(k_plan_tile_out<T>, dim3((unsigned)((r.nNew + TD - 1) / TD)), dim3(256), 0, ctx->stream, (const T *)d_tout, nd, r.nNew, d_out);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}
template int launch_plan_tile<float>(msm_ctx *, const PlanRows &, const float *, int, float *, float *, float *);
template int launch_plan_tile<double>(msm_ctx *, const PlanRows &, const double *, int, double *, double *, double *);

int launch_plan_labels(msm_ctx *ctx, const PlanRows &r, const int32_t *d_labels, int D, int32_t unassigned, int32_t *d_out) {
    const long long items = (long long)D * r.nNew;
    if (items <= 0) return MSM_OK;
    const long long blocks = (items * kVoteLanes + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(MSM_ERR_INVALID, "resampling plan: %lld label items in one launch", items);
    hipLaunchKernelGGL(k_plan_labels, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, r, d_labels, items, unassigned, d_out);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
