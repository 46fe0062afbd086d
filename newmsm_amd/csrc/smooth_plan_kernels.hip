// smooth_plan_kernels.hip -- the rows of a smoothing plan (msm_resample_plan_create_smooth, resample_plan.cpp) built on the device.
//
// smooth_data (R/resampler.cpp:168-230) is a sparse row operator: output vertex i takes the vertices n of sphLow whose unit vector lies within
// ang = 4 asin(sigma / 2R) of the centre's, each with a Gaussian of its geodesic distance, and divides by the summed weights.  The rows depend on the
// sphere and sigma alone, so they are built once -- k_smooth (kernels.hip) redoes the sweep below on every call.
//   k_smooth_plan_count   a wavefront per output vertex: the pruned sweep of k_smooth (64 chunk balls per ballot, surviving chunks in ascending order),
//                         counting the members -> the row's length
//   (host)                the lengths are summed in 64 bits, the arrays sized, launch_scan_exclusive turns the lengths into row offsets
//   k_smooth_plan_fill    the same sweep again: (col, val) written by ballot-prefix compaction, so a row is in ascending n; div and excl_out are the
//                         sums of the row's weights IN STORED ORDER from 0.0 -- the members of a chunk are added one after the other, lowest lane
//                         first, every lane holding the same running sum (no tree: the order is k_smooth's, and with it the bits)
// The expressions are smooth_device.hpp's, shared with k_smooth.  Every loop is bounded by the number of chunks or by 64 members of a chunk; nothing
// waits for another wavefront, nothing is accumulated in memory, no LDS.  The one atomic is the status word's on the error path (raise_status, as
// everywhere in the library).
#include "resample_plan.hpp"
#include "smooth_device.hpp"

namespace msm {
namespace {

__device__ __forceinline__ void raise_status(int *status, int code) { atomicMin(status, code); }

// the value lane l holds (l wave-uniform)
__device__ __forceinline__ double lane_value(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// The centre of output vertex i, validated as k_smooth does: -1 for an id outside [0, N) (status raised, nothing indexed with it) or an excluded
// centre (:200) -- both give an empty row.
__device__ __forceinline__ int smooth_centre(const SmoothRows &s, int i, int lane, int *status) {
    const int c = s.cv[i];
    if (c < 0 || c >= s.N) {
        if (lane == 0 && status) raise_status(status, c < 0 ? c : MSM_ERR_INVALID);
        return -1;
    }
    if (s.excl && !(s.excl[c] > 0)) return -1;
    return c;
}

// k_smooth's sweep for one centre; f(n, in, chord, bal) is called by the whole wavefront for every surviving chunk that holds a member: lane's vertex
// n, whether it is a member, its chord to the centre, the members' ballot
template <class F>
__device__ __forceinline__ void smooth_sweep(const SmoothRows &s, const V3 &ref, int lane, F f) {
    const int N = s.N, nchunks = (N + 63) >> 6;
    for (int c0 = 0; c0 < nchunks; c0 += 64) {
        bool cand = false;
        if (c0 + lane < nchunks) cand = smooth_chunk_candidate(s.cb[c0 + lane], ref, s.cosang);
        unsigned long long todo = __ballot(cand);
        while (todo) {
            const int n = ((c0 + __ffsll((long long)todo) - 1) << 6) + lane;
            todo &= todo - 1ull;
            bool in = false;
            double chord = 0.0;
            if (n < N) {
                const V3 a = mk(s.unit[n], s.unit[N + n], s.unit[2 * (size_t)N + n]);
                in = smooth_member(a, ref, s.cosang);
                if (in) chord = smooth_chord(ref, a);
            }
            const unsigned long long bal = __ballot(in);
            if (bal) f(n, in, chord, bal);
        }
    }
}

__global__ __launch_bounds__(256) void k_smooth_plan_count(SmoothRows s, int *__restrict__ row_len, int *status) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (i >= s.N) return;
    const int c = smooth_centre(s, i, lane, status);
    int count = 0;
    if (c >= 0) {
        const V3 ref = mk(s.unit[c], s.unit[s.N + c], s.unit[2 * (size_t)s.N + c]);
        smooth_sweep(s, ref, lane, [&](int, bool, double, unsigned long long bal) { count += __popcll(bal); });
    }
    if (lane == 0) row_len[i] = count;
}

__global__ __launch_bounds__(256) void k_smooth_plan_fill(SmoothRows s, const int *__restrict__ row_ptr, int *__restrict__ col, double *__restrict__ val,
                                                           double *__restrict__ div, double *__restrict__ excl_out) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (i >= s.N) return;
    const int c = smooth_centre(s, i, lane, nullptr);  // the count pass has raised what there is to raise
    double SUM = 0.0, excl_sum = 0.0;
    if (c >= 0) {
        const V3 ref = mk(s.unit[c], s.unit[s.N + c], s.unit[2 * (size_t)s.N + c]);
        const double gain = smooth_gain(s.sigma);
        const int end = row_ptr[i + 1];
        int at = row_ptr[i];
        smooth_sweep(s, ref, lane, [&](int n, bool in, double chord, unsigned long long bal) {
            double w = 0.0, kept = 0.0;
            if (in) {
                w = smooth_weight(chord, gain, s.sigma);
                kept = s.excl ? s.excl[n] * w : w;  // :208: the mask is part of the stored weight
                const int pos = at + __popcll(bal & ((1ull << lane) - 1ull));
                if (pos < end) col[pos] = n, val[pos] = kept;  // the two sweeps agree; a row never writes past its own end
            }
            at += __popcll(bal);
            for (unsigned long long m = bal; m; m &= m - 1ull) {  // the members in ascending n: the stored order
                const int l = __ffsll((long long)m) - 1;
                excl_sum += lane_value(w, l);
                SUM += lane_value(kept, l);
            }
        });
    }
    if (lane == 0) {
        div[i] = SUM;  // 0.0: an apply does not divide (an empty row, or weights that sum to nothing)
        if (excl_out) excl_out[i] = (c >= 0 && excl_sum != 0.0) ? SUM / excl_sum : 0.0;
    }
}

}  // namespace

int launch_smooth_plan_count(msm_ctx *ctx, const SmoothRows &s, int *d_row_len) {
    if (s.N <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_smooth_plan_count, dim3((unsigned)((s.N + 3) / 4)), dim3(256), 0, ctx->stream, s, d_row_len, ctx->d_status);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_smooth_plan_fill(msm_ctx *ctx, const SmoothRows &s, const int *d_row_ptr, int *d_col, double *d_val, double *d_div, double *d_excl_out) {
    if (s.N <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_smooth_plan_fill, dim3((unsigned)((s.N + 3) / 4)), dim3(256), 0, ctx->stream, s, d_row_ptr, d_col, d_val, d_div, d_excl_out);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
