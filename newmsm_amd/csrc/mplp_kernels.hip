// mplp_kernels.hip -- the MPLP optimiser's kernels (mplp.hpp; the definition and the serial literal: mplp_host.hpp).
//
// A sweep updates the factors in list order; a factor reads the messages of the other factors on its three nodes and writes its own.  The host has
// sorted the factors into levels whose members share no node (mcmc_build_schedule), so a level is one launch, a workgroup per factor, and whatever the
// workgroups of a launch do among themselves every factor sees the messages the serial sweep would show it.
//
// k_mplp_update: the three cavities (3 L sums over the nodes' incidence lists, in list order) go to LDS; the factor's L^3 entries are then streamed once,
// coalesced along c, each entry v = ((theta + d0[a]) + d1[b]) + d2[c] lowering three running minima in LDS.  The minima are kept as 64-bit integer keys
// that order like the doubles they stand for, so the LDS's integer minimum serves; a minimum is exact, so the order in which the lanes arrive changes no
// bit but the sign of a zero, which `+ 0.0` removes as it does in the literal.  Arithmetic is the literal's and nothing else: the file is built with
// -ffp-contract=off and the division is the correctly rounded one.
//
// What the kernel is shaped by (DESIGN.md 5.19 has the measurements): a level is a chain of dependent latencies -- incidence offsets, slots, messages,
// then the table -- and a wavefront's 64 entries mostly share one a and a few b, so 64 lanes lowering M0[a] in one LDS instruction serialise.  Hence (1)
// the first table entries of every thread are requested before the cavities are formed and the next ones while the current ones are folded in; (2) a
// node's slots and then its messages are loaded eight at a time, independent of one another, and added in list order afterwards; (3) every minimum has
// `slots` copies in LDS, lane l lowering copy l % slots (a padded row per minimum: the lanes of one instruction hit distinct banks), folded into one
// when the table is through.  slots is the largest power of two up to 64 that keeps the factor's LDS within 64 KB: 64 up to 41 labels, 1 from 683.
#include <climits>
#include <cstdlib>

#include "mplp.hpp"

namespace msm {

namespace {

__device__ __forceinline__ void raise_status(int *status, int code) { atomicMin(status, code); }

// doubles to integers of the same order (-0.0 below +0.0) and back: the map is its own inverse
__device__ __forceinline__ long long order_key(long long b) { return b ^ ((b >> 63) & 0x7fffffffffffffffLL); }
__device__ __forceinline__ long long key_of(double v) { return order_key(__double_as_longlong(v)); }
__device__ __forceinline__ double value_of(long long k) { return __longlong_as_double(order_key(k)); }

// (a, b, c) of a flat index into an L x L x L block, advanced by a fixed step without a division per entry
struct Abc {
    unsigned a, b, c, sa, sb, sc, L;
    __device__ Abc(unsigned e, unsigned step, unsigned L_) : L(L_) {
        const unsigned L2 = L * L;
        a = e / L2, b = (e - a * L2) / L, c = e - a * L2 - b * L;
        sa = step / L2, sb = (step - sa * L2) / L, sc = step - sa * L2 - sb * L;
    }
    __device__ void advance() {
        c += sc;
        if (c >= L) c -= L, ++b;
        b += sb;
        if (b >= L) b -= L, ++a;
        a += sa;
    }
};

// theta_i(x) plus the messages over the incidence of node i in order, but for slot `skip` (-1: none).  Eight slots, then their eight messages, are
// loaded side by side; the additions follow in list order.
__device__ __forceinline__ double node_sum(const MplpArgs &a, unsigned i, unsigned x, int skip) {
    const int k0 = a.inc_ptr[i], k1 = a.inc_ptr[i + 1];
    double v = a.U[(size_t)x * (unsigned)a.N + i];
    for (int k = k0; k < k1; k += 8) {
        int q[8];
        double mv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = k + j < k1 ? a.inc_slot[k + j] : skip;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (q[j] != skip && (unsigned)q[j] >= 3u * (unsigned)a.T) {  // (the host built the lists: what is out of range indexes nothing)
                raise_status(a.status, MSM_ERR_INVALID);
                q[j] = skip;
            }
            mv[j] = q[j] != skip ? a.m[(size_t)q[j] * (unsigned)a.L + x] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (q[j] != skip) v += mv[j];
    }
    return v;
}

constexpr int kMplpBatch = 4;  // table entries a thread has in flight

__device__ __forceinline__ void load_batch(const double *__restrict__ th, unsigned e0, unsigned L3, double (&v)[kMplpBatch]) {
#pragma unroll
    for (int j = 0; j < kMplpBatch; ++j) {
        const unsigned e = e0 + (unsigned)j * kMplpThreads;
        v[j] = e < L3 ? th[e] : 0.0;
    }
}

__global__ __launch_bounds__(kMplpThreads) void k_mplp_update(MplpArgs a, int begin, int count, int sweep, int slots) {
    extern __shared__ __align__(16) double s_mplp[];  // 3 L cavities, then 3 L rows of `slots` minima as keys (a row padded by one when slots > 1)
    if (sweep > 0 && a.changed[sweep - 1] == 0) return;  // the run is at its fixed point (the whole launch)
    const unsigned tid = threadIdx.x, L = (unsigned)a.L, N = (unsigned)a.N;
    if ((int)blockIdx.x >= count) return;
    const int4 r = a.sched[begin + (int)blockIdx.x];  // {triplet, node A, node B, node C}
    if ((unsigned)r.x >= (unsigned)a.T || (unsigned)r.y >= N || (unsigned)r.z >= N || (unsigned)r.w >= N) {
        if (tid == 0) raise_status(a.status, MSM_ERR_INVALID);
        return;
    }
    const unsigned L3 = L * L * L;  // L <= 1024: at most 2^30
    const double *__restrict__ th = a.tc + (size_t)r.x * L3;
    double cur[kMplpBatch], nxt[kMplpBatch];
    load_batch(th, tid, L3, cur);  // under way while the cavities are formed
    double *d = s_mplp;
    long long *M = reinterpret_cast<long long *>(s_mplp + 3 * (size_t)L);
    const unsigned S = (unsigned)slots, stride = S > 1 ? S + 1 : 1, mine = tid & (S - 1);
    const long long inf_key = key_of(__longlong_as_double(0x7ff0000000000000LL));
    for (unsigned idx = tid; idx < 3 * L * stride; idx += kMplpThreads) M[idx] = inf_key;
    for (unsigned idx = tid; idx < 3 * L; idx += kMplpThreads) {
        const unsigned s = idx / L, x = idx - s * L;
        const unsigned node = s == 0 ? (unsigned)r.y : s == 1 ? (unsigned)r.z : (unsigned)r.w;
        d[idx] = node_sum(a, node, x, 3 * r.x + (int)s);
    }
    __syncthreads();
    Abc p(tid, kMplpThreads, L);
    for (unsigned e0 = tid; e0 < L3; e0 += kMplpBatch * kMplpThreads) {
        load_batch(th, e0 + kMplpBatch * kMplpThreads, L3, nxt);
#pragma unroll
        for (int j = 0; j < kMplpBatch; ++j) {
            if (e0 + (unsigned)j * kMplpThreads >= L3) break;
            const double v = ((cur[j] + d[p.a]) + d[L + p.b]) + d[2 * L + p.c];
            const long long k = key_of(v);
            atomicMin(&M[p.a * stride + mine], k);
            atomicMin(&M[(L + p.b) * stride + mine], k);
            atomicMin(&M[(2 * L + p.c) * stride + mine], k);
            p.advance();
        }
#pragma unroll
        for (int j = 0; j < kMplpBatch; ++j) cur[j] = nxt[j];
    }
    __syncthreads();
    double *__restrict__ out = a.m + (size_t)3 * r.x * L;  // slot s, label x at s * L + x
    bool moved = false;
    for (unsigned idx = tid; idx < 3 * L; idx += kMplpThreads) {
        long long lowest = M[idx * stride];
        for (unsigned j = 1; j < S; ++j) lowest = min(lowest, M[idx * stride + j]);
        const double nv = (value_of(lowest) + 0.0) / 3.0 - d[idx];
        moved |= __double_as_longlong(nv) != __double_as_longlong(out[idx]);
        out[idx] = nv;
    }
    if (moved) a.changed[sweep] = 1;
}

// a wavefront per node: lane l takes the labels l, l + 64, ...; the lowest belief, lowest label on ties, by shuffles
__global__ __launch_bounds__(256) void k_mplp_decode(MplpArgs a, int32_t *__restrict__ label, double *__restrict__ node_terms) {
    const unsigned lane = threadIdx.x & 63u, L = (unsigned)a.L;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (long)a.N) return;  // (the whole wavefront)
    double bv = 0.0;
    int bx = INT_MAX;  // no label yet
    for (unsigned x = lane; x < L; x += 64) {
        const double v = node_sum(a, (unsigned)i, x, -1);
        if (bx == INT_MAX || v < bv) bv = v, bx = (int)x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(bv, off);
        const int ox = __shfl_down(bx, off);
        if (ox != INT_MAX && (bx == INT_MAX || ov < bv || (ov == bv && ox < bx))) bv = ov, bx = ox;
    }
    if (lane == 0) {
        if (label) label[i] = bx;
        node_terms[i] = bv;
    }
}

__global__ __launch_bounds__(kMplpThreads) void k_mplp_factor_terms(MplpArgs a, double *__restrict__ factor_terms, int sweep) {
    extern __shared__ __align__(16) double s_mplp[];  // 3 L messages, then a minimum per wavefront
    if (sweep > 0 && a.changed[sweep - 1] == 0) return;
    const unsigned tid = threadIdx.x, L = (unsigned)a.L, t = blockIdx.x;
    if (t >= (unsigned)a.T) return;
    for (unsigned idx = tid; idx < 3 * L; idx += kMplpThreads) s_mplp[idx] = a.m[(size_t)3 * t * L + idx];
    __syncthreads();
    const unsigned L3 = L * L * L;
    const double *__restrict__ th = a.tc + (size_t)t * L3;
    double lo = __longlong_as_double(0x7ff0000000000000LL);
    Abc p(tid, kMplpThreads, L);
    for (unsigned e = tid; e < L3; e += kMplpThreads, p.advance()) {
        const double v = ((th[e] - s_mplp[p.a]) - s_mplp[L + p.b]) - s_mplp[2 * L + p.c];
        if (v < lo) lo = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(lo, off);
        if (o < lo) lo = o;
    }
    double *w = s_mplp + 3 * (size_t)L;
    if ((tid & 63u) == 0) w[tid >> 6] = lo;
    __syncthreads();
    if (tid == 0) {
        for (unsigned k = 1; k < kMplpThreads / 64; ++k)
            if (w[k] < lo) lo = w[k];
        factor_terms[t] = lo;  // (the sign of a zero minimum depends on the order; the sum it joins starts at +0.0 and does not see it)
    }
}

__global__ __launch_bounds__(256) void k_mplp_finite(const double *__restrict__ U, size_t nU, const double *__restrict__ tc, size_t ntc, int32_t *flags) {
    const size_t stride = (size_t)gridDim.x * 256;
    bool bad_u = false, bad_t = false;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < nU; j += stride) bad_u |= !(U[j] - U[j] == 0.0);
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < ntc; j += stride) bad_t |= !(tc[j] - tc[j] == 0.0);
    if (bad_u) flags[0] = 1;
    if (bad_t) flags[1] = 1;
}

int check_shape(const MplpArgs &a) {
    if (a.N <= 0 || a.L <= 0 || a.L > kMplpMaxLabels || a.T < 0) return fail(MSM_ERR_INVALID, "msm_mplp_optimise_gpu: bad launch (N %d, L %d, T %d)", a.N, a.L, a.T);
    return MSM_OK;
}

}  // namespace

// copies of every minimum in LDS: the largest power of two up to 64 with 3 L cavities and 3 L padded rows of copies within 64 KB.  MSMHIP_MPLP_SLOTS=n
// (testing) lowers it to a power of two n.
int mplp_update_slots(int L) {
    int slots = 64;
    while (slots > 1 && sizeof(double) * 3 * (size_t)L * (size_t)(slots + 2) > 64 * 1024) slots >>= 1;
    if (const char *e = std::getenv("MSMHIP_MPLP_SLOTS")) {
        const int asked = std::atoi(e);
        if (asked >= 1 && (asked & (asked - 1)) == 0) slots = std::min(slots, asked);
    }
    return slots;
}

int launch_mplp_update(msm_ctx *ctx, const MplpArgs &a, int begin, int count, int sweep) {
    MSM_TRY(check_shape(a));
    if (count <= 0) return MSM_OK;
    if (begin < 0 || begin + count > a.T || sweep < 0) return fail(MSM_ERR_INVALID, "msm_mplp_optimise_gpu: bad launch (factors %d + %d of %d)", begin, count, a.T);
    const int slots = mplp_update_slots(a.L);
    const size_t lds = sizeof(double) * 3 * (size_t)a.L * (1 + (size_t)(slots > 1 ? slots + 1 : 1));
    hipLaunchKernelGGL(k_mplp_update, dim3((unsigned)count), dim3(kMplpThreads), lds, ctx->stream, a, begin, count, sweep, slots);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_mplp_decode(msm_ctx *ctx, const MplpArgs &a, int32_t *label, double *node_terms) {
    MSM_TRY(check_shape(a));
    hipLaunchKernelGGL(k_mplp_decode, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, ctx->stream, a, label, node_terms);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_mplp_factor_terms(msm_ctx *ctx, const MplpArgs &a, double *factor_terms, int sweep) {
    MSM_TRY(check_shape(a));
    if (a.T == 0) return MSM_OK;
    const size_t lds = sizeof(double) * (3 * (size_t)a.L + kMplpThreads / 64);
    hipLaunchKernelGGL(k_mplp_factor_terms, dim3((unsigned)a.T), dim3(kMplpThreads), lds, ctx->stream, a, factor_terms, sweep);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_mplp_finite(msm_ctx *ctx, const double *U, size_t nU, const double *tc, size_t ntc, int32_t *flags) {
    const size_t n = std::max(nU, ntc);
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_mplp_finite, dim3(blocks), dim3(256), 0, ctx->stream, U, nU, tc, ntc, flags);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
