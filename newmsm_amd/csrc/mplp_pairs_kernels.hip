// mplp_pairs_kernels.hip -- the kernels of MPLP over the pair tables (mplp_pairs.hpp; the definition and the serial literal: mplp_pairs_host.hpp;
// DESIGN.md 5.20).
//
// A sweep walks the pair classes of the host's colouring; pairs of one class share no node, so a class is one launch and whatever its wavefronts do among
// themselves every pair sees the messages the serial sweep would show it: the cavities of a pair read the other slots on its two nodes, and those
// belong to pairs of other classes.
//
// What shapes k_mplp_pair_update: a pair's table is L^2 doubles with a fastest (2.9 KB at 19 labels), far too little for the 256 threads the triplet
// kernel gives a factor.  Up to 64 labels a wavefront takes a pair, four pairs to a workgroup: lane a holds column a -- its cavity d0(a) and the
// running minimum M0(a) in registers -- and walks the rows b, one coalesced row per step; M1(b) is the row's minimum across the lanes, by shuffles.
// Above 64 labels the four wavefronts of a workgroup share one pair, wavefront w taking the rows b = w, w + 4, ...; a lane then holds the columns
// a = lane, lane + 64, ..., whose cavities and minima live in LDS, each wavefront lowering a copy of M0 of its own (a lane only ever touches its own
// columns of its own copy, so there is no atomic), and the four copies are folded when the table is through.  A minimum is exact, so neither shape
// changes a bit but the sign of a zero, which `+ 0.0` removes as in the literal.  Arithmetic is the literal's and nothing else: the file is built
// with -ffp-contract=off and the division by 2.0 is exact.  The cavities add in list order over incidence lists of any length (a hub of a star has
// dozens of slots): eight slots and their eight messages are loaded side by side, the additions follow in order.
//
// Registers (hipcc -O3, gfx950; none of the kernels spills or uses scratch, all at 8 waves per SIMD): k_mplp_pair_update<1> 52 VGPRs, <4> 60;
// k_mplp_pair_decode 48; k_mplp_pair_factor_terms<1> 22, <4> 26; k_mplp_pair_energy_terms 12; k_mplp_pair_polish 30.
#include <climits>

#include "mplp_pairs.hpp"

namespace msm {

namespace {

__device__ __forceinline__ void raise_status(int *status, int code) { atomicMin(status, code); }
__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// the lowest value of a wavefront, in every lane
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off);
        if (o < v) v = o;
    }
    return v;
}

// the lowest (value, label) of a wavefront, lowest label on ties, to lane 0; a lane without a label holds INT_MAX
__device__ __forceinline__ void wave_argmin(double &bv, int &bx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(bv, off);
        const int ox = __shfl_down(bx, off);
        if (ox != INT_MAX && (bx == INT_MAX || ov < bv || (ov == bv && ox < bx))) bv = ov, bx = ox;
    }
}

// what node_sum reads
struct NodeSums {
    const double *U, *m;
    const int32_t *inc_ptr, *inc_slot;
    unsigned N, L, slots;  // slots: 2 P
    int *status;
};

template <class Args>
__device__ __forceinline__ NodeSums node_sums_of(const Args &a, const double *m) {
    return {a.U, m, a.inc_ptr, a.inc_slot, (unsigned)a.N, (unsigned)a.L, 2u * (unsigned)a.P, a.status};
}

// theta_i(x) plus the messages over the incidence of node i in order, but for slot `skip` (-1: none).  Eight slots, then their eight messages, are
// loaded side by side; the additions follow in list order.
__device__ __forceinline__ double node_sum(const NodeSums &n, unsigned i, unsigned x, int skip) {
    const int k0 = n.inc_ptr[i], k1 = n.inc_ptr[i + 1];
    double v = n.U[(size_t)x * n.N + i];
    for (int k = k0; k < k1; k += 8) {
        int q[8];
        double mv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = k + j < k1 ? n.inc_slot[k + j] : skip;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (q[j] != skip && (unsigned)q[j] >= n.slots) {  // (the host built the lists: what is out of range indexes nothing)
                raise_status(n.status, MSM_ERR_INVALID);
                q[j] = skip;
            }
            mv[j] = q[j] != skip ? n.m[(size_t)q[j] * n.L + x] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (q[j] != skip) v += mv[j];
    }
    return v;
}

// the pair a wavefront works on: entry j of the class, checked; false where there is none (past the class's end, or a record out of range)
__device__ __forceinline__ bool pair_of(const MplpPairArgs &a, int begin, int count, long j, unsigned lane, unsigned &p, unsigned &A, unsigned &B) {
    if (j >= (long)count) return false;
    p = (unsigned)a.sched[begin + j];
    if (p < (unsigned)a.P) {
        A = (unsigned)a.pairs[2 * (size_t)p], B = (unsigned)a.pairs[2 * (size_t)p + 1];
        if (A < (unsigned)a.N && B < (unsigned)a.N) return true;
    }
    if (lane == 0) raise_status(a.status, MSM_ERR_INVALID);
    return false;
}

// W wavefronts to a pair, 4 / W pairs to a workgroup.  W == 1 (L <= 64): LDS holds d1 and M1 of each pair, 2 L doubles; W == 4: d1, M1, d0 and four
// copies of M0, 7 L doubles.  Every thread reaches both barriers whether its wavefront has a pair or not.
template <int W>
__global__ __launch_bounds__(256) void k_mplp_pair_update(MplpPairArgs a, int begin, int count, int sweep) {
    extern __shared__ __align__(16) double s_pair[];
    if (sweep > 0 && a.changed[sweep - 1] == 0) return;  // the run is at its fixed point (the whole launch)
    constexpr unsigned per_pair = W == 1 ? 2 : 3 + W;
    const unsigned tid = threadIdx.x, lane = tid & 63u, g = (tid >> 6) / W, w = (tid >> 6) % W, L = (unsigned)a.L;
    unsigned p = 0, A = 0, B = 0;
    const bool active = pair_of(a, begin, count, (long)blockIdx.x * (4 / W) + g, lane, p, A, B);
    double *d1 = s_pair + (size_t)g * per_pair * L, *M1 = d1 + L, *d0 = M1 + L, *M0 = d0 + L + (size_t)w * L;  // (d0, M0: W > 1 only)
    const double *__restrict__ th = a.pc + (size_t)p * L * L;
    const NodeSums n = node_sums_of(a, a.m);
    const double inf = pos_inf();
    double d0r = 0.0, m0r = inf;  // W == 1: column `lane`
    if (active) {
        for (unsigned x = lane + 64 * w; x < L; x += 64 * W) {
            d1[x] = node_sum(n, B, x, 2 * (int)p + 1);
            if constexpr (W > 1) d0[x] = node_sum(n, A, x, 2 * (int)p);
        }
        if constexpr (W == 1) {
            if (lane < L) d0r = node_sum(n, A, lane, 2 * (int)p);
        } else {
            for (unsigned x = lane; x < L; x += 64) M0[x] = inf;
        }
    }
    __syncthreads();
    if (active) {
        for (unsigned b = w; b < L; b += W) {
            const double d1b = d1[b];
            double lo = inf;
            if constexpr (W == 1) {
                if (lane < L) {
                    lo = (th[b * L + lane] + d0r) + d1b;
                    if (lo < m0r) m0r = lo;
                }
            } else {
                for (unsigned x = lane; x < L; x += 64) {
                    const double v = (th[b * L + x] + d0[x]) + d1b;
                    if (v < M0[x]) M0[x] = v;
                    if (v < lo) lo = v;
                }
            }
            lo = wave_min(lo);
            if (lane == 0) M1[b] = lo;
        }
    }
    __syncthreads();
    if (active) {
        double *__restrict__ out = a.m + (size_t)2 * p * L;  // slot s, label x at s * L + x
        bool moved = false;
        if constexpr (W == 1) {
            if (lane < L) {
                const double nv = (m0r + 0.0) / 2.0 - d0r;
                moved |= __double_as_longlong(nv) != __double_as_longlong(out[lane]);
                out[lane] = nv;
            }
        } else {
            const double *copies = d0 + L;
            for (unsigned x = lane + 64 * w; x < L; x += 64 * W) {
                double lo = copies[x];
#pragma unroll
                for (unsigned k = 1; k < W; ++k)
                    if (copies[(size_t)k * L + x] < lo) lo = copies[(size_t)k * L + x];
                const double nv = (lo + 0.0) / 2.0 - d0[x];
                moved |= __double_as_longlong(nv) != __double_as_longlong(out[x]);
                out[x] = nv;
            }
        }
        for (unsigned x = lane + 64 * w; x < L; x += 64 * W) {
            const double nv = (M1[x] + 0.0) / 2.0 - d1[x];
            moved |= __double_as_longlong(nv) != __double_as_longlong(out[L + x]);
            out[L + x] = nv;
        }
        if (moved) a.changed[sweep] = 1;
    }
}

// a wavefront per node: lane l takes the labels l, l + 64, ...; the lowest belief, lowest label on ties, by shuffles
__global__ __launch_bounds__(256) void k_mplp_pair_decode(MplpPairArgs a, int32_t *__restrict__ label, double *__restrict__ node_terms) {
    const unsigned lane = threadIdx.x & 63u, L = (unsigned)a.L;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (long)a.N) return;  // (the whole wavefront)
    const NodeSums n = node_sums_of(a, a.m);
    double bv = 0.0;
    int bx = INT_MAX;  // no label yet
    for (unsigned x = lane; x < L; x += 64) {
        const double v = node_sum(n, (unsigned)i, x, -1);
        if (bx == INT_MAX || v < bv) bv = v, bx = (int)x;
    }
    wave_argmin(bv, bx);
    if (lane == 0) {
        if (label) label[i] = bx;
        node_terms[i] = bv;
    }
}

// the pair terms of the bound: min over (a, b) of (theta_p(a, b) - m[p][0][a]) - m[p][1][b], W wavefronts to a pair as in the update (rows b by
// wavefront, columns a by lane); W == 4 folds its four minima through LDS (4 doubles)
template <int W>
__global__ __launch_bounds__(256) void k_mplp_pair_factor_terms(MplpPairArgs a, double *__restrict__ factor_terms, int sweep) {
    extern __shared__ __align__(16) double s_pair[];
    if (sweep > 0 && a.changed[sweep - 1] == 0) return;
    const unsigned tid = threadIdx.x, lane = tid & 63u, g = (tid >> 6) / W, w = (tid >> 6) % W, L = (unsigned)a.L;
    const long p = (long)blockIdx.x * (4 / W) + g;
    const bool active = p < (long)a.P;
    const double inf = pos_inf();
    double lo = inf;
    if (active) {
        const double *__restrict__ th = a.pc + (size_t)p * L * L;
        const double *__restrict__ m0 = a.m + (size_t)2 * p * L, *__restrict__ m1 = m0 + L;
        for (unsigned b = w; b < L; b += W) {
            const double m1b = m1[b];
            for (unsigned x = lane; x < L; x += 64) {
                const double v = (th[b * L + x] - m0[x]) - m1b;
                if (v < lo) lo = v;
            }
        }
        lo = wave_min(lo);
    }
    if constexpr (W == 1) {
        if (active && lane == 0) factor_terms[p] = lo;  // (the sign of a zero minimum depends on the order; the sum it joins starts at +0.0 and does not see it)
    } else {
        if (lane == 0) s_pair[w] = lo;
        __syncthreads();
        if (active && tid == 0) {
#pragma unroll
            for (unsigned k = 1; k < W; ++k)
                if (s_pair[k] < lo) lo = s_pair[k];
            factor_terms[p] = lo;
        }
    }
}

// the N + P terms of a labelling's energy, a thread per term
__global__ __launch_bounds__(256) void k_mplp_pair_energy_terms(MplpPairArgs a, const int32_t *__restrict__ lab, double *__restrict__ terms) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    const unsigned N = (unsigned)a.N, L = (unsigned)a.L;
    if (j >= (long)a.N + a.P) return;
    double v = 0.0;
    if (j < (long)N) {
        const unsigned x = (unsigned)lab[j];
        if (x < L)
            v = a.U[(size_t)x * N + (size_t)j];
        else
            raise_status(a.status, MSM_ERR_INVALID);
    } else {
        const size_t p = (size_t)(j - (long)N);
        const unsigned A = (unsigned)a.pairs[2 * p], B = (unsigned)a.pairs[2 * p + 1];
        const unsigned la = A < N ? (unsigned)lab[A] : L, lb = B < N ? (unsigned)lab[B] : L;
        if (la < L && lb < L)
            v = a.pc[(p * L + lb) * L + la];
        else
            raise_status(a.status, MSM_ERR_INVALID);
    }
    terms[j] = v;
}

// A polish pass over one node class, a wavefront per node: every other node is held, so label x costs theta_i(x) plus one table entry per incident
// slot, added in list order -- along a row of the pair's table for slot 0 (coalesced), down a column for slot 1.  The current label stays unless
// another one is strictly lower.
__global__ __launch_bounds__(256) void k_mplp_pair_polish(MplpPairPolishArgs a, int begin, int count, int pass) {
    if (pass > 0 && a.changed[pass - 1] == 0) return;  // the pass before moved no label (the whole launch)
    const unsigned lane = threadIdx.x & 63u, L = (unsigned)a.L, N = (unsigned)a.N;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= (long)count) return;  // (the whole wavefront)
    const unsigned i = (unsigned)a.cls_node[begin + n];
    if (i >= N) {
        if (lane == 0) raise_status(a.status, MSM_ERR_INVALID);
        return;
    }
    const unsigned cur = (unsigned)a.lab[i];
    if (cur >= L) {
        if (lane == 0) raise_status(a.status, MSM_ERR_INVALID);
        return;
    }
    const int k0 = a.inc_ptr[i], k1 = a.inc_ptr[i + 1];
    double bv = 0.0, cv = 0.0;
    int bx = INT_MAX;
    for (unsigned x = lane; x < L; x += 64) {
        double v = a.U[(size_t)x * N + i];
        for (int k = k0; k < k1; ++k) {
            const unsigned q = (unsigned)a.inc_slot[k];
            if (q >= 2u * (unsigned)a.P) {
                raise_status(a.status, MSM_ERR_INVALID);
                continue;
            }
            const unsigned j = (unsigned)a.pairs[q ^ 1u];  // the pair's other node
            const unsigned lj = j < N ? (unsigned)a.lab[j] : L;
            if (lj >= L) {
                raise_status(a.status, MSM_ERR_INVALID);
                continue;
            }
            const double *__restrict__ th = a.pc + (size_t)(q >> 1) * L * L;
            v += (q & 1u) == 0 ? th[lj * L + x] : th[x * L + lj];
        }
        if (x == cur) cv = v;
        if (bx == INT_MAX || v < bv) bv = v, bx = (int)x;
    }
    wave_argmin(bv, bx);
    cv = __shfl(cv, (int)(cur & 63u));
    if (lane == 0 && bv < cv) {
        a.lab[i] = bx;
        a.changed[pass] = 1;
    }
}

int check_shape(const MplpPairArgs &a) {
    if (a.N <= 0 || a.L <= 0 || a.L > kMplpMaxLabels || a.P < 0)
        return fail(MSM_ERR_INVALID, "msm_mplp_pairs_optimise_gpu: bad launch (N %d, L %d, P %d)", a.N, a.L, a.P);
    return MSM_OK;
}

}  // namespace

int launch_mplp_pair_update(msm_ctx *ctx, const MplpPairArgs &a, int begin, int count, int sweep) {
    MSM_TRY(check_shape(a));
    if (count <= 0) return MSM_OK;
    if (begin < 0 || begin + count > a.P || sweep < 0) return fail(MSM_ERR_INVALID, "msm_mplp_pairs_optimise_gpu: bad launch (pairs %d + %d of %d)", begin, count, a.P);
    if (a.L <= kMplpPairWaveLabels)
        hipLaunchKernelGGL(k_mplp_pair_update<1>, dim3((unsigned)((count + 3) / 4)), dim3(256), sizeof(double) * 4 * 2 * (size_t)a.L, ctx->stream, a, begin, count, sweep);
    else
        hipLaunchKernelGGL(k_mplp_pair_update<4>, dim3((unsigned)count), dim3(256), sizeof(double) * 7 * (size_t)a.L, ctx->stream, a, begin, count, sweep);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_mplp_pair_decode(msm_ctx *ctx, const MplpPairArgs &a, int32_t *label, double *node_terms) {
    MSM_TRY(check_shape(a));
    hipLaunchKernelGGL(k_mplp_pair_decode, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, ctx->stream, a, label, node_terms);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_mplp_pair_factor_terms(msm_ctx *ctx, const MplpPairArgs &a, double *factor_terms, int sweep) {
    MSM_TRY(check_shape(a));
    if (a.P == 0) return MSM_OK;
    if (a.L <= kMplpPairWaveLabels)
        hipLaunchKernelGGL(k_mplp_pair_factor_terms<1>, dim3((unsigned)((a.P + 3) / 4)), dim3(256), 0, ctx->stream, a, factor_terms, sweep);
    else
        hipLaunchKernelGGL(k_mplp_pair_factor_terms<4>, dim3((unsigned)a.P), dim3(256), sizeof(double) * 4, ctx->stream, a, factor_terms, sweep);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_mplp_pair_energy_terms(msm_ctx *ctx, const MplpPairArgs &a, const int32_t *labeling, double *terms) {
    MSM_TRY(check_shape(a));
    const size_t n = (size_t)a.N + (size_t)a.P;
    hipLaunchKernelGGL(k_mplp_pair_energy_terms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a, labeling, terms);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_mplp_pair_polish(msm_ctx *ctx, const MplpPairPolishArgs &a, int begin, int count, int pass) {
    if (a.N <= 0 || a.L <= 0 || a.L > kMplpMaxLabels || a.P < 0 || begin < 0 || count < 0 || begin + count > a.N || pass < 0)
        return fail(MSM_ERR_INVALID, "msm_mplp_pairs_polish_gpu: bad launch (N %d, L %d, P %d, nodes %d + %d, pass %d)", a.N, a.L, a.P, begin, count, pass);
    if (count == 0) return MSM_OK;
    hipLaunchKernelGGL(k_mplp_pair_polish, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, ctx->stream, a, begin, count, pass);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
