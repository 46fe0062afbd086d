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
//
// The rounding of the messages to a labelling (k_mplp_round, k_mplp_polish; DESIGN.md 5.19 "Rounding") walks the colour classes of the nodes, a launch per
// class: nodes of one class share no triplet, so whatever the workgroups of a launch do among themselves every node sees the labels the serial walk
// would show it.
#include <climits>
#include <cstdlib>
#include <type_traits>

#include "mplp.hpp"

namespace msm {

namespace {

__device__ __forceinline__ void raise_status(int *status, int code) { atomicMin(status, code); }
__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

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

// Forbidden entries: the kernels that read the triplet table come in two instantiations.  F = true reads an entry that is NaN or +inf
// as +inf -- one compare and one select -- and keeps +inf messages out of every subtraction; F = false is the plain code, unchanged.  A batch in flight
// is mapped where it is folded in, not where it is requested: a compare beside the load would wait for the load there and end the overlap the
// batches exist for (measured: 0.70 against 0.44 ms per sweep on the ico4 table).
template <bool F>
__device__ __forceinline__ double hat(double v) {
    if constexpr (F) return v < pos_inf() ? v : pos_inf();
    return v;
}

__device__ __forceinline__ void load_batch(const double *__restrict__ th, unsigned e0, unsigned L3, double (&v)[kMplpBatch]) {
#pragma unroll
    for (int j = 0; j < kMplpBatch; ++j) {
        const unsigned e = e0 + (unsigned)j * kMplpThreads;
        v[j] = e < L3 ? th[e] : 0.0;
    }
}

template <bool F>
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
    const long long inf_key = key_of(pos_inf());
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
            const double v = ((hat<F>(cur[j]) + d[p.a]) + d[L + p.b]) + d[2 * L + p.c];
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
        double nv = (value_of(lowest) + 0.0) / 3.0 - d[idx];
        if constexpr (F)
            if (lowest == inf_key) nv = value_of(inf_key);  // no combination with this label is below +inf: the label is proved infeasible
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
    // (wave_argmin spelled out: through the helper the compiler orders this kernel's instructions differently, and its schedule stays as measured)
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

template <bool F>
__global__ __launch_bounds__(kMplpThreads) void k_mplp_factor_terms(MplpArgs a, double *__restrict__ factor_terms, int sweep) {
    extern __shared__ __align__(16) double s_mplp[];  // 3 L messages, then a minimum per wavefront
    if (sweep > 0 && a.changed[sweep - 1] == 0) return;
    const unsigned tid = threadIdx.x, L = (unsigned)a.L, t = blockIdx.x;
    if (t >= (unsigned)a.T) return;
    for (unsigned idx = tid; idx < 3 * L; idx += kMplpThreads) s_mplp[idx] = a.m[(size_t)3 * t * L + idx];
    __syncthreads();
    const unsigned L3 = L * L * L;
    const double *__restrict__ th = a.tc + (size_t)t * L3;
    const double inf = pos_inf();
    double lo = inf;
    Abc p(tid, kMplpThreads, L);
    for (unsigned e = tid; e < L3; e += kMplpThreads, p.advance()) {
        const double m0 = s_mplp[p.a], m1 = s_mplp[L + p.b], m2 = s_mplp[2 * L + p.c], en = th[e];
        double v = ((en - m0) - m1) - m2;
        if constexpr (F) v = en < inf && m0 < inf && m1 < inf && m2 < inf ? v : inf;  // only combinations that are below +inf in all four
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

// One pass over both tables: counts[0] non-finite unary entries, counts[1..3] NaN / +inf / -inf triplet entries.  A wavefront reduces its four counts by
// shuffles, the workgroup's four wavefronts meet in LDS, and thread c adds the workgroup's count c with one 64-bit atomic (none where it is zero).
__global__ __launch_bounds__(256) void k_mplp_classify(const double *__restrict__ U, size_t nU, const double *__restrict__ tc, size_t ntc,
                                                       unsigned long long *__restrict__ counts) {
    __shared__ unsigned s_cnt[4][4];
    const size_t stride = (size_t)gridDim.x * 256;
    const double inf = pos_inf();
    unsigned n[4] = {0, 0, 0, 0};  // (a thread sees at most ceil(2^63 / stride) entries; the grid keeps that far below 2^32)
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < nU; j += stride) n[0] += !(U[j] - U[j] == 0.0);
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < ntc; j += stride) {
        const double v = tc[j];
        n[1] += v != v;
        n[2] += v == inf;
        n[3] += v == -inf;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n[c] += __shfl_down(n[c], off);
    if ((threadIdx.x & 63u) == 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) s_cnt[threadIdx.x >> 6][c] = n[c];
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long total = (unsigned long long)s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (total) atomicAdd(&counts[threadIdx.x], total);
    }
}

// ---------------------------------------------------------------- rounding (DESIGN.md 5.19 "Rounding"; the literal: mplp_round_host)

// the lowest (value, label) of a wavefront, lowest label on ties, to lane 0; a lane without a label holds INT_MAX
__device__ __forceinline__ void wave_argmin(double &bv, int &bx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(bv, off);
        const int ox = __shfl_down(bx, off);
        if (ox != INT_MAX && (bx == INT_MAX || ov < bv || (ov == bv && ox < bx))) bv = ov, bx = ox;
    }
}

// The conditioned decode of one class: a workgroup per node.  The L scores sit in LDS, label x owned by thread x % 256; every incident slot adds its
// g(x) in list order.  With neither other node fixed the factor's L^3 block is streamed as k_mplp_update streams it, each entry lowering g[x_s] in a
// padded row of `slots` key copies; with one fixed the L^2 sub-block at its label goes the same way, threads along the faster free axis; with both
// fixed thread x reads its own entry.
template <bool F>
__global__ __launch_bounds__(kMplpThreads) void k_mplp_round(MplpRoundArgs a, int begin, int count, int frontier, int slots) {
    extern __shared__ __align__(16) double s_mplp[];  // L scores, 2 L staged messages, 8 words of the argmin, L rows of `slots` keys (padded by one)
    const unsigned tid = threadIdx.x, L = (unsigned)a.L, N = (unsigned)a.N;
    if ((int)blockIdx.x >= count) return;
    const unsigned i = (unsigned)a.cls_node[begin + (int)blockIdx.x];
    if (i >= N) {
        if (tid == 0) raise_status(a.status, MSM_ERR_INVALID);
        return;
    }
    double *score = s_mplp, *mo = s_mplp + L, *w = s_mplp + 3 * (size_t)L;
    long long *G = reinterpret_cast<long long *>(w + 8);
    const unsigned S = (unsigned)slots, stride = S > 1 ? S + 1 : 1, mine = tid & (S - 1);
    const unsigned L2 = L * L, L3 = L2 * L;
    const double inf = pos_inf();
    const long long inf_key = key_of(inf);
    for (unsigned x = tid; x < L; x += kMplpThreads) score[x] = a.U[(size_t)x * N + i];
    const int k0 = a.inc_ptr[i], k1 = a.inc_ptr[i + 1];
    for (int k = k0; k < k1; ++k) {  // (everything that decides a branch below is the same in every thread of the workgroup)
        const unsigned q = (unsigned)a.inc_slot[k];
        if (q >= 3u * (unsigned)a.T) {
            if (tid == 0) raise_status(a.status, MSM_ERR_INVALID);
            return;
        }
        const unsigned t = q / 3, s = q - 3 * t, s1 = s == 0 ? 1 : 0, s2 = s == 2 ? 1 : 2;
        const int4 r = a.tri[t];  // {triplet, node A, node B, node C}
        const unsigned j1 = (unsigned)(s1 == 0 ? r.y : r.z), j2 = (unsigned)(s2 == 1 ? r.z : r.w);
        if (j1 >= N || j2 >= N) {
            if (tid == 0) raise_status(a.status, MSM_ERR_INVALID);
            return;
        }
        const bool f1 = a.colour[j1] < frontier, f2 = a.colour[j2] < frontier;
        const unsigned l1 = f1 ? (unsigned)a.lab[j1] : 0u, l2 = f2 ? (unsigned)a.lab[j2] : 0u;
        if (l1 >= L || l2 >= L) {
            if (tid == 0) raise_status(a.status, MSM_ERR_INVALID);
            return;
        }
        const double *__restrict__ th = a.tc + (size_t)t * L3;
        const unsigned st = s == 0 ? L2 : s == 1 ? L : 1u, st1 = s1 == 0 ? L2 : L, st2 = s2 == 1 ? L : 1u;
        if (f1 && f2) {
            for (unsigned x = tid; x < L; x += kMplpThreads) score[x] += hat<F>(th[x * st + l1 * st1 + l2 * st2]);
            continue;
        }
        for (unsigned idx = tid; idx < L * stride; idx += kMplpThreads) G[idx] = inf_key;
        if (!f1 && !f2) {
            double cur[kMplpBatch], nxt[kMplpBatch];
            load_batch(th, tid, L3, cur);
            for (unsigned idx = tid; idx < 2 * L; idx += kMplpThreads) {
                const unsigned so = idx < L ? s1 : s2, y = idx < L ? idx : idx - L;
                mo[idx] = a.m ? a.m[((size_t)3 * t + so) * L + y] : 0.0;
            }
            __syncthreads();
            Abc p(tid, kMplpThreads, L);
            for (unsigned e0 = tid; e0 < L3; e0 += kMplpBatch * kMplpThreads) {
                load_batch(th, e0 + kMplpBatch * kMplpThreads, L3, nxt);
#pragma unroll
                for (int j = 0; j < kMplpBatch; ++j) {
                    if (e0 + (unsigned)j * kMplpThreads >= L3) break;
                    const unsigned x = s == 0 ? p.a : s == 1 ? p.b : p.c, y1 = s1 == 0 ? p.a : p.b, y2 = s2 == 1 ? p.b : p.c;
                    double v = (cur[j] - mo[y1]) - mo[L + y2];
                    if constexpr (F) v = cur[j] < inf && mo[y1] < inf && mo[L + y2] < inf ? v : inf;  // a forbidden entry (NaN too) or a +inf message
                    atomicMin(&G[x * stride + mine], key_of(v));
                    p.advance();
                }
#pragma unroll
                for (int j = 0; j < kMplpBatch; ++j) cur[j] = nxt[j];
            }
        } else {
            // one other fixed at label lf of slot sf; the free axes are s and su, `lo` the one that runs faster in the table
            const unsigned su = f1 ? s2 : s1, stu = f1 ? st2 : st1, base = f1 ? l1 * st1 : l2 * st2;
            for (unsigned y = tid; y < L; y += kMplpThreads) mo[y] = a.m ? a.m[((size_t)3 * t + su) * L + y] : 0.0;
            __syncthreads();
            const bool x_fast = s > su;
            const unsigned st_hi = x_fast ? stu : st, st_lo = x_fast ? st : stu;
            for (unsigned e = tid; e < L2; e += kMplpThreads) {
                const unsigned hi = e / L, lo = e - hi * L;
                const unsigned x = x_fast ? lo : hi, y = x_fast ? hi : lo;
                const double en = hat<F>(th[base + hi * st_hi + lo * st_lo]);
                double v = en - mo[y];
                if constexpr (F) v = en < inf && mo[y] < inf ? v : inf;
                atomicMin(&G[x * stride + mine], key_of(v));
            }
        }
        __syncthreads();
        for (unsigned x = tid; x < L; x += kMplpThreads) {
            long long lowest = G[x * stride];
            for (unsigned j = 1; j < S; ++j) lowest = min(lowest, G[x * stride + j]);
            score[x] += value_of(lowest) + 0.0;
        }
        __syncthreads();  // the rows and the staged messages are free again
    }
    double bv = 0.0;
    int bx = INT_MAX;
    for (unsigned x = tid; x < L; x += kMplpThreads) {
        const double v = score[x];
        if (bx == INT_MAX || v < bv) bv = v, bx = (int)x;
    }
    wave_argmin(bv, bx);
    int *wx = reinterpret_cast<int *>(w + 4);
    if ((tid & 63u) == 0) w[tid >> 6] = bv, wx[tid >> 6] = bx;
    __syncthreads();
    if (tid == 0) {
        for (unsigned j = 1; j < kMplpThreads / 64; ++j)
            if (wx[j] != INT_MAX && (w[j] < bv || (w[j] == bv && wx[j] < bx))) bv = w[j], bx = wx[j];
        a.lab[i] = bx;
    }
}

// A polish pass over one class, a wavefront per node: every other node is fixed, so label x costs theta_i(x) plus one table entry per incident slot,
// added in list order.  The current label stays unless another one is strictly lower.
template <bool F>
__global__ __launch_bounds__(256) void k_mplp_polish(MplpRoundArgs a, int begin, int count, int pass) {
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
    const unsigned L2 = L * L, L3 = L2 * L;
    const int k0 = a.inc_ptr[i], k1 = a.inc_ptr[i + 1];
    double bv = 0.0, cv = 0.0;
    int bx = INT_MAX;
    for (unsigned x = lane; x < L; x += 64) {
        double v = a.U[(size_t)x * N + i];
        for (int k = k0; k < k1; ++k) {
            const unsigned q = (unsigned)a.inc_slot[k];
            if (q >= 3u * (unsigned)a.T) {
                raise_status(a.status, MSM_ERR_INVALID);
                continue;
            }
            const unsigned t = q / 3, s = q - 3 * t;
            const int4 r = a.tri[t];
            const unsigned j1 = (unsigned)(s == 0 ? r.z : r.y), j2 = (unsigned)(s == 2 ? r.z : r.w);
            if (j1 >= N || j2 >= N) {
                raise_status(a.status, MSM_ERR_INVALID);
                continue;
            }
            const unsigned l1 = (unsigned)a.lab[j1], l2 = (unsigned)a.lab[j2];
            if (l1 >= L || l2 >= L) {
                raise_status(a.status, MSM_ERR_INVALID);
                continue;
            }
            const unsigned st = s == 0 ? L2 : s == 1 ? L : 1u, st1 = s == 0 ? L : L2, st2 = s == 2 ? L : 1u;
            v += hat<F>(a.tc[(size_t)t * L3 + x * st + l1 * st1 + l2 * st2]);
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

int check_shape(const MplpArgs &a) {
    if (a.N <= 0 || a.L <= 0 || a.L > kMplpMaxLabels || a.T < 0) return fail(MSM_ERR_INVALID, "msm_mplp_optimise_gpu: bad launch (N %d, L %d, T %d)", a.N, a.L, a.T);
    return MSM_OK;
}

// launch(std::true_type) or launch(std::false_type): the one choice between a kernel's forbidden-aware instantiation and its plain one
template <class Launch>
int launch_either(bool forbid, Launch launch) {
    if (forbid)
        launch(std::true_type());
    else
        launch(std::false_type());
    MSM_HIP(hipGetLastError());
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

int launch_mplp_update(msm_ctx *ctx, const MplpArgs &a, int begin, int count, int sweep, bool forbid) {
    MSM_TRY(check_shape(a));
    if (count <= 0) return MSM_OK;
    if (begin < 0 || begin + count > a.T || sweep < 0) return fail(MSM_ERR_INVALID, "msm_mplp_optimise_gpu: bad launch (factors %d + %d of %d)", begin, count, a.T);
    const int slots = mplp_update_slots(a.L);
    const size_t lds = sizeof(double) * 3 * (size_t)a.L * (1 + (size_t)(slots > 1 ? slots + 1 : 1));
    return launch_either(forbid, [&](auto F) {
        hipLaunchKernelGGL(k_mplp_update<decltype(F)::value>, dim3((unsigned)count), dim3(kMplpThreads), lds, ctx->stream, a, begin, count, sweep, slots);
    });
}

int launch_mplp_decode(msm_ctx *ctx, const MplpArgs &a, int32_t *label, double *node_terms) {
    MSM_TRY(check_shape(a));
    hipLaunchKernelGGL(k_mplp_decode, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, ctx->stream, a, label, node_terms);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_mplp_factor_terms(msm_ctx *ctx, const MplpArgs &a, double *factor_terms, int sweep, bool forbid) {
    MSM_TRY(check_shape(a));
    if (a.T == 0) return MSM_OK;
    const size_t lds = sizeof(double) * (3 * (size_t)a.L + kMplpThreads / 64);
    return launch_either(forbid, [&](auto F) {
        hipLaunchKernelGGL(k_mplp_factor_terms<decltype(F)::value>, dim3((unsigned)a.T), dim3(kMplpThreads), lds, ctx->stream, a, factor_terms, sweep);
    });
}

int launch_mplp_classify(msm_ctx *ctx, const double *U, size_t nU, const double *tc, size_t ntc, unsigned long long *counts) {
    const size_t n = std::max(nU, ntc);
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_mplp_classify, dim3(blocks), dim3(256), 0, ctx->stream, U, nU, tc, ntc, counts);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

static int check_round_launch(const MplpRoundArgs &a, int begin, int count) {
    if (a.N <= 0 || a.L <= 0 || a.L > kMplpMaxLabels || a.T < 0 || begin < 0 || count < 0 || begin + count > a.N)
        return fail(MSM_ERR_INVALID, "msm_mplp_round_gpu: bad launch (N %d, L %d, T %d, nodes %d + %d)", a.N, a.L, a.T, begin, count);
    return MSM_OK;
}

int launch_mplp_round(msm_ctx *ctx, const MplpRoundArgs &a, int begin, int count, int frontier, bool forbid) {
    MSM_TRY(check_round_launch(a, begin, count));
    if (count == 0) return MSM_OK;
    const int slots = mplp_update_slots(a.L);
    const size_t lds = sizeof(double) * (3 * (size_t)a.L + 8 + (size_t)a.L * (size_t)(slots > 1 ? slots + 1 : 1));
    return launch_either(forbid, [&](auto F) {
        hipLaunchKernelGGL(k_mplp_round<decltype(F)::value>, dim3((unsigned)count), dim3(kMplpThreads), lds, ctx->stream, a, begin, count, frontier, slots);
    });
}

int launch_mplp_polish(msm_ctx *ctx, const MplpRoundArgs &a, int begin, int count, int pass, bool forbid) {
    MSM_TRY(check_round_launch(a, begin, count));
    if (count == 0) return MSM_OK;
    if (pass < 0) return fail(MSM_ERR_INVALID, "msm_mplp_round_gpu: bad launch (pass %d)", pass);
    return launch_either(forbid, [&](auto F) {
        hipLaunchKernelGGL(k_mplp_polish<decltype(F)::value>, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, ctx->stream, a, begin, count, pass);
    });
}

}  // namespace msm
