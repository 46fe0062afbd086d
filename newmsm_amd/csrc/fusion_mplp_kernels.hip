// fusion_mplp_kernels.hip -- k_fusion_mplp: MPLP over the binary problem of one label step, the whole solve in one launch of ONE workgroup (fusion_mplp.hpp;
// the definition is DESIGN.md 5.19's at L = 2, the literal mplp_run_host + mplp_round_host of mplp_host.hpp).
//
// A factor has eight entries, so a sweep is no throughput problem but a chain of dependent levels (mcmc_build_schedule: the factors of a level share no
// node).  One thread takes one factor of a level -- eight entries, six cavities, six messages, all in registers --, a __syncthreads() stands between two
// levels, and nothing ever waits for another workgroup: no grid barrier, no cooperative launch.  Behind the sweeps, in the same launch: the decode of
// every sweep with its energy and bound terms, the test for a fixed point (a workgroup-uniform exit), the conditioned decode over the node colours, the
// polish passes.  Every candidate labelling is written out; the host picks the winners after its one synchronisation.
//
// The messages (48 T bytes) live in LDS where they fit and in global memory otherwise (template LDS); the code is the same and so are the bits.
//
// What a level waits for: the factor's record and, per slot, the record of its node's other slots (FusionMplpPlan::nbr) are indexed by the schedule
// position alone, so a cavity is one load of records and then its messages -- two dependent loads where the incidence lists would make four.
//
// Sums: the literal adds a candidate's N + T terms serially, and floating-point addition does not reassociate.  The terms are therefore written out
// while the candidates arise, a column per candidate in blocks of eight terms (fusion_term_index), and at the end one thread per sum adds a column in
// the literal's order: all candidates side by side, thirty-two loads in flight per thread.  Arithmetic is the literal's and nothing else: the file is
// built with -ffp-contract=off, the division is the correctly rounded one, stores are plain vector stores.
#include "fusion_mplp.hpp"

namespace msm {

namespace {

__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }
// where term j of column c lies in a term array of C columns (fusion_term_index, fusion_mplp.hpp): eight consecutive terms of a column share a line
__device__ __forceinline__ size_t term_at(size_t j, size_t C, size_t c) { return fusion_term_index(j, C, c); }

// theta_i(x) plus the messages over the incidence of node i in list order, but for slot `skip` (-1: none), for x = 0 and 1 at once
__device__ __forceinline__ void node_sum2(const FusionMplpArgs &a, const double *u2, const double *m, unsigned i, int skip, double &v0, double &v1) {
    const int k0 = a.inc_ptr[i], k1 = a.inc_ptr[i + 1];
    v0 = u2[2 * (size_t)i], v1 = u2[2 * (size_t)i + 1];
    for (int k = k0; k < k1; ++k) {
        const int q = a.inc_slot[k];
        if (q == skip) continue;
        v0 += m[2 * (size_t)q];
        v1 += m[2 * (size_t)q + 1];
    }
}

// the cavity of node i at the slot whose record is (n0, n1): theta_i plus the messages of the node's other slots in incidence order -- listed in the
// record (n0.x of them, at most kFusionNbr) so that nothing but the messages waits for a load, or, n0.x < 0, walked through the incidence lists
__device__ __forceinline__ void cavity(const FusionMplpArgs &a, const double *u2, const double *m, unsigned i, int skip, const int4 n0, const int4 n1, double &v0,
                                       double &v1) {
    if (n0.x < 0) {
        node_sum2(a, u2, m, i, skip, v0, v1);
        return;
    }
    const int q[kFusionNbr] = {n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
    double m0[kFusionNbr], m1[kFusionNbr];
    v0 = u2[2 * (size_t)i], v1 = u2[2 * (size_t)i + 1];
#pragma unroll
    for (int k = 0; k < kFusionNbr; ++k)
        if (k < n0.x) m0[k] = m[2 * (size_t)q[k]], m1[k] = m[2 * (size_t)q[k] + 1];
#pragma unroll
    for (int k = 0; k < kFusionNbr; ++k)
        if (k < n0.x) v0 += m0[k], v1 += m1[k];
}

// the update of the factor at schedule position idx (mplp_update_factor at L = 2); returns whether a message's bits changed
__device__ __forceinline__ bool update_factor(const FusionMplpArgs &a, const double *u2, double *m, int idx) {
    const int4 r = a.sched[idx];
    const int4 *nb = a.nbr + 6 * (size_t)idx;
    const int4 n00 = nb[0], n01 = nb[1], n10 = nb[2], n11 = nb[3], n20 = nb[4], n21 = nb[5];
    const int t = r.x;
    double d[3][2], th[8], M[3][2];
#pragma unroll
    for (int e = 0; e < 8; ++e) th[e] = a.octets[8 * (size_t)t + e];
    cavity(a, u2, m, (unsigned)r.y, 3 * t, n00, n01, d[0][0], d[0][1]);
    cavity(a, u2, m, (unsigned)r.z, 3 * t + 1, n10, n11, d[1][0], d[1][1]);
    cavity(a, u2, m, (unsigned)r.w, 3 * t + 2, n20, n21, d[2][0], d[2][1]);
#pragma unroll
    for (int s = 0; s < 3; ++s) M[s][0] = M[s][1] = pos_inf();
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int z = 0; z < 2; ++z) {
                const double v = ((th[4 * x + 2 * y + z] + d[0][x]) + d[1][y]) + d[2][z];
                if (v < M[0][x]) M[0][x] = v;
                if (v < M[1][y]) M[1][y] = v;
                if (v < M[2][z]) M[2][z] = v;
            }
    bool changed = false;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const double nv = (M[s][x] + 0.0) / 3.0 - d[s][x];
            double *dst = m + (size_t)6 * t + 2 * s + x;
            changed |= __double_as_longlong(*dst) != __double_as_longlong(nv);
            *dst = nv;
        }
    return changed;
}

// beliefs and decode (the lowest label on ties; lab may be null) with the N node terms of the bound, then its T factor terms, into column k of bterms
__device__ __forceinline__ void decode_and_bound(const FusionMplpArgs &a, const double *u2, const double *m, uint8_t *lab, size_t SB, size_t k, unsigned tid) {
    const unsigned N = (unsigned)a.N, T = (unsigned)a.T;
    for (unsigned i = tid; i < N; i += kFusionThreads) {
        double b0, b1;
        node_sum2(a, u2, m, i, -1, b0, b1);
        const int best = b1 < b0 ? 1 : 0;
        if (lab) lab[i] = (uint8_t)best;
        a.bterms[term_at(i, SB, k)] = best ? b1 : b0;
    }
    for (unsigned t = tid; t < T; t += kFusionThreads) {
        const double *mt = m + 6 * (size_t)t;
        double lo = pos_inf();
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int z = 0; z < 2; ++z) {
                    const double v = ((a.octets[8 * (size_t)t + 4 * x + 2 * y + z] - mt[x]) - mt[2 + y]) - mt[4 + z];
                    if (v < lo) lo = v;
                }
        a.bterms[term_at((size_t)N + t, SB, k)] = lo;
    }
}

// the energy terms of candidate `slot` (its labelling: lab): nodes, then factors
__device__ __forceinline__ void energy_terms(const FusionMplpArgs &a, const double *u2, const uint8_t *lab, size_t C, size_t slot, unsigned tid) {
    for (unsigned i = tid; i < (unsigned)a.N; i += kFusionThreads) a.eterms[term_at(i, C, slot)] = u2[2 * (size_t)i + lab[i]];
    for (unsigned t = tid; t < (unsigned)a.T; t += kFusionThreads) {
        const unsigned xa = lab[a.triplets[3 * (size_t)t]], xb = lab[a.triplets[3 * (size_t)t + 1]], xc = lab[a.triplets[3 * (size_t)t + 2]];
        a.eterms[term_at((size_t)a.N + t, C, slot)] = a.octets[8 * (size_t)t + 4 * xa + 2 * xb + xc];
    }
}

// score(x) of node i at `frontier` (mplp_round_scores at L = 2): node j is fixed when colour[j] < frontier; polish: every node is fixed and no message read
template <bool POLISH>
__device__ __forceinline__ void round_scores(const FusionMplpArgs &a, const double *u2, const double *m, const uint8_t *lab, unsigned i, int frontier, double &sc0,
                                             double &sc1) {
    double score[2] = {u2[2 * (size_t)i], u2[2 * (size_t)i + 1]};
    const int k0 = a.inc_ptr[i], k1 = a.inc_ptr[i + 1];
    for (int k = k0; k < k1; ++k) {
        const int q = a.inc_slot[k], t = q / 3, s = q - 3 * t;
        const int s1 = s == 0 ? 1 : 0, s2 = s == 2 ? 1 : 2;
        const int j1 = a.triplets[3 * (size_t)t + s1], j2 = a.triplets[3 * (size_t)t + s2];
        const bool f1 = POLISH || a.colour[j1] < frontier, f2 = POLISH || a.colour[j2] < frontier;
        const int l1 = f1 ? lab[j1] : 0, l2 = f2 ? lab[j2] : 0;
        const int st = 4 >> s, st1 = 4 >> s1, st2 = 4 >> s2;
        const double *th = a.octets + 8 * (size_t)t;
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const double *row = th + x * st;
            double g;
            if (f1 && f2)
                g = row[l1 * st1 + l2 * st2];
            else {
                g = pos_inf();
                for (int y1 = 0; y1 < 2; ++y1) {
                    if (f1 && y1 != l1) continue;
                    for (int y2 = 0; y2 < 2; ++y2) {
                        if (f2 && y2 != l2) continue;
                        double v = row[y1 * st1 + y2 * st2];
                        if (!f1) v = v - m[2 * ((size_t)3 * t + s1) + y1];
                        if (!f2) v = v - m[2 * ((size_t)3 * t + s2) + y2];
                        if (v < g) g = v;
                    }
                }
                g = g + 0.0;
            }
            score[x] += g;
        }
    }
    sc0 = score[0], sc1 = score[1];
}

// n terms of column `col` of a term array with C columns, from 0.0 in ascending order; thirty-two loads side by side, the additions in order
__device__ __forceinline__ double serial_sum(const double *terms, size_t first, size_t n, size_t C, size_t col) {
    double s = 0.0;
    size_t j = 0;
    for (; j + 32 <= n; j += 32) {
        double v[32];
#pragma unroll
        for (int e = 0; e < 32; ++e) v[e] = terms[term_at(first + j + e, C, col)];
#pragma unroll
        for (int e = 0; e < 32; ++e) s += v[e];
    }
    for (; j < n; ++j) s += terms[term_at(first + j, C, col)];
    return s;
}

template <bool LDS>
__global__ __launch_bounds__(kFusionThreads) void k_fusion_mplp(FusionMplpArgs a) {
    extern __shared__ __align__(16) double s_fusion_m[];  // the 6 T messages (LDS = true)
    __shared__ int s_changed, s_bad[3];
    double *m = LDS ? s_fusion_m : a.m;
    const unsigned tid = threadIdx.x, N = (unsigned)a.N, T = (unsigned)a.T;
    const size_t S = (size_t)a.S, P = (size_t)a.P, C = S + P + 2, SB = S > 0 ? S : 1;  // (a bound column even without a sweep)
    if (tid == 0) s_changed = 0, s_bad[0] = s_bad[1] = s_bad[2] = 0;
    __syncthreads();

    // ---- the two tables: theta (gathered from the cost function's unary table where one is given), candidate 0 (x = 0) and its terms, zero messages
    const double *u2 = a.u2;
    if (a.U) {
        double *w = a.u2w;
        for (unsigned i = tid; i < N; i += kFusionThreads) {
            unsigned l = (unsigned)a.labeling[i];
            if (l >= (unsigned)a.L) {  // (the host has checked the labelling: what is out of range indexes nothing)
                atomicMin(a.status, MSM_ERR_INVALID);
                l = 0;
            }
            w[2 * (size_t)i] = a.U[(size_t)l * N + i];
            w[2 * (size_t)i + 1] = a.U[(size_t)a.label * N + i];
        }
        u2 = w;
        __syncthreads();
    }
    bool bad_u = false, bad_o = false;
    for (unsigned i = tid; i < N; i += kFusionThreads) {
        const double u0 = u2[2 * (size_t)i], u1 = u2[2 * (size_t)i + 1];
        bad_u |= !finite(u0) || !finite(u1);
        a.eterms[term_at(i, C, 0)] = u0;
        a.cand[i] = 0;
    }
    for (unsigned t = tid; t < T; t += kFusionThreads) {
#pragma unroll
        for (int e = 0; e < 8; ++e) bad_o |= !finite(a.octets[8 * (size_t)t + e]);
        a.eterms[term_at((size_t)N + t, C, 0)] = a.octets[8 * (size_t)t];
#pragma unroll
        for (int e = 0; e < 6; ++e) m[6 * (size_t)t + e] = 0.0;
    }
    if (bad_u) s_bad[0] = 1;
    if (bad_o) s_bad[1] = 1;
    __syncthreads();

    // ---- the sweeps
    int run = 0;
    for (int k = 0; k < a.S && T > 0; ++k) {
        for (int lv = 0; lv < a.levels; ++lv) {
            const int begin = a.level_off[lv], end = a.level_off[lv + 1];
            bool ch = false;
            for (int idx = begin + (int)tid; idx < end; idx += kFusionThreads) ch |= update_factor(a, u2, m, idx);
            if (ch) s_changed = 1;
            __syncthreads();
        }
        const int changed = s_changed;
        run = k + 1;
        uint8_t *lab = a.cand + (size_t)(k + 1) * N;
        decode_and_bound(a, u2, m, lab, SB, (size_t)k, tid);
        __syncthreads();  // the decode is complete (and every thread has read s_changed)
        energy_terms(a, u2, lab, C, (size_t)k + 1, tid);
        if (tid == 0) s_changed = 0;
        __syncthreads();
        if (!changed) break;  // a fixed point: every thread read the same word
    }

    if (run == 0) {  // no sweep ran: the bound of the zero messages
        decode_and_bound(a, u2, m, nullptr, SB, 0, tid);
        __syncthreads();
    }

    // ---- the rounding: conditioned decode over the colour classes, then the polish passes
    int passes = 0;
    if (a.P > 0) {
        bool bad_m = false;
        for (size_t idx = tid; idx < 6 * (size_t)T; idx += kFusionThreads) bad_m |= !finite(m[idx]);
        if (bad_m) s_bad[2] = 1;
        uint8_t *cur = a.cand + (S + 1) * N;
        for (int c = 0; c < a.classes; ++c) {
            const int begin = a.class_off[c], end = a.class_off[c + 1];
            for (int p = begin + (int)tid; p < end; p += kFusionThreads) {
                const unsigned i = (unsigned)a.cls_node[p];
                double s0, s1;
                round_scores<false>(a, u2, m, cur, i, c, s0, s1);
                cur[i] = (uint8_t)(s1 < s0 ? 1 : 0);
            }
            __syncthreads();
        }
        energy_terms(a, u2, cur, C, S + 1, tid);
        __syncthreads();
        for (int p = 0; p < a.P; ++p) {
            const uint8_t *prev = a.cand + (S + 1 + p) * N;
            uint8_t *lab = a.cand + (S + 2 + p) * N;
            for (unsigned i = tid; i < N; i += kFusionThreads) lab[i] = prev[i];
            __syncthreads();
            for (int c = 0; c < a.classes; ++c) {
                const int begin = a.class_off[c], end = a.class_off[c + 1];
                bool ch = false;
                for (int q = begin + (int)tid; q < end; q += kFusionThreads) {
                    const unsigned i = (unsigned)a.cls_node[q];
                    double sc[2];
                    round_scores<true>(a, u2, m, lab, i, 0, sc[0], sc[1]);
                    const int mine = lab[i];
                    int best = sc[1] < sc[0] ? 1 : 0;
                    if (!((best ? sc[1] : sc[0]) < (mine ? sc[1] : sc[0]))) best = mine;  // kept unless another label is strictly lower
                    if (best != mine) lab[i] = (uint8_t)best, ch = true;
                }
                if (ch) s_changed = 1;
                __syncthreads();
            }
            const int changed = s_changed;
            passes = p + 1;
            energy_terms(a, u2, lab, C, S + 2 + p, tid);
            __syncthreads();
            if (tid == 0) s_changed = 0;
            __syncthreads();
            if (!changed) break;  // a fixed point
        }
    }
    __syncthreads();

    // ---- the sums, a thread per sum, in the literal's order: usum and tsum of every candidate that arose, the bound of every sweep that ran
    for (size_t j = tid; j < 2 * C + SB; j += kFusionThreads) {
        double v = 0.0;
        if (j < 2 * C) {
            const size_t slot = j < C ? j : j - C;
            const bool arose = slot == 0 || (slot <= S ? slot <= (size_t)run : slot == S + 1 ? a.P > 0 : slot - (S + 2) < (size_t)passes);
            if (arose) v = j < C ? serial_sum(a.eterms, 0, N, C, slot) : serial_sum(a.eterms, N, T, C, slot);
        } else if (j - 2 * C < (size_t)(run > 0 ? run : 1))
            v = serial_sum(a.bterms, 0, (size_t)N + T, SB, j - 2 * C);
        a.sums[j] = v;
    }
    if (tid == 0) {
        a.head[0] = run;
        a.head[1] = passes;
        a.head[2] = s_bad[2];
        a.head[3] = s_bad[0];
        a.head[4] = s_bad[1];
        a.head[5] = a.head[6] = a.head[7] = 0;
    }
}

}  // namespace

int launch_fusion_mplp(msm_ctx *ctx, const FusionMplpArgs &a, bool lds) {
    const size_t bytes = lds ? sizeof(double) * 6 * (size_t)a.T : 0;
    if (bytes > kFusionLdsBudget) return fail(MSM_ERR_CAPACITY, "msm_fusion_mplp_step: %zu bytes of messages do not fit in LDS", bytes);
    if (lds) {
        if (bytes > 64 * 1024)
            MSM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fusion_mplp<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(k_fusion_mplp<true>, dim3(1), dim3(kFusionThreads), bytes, ctx->stream, a);
    } else
        hipLaunchKernelGGL(k_fusion_mplp<false>, dim3(1), dim3(kFusionThreads), 0, ctx->stream, a);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
