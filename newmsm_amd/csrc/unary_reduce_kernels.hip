// unary_reduce_kernels.hip -- the unary label-cost table's reductions, U[label * N + node] = AbsoluteWeights[node] * similarity of the moving patch
// with the label's sampled target patch, and the two launchers of a table: sampler (unary_kernels.hip: launch_samples), then one of
//
//   univariate (the samplers filled tval)
//     k_unary_reduce_rows         correlation / SSD, behind either sampler, patches up to 96 points: eight lanes per table row, the moving side
//                                 prepared by the passengers of the fix-up launch (unary_kernels.hip: k_unary_fixup)
//     k_unary_reduce_flat         the same for larger patches: a workgroup per control point, eight lanes per label, the moving patch staged in LDS
//     k_unary_reduce_univariate   DICE / genDICE, a wavefront per label: all control points behind k_unary_rays; behind k_unary_samples only the
//                                 control points of its redo list (that sampler reduces the ones it settles itself)
//   multivariate / patchwise (the samplers stored triangle and raw weights per sample), behind either sampler
//     k_unary_reduce_mv8          multivariate, 12 <= D <= 64, correlation / SSD: eight lanes per patch point
//     k_unary_reduce_pw8<4|8>     patchwise, 12 <= D <= 32 | 64, correlation / SSD: the same layout
//     k_unary_reduce_features     every other D, and DICE: a lane per patch point
//
// Which of them runs is the plan's decision (unary_plan.cpp: unary_plan), not this unit's; only the form of the plan's "flat" reduction (rows or the
// staged kernel, unary.hpp: unary_row_form) is settled here, in launch_unary_univariate.
#include <algorithm>

#include "similarity_device.hpp"
#include "unary.hpp"

namespace msm {

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace

// One argument block for the six kernels; each reads the members its comment names and ignores the rest.
struct ReduceArgs {
    int N, L, Nsrc, D;
    const int *pptr, *pidx;
    const int *nodes;             // the nodes this launch reduces, in this order, or nullptr for all N (flat, univariate, mv8, pw8)
    const unsigned int *nnodes;   // how many of them, read on the device, or nullptr for N (univariate)
    const double *absw;
    const double *sfeat;          // D x Nsrc
    const double *cfw;            // rows x Nsrc or nullptr
    int cfw_rows;
    const double *sfeat_vm;       // Nsrc x D vertex-major copy of the moving features (mv8, pw8)
    const double *cfw_vm;         // Nsrc x cfw_rows vertex-major copy of the weights, or nullptr (mv8, pw8)
    const double *tval;           // the samples' values (flat, univariate)
    const int *stri;              // the samples' triangles and raw weights (features, mv8, pw8)
    const double *sw3;
    const double *tfeat;          // V x D vertex-major (features, mv8, pw8)
    const TriRec *rec;
    int simmeasure;
    double percentile;            // DICE measures (univariate, features)
    int patchwise;                // features
    int pmax;                     // the LDS slices' stride (flat, univariate, features)
    double *U;
    const double *mov_a, *mov_w, *mov_stat;  // the prepared moving side (rows): patches and weights in patch order, 3 x N statistics
};

// ------------------------------------------------------------------------------------------------
// Univariate DICE / genDICE reduction: AbsoluteWeights[node] * get_sim_for_min(source patch, target patch)
// (UnivariateNonLinearSRegDiscreteCostFunction::computeUnaryCost, :378-383; M/similarities.h:48-58), one wavefront per label.  Only these two
// measures reach it (correlation and SSD go to k_unary_reduce_flat); they rank values and read no weights.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unary_reduce_univariate(ReduceArgs a) {
    extern __shared__ __align__(16) double lds[];
    double *sA = lds;  // pmax doubles; the launch's second slice is reserved and unread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned n = a.nnodes ? *a.nnodes : (unsigned)a.N;
    for (unsigned k = blockIdx.x; k < n; k += gridDim.x) {
        const int node = a.nodes ? a.nodes[k] : (int)k;
        const int beg = a.pptr[node], P = a.pptr[node + 1] - beg;
        __syncthreads();
        for (int i = tid; i < P; i += 256) sA[i] = a.sfeat[a.pidx[beg + i]];
        __syncthreads();
        const double absw = a.absw[node];
        for (int l = wave; l < a.L; l += 4) {
            const double cost = patch_dice(sA, a.tval + (size_t)a.L * beg + (size_t)l * P, P, lane, a.simmeasure, a.percentile);
            if (lane == 0) a.U[(size_t)l * a.N + node] = absw * cost;
        }
    }
}

// The correlation / SSD reduction of a whole table: one workgroup per control point stages the moving patch (feature, weight) in LDS once; an 8-lane
// group per label (32 labels per pass) reads that label's sampled target patch, contiguous in tval, into registers while the staging loads are still in
// flight -- the kernel is a chain of dependent loads, so they are issued as early as they can be.  The 8-lane sums
// are DPP row operations.  The weighted mean and variance of the moving patch do not depend on the label and are
// computed once.  The last kernel of the launch, it also clears the fix-up counters for the next one.
constexpr int kRedLanes = 8;      // lanes per label
constexpr int kRedKeep = 12;      // target values per lane kept in registers (patches up to 96 points)

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int off = kRedLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kRedLanes);
    return v;
}

__global__ __launch_bounds__(256) void k_unary_reduce_flat(ReduceArgs a, unsigned int *clear, int clear_words) {
    extern __shared__ __align__(16) double lds[];
    double *sA = lds, *sW = sA + a.pmax;
    __shared__ double s_stat[3];  // sum of weights, weighted mean of A, weighted variance sum of A
    const int tid = threadIdx.x, sub = tid & (kRedLanes - 1), grp = tid / kRedLanes;
    if (blockIdx.x == 0 && clear)
        for (int k = tid; k < clear_words; k += 256) clear[k] = 0u;
    const int node = a.nodes ? a.nodes[blockIdx.x] : (int)blockIdx.x;  // launch order = Morton order
    const int beg = a.pptr[node], P = a.pptr[node + 1] - beg;
    const bool has_w = a.cfw && a.cfw_rows >= 1;
    double breg[kRedKeep];  // the first kRedKeep values per lane always travel through registers
#pragma unroll
    for (int k = 0; k < kRedKeep; ++k) breg[k] = 0.0;
    if (grp < a.L) {
        const double *B = a.tval + (size_t)a.L * beg + (size_t)grp * P;
#pragma unroll
        for (int k = 0; k < kRedKeep; ++k) breg[k] = (sub + kRedLanes * k < P) ? B[sub + kRedLanes * k] : 0.0;
    }
    for (int i = tid; i < P; i += 256) {
        const int s = a.pidx[beg + i];
        sA[i] = a.sfeat[s];
        sW[i] = has_w ? a.cfw[s] : 1.0;
    }
    __syncthreads();
    if (a.simmeasure == 2) {
        if (tid < 64) {  // one wavefront: moving-patch statistics
            double sw = 0, ma = 0;
            for (int i = tid; i < P; i += 64) {
                sw += sW[i];
                ma += sW[i] * sA[i];
            }
            sw = wave_sum(sw);
            ma = wave_sum(ma);
            if (sw > 0.0) ma /= sw;
            double va = 0;
            for (int i = tid; i < P; i += 64) {
                const double da = sA[i] - ma;
                va += sW[i] * da * da;
            }
            va = wave_sum(va);
            if (tid == 0) s_stat[0] = sw, s_stat[1] = ma, s_stat[2] = va;
        }
        __syncthreads();
    }
    const double absw = a.absw[node];
    for (int l = grp; l < a.L; l += 256 / kRedLanes) {
        const double *B = a.tval + (size_t)a.L * beg + (size_t)l * P;
        if (l != grp) {  // not prefetched: more than 32 labels
#pragma unroll
            for (int k = 0; k < kRedKeep; ++k) breg[k] = (sub + kRedLanes * k < P) ? B[sub + kRedLanes * k] : 0.0;
        }
        double cost;
        if (a.simmeasure == 2) {  // sparsesimkernel::corr, M/similarities.cpp:129-158
            const double sw = s_stat[0], ma = s_stat[1];
            double mb = 0;
#pragma unroll
            for (int k = 0; k < kRedKeep; ++k) {
                const int i = sub + kRedLanes * k;
                if (i < P) mb += sW[i] * breg[k];
            }
            for (int i = sub + kRedLanes * kRedKeep; i < P; i += kRedLanes) mb += sW[i] * B[i];
            mb = group_sum(mb);
            if (sw > 0.0) mb /= sw;
            double pr = 0, vb = 0;
#pragma unroll
            for (int k = 0; k < kRedKeep; ++k) {
                const int i = sub + kRedLanes * k;
                if (i < P) {
                    const double da = sA[i] - ma, db = breg[k] - mb;
                    pr += sW[i] * da * db;
                    vb += sW[i] * db * db;
                }
            }
            for (int i = sub + kRedLanes * kRedKeep; i < P; i += kRedLanes) {
                const double da = sA[i] - ma, db = B[i] - mb;
                pr += sW[i] * da * db;
                vb += sW[i] * db * db;
            }
            pr = group_sum(pr);
            vb = group_sum(vb);
            double va = s_stat[2];
            if (sw > 0.0) {
                pr /= sw;
                va /= sw;
                vb /= sw;
            }
            const double r = (va == 0.0 || vb == 0.0) ? 0.0 : pr / (sqrt(va) * sqrt(vb));
            cost = 1 - (1 + r) * 0.5;
        } else {  // sparsesimkernel::SSD, M/similarities.cpp:179-188
            double pr = 0;
#pragma unroll
            for (int k = 0; k < kRedKeep; ++k) {
                const int i = sub + kRedLanes * k;
                if (i < P) {
                    const double df = sA[i] - breg[k];
                    pr += sW[i] * df * df;
                }
            }
            for (int i = sub + kRedLanes * kRedKeep; i < P; i += kRedLanes) {
                const double df = sA[i] - B[i];
                pr += sW[i] * df * df;
            }
            pr = group_sum(pr);
            cost = sqrt(pr) / P;
        }
        if (sub == 0) a.U[(size_t)l * a.N + node] = absw * cost;
    }
}

// The same reduction by table row, for patches that fit the registers (P <= kRedKeep * kRedLanes): row r = node * L + l belongs to one 8-lane group,
// 32 rows to a workgroup, nodes in their natural order.  The moving patch arrives prepared (mov_a, mov_w in patch order, mov_stat: k_unary_fixup's
// passengers), so a group depends on pptr alone before it issues every load it needs in one batch, and nothing ties it to the other rows of its control
// point: no LDS, no barrier, every lane at work, and the whole table of the benchmark resident at once.  The arithmetic is k_unary_reduce_flat's,
// statement for statement (W: a weight row exists; without one the weights are 1.0 and the products by them are left out, 1.0 * x being x).
static_assert(kRedKeep * kRedLanes == kRowsPmax, "the row form's patch bound is what one group keeps in registers");

template <bool W>
__global__ __launch_bounds__(256) void k_unary_reduce_rows(ReduceArgs a, unsigned int *clear, int clear_words) {
    const int tid = threadIdx.x, sub = tid & (kRedLanes - 1);
    if (blockIdx.x == 0 && clear)
        for (int k = tid; k < clear_words; k += 256) clear[k] = 0u;
    const long long row = (long long)blockIdx.x * (256 / kRedLanes) + tid / kRedLanes;
    if (row >= (long long)a.N * a.L) return;  // whole groups leave: the sums below stay inside a group
    const int node = (int)(row / a.L), l = (int)(row - (long long)node * a.L);
    const int beg = a.pptr[node], P = a.pptr[node + 1] - beg;
    const double *B = a.tval + (size_t)a.L * beg + (size_t)l * P;
    const double *A = a.mov_a + beg, *Wt = W ? a.mov_w + beg : nullptr;
    double breg[kRedKeep], areg[kRedKeep], wreg[kRedKeep];  // (wreg: unread without a weight row)
#pragma unroll
    for (int k = 0; k < kRedKeep; ++k) {
        const int i = sub + kRedLanes * k;
        breg[k] = i < P ? B[i] : 0.0;
        areg[k] = i < P ? A[i] : 0.0;
        wreg[k] = (W && i < P) ? Wt[i] : 0.0;
    }
    const double absw = a.absw[node];
    double cost;
    if (a.simmeasure == 2) {  // sparsesimkernel::corr, M/similarities.cpp:129-158
        const double sw = a.mov_stat[3 * (size_t)node], ma = a.mov_stat[3 * (size_t)node + 1];
        double va = a.mov_stat[3 * (size_t)node + 2];
        double mb = 0;
#pragma unroll
        for (int k = 0; k < kRedKeep; ++k)
            if (sub + kRedLanes * k < P) mb += W ? wreg[k] * breg[k] : breg[k];
        mb = group_sum(mb);
        if (sw > 0.0) mb /= sw;
        double pr = 0, vb = 0;
#pragma unroll
        for (int k = 0; k < kRedKeep; ++k)
            if (sub + kRedLanes * k < P) {
                const double da = areg[k] - ma, db = breg[k] - mb;
                pr += W ? wreg[k] * da * db : da * db;
                vb += W ? wreg[k] * db * db : db * db;
            }
        pr = group_sum(pr);
        vb = group_sum(vb);
        if (sw > 0.0) {
            pr /= sw;
            va /= sw;
            vb /= sw;
        }
        const double r = (va == 0.0 || vb == 0.0) ? 0.0 : pr / (sqrt(va) * sqrt(vb));
        cost = 1 - (1 + r) * 0.5;
    } else {  // sparsesimkernel::SSD, M/similarities.cpp:179-188
        double pr = 0;
#pragma unroll
        for (int k = 0; k < kRedKeep; ++k)
            if (sub + kRedLanes * k < P) {
                const double df = areg[k] - breg[k];
                pr += W ? wreg[k] * df * df : df * df;
            }
        pr = group_sum(pr);
        cost = sqrt(pr) / P;
    }
    if (sub == 0) a.U[(size_t)l * a.N + node] = absw * cost;
}

// ------------------------------------------------------------------------------------------------
// Multivariate / patchwise reductions from the stored (triangle, raw weights) of every sample.
//   multivariate (M/DiscreteCostFunction.cpp:444-458): mean over the patch points of a D-long feature-vector
//                similarity; one lane per patch point, the D loop runs inside the lane;
//   patchwise    (:680-692): per feature channel a patch similarity (lanes over points, shuffle reduction),
//                averaged over the channels.
// One workgroup per control point, one wavefront per label.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unary_reduce_features(ReduceArgs a) {
    const int node = blockIdx.x;
    const int beg = a.pptr[node], P = a.pptr[node + 1] - beg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double absw = a.absw[node];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int nwaves = blockDim.x >> 6;  // 4, or 1 when a patch is so large that only one wavefront's LDS slice fits
    for (int l = wave; l < a.L; l += nwaves) {
        const size_t g0 = (size_t)a.L * beg + (size_t)l * P;
        double cost;
        if (!a.patchwise) {
            double acc = 0.0;
            bool bad = false;
            for (int i = lane; i < P; i += 64) {
                const int t = a.stri[g0 + i];
                if (t < 0) {
                    bad = true;
                    continue;
                }
                const TriRec &r = a.rec[t];
                const double *f0 = a.tfeat + (size_t)r.id[0] * a.D, *f1 = a.tfeat + (size_t)r.id[1] * a.D, *f2 = a.tfeat + (size_t)r.id[2] * a.D;
                acc += feature_vector_similarity(a.simmeasure, a.percentile, a.sfeat, a.cfw, a.cfw_rows, a.Nsrc, a.pidx[beg + i], a.D, f0, f1, f2,
                                                 a.sw3[3 * (g0 + i)], a.sw3[3 * (g0 + i) + 1], a.sw3[3 * (g0 + i) + 2]);
            }
            acc = wave_sum(acc);
            cost = P > 0 ? acc / P : acc;
            if (__ballot(bad)) cost = nan;
        } else {
            double total = 0.0;
            bool bad = false;
            for (int d = 0; d < a.D; ++d) {
                const double *A = a.sfeat + (size_t)d * a.Nsrc;
                auto Bv = [&](int i) {
                    const int t = a.stri[g0 + i];
                    if (t < 0) {
                        bad = true;
                        return nan;
                    }
                    const TriRec &r = a.rec[t];
                    return a.sw3[3 * (g0 + i)] * a.tfeat[(size_t)r.id[0] * a.D + d] + a.sw3[3 * (g0 + i) + 1] * a.tfeat[(size_t)r.id[1] * a.D + d] +
                           a.sw3[3 * (g0 + i) + 2] * a.tfeat[(size_t)r.id[2] * a.D + d];
                };
                auto Wv = [&](int i) { return (a.cfw && a.cfw_rows >= 1) ? a.cfw[a.pidx[beg + i]] : 1.0; };
                double c;
                if (a.simmeasure == 4 || a.simmeasure == 5) {
                    // DICE ranks every value against every other one: stage the two patches of this channel in the
                    // wavefront's LDS slice first (the wavefront runs in lockstep: its own LDS writes are visible to all
                    // of its lanes once they have been issued and waited for)
                    extern __shared__ __align__(16) double lds[];
                    double *pa = lds + (size_t)wave * 2 * a.pmax, *pb = pa + a.pmax;
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    for (int i = lane; i < P; i += 64) {
                        pa[i] = A[a.pidx[beg + i]];
                        pb[i] = Bv(i);
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    c = patch_dice(pa, pb, P, lane, a.simmeasure, a.percentile);
                } else if (a.simmeasure == 2) {
                    double sw = 0, ma = 0, mb = 0;
                    for (int i = lane; i < P; i += 64) {
                        const double w = Wv(i);
                        sw += w;
                        ma += w * A[a.pidx[beg + i]];
                        mb += w * Bv(i);
                    }
                    sw = wave_sum(sw);
                    ma = wave_sum(ma);
                    mb = wave_sum(mb);
                    if (sw > 0.0) {
                        ma /= sw;
                        mb /= sw;
                    }
                    double pr = 0, va = 0, vb = 0;
                    for (int i = lane; i < P; i += 64) {
                        const double w = Wv(i), da = A[a.pidx[beg + i]] - ma, db = Bv(i) - mb;
                        pr += w * da * db;
                        va += w * da * da;
                        vb += w * db * db;
                    }
                    pr = wave_sum(pr);
                    va = wave_sum(va);
                    vb = wave_sum(vb);
                    if (sw > 0.0) {
                        pr /= sw;
                        va /= sw;
                        vb /= sw;
                    }
                    const double r = (va == 0.0 || vb == 0.0) ? 0.0 : pr / (sqrt(va) * sqrt(vb));
                    c = 1 - (1 + r) * 0.5;
                } else {
                    double pr = 0;
                    for (int i = lane; i < P; i += 64) {
                        const double df = A[a.pidx[beg + i]] - Bv(i);
                        pr += Wv(i) * df * df;
                    }
                    pr = wave_sum(pr);
                    c = sqrt(pr) / P;
                }
                total += c;
            }
            cost = total / a.D;
            if (__ballot(bad)) cost = nan;
        }
        if (lane == 0) a.U[(size_t)l * a.N + node] = absw * cost;
    }
}

// ------------------------------------------------------------------------------------------------
// Multivariate reduction, D <= 64, SSD / correlation (M/DiscreteCostFunction.cpp:444-458): eight lanes per patch point.
// With a lane per point and the D loop inside the lane (k_unary_reduce_features) every one of the ~4 D loads of a
// point is its own cache-line lookup (moving features D x Nsrc row-major: a different line per dimension) -- about 250
// lookups per sample, 1.9 ms per table at D = 32.  Here lane j of a group owns the dimensions j, j + 8, ...: the
// group reads the three target rows (vertex-major) and the moving row (a vertex-major copy) as contiguous 64-byte
// pieces, and the sums over the dimensions are 8-lane DPP reductions.  One wavefront per label, eight points at a time.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unary_reduce_mv8(ReduceArgs a) {
    const int node = a.nodes[blockIdx.x];
    const int beg = a.pptr[node], P = a.pptr[node + 1] - beg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane / kMvLanes, j = lane % kMvLanes;
    const double absw = a.absw[node];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int D = a.D;
    for (int l = wave; l < a.L; l += 4) {
        const size_t g0 = (size_t)a.L * beg + (size_t)l * P;
        double acc = 0.0;  // this group's points (lane 0 of the group holds the value)
        bool bad = false;
        for (int i0 = 0; i0 < P; i0 += 64 / kMvLanes) {  // wavefront-uniform: the group sums need all lanes
            const int i = i0 + grp;
            const bool have = i < P;
            int t = -1, sv = 0;
            double wa = 0, wb = 0, wc = 0;
            if (have) {
                t = a.stri[g0 + i];
                sv = a.pidx[beg + i];
                wa = a.sw3[3 * (g0 + i)], wb = a.sw3[3 * (g0 + i) + 1], wc = a.sw3[3 * (g0 + i) + 2];
            }
            if (have && t < 0) bad = true;
            const bool go = have && t >= 0;
            const double *f0 = a.tfeat, *f1 = a.tfeat, *f2 = a.tfeat, *sa = a.sfeat_vm, *cw = nullptr;
            if (go) {
                const TriRec &r = a.rec[t];
                f0 = a.tfeat + (size_t)r.id[0] * D, f1 = a.tfeat + (size_t)r.id[1] * D, f2 = a.tfeat + (size_t)r.id[2] * D;
                sa = a.sfeat_vm + (size_t)sv * D;
                cw = a.cfw_vm ? a.cfw_vm + (size_t)sv * a.cfw_rows : nullptr;
            }
            const double c = feature_vector_similarity8(a.simmeasure, go, j, D, sa, cw, a.cfw_rows, f0, f1, f2, wa, wb, wc);
            if (go && j == 0) acc += c;
        }
        // the groups' partial sums: one value per group in its lane 0
        double tot = (j == 0) ? acc : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
        double cost = P > 0 ? tot / P : tot;
        if (__ballot(bad)) cost = nan;
        if (lane == 0) a.U[(size_t)l * a.N + node] = absw * cost;
    }
}

// ------------------------------------------------------------------------------------------------
// Patchwise reduction, D <= 8 * K, SSD / correlation (M/DiscreteCostFunction.cpp:680-692: per feature channel a patch
// similarity, averaged over the channels), in the layout of k_unary_reduce_mv8: eight lanes per patch point, lane j owns
// the channels j, j + 8, ...; here the sums run over the POINTS, so every lane accumulates its channels over its group's
// points and the eight groups of the wavefront are combined with three shuffle steps.  Two passes over the patch
// (means, then moments); the second pass re-reads the rows (cache hits) instead of keeping them in registers.
// ------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void k_unary_reduce_pw8(ReduceArgs a) {
    const int node = a.nodes[blockIdx.x];
    const int beg = a.pptr[node], P = a.pptr[node + 1] - beg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane / kMvLanes, j = lane % kMvLanes;
    const double absw = a.absw[node];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int D = a.D;
    auto across_groups = [](double v) {  // lanes with the same j: the eight groups of the wavefront
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        return v;
    };
    for (int l = wave; l < a.L; l += 4) {
        const size_t g0 = (size_t)a.L * beg + (size_t)l * P;
        bool bad = false;
        // one point of the patch for this lane's group: moving row, interpolated target row (this lane's channels), weight
        auto fetch = [&](int i, double *A, double *B, double &w) {
            const int t = a.stri[g0 + i];
            const int sv = a.pidx[beg + i];
            w = (a.cfw_vm && a.cfw_rows >= 1) ? a.cfw_vm[(size_t)sv * a.cfw_rows] : 1.0;
            if (t < 0) {
                bad = true;
#pragma unroll
                for (int k = 0; k < K; ++k) A[k] = B[k] = nan;
                return;
            }
            const TriRec &r = a.rec[t];
            const double *f0 = a.tfeat + (size_t)r.id[0] * D, *f1 = a.tfeat + (size_t)r.id[1] * D, *f2 = a.tfeat + (size_t)r.id[2] * D;
            const double *sa = a.sfeat_vm + (size_t)sv * D;
            const double wa = a.sw3[3 * (g0 + i)], wb = a.sw3[3 * (g0 + i) + 1], wc = a.sw3[3 * (g0 + i) + 2];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int d = j + kMvLanes * k;
                A[k] = d < D ? sa[d] : 0.0;
                B[k] = d < D ? wa * f0[d] + wb * f1[d] + wc * f2[d] : 0.0;
            }
        };
        double c[K];
        if (a.simmeasure == 2) {  // sparsesimkernel::corr over the patch points, per channel
            double sw = 0.0, ma[K], mb[K];
#pragma unroll
            for (int k = 0; k < K; ++k) ma[k] = mb[k] = 0.0;
            for (int i = grp; i < P; i += 64 / kMvLanes) {
                double A[K], B[K], w;
                fetch(i, A, B, w);
                sw += w;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    ma[k] += w * A[k];
                    mb[k] += w * B[k];
                }
            }
            sw = across_groups(sw);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                ma[k] = across_groups(ma[k]);
                mb[k] = across_groups(mb[k]);
                if (sw > 0.0) {
                    ma[k] /= sw;
                    mb[k] /= sw;
                }
            }
            double pr[K], va[K], vb[K];
#pragma unroll
            for (int k = 0; k < K; ++k) pr[k] = va[k] = vb[k] = 0.0;
            for (int i = grp; i < P; i += 64 / kMvLanes) {
                double A[K], B[K], w;
                fetch(i, A, B, w);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double da = A[k] - ma[k], db = B[k] - mb[k];
                    pr[k] += w * da * db;
                    va[k] += w * da * da;
                    vb[k] += w * db * db;
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double p = across_groups(pr[k]), x = across_groups(va[k]), y = across_groups(vb[k]);
                if (sw > 0.0) {
                    p /= sw;
                    x /= sw;
                    y /= sw;
                }
                const double rr = (x == 0.0 || y == 0.0) ? 0.0 : p / (sqrt(x) * sqrt(y));
                c[k] = 1 - (1 + rr) * 0.5;
            }
        } else {  // sparsesimkernel::SSD
            double pr[K];
#pragma unroll
            for (int k = 0; k < K; ++k) pr[k] = 0.0;
            for (int i = grp; i < P; i += 64 / kMvLanes) {
                double A[K], B[K], w;
                fetch(i, A, B, w);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double df = A[k] - B[k];
                    pr[k] += w * df * df;
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) c[k] = sqrt(across_groups(pr[k])) / P;
        }
        double total = 0.0;  // this lane's channels, then the eight lanes of the group (all groups hold the same values)
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (j + kMvLanes * k < D) total += c[k];
        total = mv_group_sum(total);
        double cost = total / D;
        if (__ballot(bad)) cost = nan;
        if (lane == 0) a.U[(size_t)l * a.N + node] = absw * cost;
    }
}

// ------------------------------------------------------------------------------------------------
// launch: plan check, LDS attribute, sampler, arguments, the plan's reduction
// ------------------------------------------------------------------------------------------------
static ReduceArgs reduce_args(const UnaryLaunch &u, const UnaryWeightsScratch *w) {
    ReduceArgs r;
    r.N = u.N, r.L = u.L, r.Nsrc = u.Nsrc, r.D = u.D;
    r.pptr = u.pptr, r.pidx = u.pidx;
    r.nodes = u.order;  // all control points, in launch order
    r.nnodes = nullptr;
    r.absw = u.absw;
    r.sfeat = u.sfeat, r.cfw = u.cfw, r.cfw_rows = u.cfw_rows;
    r.sfeat_vm = u.sfeat_vm, r.cfw_vm = u.cfw_vm;
    r.tval = u.tval;
    r.stri = w ? w->stri : nullptr, r.sw3 = w ? w->sw3 : nullptr;
    r.tfeat = u.tfeat, r.rec = u.tree.rec;
    r.simmeasure = u.simmeasure, r.percentile = u.percentile;
    r.patchwise = 0;
    r.pmax = u.pmax;
    r.U = u.U;
    r.mov_a = u.mov_a, r.mov_w = u.mov_w, r.mov_stat = u.mov_stat;
    return r;
}

int launch_unary_univariate(msm_ctx *ctx, const UnaryLaunch &u) {
    const bool dice = u.simmeasure == 4 || u.simmeasure == 5;
    if (!u.plan) return fail(MSM_ERR_STATE, "launch_unary_univariate: no launch plan");
    const UnaryPlan &plan = *u.plan;
    MSM_TRY(unary_plan_refusal(plan, u.pmax));
    // Correlation / SSD: both search paths only fill tval and one kernel reduces it, so the table does not depend on
    // which of them ran (the ray table of a target arrives in the background, api.cpp: ensure_rays).  DICE costs are
    // ratios of counts -- the same from any summation order -- and keep the reduction fused into the complete sampler.
    // ... and one of two kernels: by rows where every patch fits a group's registers and the cost object brought the buffers of the moving side
    const bool rows = !dice && unary_row_form(u.simmeasure, u.pmax) && u.mov_a && u.mov_stat;
    if (!rows) MSM_TRY(dice ? allow_lds(k_unary_reduce_univariate, plan.reduce_lds) : allow_lds(k_unary_reduce_flat, plan.reduce_lds));
    MSM_TRY(launch_samples(ctx, u, plan, nullptr, dice, rows));
    ReduceArgs r = reduce_args(u, nullptr);
    if (u.route) *u.route = plan.reduce;
    if (u.form) *u.form = rows ? MSM_UNARY_FORM_ROWS : MSM_UNARY_FORM_STAGED;
    if (rows) {
        const unsigned blocks = (unsigned)(((long long)u.N * u.L + 256 / kRedLanes - 1) / (256 / kRedLanes));
        if (u.cfw && u.cfw_rows >= 1) {
            hipLaunchKernelGGL(k_unary_reduce_rows<true>, dim3(blocks), dim3(256), 0, ctx->stream, r, u.fix_cnt, (int)unary_fix_counter_words());
        } else {
            hipLaunchKernelGGL(k_unary_reduce_rows<false>, dim3(blocks), dim3(256), 0, ctx->stream, r, u.fix_cnt, (int)unary_fix_counter_words());
        }
    } else if (!dice) {
        hipLaunchKernelGGL(k_unary_reduce_flat, dim3(u.N), dim3(256), plan.reduce_lds, ctx->stream, r, u.fix_cnt, (int)unary_fix_counter_words());
    } else {
        int blocks = 64;
        if (plan.sampler == MSM_SAMPLER_RAYS) {  // all control points, in their own order
            r.nodes = nullptr;
            blocks = std::min(u.N, 2048);
        } else {  // the control points that had deferred samples, now that the fix-up kernel has filled them in
            r.nodes = u.redo_list;
            r.nnodes = u.fix_cnt;
        }
        hipLaunchKernelGGL(k_unary_reduce_univariate, dim3(blocks), dim3(256), plan.reduce_lds, ctx->stream, r);
        MSM_HIP(hipMemsetAsync(u.fix_cnt, 0, unary_fix_counter_words() * sizeof(unsigned), ctx->stream));  // counters are zero between launches
    }
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_unary_multivariate(msm_ctx *ctx, const UnaryLaunch &u, const UnaryWeightsScratch &w, bool patchwise) {
    if (!u.plan) return fail(MSM_ERR_STATE, "launch_unary_multivariate: no launch plan");
    const UnaryPlan &plan = *u.plan;
    MSM_TRY(unary_plan_refusal(plan, u.pmax));
    if (plan.reduce != MSM_UNARY_FEATURES && !u.sfeat_vm) return fail(MSM_ERR_STATE, "vertex-major features missing");
    if (plan.reduce == MSM_UNARY_FEATURES) MSM_TRY(allow_lds(k_unary_reduce_features, plan.reduce_lds));
    MSM_TRY(launch_samples(ctx, u, plan, &w, false));
    ReduceArgs r = reduce_args(u, &w);
    r.patchwise = patchwise ? 1 : 0;
    if (plan.reduce == MSM_UNARY_MV8) {
        hipLaunchKernelGGL(k_unary_reduce_mv8, dim3(u.N), dim3(256), 0, ctx->stream, r);
    } else if (plan.reduce == MSM_UNARY_PW8_4) {
        hipLaunchKernelGGL(k_unary_reduce_pw8<4>, dim3(u.N), dim3(256), 0, ctx->stream, r);
    } else if (plan.reduce == MSM_UNARY_FEATURES) {
        hipLaunchKernelGGL(k_unary_reduce_features, dim3(u.N), dim3(plan.reduce_threads), plan.reduce_lds, ctx->stream, r);
    } else {
        hipLaunchKernelGGL(k_unary_reduce_pw8<8>, dim3(u.N), dim3(256), 0, ctx->stream, r);
    }
    if (u.route) *u.route = plan.reduce;
    MSM_HIP(hipGetLastError());
    MSM_HIP(hipMemsetAsync(u.fix_cnt, 0, unary_fix_counter_words() * sizeof(unsigned), ctx->stream));  // counters are zero between launches
    return MSM_OK;
}

}  // namespace msm
