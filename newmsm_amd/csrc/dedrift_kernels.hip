// dedrift_kernels.hip -- the post-processing of a groupwise run on gfx950 (gMSM_scripts/gMSM_tutorial/gw_MSM.sh:65-128 and compare_stats.py, which
// the reference runs through wb_command and nibabel): the dedrift warp, the distortion maps of the corrected spheres and the group statistics.
//
//   k_dedrift_accumulate  one lane per template vertex: the subject's input sphere interpolated with the weights the search found on its registered
//                         sphere (project_anatomical_mesh's sum, ascending vertex id), added to the running sum.  One launch per subject on the
//                         context's stream: the order of the additions is the order of the calls.
//   k_dedrift_finish      one workgroup: drift = sum / S, its bounding box (min / max: exact in any order, reduced in a fixed tree anyway), recentred on
//                         the box's midpoint and scaled to radius 100.
//   k_vertex_distortion   one lane per vertex: J and R of triangle_strain (strain_device.hpp) for each incident triangle in trID order, the plain mean
//                         of log2 J and log2 R.
// The group statistics, over a list of the resident subjects (nullptr: all of them in order) and the template vertices a mask keeps (nullptr: all K = Vt
// of them); per-map results and the matrices are indexed by list position:
//   k_dedrift_moments     one lane per map element: mean over the listed subjects, then the population standard deviation about it, both in list order.
//   k_dedrift_map_stats   one workgroup per listed map: its mean and the root of its summed squared deviations over the kept vertices (a fixed 256-leaf
//                         tree each, reduce_device.hpp: block_sum).
//   k_dedrift_masks       one workgroup per listed map: the two order statistics numpy.percentile interpolates between, by a radix select over an
//                         order-preserving integer key (8 passes of 8 bits, integer LDS counters; the histogram counts kept keys, order statistics and
//                         the interpolation take K); the threshold; the mask x > threshold as one ballot word per 64 kept vertices (bit j of a map's mask
//                         belongs to the j-th kept vertex); its population count.
//   k_dedrift_tile_cc     one workgroup per (tile of 8 x 8 listed subjects, feature): a lane loads one vertex of the tile's 16 map rows and feeds all 64
//                         pairs from it, so a map row is read once per tile and not once per pair; the 64 sums of a lane are reduced over block_sum's
//                         tree, eight side by side (tile_sums), and divided by the two roots.  The tile comes from the grid's coordinates (the lower
//                         triangle's workgroups leave at once): no search for the pair.
//   k_dedrift_tile_dice   the same tiling over the mask words: AND + popcount, integer sums over the same tree.  Integer work: exact.
//   k_dedrift_pair_cc     for a small whole set without a mask (dedrift.cpp: kPerPairMax), where one or three tiles leave the device idle: one workgroup
//                         per (pair, feature), the sum of products of deviations over the same tree, divided by the two roots: the tile kernel's bits.
//   k_dedrift_pair_dice   its companion: one wavefront per (pair, feature), popcount of the ANDed masks.
//   k_dedrift_pair_mean   one workgroup per matrix: the sum over the upper triangle (lane t takes the columns i + 1 + t, + 256, ... of every row i, rows
//                         ascending; block_sum), divided by the number of pairs; NaN for a single subject.
//
// No floating-point atomics anywhere: every floating-point sum has a fixed shape, two runs give the same bits.
#include "dedrift.hpp"
#include "reduce_device.hpp"
#include "strain_device.hpp"

namespace msm {

namespace {

constexpr int kBlock = kSumBlock;
constexpr int kWide = 1024;

__global__ __launch_bounds__(kBlock) void k_dedrift_accumulate(const int32_t *__restrict__ vid, const double *__restrict__ w, int Vt,
                                                               const double *__restrict__ m, int Vs, double *__restrict__ sum,
                                                               double *__restrict__ inverse) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Vt) return;
    if (vid[i] < 0) return;  // a failed search: the query kernel has raised the status, the call fails
    // get_barycentric_weights' std::map: ascending vertex id, a later duplicate overwrites (as kernels.hip: WarpPayload)
    int n = 0, kid[3];
    double kw[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int id = vid[(size_t)j * Vt + i];
        const double wt = w[(size_t)j * Vt + i];
        int pos = 0;
        while (pos < n && kid[pos] < id) ++pos;
        if (pos < n && kid[pos] == id) {
            kw[pos] = wt;
            continue;
        }
        for (int s = n; s > pos; --s) kid[s] = kid[s - 1], kw[s] = kw[s - 1];
        kid[pos] = id, kw[pos] = wt;
        ++n;
    }
    V3 p = mk(0.0, 0.0, 0.0);
    for (int j = 0; j < n; ++j) {
        p.x += m[kid[j]] * kw[j];
        p.y += m[(size_t)Vs + kid[j]] * kw[j];
        p.z += m[2 * (size_t)Vs + kid[j]] * kw[j];
    }
    if (inverse) inverse[i] = p.x, inverse[(size_t)Vt + i] = p.y, inverse[2 * (size_t)Vt + i] = p.z;
    sum[i] += p.x;
    sum[(size_t)Vt + i] += p.y;
    sum[2 * (size_t)Vt + i] += p.z;
}

__global__ __launch_bounds__(kWide) void k_dedrift_finish(const double *__restrict__ sum, int Vt, int S, double *__restrict__ drift,
                                                          double *__restrict__ warp) {
    __shared__ double lo[3][kWide], hi[3][kWide];
    const int t = threadIdx.x;
    const double s = (double)S;
    for (int c = 0; c < 3; ++c) {
        double l = DBL_MAX, h = -DBL_MAX;
        for (int i = t; i < Vt; i += kWide) {
            const double v = sum[(size_t)c * Vt + i] / s;
            drift[(size_t)c * Vt + i] = v;
            l = fmin(l, v), h = fmax(h, v);
        }
        lo[c][t] = l, hi[c][t] = h;
    }
    __syncthreads();
    for (int st = kWide / 2; st > 0; st >>= 1) {
        if (t < st)
            for (int c = 0; c < 3; ++c) lo[c][t] = fmin(lo[c][t], lo[c][t + st]), hi[c][t] = fmax(hi[c][t], hi[c][t + st]);
        __syncthreads();
    }
    const V3 mid = mk((lo[0][0] + hi[0][0]) / 2, (lo[1][0] + hi[1][0]) / 2, (lo[2][0] + hi[2][0]) / 2);
    for (int i = t; i < Vt; i += kWide) {  // every lane reads back what it wrote itself
        const V3 p = scale(normalized(sub(mk(drift[i], drift[(size_t)Vt + i], drift[2 * (size_t)Vt + i]), mid)), kRad);
        warp[i] = p.x, warp[(size_t)Vt + i] = p.y, warp[2 * (size_t)Vt + i] = p.z;
    }
}

__global__ __launch_bounds__(kBlock) void k_vertex_distortion(const double *__restrict__ m, const double *__restrict__ c, int V,
                                                              const int32_t *__restrict__ tri, int T, const int32_t *__restrict__ tid_ptr,
                                                              const int32_t *__restrict__ tid, double *__restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int e0 = tid_ptr[v], e1 = tid_ptr[v + 1];
    double sj = 0.0, sr = 0.0;
    for (int e = e0; e < e1; ++e) {
        const int t = tid[e];
        V3 o[3], f[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int id = tri[(size_t)k * T + t];
            o[k] = mk(m[id], m[(size_t)V + id], m[2 * (size_t)V + id]);
            f[k] = mk(c[id], c[(size_t)V + id], c[2 * (size_t)V + id]);
        }
        double J, R;
        triangular_strain_JR(strain_frame(o), f, J, R);
        sj += log2(J);
        sr += log2(R);
    }
    const int n = e1 - e0;
    out[v] = n > 0 ? sj / n : 0.0;
    out[(size_t)V + v] = n > 0 ? sr / n : 0.0;
}

// the group statistics read the resident maps through a list of subjects: position a is subject list[a], or subject a where list is nullptr
__device__ __forceinline__ int listed(const int32_t *list, int a) { return list ? list[a] : a; }

__global__ __launch_bounds__(kBlock) void k_dedrift_moments(const double *__restrict__ maps, const int32_t *__restrict__ list, int S, size_t n,
                                                            double *__restrict__ mean, double *__restrict__ sd) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += maps[(size_t)listed(list, s) * n + i];
    const double mu = a / S;
    double q = 0.0;
    for (int s = 0; s < S; ++s) {
        const double d = maps[(size_t)listed(list, s) * n + i] - mu;
        q += d * d;
    }
    mean[i] = mu;
    sd[i] = sqrt(q / S);
}

// a map row as it is (X = const double *), or its entries at the kept vertices only
struct KeptRow {
    const double *x;
    const int32_t *kept;  // ascending vertex ids
    __device__ __forceinline__ double operator[](int j) const { return x[kept[j]]; }
};

// mean of x[0 .. n) and the root of its summed squared deviations, a fixed 256-leaf tree each
template <class X>
__device__ __forceinline__ void map_mean_root(const X x, int n, double *lds, double &mu, double &root) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) a += x[i];
    mu = block_sum(a, lds) / n;
    double q = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const double d = x[i] - mu;
        q += d * d;
    }
    root = sqrt(block_sum(q, lds));
}

// workgroup a * D + d: row d of listed subject a, over the K kept vertices (kept == nullptr: all Vt = K of them)
__global__ __launch_bounds__(kBlock) void k_dedrift_map_stats(const double *__restrict__ maps, const int32_t *__restrict__ list, int D, int Vt,
                                                              const int32_t *__restrict__ kept, int K, double *__restrict__ stats) {
    __shared__ double lds[kBlock];
    const double *x = maps + ((size_t)listed(list, blockIdx.x / D) * D + blockIdx.x % D) * Vt;
    double mu, root;
    if (kept)
        map_mean_root(KeptRow{x, kept}, K, lds, mu, root);
    else
        map_mean_root(x, K, lds, mu, root);
    if (threadIdx.x == 0) stats[2 * (size_t)blockIdx.x] = mu, stats[2 * (size_t)blockIdx.x + 1] = root;
}

// an integer key with the order of the doubles (negative values: all bits flipped; others: the sign bit set)
__device__ __forceinline__ unsigned long long order_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)u);
}

// the masks of one map x[0 .. n) for a kWide-wide workgroup; results go to slot `out` of thr_out, bits (words words per slot) and count
template <class X>
__device__ __forceinline__ void percentile_mask(const X x, int n, int k, double gamma, int out, double *__restrict__ thr_out,
                                                unsigned long long *__restrict__ bits, int words, int32_t *__restrict__ count) {
    __shared__ int hist[256];
    __shared__ unsigned long long s_prefix, s_min;
    __shared__ int s_k, s_cnt;
    const int t = threadIdx.x;
    if (t == 0) s_prefix = 0, s_k = k;
    // the k-th smallest key (0-based), eight bits at a time from the top
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (t < 256) hist[t] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix, himask = pass == 0 ? 0ull : (~0ull << (shift + 8));
        for (int i = t; i < n; i += kWide) {
            const unsigned long long key = order_key(x[i]);
            if ((key & himask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        if (t == 0) {
            int cum = 0, kk = s_k;
            for (int b = 0; b < 256; ++b) {
                if (cum + hist[b] > kk) {
                    s_prefix = prefix | ((unsigned long long)b << shift);
                    s_k = kk - cum;
                    break;
                }
                cum += hist[b];
            }
        }
        __syncthreads();
    }
    const unsigned long long lo_key = s_prefix;
    // the next order statistic: the same value when more than k + 1 values are <= it, the smallest larger value otherwise
    if (t == 0) s_cnt = 0, s_min = ~0ull;
    __syncthreads();
    int cnt = 0;
    unsigned long long mn = ~0ull;
    for (int i = t; i < n; i += kWide) {
        const unsigned long long key = order_key(x[i]);
        if (key <= lo_key)
            ++cnt;
        else if (key < mn)
            mn = key;
    }
    atomicAdd(&s_cnt, cnt);
    atomicMin(&s_min, mn);
    __syncthreads();
    const unsigned long long hi_key = (k + 1 >= n || s_cnt > k + 1) ? lo_key : s_min;
    // numpy's _lerp: a + (b - a) t, and b - (b - a) (1 - t) from t = 0.5 on
    const double a = key_value(lo_key), b = key_value(hi_key), diff = b - a;
    const double thr = gamma >= 0.5 ? b - diff * (1 - gamma) : a + diff * gamma;
    __syncthreads();
    if (t == 0) s_cnt = 0;
    __syncthreads();
    const int lane = t & 63;
    int ones = 0;
    for (int base = (t >> 6) * 64; base < words * 64; base += kWide) {  // wavefront-uniform
        const int i = base + lane;
        const unsigned long long word = __ballot(i < n && x[i] > thr);
        if (lane == 0) {
            bits[(size_t)out * words + (base >> 6)] = word;
            ones += __popcll(word);
        }
    }
    if (lane == 0) atomicAdd(&s_cnt, ones);
    __syncthreads();
    if (t == 0) thr_out[out] = thr, count[out] = s_cnt;
}

// workgroup a * D + d: row d of listed subject a, over the K kept vertices (kept == nullptr: all Vt = K of them); words = ceil(K / 64)
__global__ __launch_bounds__(kWide) void k_dedrift_masks(const double *__restrict__ maps, const int32_t *__restrict__ list, int D, int Vt,
                                                         const int32_t *__restrict__ kept, int K, int k, double gamma, double *__restrict__ thr_out,
                                                         unsigned long long *__restrict__ bits, int words, int32_t *__restrict__ count) {
    const double *x = maps + ((size_t)listed(list, blockIdx.x / D) * D + blockIdx.x % D) * Vt;
    if (kept)
        percentile_mask(KeptRow{x, kept}, K, k, gamma, blockIdx.x, thr_out, bits, words, count);
    else
        percentile_mask(x, K, k, gamma, blockIdx.x, thr_out, bits, words, count);
}

// --- the whole set without a mask, up to dedrift.cpp's kPerPairMax subjects: one workgroup per pair, which a few pairs finish sooner than a tile does.
// The same sums over the same tree as the tile kernels: the same bits.
// pair p of the list (0,1) (0,2) ... (0,S-1) (1,2) ...
__device__ __forceinline__ void pair_of(int p, int S, int &i, int &j) {
    i = 0;
    while (p >= S - 1 - i) p -= S - 1 - i, ++i;
    j = i + 1 + p;
}

__global__ __launch_bounds__(kBlock) void k_dedrift_pair_cc(const double *__restrict__ maps, int S, int D, int Vt, const double *__restrict__ stats,
                                                            double *__restrict__ cc) {
    __shared__ double lds[kBlock];
    const int d = blockIdx.y, npairs = S * (S - 1) / 2;
    if ((int)blockIdx.x >= npairs) {  // the S workgroups after the pairs: the diagonal
        const int s = blockIdx.x - npairs;
        if (threadIdx.x == 0) cc[((size_t)d * S + s) * S + s] = 1.0;
        return;
    }
    int i, j;
    pair_of(blockIdx.x, S, i, j);
    const size_t mi = (size_t)i * D + d, mj = (size_t)j * D + d;
    const double *x = maps + mi * Vt, *y = maps + mj * Vt;
    const double mx = stats[2 * mi], my = stats[2 * mj];
    double a = 0.0;
    for (int k = threadIdx.x; k < Vt; k += kBlock) a += (x[k] - mx) * (y[k] - my);
    const double dot = block_sum(a, lds);
    if (threadIdx.x == 0) {
        const double r = dot / (stats[2 * mi + 1] * stats[2 * mj + 1]);
        double *out = cc + (size_t)d * S * S;
        out[(size_t)i * S + j] = r;
        out[(size_t)j * S + i] = r;
    }
}

__global__ __launch_bounds__(64) void k_dedrift_pair_dice(const unsigned long long *__restrict__ bits, const int32_t *__restrict__ count, int S, int D,
                                                          int words, double *__restrict__ dice) {
    __shared__ int s_both;
    const int d = blockIdx.y, npairs = S * (S - 1) / 2;
    if ((int)blockIdx.x >= npairs) {  // the diagonal: the formula on a mask and itself (NaN for an empty mask, as the formula gives)
        const int s = blockIdx.x - npairs, c = count[(size_t)s * D + d];
        if (threadIdx.x == 0) dice[((size_t)d * S + s) * S + s] = 2.0 * c / (double)(c + c);
        return;
    }
    int i, j;
    pair_of(blockIdx.x, S, i, j);
    const size_t mi = (size_t)i * D + d, mj = (size_t)j * D + d;
    if (threadIdx.x == 0) s_both = 0;
    __syncthreads();
    int both = 0;
    for (int k = threadIdx.x; k < words; k += 64) both += __popcll(bits[mi * words + k] & bits[mj * words + k]);
    atomicAdd(&s_both, both);
    __syncthreads();
    if (threadIdx.x == 0) {
        double *out = dice + (size_t)d * S * S;
        const double r = 2.0 * s_both / (double)(count[mi] + count[mj]);
        out[(size_t)i * S + j] = r;
        out[(size_t)j * S + i] = r;
    }
}

constexpr int kTile = 8;  // listed subjects along each side of a pair tile

// workgroup (tj, ti, d), ti <= tj: the pairs of the listed subjects ti * 8 + a and tj * 8 + b of feature d.  A position past the list's end reads
// the list's last subject and writes nothing.  stats is indexed by list position.
__global__ __launch_bounds__(kBlock) void k_dedrift_tile_cc(const double *__restrict__ maps, const int32_t *__restrict__ list, int n, int D, int Vt,
                                                            const int32_t *__restrict__ kept, int K, const double *__restrict__ stats,
                                                            double *__restrict__ cc) {
    __shared__ double lds[kTile][kBlock];
    const int tj = blockIdx.x, ti = blockIdx.y, d = blockIdx.z;
    if (ti > tj) return;
    const double *xr[kTile], *xc[kTile];
    double mr[kTile], mc[kTile];
#pragma unroll
    for (int a = 0; a < kTile; ++a) {
        const int ia = min(ti * kTile + a, n - 1), ib = min(tj * kTile + a, n - 1);
        xr[a] = maps + ((size_t)listed(list, ia) * D + d) * Vt, mr[a] = stats[2 * ((size_t)ia * D + d)];
        xc[a] = maps + ((size_t)listed(list, ib) * D + d) * Vt, mc[a] = stats[2 * ((size_t)ib * D + d)];
    }
    double acc[kTile][kTile];
#pragma unroll
    for (int a = 0; a < kTile; ++a)
#pragma unroll
        for (int b = 0; b < kTile; ++b) acc[a][b] = 0.0;
    for (int j = threadIdx.x; j < K; j += kBlock) {
        const int v = kept ? kept[j] : j;
        double r[kTile], c[kTile];
#pragma unroll
        for (int a = 0; a < kTile; ++a) r[a] = xr[a][v] - mr[a], c[a] = xc[a][v] - mc[a];
#pragma unroll
        for (int a = 0; a < kTile; ++a)
#pragma unroll
            for (int b = 0; b < kTile; ++b) acc[a][b] += r[a] * c[b];
    }
    double *out = cc + (size_t)d * n * n;
#pragma unroll
    for (int a = 0; a < kTile; ++a) {
        const double dot = tile_sums(acc[a], lds);
        const int ia = ti * kTile + a, ib = tj * kTile + (int)threadIdx.x;
        if (threadIdx.x >= kTile || ia >= n || ib >= n) continue;
        if (ia == ib) out[(size_t)ia * n + ia] = 1.0;
        if (ia < ib) {  // a diagonal tile holds every pair twice: the copy above the diagonal serves both entries
            const double rho = dot / (stats[2 * ((size_t)ia * D + d) + 1] * stats[2 * ((size_t)ib * D + d) + 1]);
            out[(size_t)ia * n + ib] = rho;
            out[(size_t)ib * n + ia] = rho;
        }
    }
}

// the same tiles over the masks (bits, count: indexed by list position); the diagonal follows the formula (NaN for an empty mask)
__global__ __launch_bounds__(kBlock) void k_dedrift_tile_dice(const unsigned long long *__restrict__ bits, const int32_t *__restrict__ count, int n, int D,
                                                              int words, double *__restrict__ dice) {
    __shared__ int lds[kTile][kBlock];
    const int tj = blockIdx.x, ti = blockIdx.y, d = blockIdx.z;
    if (ti > tj) return;
    const unsigned long long *br[kTile], *bc[kTile];
#pragma unroll
    for (int a = 0; a < kTile; ++a) {
        br[a] = bits + ((size_t)min(ti * kTile + a, n - 1) * D + d) * words;
        bc[a] = bits + ((size_t)min(tj * kTile + a, n - 1) * D + d) * words;
    }
    int acc[kTile][kTile];
#pragma unroll
    for (int a = 0; a < kTile; ++a)
#pragma unroll
        for (int b = 0; b < kTile; ++b) acc[a][b] = 0;
    for (int j = threadIdx.x; j < words; j += kBlock) {
        unsigned long long r[kTile], c[kTile];
#pragma unroll
        for (int a = 0; a < kTile; ++a) r[a] = br[a][j], c[a] = bc[a][j];
#pragma unroll
        for (int a = 0; a < kTile; ++a)
#pragma unroll
            for (int b = 0; b < kTile; ++b) acc[a][b] += __popcll(r[a] & c[b]);
    }
    double *out = dice + (size_t)d * n * n;
#pragma unroll
    for (int a = 0; a < kTile; ++a) {
        const int both = tile_sums(acc[a], lds);
        const int ia = ti * kTile + a, ib = tj * kTile + (int)threadIdx.x;
        if (threadIdx.x >= kTile || ia >= n || ib >= n || ia > ib) continue;
        const double r = 2.0 * both / (double)(count[(size_t)ia * D + d] + count[(size_t)ib * D + d]);
        out[(size_t)ia * n + ib] = r;
        out[(size_t)ib * n + ia] = r;
    }
}

// workgroup m: the mean over the pairs a < b of matrix m (n x n)
__global__ __launch_bounds__(kBlock) void k_dedrift_pair_mean(const double *__restrict__ mat, int n, double *__restrict__ out) {
    __shared__ double lds[kBlock];
    const double *m = mat + (size_t)blockIdx.x * n * n;
    double a = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1 + threadIdx.x; j < n; j += kBlock) a += m[(size_t)i * n + j];
    const double sum = block_sum(a, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = n > 1 ? sum / (n * (n - 1) / 2.0) : NAN;
}

}  // namespace

int launch_dedrift_accumulate(msm_ctx *ctx, const int32_t *d_vid, const double *d_w, int Vt, const double *d_m, int Vs, double *d_sum, double *d_inverse) {
    if (Vt <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_dedrift_accumulate, dim3((Vt + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, d_vid, d_w, Vt, d_m, Vs, d_sum, d_inverse);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_dedrift_finish(msm_ctx *ctx, const double *d_sum, int Vt, int S, double *d_drift, double *d_warp) {
    hipLaunchKernelGGL(k_dedrift_finish, dim3(1), dim3(kWide), 0, ctx->stream, d_sum, Vt, S, d_drift, d_warp);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_vertex_distortion(msm_ctx *ctx, const double *d_m, const double *d_c, int V, const int32_t *d_tri, int T, const int32_t *d_tid_ptr,
                             const int32_t *d_tid, double *d_out) {
    if (V <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_vertex_distortion, dim3((V + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, d_m, d_c, V, d_tri, T, d_tid_ptr, d_tid, d_out);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_dedrift_moments(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, size_t nmap, double *d_mean, double *d_sd) {
    if (nmap == 0) return MSM_OK;
    hipLaunchKernelGGL(k_dedrift_moments, dim3((unsigned)((nmap + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, d_maps, d_list, n, nmap, d_mean, d_sd);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_dedrift_map_stats(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, int D, int Vt, const int32_t *d_kept, int K, double *d_stats) {
    hipLaunchKernelGGL(k_dedrift_map_stats, dim3(n * D), dim3(kBlock), 0, ctx->stream, d_maps, d_list, D, Vt, d_kept, K, d_stats);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_dedrift_masks(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, int D, int Vt, const int32_t *d_kept, int K, int k, double gamma,
                         double *d_thr, unsigned long long *d_bits, int words, int32_t *d_count) {
    hipLaunchKernelGGL(k_dedrift_masks, dim3(n * D), dim3(kWide), 0, ctx->stream, d_maps, d_list, D, Vt, d_kept, K, k, gamma, d_thr, d_bits, words, d_count);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

// both pair kernels: S (S - 1) / 2 workgroups for the pairs, then S for the diagonal
int launch_dedrift_pair_cc(msm_ctx *ctx, const double *d_maps, int S, int D, int Vt, const double *d_stats, double *d_cc) {
    const int npairs = S * (S - 1) / 2;
    hipLaunchKernelGGL(k_dedrift_pair_cc, dim3(npairs + S, D), dim3(kBlock), 0, ctx->stream, d_maps, S, D, Vt, d_stats, d_cc);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_dedrift_pair_dice(msm_ctx *ctx, const unsigned long long *d_bits, const int32_t *d_count, int S, int D, int words, double *d_dice) {
    const int npairs = S * (S - 1) / 2;
    hipLaunchKernelGGL(k_dedrift_pair_dice, dim3(npairs + S, D), dim3(64), 0, ctx->stream, d_bits, d_count, S, D, words, d_dice);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

// both tile kernels: ceil(n / 8)^2 workgroups per feature, of which the lower triangle's leave at once
int launch_dedrift_tile_cc(msm_ctx *ctx, const double *d_maps, const int32_t *d_list, int n, int D, int Vt, const int32_t *d_kept, int K,
                           const double *d_stats, double *d_cc) {
    const int nt = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_dedrift_tile_cc, dim3(nt, nt, D), dim3(kBlock), 0, ctx->stream, d_maps, d_list, n, D, Vt, d_kept, K, d_stats, d_cc);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_dedrift_tile_dice(msm_ctx *ctx, const unsigned long long *d_bits, const int32_t *d_count, int n, int D, int words, double *d_dice) {
    const int nt = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_dedrift_tile_dice, dim3(nt, nt, D), dim3(kBlock), 0, ctx->stream, d_bits, d_count, n, D, words, d_dice);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_dedrift_pair_mean(msm_ctx *ctx, const double *d_mat, int nmat, int n, double *d_out) {
    hipLaunchKernelGGL(k_dedrift_pair_mean, dim3(nmat), dim3(kBlock), 0, ctx->stream, d_mat, n, d_out);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
