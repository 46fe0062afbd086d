// unary_kernels.hip -- the sampling kernels of the unary label-cost table (computeUnaryCosts, M/DiscreteCostFunction.cpp:236-243): every patch
// point of every control point, rotated by every label, gets the target triangle that contains it and the target's value there (get_target_data,
// :353-376).  The reductions that turn the samples into costs are in unary_reduce_kernels.hip, the launch decisions in unary_plan.cpp.
//
//   k_unary_rays      the sampler of a target with a direction table (unary_uses_ray_table), the usual case and the kernel the benchmark times:
//                     one cell load and ~1.3 candidate records per sample; its own comment below has the details.  It only fills tval (or
//                     triangle and weights); a reduction kernel always follows.
//   k_unary_samples   the complete sampler, the fallback while a target has no direction table (it arrives in the background) or can have none.
//                     One workgroup per control point and label range.  The control
//                     point's patch (source coordinates: the "neighbour ring") and its L rotation matrices are
//                     staged in LDS once and reused by all L*P point samples.  Each sample = rotate, find
//                     the nearest target triangle, interpolate.  The search
//                     is split into three LDS-connected phases so that every phase keeps all 64 lanes of a
//                     wavefront busy with the same kind of work:
//                       A  per sample: dense-grid cell -> octree leaf, float cone filter over the leaf's
//                          entries; surviving (sample, triangle) pairs go to an LDS queue;
//                       B  per pair (evenly spread over the lanes): the exact FP64 inside test of the
//                          reference (project_point + point_in_triangle);
//                       C  per sample: exactly one triangle contains the projection (the normal case) ->
//                          barycentric interpolation of the reference feature, value written to HBM.
//                     Samples with zero or several containing triangles need the reference's tie-breaks
//                     and fallbacks; they are rare and are appended to a fix-up list instead of being
//                     handled here (keeps this kernel's register budget small = more waves per SIMD).
//                     For DICE / genDICE (launch_samples: fused_reduction) it also reduces the control points all of whose samples it
//                     settled, straight from LDS, and lists the others for k_unary_reduce_univariate.
//   k_unary_fixup     behind either sampler: re-does the listed samples with the complete search (search_device.hpp).  Workgroups behind its own
//                     4 096 prepare the moving patches for k_unary_reduce_rows where that kernel follows.
//
// Decisions (which triangle) use the reference's FP64 arithmetic; see search_device.hpp.
#include "search_device.hpp"
#include "similarity_device.hpp"
#include "unary.hpp"

namespace msm {

namespace {

constexpr int kDeferred = 1 << 20; // nin marker: leave this sample to the fix-up kernel
constexpr unsigned kInvalidPair = 0xffffffffu;  // queue slot reserved by a sample that was deferred (sample ids stay below 1023)

__device__ __forceinline__ void raise_status(int *status, int code) { atomicMin(status, code); }

struct SamplesArgs {
    DevTree tree;
    const double *tfeat;   // target features, V x tD vertex-major (the univariate class reads row 1 = column 0 only,
    int tD;                // M/DiscreteCostFunction.cpp:371), or nullptr when only weights are wanted
    int N, L;
    const double *rnl;     // N x L x 9
    const double *src;     // 3 x Nsrc SoA
    int Nsrc;
    const int *pptr, *pidx;
    const int *order;      // launch order of the control points
    int pmax;
    int nsplit;            // workgroups per control point (label ranges)
    // outputs, indexed by global sample id g = L*pptr[node] + l*P + i
    double *tval;          // D == 1: interpolated reference feature
    int *stri;             // otherwise: triangle id and the three raw barycentric weights
    double *sw3;           // 3 doubles per sample
    // Fix-up list: kFixSegs segments (a workgroup appends to segment blockIdx % kFixSegs, which is sized for all
    // samples of its workgroups: it cannot overflow).  One list with one counter would funnel every append of
    // the chip through a single address; measured: 10 ns per append, i.e. most of the kernel's time.
    unsigned long long *fix_list;  // global sample id (L * pptr[node] + local sample)
    double *fix_pt;                // the rotated point of the listed sample, 3 doubles per slot: the fix-up kernel starts from it
    unsigned int *fix_cnt;         // counter of segment s at fix_cnt[kCntStride * (1 + s)]; [0] is the redo counter
    const unsigned int *fix_off;   // kFixSegs + 1 segment offsets into fix_list
    // fused reduction (univariate DICE / genDICE): moving feature, AbsoluteWeights, output table
    const double *sfeat;   // Nsrc (feature row 1)
    const double *cfw;     // unread (DICE has no weights); it keeps its place so that the block's layout stays what it was
    const double *absw;    // N
    int simmeasure;
    double percentile;     // DICE measures
    double *U;             // L x N
    int *redo_list;        // nodes whose reduction must wait for the fix-up kernel
    unsigned int *redo_count;
    int *status;
    // the prepare blocks of the fix-up launch (behind every member the samplers read, whose places stay what they were): the moving side of
    // k_unary_reduce_rows, or all nullptr when that kernel does not follow
    const double *mov_cfw;  // the weight row, Nsrc, or nullptr
    double *mov_a, *mov_w;  // moving patches and their weights in patch order (mov_w: nullptr without weights)
    double *mov_stat;       // 3 x N: sum of weights, weighted mean, weighted variance sum (correlation only)
};

// get_target_data's tail (:361-375): barycentric_interpolation on the raw (un-projected) point
__device__ __forceinline__ double emit_sample(const SamplesArgs &a, size_t g, const V3 &p, int t) {
    const TriRec &r = a.tree.rec[t];
    double wa, wb, wc;
    area_weights(rec_v0(r), rec_v1(r), rec_v2(r), p, wa, wb, wc);
    if (a.tval) {
        const double v = wa * a.tfeat[(size_t)r.id[0] * a.tD] + wb * a.tfeat[(size_t)r.id[1] * a.tD] + wc * a.tfeat[(size_t)r.id[2] * a.tD];
        a.tval[g] = v;
        return v;
    } else {
        a.stri[g] = t;
        a.sw3[3 * g] = wa;
        a.sw3[3 * g + 1] = wb;
        a.sw3[3 * g + 2] = wc;
    }
    return 0.0;
}

__device__ __forceinline__ void emit_failure(const SamplesArgs &a, size_t g, int code) {
    raise_status(a.status, code);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (a.tval) {
        a.tval[g] = nan;
    } else {
        a.stri[g] = code;
        a.sw3[3 * g] = a.sw3[3 * g + 1] = a.sw3[3 * g + 2] = nan;
    }
}

// how many lanes below this one are set in a ballot (no lane mask to keep in registers over the sample loop)
__device__ __forceinline__ int set_below(unsigned long long m) {
#ifdef __HIP_DEVICE_COMPILE__
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
#else
    return 0;
#endif
}

// Lane pairs of k_unary_rays (lanes 2j and 2j + 1): a value of the other lane of the pair, by one DPP move (quad_perm:[1,0,3,2], every row and
// bank).  Both lanes of a pair must be switched on where this stands.
__device__ __forceinline__ int pair_swap(int v) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false);
#else
    return v;
#endif
}

#ifdef __HIP_DEVICE_COMPILE__
// One even and one odd piece of each lane's own record from what a pair of lanes loaded.  X is this lane's piece of the even lane's record
// (the even piece in the even lane, the odd piece in the odd lane), Y its piece of the odd lane's record.  The even lane keeps X and takes the
// odd lane's X for its odd piece; the odd lane keeps Y and takes the even lane's Y for its even piece.  In place, three instructions a dword
// with the even lanes' mask in VCC (a DPP bank mask names groups of four lanes and cannot tell the two lanes of a pair apart):
//     t = the partner's x;    x = even ? x : the partner's y;    y = even ? t : y
// Written as assembly because the compiler has no way to be told "in the registers of the loads": from builtins and selects it makes two moves
// and two selects a dword into 24 registers of their own, and the kernel, which stands at 72 for seven waves per SIMD, spills.  No instruction
// here reads through DPP a register that an earlier one of the statement wrote, and the operands come from loads, so the two wait states
// between a VALU write and a DPP read of the same register are none of this statement's business; the leading s_nop covers whatever VALU
// instruction the compiler may have put in front.
typedef int pair_v4i __attribute__((ext_vector_type(4)));
#define MSM_PAIR_DPP " quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
#define MSM_PAIR_DWORD(x, y)                                                 \
    "v_mov_b32_dpp %[t], " x MSM_PAIR_DPP                                    \
    "v_cndmask_b32_dpp " x ", " y ", " x ", vcc" MSM_PAIR_DPP                \
    "v_cndmask_b32_e32 " y ", " y ", %[t], vcc\n\t"
__device__ __forceinline__ void pair_merge(pair_v4i X, pair_v4i Y, double2 &even_piece, double2 &odd_piece) {
    int x0 = X.x, x1 = X.y, x2 = X.z, x3 = X.w, y0 = Y.x, y1 = Y.y, y2 = Y.z, y3 = Y.w, t;
    asm volatile("s_mov_b32 vcc_lo, 0x55555555\n\t"
                 "s_mov_b32 vcc_hi, 0x55555555\n\t"
                 "s_nop 1\n\t"
                 MSM_PAIR_DWORD("%[x0]", "%[y0]") MSM_PAIR_DWORD("%[x1]", "%[y1]") MSM_PAIR_DWORD("%[x2]", "%[y2]") MSM_PAIR_DWORD("%[x3]", "%[y3]")
                 : [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2), [x3] "+v"(x3), [y0] "+v"(y0), [y1] "+v"(y1), [y2] "+v"(y2), [y3] "+v"(y3), [t] "=&v"(t)
                 :
                 : "vcc");
    even_piece = make_double2(__hiloint2double(x1, x0), __hiloint2double(x3, x2));
    odd_piece = make_double2(__hiloint2double(y1, y0), __hiloint2double(y3, y2));
}
#undef MSM_PAIR_DWORD
#undef MSM_PAIR_DPP
#endif

}  // namespace

__global__ __launch_bounds__(256) void k_unary_samples(SamplesArgs a) {
    extern __shared__ __align__(16) double lds[];
    double *sx = lds, *sy = sx + a.pmax, *sz = sy + a.pmax;
    double *sA = sz + a.pmax;                                    // moving feature of the patch; the pmax doubles behind it are reserved and unread
    double *sR = sA + 2 * a.pmax;                                // L x 9
    double *sT = sR + 9 * a.L;                                   // (labels of this workgroup) x pmax sampled target values
    unsigned *queue = reinterpret_cast<unsigned *>(sT + (size_t)unary_labels_per_workgroup(a.L, a.nsplit) * a.pmax);  // kQueueCap
    int *nin = reinterpret_cast<int *>(queue + kQueueCap);         // kChunk: containing triangles found
    int *win = nin + kChunk;                                        // kChunk: one of them
    __shared__ int s_qn, s_ndefer;
    const int tid = threadIdx.x, lane = tid & 63;

    {
        int at, l_beg, l_end;  // this workgroup's control point and labels
        if (!unary_workgroup_share(blockIdx.x, a.N, a.L, a.nsplit, at, l_beg, l_end)) return;
        const int node = a.order[at];
        const int beg = a.pptr[node], P = a.pptr[node + 1] - beg;
        const size_t gbase = (size_t)a.L * beg;
        for (int i = tid; i < P; i += 256) {
            const int s = a.pidx[beg + i];
            sx[i] = a.src[s];
            sy[i] = a.src[a.Nsrc + s];
            sz[i] = a.src[2 * a.Nsrc + s];
            if (a.U) sA[i] = a.sfeat[s];
        }
        for (int k = tid; k < 9 * a.L; k += 256) sR[k] = a.rnl[(size_t)node * a.L * 9 + k];
        if (tid == 0) s_ndefer = 0;
        const int sbeg = l_beg * P, send = l_end * P;  // this workgroup's samples: s = label * P + patch point
        const float invP = 1.0f / (float)max(P, 1);

        for (int base = sbeg; base < send; base += kChunk) {
            const int nchunk = min(kChunk, send - base);
            for (int k = tid; k < kChunk; k += 256) nin[k] = 0;
            if (tid == 0) s_qn = 0;
            __syncthreads();

            // ---- phase A: per sample (one lane each): rotate, locate the octree leaf, cone-filter its entries.
            // Every lane runs the same number of rounds so that the queue reservation can use wavefront shuffles.
            for (int r0 = 0; r0 < nchunk; r0 += 256) {
                const int sl = r0 + tid;
                unsigned long long pm = 0ull;  // entries that passed the cone filter
                int lbeg = 0;
                bool defer = false;
                if (sl < nchunk) {
                    const int s = base + sl;
                    const int l = fast_div(s, P, invP), i = s - l * P;
                    const V3 p = rotate(sR + 9 * l, mk(sx[i], sy[i], sz[i]));
                    if (outside_root(p)) {
                        nin[sl] = -1;
                    } else {
                        int sub;
                        const int4 leaf = locate_leaf(a.tree, p, sub);
                        lbeg = leaf.y;
                        if (leaf.z < 0) {
                            // no masks: an oversized leaf (the split heuristic refused to split it) needs the complete
                            // search; an empty one yields no pair and reaches the fix-up list through nin == 0
                            defer = (-leaf.x - 1) > 64;
                        } else {
                            const float qx = (float)p.x, qy = (float)p.y, qz = (float)p.z;
                            const float inv = rsqrtf(qx * qx + qy * qy + qz * qz);
                            const float fx = qx * inv, fy = qy * inv, fz = qz * inv;
                            const float4 *cone = a.tree.cone + leaf.y;
                            // entries a point of this sub-cell can hit at all; cone-test those, four loads in flight
                            unsigned long long mm = a.tree.mask[(size_t)leaf.z * 64 + sub];
                            while (mm) {
                                int e[4];
                                bool v[4];
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    v[k] = mm != 0ull;
                                    e[k] = v[k] ? __ffsll((long long)mm) - 1 : 0;
                                    mm &= mm - 1ull;  // 0 stays 0
                                }
                                float4 c[4];
#pragma unroll
                                for (int k = 0; k < 4; ++k) c[k] = cone[e[k]];
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    const float dt = fabsf(__builtin_fmaf(c[k].z, fz, __builtin_fmaf(c[k].y, fy, c[k].x * fx)));
                                    if (v[k] && dt >= c[k].w) pm |= 1ull << e[k];
                                }
                            }
                        }
                    }
                }
                // reserve queue space: wavefront prefix sum of the per-lane pair counts, one LDS atomic per wave
                const int cntp = __popcll(pm);
                int incl = cntp;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int up = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += up;
                }
                int wbase = 0;
                if (lane == 63 && incl > 0) wbase = atomicAdd(&s_qn, incl);
                wbase = __shfl(wbase, 63, 64);
                int pos = wbase + incl - cntp;
                if (cntp > 0) {
                    if (pos + cntp > kQueueCap) {
                        defer = true;  // queue full: the fix-up kernel takes this sample; its reserved slots must not stay stale
                        for (int j = pos; j < kQueueCap; ++j) queue[j] = kInvalidPair;
                    } else {
                        const int *lt = a.tree.leaf_tri + lbeg;
                        const unsigned tag = (unsigned)sl << kTriBits;
                        while (pm) {
                            const int e = __ffsll((long long)pm) - 1;
                            pm &= pm - 1ull;
                            queue[pos++] = tag | (unsigned)lt[e];
                        }
                    }
                }
                if (defer) nin[sl] = kDeferred;  // the fix-up kernel handles this sample
            }
            __syncthreads();

            // ---- phase B: exact inside test per (sample, triangle) pair
            const int qn = min(s_qn, kQueueCap);
            for (int j = tid; j < qn; j += 256) {
                const unsigned e = queue[j];
                if (e == kInvalidPair) continue;
                const int sl = (int)(e >> kTriBits), t = (int)(e & ((1u << kTriBits) - 1));
                const int s = base + sl;
                const int l = fast_div(s, P, invP), i = s - l * P;
                const V3 p = rotate(sR + 9 * l, mk(sx[i], sy[i], sz[i]));
                V3 mp;
                if (inside_test(a.tree.rec[t], p, mp)) {
                    win[sl] = t;
                    atomicAdd(&nin[sl], 1);
                }
            }
            __syncthreads();

            // ---- phase C: interpolate, or defer
            for (int sl = tid; sl < nchunk; sl += 256) {
                const int s = base + sl;
                const int n = nin[sl];
                if (n == 1) {
                    const int l = fast_div(s, P, invP), i = s - l * P;
                    const V3 p = rotate(sR + 9 * l, mk(sx[i], sy[i], sz[i]));
                    const double v = emit_sample(a, gbase + s, p, win[sl]);
                    if (a.U) sT[(l - l_beg) * a.pmax + i] = v;
                } else if (n < 0) {
                    emit_failure(a, gbase + s, MSM_ERR_OUTSIDE);
                    atomicAdd(&s_ndefer, 1);
                } else {
                    atomicAdd(&s_ndefer, 1);
                    const int seg = blockIdx.x % kFixSegs;
                    const unsigned slot = a.fix_off[seg] + atomicAdd(&a.fix_cnt[kCntStride * (1 + seg)], 1u);
                    if (slot < a.fix_off[seg + 1]) {
                        const int l = fast_div(s, P, invP), i = s - l * P;
                        const V3 p = rotate(sR + 9 * l, mk(sx[i], sy[i], sz[i]));
                        a.fix_list[slot] = gbase + (unsigned long long)s;
                        a.fix_pt[3 * (size_t)slot] = p.x;
                        a.fix_pt[3 * (size_t)slot + 1] = p.y;
                        a.fix_pt[3 * (size_t)slot + 2] = p.z;
                    } else {
                        raise_status(a.status, MSM_ERR_CAPACITY);
                    }
                }
            }
            __syncthreads();
        }
        // ---- reduction (DICE / genDICE): every sample of this control point is in LDS unless some were deferred
        if (a.U) {
            __syncthreads();  // s_ndefer and sT are final (also when the patch is empty and the loop never ran)
            if (s_ndefer == 0) {
                const double absw = a.absw[node];
                for (int l = l_beg + (tid >> 6); l < l_end; l += 4) {
                    const double cost = patch_dice(sA, sT + (l - l_beg) * a.pmax, P, lane, a.simmeasure, a.percentile);
                    if (lane == 0) a.U[(size_t)l * a.N + node] = absw * cost;
                }
            } else if (tid == 0) {
                a.redo_list[atomicAdd(a.redo_count, 1u)] = node;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Simple-surface targets: the ray table (search_device.hpp, octree.cpp: build_ray_table) settles a sample with one
// direction-cell load and ~1.3 candidate records; what it cannot settle (about 2 % on an icosphere target) goes to
// the fix-up list, where k_unary_fixup runs the complete search.  Same workgroup -> control point mapping as
// k_unary_samples (unary.hpp: unary_workgroup_share); after staging every wavefront strides over the samples on its own.
//
// The kernel is bound by the vector L1's line-lookup rate (one 128-byte line per cycle per CU: a load whose 64
// lanes hit 64 different lines costs 64 cycles, whatever its width), not by HBM or the ALUs: about 13 line
// lookups per sample (cell 1, edge planes 3, vertices + features 6, retries) = 4.1e7 per table, 161 k cycles per CU,
// before the cells named their first candidate by sub-cell; DESIGN.md section 5.2 has the counters with and without the hints.
// Two variants in which the wavefront fetches the 64 records as a team (lane j of load k reads piece (64k+j) % 9 of
// the record of lane (64k+j) / 9, straight into LDS with global_load_lds_dwordx4) halved the lookups, but at 9 KB of
// LDS per wavefront they cut the occupancy to 3 waves per SIMD and lengthen the dependent chain (shuffle -> load ->
// LDS -> test): 123 us (all four candidate rounds as a team) and 107 us (first candidate only) against 85 us for
// the plain per-lane loads below.
// Three of the nine pieces of the first candidate's record (the edge planes) exist only to accept it.  A cell carries one bit per sub-cell that
// says the hinted candidate passes for every direction of the sub-cell and needs no vouching (internal.hpp: kRayWBits; octree.cpp: build_ray_table
// has the proof); 0.57 of the samples of an ico6 target fall into such a sub-cell.  Their lanes are switched off for the three plane loads -- a lane
// predicate: an inactive lane looks no line up -- and take the candidate untested; everything after acceptance is as it was, and so is every result
// (a certificate only skips a test that would have passed).  72 VGPRs and seven waves per SIMD as before, which takes the two empty asm statements
// in the loop and the occupancy request on the kernel (without it the retry path's packed multiplies push the allocator to 74).  DESIGN.md section
// 5.2 has the counters.
// The other six pieces of the first candidate's record (its vertices and features) are fetched by lane pairs: lanes 2j and 2j + 1 load both their
// records together, each load instruction taking two adjacent pieces of one record for the pair -- one line look-up where it was two, but for the one
// record in eight whose 32 bytes straddle a line -- and swap half of what they loaded by DPP moves, in the registers of the loads (pair_merge: 36 VALU
// instructions a wavefront round).  Pairs, not the quads that were measured earlier (39 % fewer look-ups, 47 % more VALU instructions, the same time),
// and the vertex pieces only; every lane ends with the bytes it loaded for itself before.  DESIGN.md section 5.2 has the counters.
// Behind a first-candidate miss (one lane in ten, so nearly every wavefront round has some): the answer is the second candidate for two misses in
// three, the third to seventh for the rest (msm_ray_depth_check).  A rolled loop over the further candidates, one dependent round trip each until the
// deepest lane of the wavefront is served, and a last trip for the accepted candidate's vertex pieces would make about six trips per round, of which
// four serve a tenth of the lanes.  The kernel makes three: round A tests the second candidate and fetches the cell's ray_more entry, round T has the
// wavefront test everything that is left for up to eight lanes at a time, eight helper lanes per unsettled lane, by shuffles and one ballot, and one
// reload brings the vertex pieces of what either round accepted.  The tests and their operands are the rolled loop's, so the table is the same bit for
// bit; 72 VGPRs, no scratch, seven waves per SIMD -- which is why the unsettled list counts with mbcnt (set_below).  DESIGN.md section 5.2 has what else
// was measured and lost: the rolled loop itself, and the second candidate's vertex pieces requested with its planes, before and without round T.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7))) void k_unary_rays(SamplesArgs a) {
    extern __shared__ __align__(16) double lds[];
    double *sx = lds, *sy = sx + a.pmax, *sz = sy + a.pmax, *sR = sz + a.pmax;
    const int tid = threadIdx.x, lane = tid & 63;
    // unary_workgroup_share (unary.hpp), written out: called here it compiles to the same instructions but for the order of two scalar loads, and
    // this kernel's instruction stream is kept as it is.  Whoever changes the mapping changes it there and here.
    const int per = (a.N + 7) >> 3;
    const int slots = 8 * per;
    const int part = blockIdx.x / slots, slot = blockIdx.x - part * slots;
    const int at = (slot & 7) * per + (slot >> 3);
    if (at >= a.N) return;
    const int node = a.order[at];
    const int lper = (a.L + a.nsplit - 1) / a.nsplit;
    const int l_beg = part * lper, l_end = min(a.L, l_beg + lper);
    if (l_beg >= l_end) return;
    const int beg = a.pptr[node], P = a.pptr[node + 1] - beg;
    const size_t gbase = (size_t)a.L * beg;
    for (int i = tid; i < P; i += 256) {
        const int s = a.pidx[beg + i];
        sx[i] = a.src[s];
        sy[i] = a.src[a.Nsrc + s];
        sz[i] = a.src[2 * a.Nsrc + s];
    }
    for (int k = 9 * l_beg + tid; k < 9 * l_end; k += 256) sR[k] = a.rnl[(size_t)node * a.L * 9 + k];
    const int sbeg = l_beg * P, send = l_end * P;
    const float invP = 1.0f / (float)max(P, 1);
    // unsettled samples are collected in LDS and appended to the global list with ONE atomic per workgroup
    // (a returning atomic per wavefront on one address was measured to triple the kernel's time)
    int *sleft = reinterpret_cast<int *>(sR + 9 * a.L);
    __shared__ int s_nleft;
    __shared__ unsigned s_base;
    if (tid == 0) s_nleft = 0;
    __syncthreads();
    for (int s0 = sbeg; s0 < send; s0 += 256) {
        const int s = s0 + tid;
        const bool act = s < send;
        bool done = false;
        V3 p = mk(0.0, 0.0, 0.0);
        float fx = 0.f, fy = 0.f, fz = 0.f;
        int4 c = make_int4(-1, -1, -1, -1);
        bool cert = false;
        if (act) {
            const int l = fast_div(s, P, invP), i = s - l * P;
            p = rotate(sR + 9 * l, mk(sx[i], sy[i], sz[i]));
            c = ray_cell_of(a.tree, p, fx, fy, fz, cert);
        }
        // (what a sample carries from its first candidate to its end; out here because round T runs at wave-uniform control flow)
        int t = -1;
        int excl = -1;  // the accepted candidate's exclusion record (its e1.w), negative: none -- as for a certified candidate
        double2 d0, d1, d2, d3, d4, d5;
        bool pend = false;  // unsettled behind round A, with a third candidate to try
        bool got = false;   // settled behind the first candidate, the vertex pieces still to be fetched
        int4 mo;
#ifdef __HIP_DEVICE_COMPILE__
        {  // no value on the paths that never read them, and no instruction: as for the planes below
            typedef double v2d __attribute__((ext_vector_type(2)));
            typedef int v4i __attribute__((ext_vector_type(4)));
            v2d u0, u1, u2, u3, u4, u5;
            v4i um;
            asm volatile("" : "=v"(u0), "=v"(u1), "=v"(u2), "=v"(u3), "=v"(u4), "=v"(u5), "=v"(um));
            d0 = make_double2(u0.x, u0.y), d1 = make_double2(u1.x, u1.y), d2 = make_double2(u2.x, u2.y);
            d3 = make_double2(u3.x, u3.y), d4 = make_double2(u4.x, u4.y), d5 = make_double2(u5.x, u5.y);
            mo = make_int4(um.x, um.y, um.z, um.w);
        }
#else
        d0 = d1 = d2 = d3 = d4 = d5 = make_double2(0.0, 0.0);
        mo = make_int4(-1, -1, -1, -1);
#endif
        // The first candidate -- the one the cell's hint names for this sub-cell (ray_cell_of) -- is the answer nine times out of ten (three out of
        // four for the best-ranked candidate of the whole cell): its vertex pieces are requested together with its edge planes, so a settled
        // sample costs two dependent loads after the cell.  The six vertex pieces (3-8 of the record) are fetched by lane pairs, 2j and 2j + 1:
        // every load instruction has the two lanes of a pair read two adjacent pieces of ONE record, 32 bytes that lie in one 128-byte line seven
        // times out of eight, and the vector L1 looks a line up once for neighbouring lanes that share it.  With par = lane & 1, each lane loads
        // the pieces 3 + par, 5 + par and 7 + par of the even lane's record (X) and of the odd lane's (Y); the even lane then takes its odd pieces
        // from the odd lane's X, the odd lane its even pieces from the even lane's Y, by one DPP move and one select per dword (pair_merge).
        // Six loads per lane as before and the same bytes in d0..d5, for 1.125 line look-ups per pair and load instead of 2.  A lane without a
        // first candidate (no sample, or a point outside the table's radius range) helps its partner with the partner's record, which is why
        // this block stands outside `act`: a DPP move reads nothing from a lane that is switched off, so the two lanes of a pair take every
        // branch around the moves together.  The bank mask of a DPP move names groups of four lanes and cannot tell the lanes of a pair apart.
        {
            const int tc = c.x;  // negative: no first candidate (as c was initialised for a lane without a sample)
            const int tp = pair_swap(tc);
            if ((tc & tp) >= 0) {  // either lane has one: the same decision in both lanes of the pair
                const unsigned par = (unsigned)lane & 1u;
                int te = par ? tp : tc, to = par ? tc : tp;  // the even lane's candidate and the odd lane's, each standing in for the other where that has none
                te = te < 0 ? to : te, to = to < 0 ? te : to;
                // 32-bit byte offsets from the table's base (a scalar pair): per-lane 64-bit pointers cost the registers that keep seven waves per SIMD
                static_assert(16ull * kRayPieces * kRayMaxTris < (1ull << 32), "a ray record's byte offset fits 32 bits");
                const char *tab = reinterpret_cast<const char *>(a.tree.ray_tri);
                const unsigned ox = 16u * ((unsigned)kRayPieces * (unsigned)te + 3u + par), oy = 16u * ((unsigned)kRayPieces * (unsigned)to + 3u + par);
                // A lane whose sub-cell is certified (internal.hpp: kRayWBits) knows that this candidate passes and needs no vouching: it sits
                // out the three edge-plane loads -- a lane that is switched off looks no line up -- and takes the candidate as it is.
                // (a lane predicate: the six vertex loads are requested in the same breath, by every lane of the pair, and nothing waits in between)
                const bool test = tc >= 0 && !cert;
#ifdef __HIP_DEVICE_COMPILE__
                // The certified lanes never read the planes, so nothing need be written for them: the first empty statement names the
                // twelve registers, without an instruction.  (Left to variables without a value, the allocator keeps the registers for the
                // whole sample loop -- 85 instead of 72, two wavefronts per SIMD; written as zeros they cost twelve moves a round.)  The
                // second one keeps the planes out of sight until the vertex loads are out: the packed multiplies of the test want two of
                // their words side by side, and the compiler would otherwise wait for them, and move them, before it requests the vertices.
                typedef float v4f __attribute__((ext_vector_type(4)));
                typedef int v4i __attribute__((ext_vector_type(4)));
                v4f q0, q1, q2;
                asm volatile("" : "=v"(q0), "=v"(q1), "=v"(q2));
                if (test) {
                    const v4f *rq = reinterpret_cast<const v4f *>(tab + 16u * ((unsigned)kRayPieces * (unsigned)tc));
                    q0 = rq[0], q1 = rq[1], q2 = rq[2];
                }
                const v4i *px = reinterpret_cast<const v4i *>(tab + ox), *py = reinterpret_cast<const v4i *>(tab + oy);
                const v4i X0 = px[0], Y0 = py[0], X1 = px[2], Y1 = py[2], X2 = px[4], Y2 = py[4];
                pair_merge(X0, Y0, d0, d1);
                pair_merge(X1, Y1, d2, d3);
                pair_merge(X2, Y2, d4, d5);
#else
                const double2 *dv = reinterpret_cast<const double2 *>(tab + (par ? oy : ox) - 16u * par);
                d0 = dv[0], d1 = dv[1], d2 = dv[2], d3 = dv[3], d4 = dv[4], d5 = dv[5];
#endif
                if (tc >= 0) {
                    t = tc;
                    bool retry = false;
                    if (test) {
#ifdef __HIP_DEVICE_COMPILE__
                        asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2));
                        const float4 e0 = make_float4(q0.x, q0.y, q0.z, q0.w), e1 = make_float4(q1.x, q1.y, q1.z, q1.w), e2 = make_float4(q2.x, q2.y, q2.z, q2.w);
#else
                        const float4 *rec = a.tree.ray_tri + (size_t)kRayPieces * tc;
                        const float4 e0 = rec[0], e1 = rec[1], e2 = rec[2];
#endif
                        excl = __float_as_int(e1.w);
                        retry = !ray_accepts(e0, e1, e2, fx, fy, fz);
                    }
                    if (retry) {
                        t = -1;
                        mo = make_int4(c.w, -1, -1, -1);
                        // Round A: the second candidate is the answer for two misses in three (msm_ray_depth_check).  Its planes and the cell's ray_more entry
                        // are requested together, one round trip; its vertex pieces are not (the look-ups they add cost more than the reload they save).
                        if (c.y >= 0) {
                            const float4 *r2 = a.tree.ray_tri + (size_t)kRayPieces * c.y;
                            const float4 g0 = r2[0], g1 = r2[1], g2 = r2[2];
                            if (c.w < -1) mo = a.tree.ray_more[-2 - c.w];  // a cell with more than four candidates
                            if (ray_accepts(g0, g1, g2, fx, fy, fz)) {
                                t = c.y;
                                excl = __float_as_int(g1.w);
                                got = true;  // (its vertex pieces come with round T's)
                            }
                            pend = t < 0 && c.z >= 0;  // (a list ends at its first negative id: rank_and_fill_cells packs them)
                        }
                    }
                }
            }
        }
        // Round T, the team round: what is still unsettled has its remaining candidates (the third of the cell, then the four of its ray_more entry) tested
        // together, eight lanes per unsettled lane as k_unary_fixup gives a listed sample eight lanes -- every lane of the wavefront helps, with or without
        // a sample of its own.  Lane `sub` of a group fetches its owner's direction and candidate `sub` by shuffle, loads that candidate's planes and runs
        // the same ray_accepts on the same operands; one ballot returns the results.  At most one listed candidate passes, so the first set bit of a
        // group's byte is what the rolled loop would have found.  Eight unsettled lanes are served per pass (a second pass: about 5e-4 of the wavefront
        // rounds with certificates, routinely without).  No LDS.
        for (unsigned long long want = __ballot(pend); want != 0ull;) {
            const int grp = lane >> 3, sub = lane & 7;
            int owner = -1;
            unsigned long long rest = want;  // (wave-uniform: scalar code)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int o = __ffsll((long long)rest) - 1;  // -1 once `rest` is empty
                if (grp == i) owner = o;
                rest &= rest - 1ull;
            }
            const int from = owner < 0 ? lane : owner;
            const float ox = __shfl(fx, from, 64), oy = __shfl(fy, from, 64), oz = __shfl(fz, from, 64);
            const int k0 = __shfl(c.z, from, 64), k1 = __shfl(mo.x, from, 64), k2 = __shfl(mo.y, from, 64), k3 = __shfl(mo.z, from, 64), k4 = __shfl(mo.w, from, 64);
            int ck = sub == 0 ? k0 : (sub == 1 ? k1 : (sub == 2 ? k2 : (sub == 3 ? k3 : (sub == 4 ? k4 : -1))));
            if (owner < 0) ck = -1;
            bool ok = false;
            int ex = -1;
            if (ck >= 0) {
                const float4 *r2 = a.tree.ray_tri + (size_t)kRayPieces * ck;
                const float4 g0 = r2[0], g1 = r2[1], g2 = r2[2];
                ok = ray_accepts(g0, g1, g2, ox, oy, oz);
                ex = __float_as_int(g1.w);
            }
            const unsigned long long hit = __ballot(ok);
            const int rank = set_below(want);
            const bool served = pend && rank < 8;
            const unsigned byte = served ? (unsigned)(hit >> (8 * rank)) & 0xffu : 0u;
            const int helper = byte ? 8 * rank + __ffs((int)byte) - 1 : lane;
            const int hck = __shfl(ck, helper, 64), hex = __shfl(ex, helper, 64);
            if (byte) t = hck, excl = hex, got = true;
            if (served) pend = false;
            want = rest;
        }
        // the reload: the vertex pieces of a candidate accepted in round A or in round T
        if (got) {
            const double2 *dv = reinterpret_cast<const double2 *>(a.tree.ray_tri + (size_t)kRayPieces * t + 3);
            d0 = dv[0], d1 = dv[1], d2 = dv[2], d3 = dv[3], d4 = dv[4], d5 = dv[5];
        }
        // The end of a sample: the accepted triangle t (negative: none) vouched for, get_target_data's weights from the record's vertex pieces d0..d5,
        // the stores.  (In place: hoisted into a function or a lambda the same statements cost the kernel 12 bytes of scratch per lane.)
        if (act) {
            if (t >= 0 && excl >= 0 && !ray_vouches(a.tree, make_float4(0.f, 0.f, 0.f, __int_as_float(excl)), p)) t = -1;  // its leaf may not list it
            if (t >= 0) {
                double wa, wb, wc;
                area_weights(mk(d0.x, d0.y, d1.x), mk(d1.y, d2.x, d2.y), mk(d3.x, d3.y, d4.x), p, wa, wb, wc);
                const size_t g = gbase + s;
                if (a.tval) {
                    a.tval[g] = wa * d4.y + wb * d5.x + wc * d5.y;
                } else {
                    a.stri[g] = t;
                    a.sw3[3 * g] = wa;
                    a.sw3[3 * g + 1] = wb;
                    a.sw3[3 * g + 2] = wc;
                }
                done = true;
            }
        }
        const bool left = act && !done;
        const unsigned long long bal = __ballot(left);
        if (bal) {
            const int leader = __ffsll((long long)bal) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&s_nleft, __popcll(bal));
            base = __shfl(base, leader, 64);
            if (left) sleft[base + set_below(bal)] = s;
        }
    }
    __syncthreads();
    const int nleft = s_nleft;
    if (nleft > 0) {
        const int seg = blockIdx.x % kFixSegs;
        if (tid == 0) s_base = a.fix_off[seg] + atomicAdd(&a.fix_cnt[kCntStride * (1 + seg)], (unsigned)nleft);
        __syncthreads();
        const unsigned base = s_base, end = a.fix_off[seg + 1];
        for (int j = tid; j < nleft; j += 256) {
            if (base + j < end) {
                const int s = sleft[j];
                const int l = fast_div(s, P, invP), i = s - l * P;
                const V3 p = rotate(sR + 9 * l, mk(sx[i], sy[i], sz[i]));  // as in the loop above: the fix-up kernel need not look anything up
                a.fix_list[base + j] = gbase + (unsigned long long)s;
                a.fix_pt[3 * (size_t)(base + j)] = p.x;
                a.fix_pt[3 * (size_t)(base + j) + 1] = p.y;
                a.fix_pt[3 * (size_t)(base + j) + 2] = p.z;
            } else {
                raise_status(a.status, MSM_ERR_CAPACITY);
            }
        }
    }
}

// The listed samples, eight lanes each.  The list is short (a few per cent of the samples at most), so what
// counts is the length of one wavefront's dependent chain, not throughput: with a lane per sample the exact
// tests of 64 lanes end up at 64 different loop positions and run one after the other (32 us for 2 % of an ico6
// table).  Here the eight lanes of a group share the point and split the leaf's entries (entry e goes to lane
// e % 8): sub-cell mask bit, cone test, exact inside test -- every lane at most 8 times, and the tests of one round
// run together.  Exactly one containing triangle = the reference's answer (R/octree.cpp:166-178: a single passing
// triangle wins whatever its distance); anything else (tie-break by dist_to_point, sibling leaves, nearest vertex,
// oversized leaves) is redone by the group's first lane with the complete search of search_device.hpp (with the
// exclusion boxes and overflow candidates of the ray table these are a handful per table).
//
// Passengers: the workgroups behind the first kFixBlocks prepare the moving side of k_unary_reduce_rows (launch_samples: prepare_rows), a wavefront
// per control point.  Nothing they read comes from the sampler or the fix-up list, and this launch leaves most of the chip idle; the row kernel then
// finds each moving patch contiguous, in patch order, with its statistics done.  The statistics are k_unary_reduce_flat's own statements in their
// own order (lane t sums the points t, t + 64, ...; wave_sum; the same divisions), so the two reductions give the same bits.
__device__ __forceinline__ double fixup_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void prepare_moving_patch(const SamplesArgs &a, int node, int t) {
    const int beg = a.pptr[node], P = a.pptr[node + 1] - beg;
    // patches of the row form have at most kRowsPmax <= 128 points: two per lane, kept in registers between the two sums
    double A[2], W[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = t + 64 * k;
        A[k] = 0.0, W[k] = 1.0;
        if (i < P) {
            const int s = a.pidx[beg + i];
            A[k] = a.sfeat[s];
            if (a.mov_cfw) W[k] = a.mov_cfw[s];
            a.mov_a[beg + i] = A[k];
            if (a.mov_w) a.mov_w[beg + i] = W[k];
        }
    }
    if (a.simmeasure != 2) return;
    double sw = 0, ma = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (t + 64 * k < P) {
            sw += W[k];
            ma += W[k] * A[k];
        }
    sw = fixup_wave_sum(sw);
    ma = fixup_wave_sum(ma);
    if (sw > 0.0) ma /= sw;
    double va = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (t + 64 * k < P) {
            const double da = A[k] - ma;
            va += W[k] * da * da;
        }
    va = fixup_wave_sum(va);
    if (t == 0) a.mov_stat[3 * (size_t)node] = sw, a.mov_stat[3 * (size_t)node + 1] = ma, a.mov_stat[3 * (size_t)node + 2] = va;
}

__global__ __launch_bounds__(256) void k_unary_fixup(SamplesArgs a) {
    if (blockIdx.x >= kFixBlocks) {  // uniform over the workgroup, ahead of the barrier below
        const int node = (blockIdx.x - kFixBlocks) * 4 + (threadIdx.x >> 6);
        if (node < a.N) prepare_moving_patch(a, node, threadIdx.x & 63);
        return;
    }
    // dense index over the segments: prefix sums of the segment counts (one wavefront, kFixSegs == 64)
    __shared__ unsigned s_pre[kFixSegs + 1];
    if (threadIdx.x < kFixSegs) {
        const int seg = threadIdx.x;
        const unsigned cnt = min(a.fix_cnt[kCntStride * (1 + seg)], a.fix_off[seg + 1] - a.fix_off[seg]);
        unsigned incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off, 64);
            if (seg >= off) incl += up;
        }
        s_pre[seg + 1] = incl;
        if (seg == 0) s_pre[0] = 0;
    }
    __syncthreads();
    const unsigned n = s_pre[kFixSegs];
    const int lane = threadIdx.x & 63, sub = lane & 7, grp = lane >> 3;
    const unsigned per_block = 256 / 8, stride = kFixBlocks * per_block;  // (the grid may be longer: the passengers above)
    // wavefront-uniform loop: the ballots below need all 64 lanes
    for (unsigned j0 = blockIdx.x * per_block + (threadIdx.x >> 6) * 8; j0 < n; j0 += stride) {
        const unsigned j = j0 + grp;
        const bool valid = j < n;
        V3 p = mk(0.0, 0.0, 0.0);
        size_t g = 0;
        if (valid) {
            int seg = 0;
#pragma unroll
            for (int step = kFixSegs / 2; step > 0; step >>= 1)
                if (s_pre[seg + step] <= j) seg += step;
            const size_t slot = a.fix_off[seg] + (j - s_pre[seg]);
            g = (size_t)a.fix_list[slot];
            p = mk(a.fix_pt[3 * slot], a.fix_pt[3 * slot + 1], a.fix_pt[3 * slot + 2]);
        }
        const int found = group8_find(a.tree, valid, p, lane);
        if (valid && sub == 0) {
            const int t = found == kGroupUndecided ? find_closest_triangle(a.tree, p) : found;  // nothing in the leaf, no masks, outside the root
            if (t < 0) emit_failure(a, g, t);
            else emit_sample(a, g, p, t);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// launch: the plan's sampler, then the fix-up kernel
// ------------------------------------------------------------------------------------------------
int launch_samples(msm_ctx *ctx, const UnaryLaunch &u, const UnaryPlan &plan, const UnaryWeightsScratch *w, bool fused_reduction, bool prepare_rows) {
    if (prepare_rows && (!u.mov_a || !u.mov_stat || (u.cfw && u.cfw_rows >= 1 && !u.mov_w) || u.pmax > kRowsPmax))
        return fail(MSM_ERR_STATE, "launch_samples: the row form's buffers are missing, or a patch of %d points does not fit it", u.pmax);
    if (u.tree.nnodes <= 0 || !u.tree.mask) return fail(MSM_ERR_STATE, "target search structure missing");
    if (u.ntri >= (1 << kTriBits)) return fail(MSM_ERR_CAPACITY, "target mesh has %d triangles; the sample queue packs ids in %d bits", u.ntri, kTriBits);
    const bool rays = plan.sampler == MSM_SAMPLER_RAYS;
    SamplesArgs a;
    a.tree = u.tree;
    a.tfeat = u.tfeat;
    a.tD = u.D > 0 ? u.D : 1;
    a.N = u.N;
    a.L = u.L;
    a.rnl = u.rnl;
    a.src = u.src;
    a.Nsrc = u.Nsrc;
    a.pptr = u.pptr;
    a.pidx = u.pidx;
    a.order = u.order;
    a.pmax = u.pmax;
    a.nsplit = plan.nsplit;
    a.tval = w ? nullptr : u.tval;
    a.stri = w ? w->stri : nullptr;
    a.sw3 = w ? w->sw3 : nullptr;
    a.fix_list = u.fix_list;
    a.fix_pt = u.fix_pt;
    a.fix_cnt = u.fix_cnt;
    a.fix_off = u.fix_off;
    a.sfeat = u.sfeat;
    a.cfw = nullptr;
    a.absw = u.absw;
    a.simmeasure = u.simmeasure;
    a.percentile = u.percentile;
    a.U = (w || !fused_reduction || rays) ? nullptr : u.U;  // only k_unary_samples reduces, and only the univariate table
    a.redo_list = u.redo_list;
    a.redo_count = u.fix_cnt;
    a.status = ctx->d_status;
    const bool mov_weights = prepare_rows && u.cfw && u.cfw_rows >= 1;
    a.mov_cfw = mov_weights ? u.cfw : nullptr;
    a.mov_a = prepare_rows ? u.mov_a : nullptr;
    a.mov_w = mov_weights ? u.mov_w : nullptr;
    a.mov_stat = prepare_rows ? u.mov_stat : nullptr;
    MSM_TRY(rays ? allow_lds(k_unary_rays, plan.sampler_lds) : allow_lds(k_unary_samples, plan.sampler_lds));
    const int blocks = unary_workgroups(u.N, plan.nsplit);
    if (u.ev_start) MSM_HIP(hipEventRecord(u.ev_start, ctx->stream));
    if (rays) {
        hipLaunchKernelGGL(k_unary_rays, dim3(blocks), dim3(256), plan.sampler_lds, ctx->stream, a);
    } else {
        hipLaunchKernelGGL(k_unary_samples, dim3(blocks), dim3(256), plan.sampler_lds, ctx->stream, a);
    }
    MSM_HIP(hipGetLastError());
    if (u.ev_stop) MSM_HIP(hipEventRecord(u.ev_stop, ctx->stream));
    hipLaunchKernelGGL(k_unary_fixup, dim3(kFixBlocks + (prepare_rows ? (u.N + 3) / 4 : 0)), dim3(256), 0, ctx->stream, a);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
