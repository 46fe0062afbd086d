// unary.hpp -- the unary label-cost table (computeUnaryCosts, M/DiscreteCostFunction.cpp:236-243): what its three units share.
//
//   unary_plan.cpp             host only: every decision that depends on the largest patch (the plan, the LDS formulae, the refusals), the
//                              fix-up list's segments and the control points' launch order
//   unary_kernels.hip          the samplers: k_unary_rays (targets with a direction table), k_unary_samples (the complete sampler, the
//                              fallback) and k_unary_fixup behind either, with the prepare blocks of the row form as its passengers
//   unary_reduce_kernels.hip   the six reductions, and the two launchers that cost.cpp calls
#pragma once

#include "internal.hpp"

namespace msm {

// ---- constants the plan shares with the kernels ----
constexpr int kChunk = 768;       // k_unary_samples: samples per LDS pass (3 rounds of 256 lanes)
constexpr int kQueueCap = 3072;   // ... (sample, triangle) pairs per pass
constexpr int kTriBits = 22;      // ... queue entry = sample << 22 | triangle
constexpr int kFixSegs = MSM_UNARY_FIX_SEGMENTS;  // segments of the fix-up list (unary_kernels.hip: SamplesArgs); k_unary_fixup scans them with one wavefront
static_assert(kFixSegs == 64, "k_unary_fixup's prefix sum is one wavefront wide");
constexpr int kCntStride = 32;    // the fix-up counters sit 128 bytes apart
// A workgroup of gfx950 can address 160 KB of LDS, static variables included; above 64 KB of dynamic LDS a kernel needs its attribute raised first.
constexpr size_t kLdsWorkgroup = 160 * 1024, kLdsDefault = 64 * 1024;
constexpr size_t kStaticSampler = 16;  // k_unary_samples: s_qn, s_ndefer; k_unary_rays: s_nleft, s_base
constexpr size_t kStaticFlat = 32;     // k_unary_reduce_flat: s_stat[3]
constexpr int kFixBlocks = 4096;       // k_unary_fixup's own workgroups; the prepare blocks of the row form ride behind them in the same launch
constexpr int kRowsPmax = 96;          // k_unary_reduce_rows keeps a whole patch in registers: 12 values in each of a row's 8 lanes

// The form of the univariate correlation / SSD reduction (msm_cost_routes: routes[MSM_ROUTE_UNARY_FORM]).  Rows: the fix-up launch also writes every
// control point's moving patch in patch order with its statistics, and k_unary_reduce_rows reduces one table row per 8-lane group from them.
// Otherwise (a patch that does not fit the registers) k_unary_reduce_flat stages the moving patch per workgroup as before.
inline bool unary_row_form(int simmeasure, int pmax) { return (simmeasure == 1 || simmeasure == 2) && pmax <= kRowsPmax; }

// ---- the sampling kernels' grid: which workgroup takes which control point and which of its labels ----
// The workgroups of one XCD (workgroup % 8, round-robin dispatch) get a contiguous range of launch positions, i.e. spatial neighbours on
// the icosphere (unary_launch_order), so each XCD's L2 keeps its own part of the target.  (A device-side work queue was measured 2.4x slower
// here: the returning atomics serialise the workgroups.)  The labels of a control point are split over nsplit workgroups (same XCD) so that one
// workgroup's samples fit a single LDS pass and the grid has enough workgroups to balance over the 256 CUs.
__host__ __device__ inline int unary_labels_per_workgroup(int L, int nsplit) { return (L + nsplit - 1) / nsplit; }
__host__ __device__ inline int unary_workgroups(int N, int nsplit) { return nsplit * 8 * ((N + 7) >> 3); }
// Workgroup wg of unary_workgroups(N, nsplit): the position `at` of its control point in the launch order and its labels [l_beg, l_end);
// false: the workgroup is idle (padding of the eight ranges, or no label left for it).
__host__ __device__ inline bool unary_workgroup_share(unsigned wg, int N, int L, int nsplit, int &at, int &l_beg, int &l_end) {
    const int per = (N + 7) >> 3, slots = 8 * per;
    const int part = wg / slots, slot = wg - part * slots;
    at = (slot & 7) * per + (slot >> 3);
    if (at >= N) return false;
    const int lper = unary_labels_per_workgroup(L, nsplit);
    l_beg = part * lper;
    l_end = L < l_beg + lper ? L : l_beg + lper;
    return l_beg < l_end;
}

// ---- the plan (unary_plan.cpp) ----
// What a unary-table launch does for (cost kind, similarity, D, L, largest patch, sampler): unary_plan() takes every decision that depends on the
// largest patch, the launchers act on the plan they are handed (UnaryLaunch::plan) and msm_unary_launch_plan shows it to the tests.
struct UnaryPlan {
    int nsplit = 1;              // workgroups (label ranges) per control point
    int sampler = 0;             // MSM_SAMPLER_*
    size_t sampler_lds = 0;      // dynamic LDS of the sampling kernel, bytes
    int reduce = 0;              // MSM_UNARY_*: the reduction kernel
    size_t reduce_lds = 0;       // its dynamic LDS, bytes
    int reduce_threads = 256;    // its workgroup size
    int refused = 0;             // MSM_PLAN_REFUSED_*: a kernel's LDS does not fit a workgroup; nothing is launched
};
UnaryPlan unary_plan(int kind, int simmeasure, int D, int L, int pmax, bool ray_table);
int unary_plan_refusal(const UnaryPlan &p, int pmax);  // MSM_OK, or MSM_ERR_CAPACITY with the message that names the patch size
bool unary_uses_ray_table(const DevTree &t);
int unary_nsplit(int L, int pmax);
int unary_fix_segments();
size_t unary_fix_counter_words();
void unary_fix_offsets(int N, int L, int pmax, const int32_t *pptr, const int32_t *order, std::vector<uint32_t> &off);
// launch order of the control points in the unary kernels: Morton order of their positions (cp: 3 x N)
void unary_launch_order(const double *cp, int N, std::vector<int32_t> &order);

// ---- the launch (unary_kernels.hip, unary_reduce_kernels.hip) ----
struct UnaryLaunch {
    DevTree tree;
    const double *tfeat;   // target features, V x D vertex-major
    int D;
    int N, L;
    const double *cp;      // 3 x N
    const double *rnl;     // N x L x 9 from launch_label_rotations
    const double *labels;  // 3 x L
    const double *src;     // 3 x Nsrc
    int Nsrc;
    const double *sfeat;   // D x Nsrc
    const double *cfw;     // rows x Nsrc or nullptr
    int cfw_rows;
    const double *sfeat_vm = nullptr;  // Nsrc x D and Nsrc x rows vertex-major copies (multivariate reduction), optional
    const double *cfw_vm = nullptr;
    const int *pptr, *pidx;
    const int *order;      // launch order of the control points (a permutation of 0..N-1)
    const double *absw;
    int pmax;
    int simmeasure;
    double percentile;     // DICE measures (sparsesimkernel::percentile)
    double *U;             // L x N
    // scratch owned by the cost object
    int ntri;                      // triangles in the target mesh
    double *tval;                  // one double per point sample (L * total patch points)
    unsigned long long *fix_list;  // one slot per point sample
    double *fix_pt;                // three doubles per slot
    unsigned int *fix_cnt;         // unary_fix_counter_words() words (zeroed by the launch)
    const unsigned int *fix_off;   // unary_fix_segments() + 1 offsets from unary_fix_offsets()
    int *redo_list;                // N * plan->nsplit ints: every workgroup of a control point may list it
    // the row form's moving side (univariate correlation / SSD with unary_row_form(); all nullptr otherwise): written by the prepare blocks of the
    // fix-up launch for every table, read by k_unary_reduce_rows
    double *mov_a = nullptr;       // the moving patches in patch order, one double per patch point (pptr's offsets)
    double *mov_w = nullptr;       // their weight row likewise, or nullptr without weights
    double *mov_stat = nullptr;    // 3 x N: sum of weights, weighted mean, weighted variance sum of each moving patch
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;  // optional: recorded around the samples kernel
    int *route = nullptr;          // optional: the launcher writes the MSM_UNARY_* value of the reduction kernel it chose
    int *form = nullptr;           // optional: ... and 1 where k_unary_reduce_rows stood in for k_unary_reduce_flat, else 0
    const UnaryPlan *plan = nullptr;  // unary_plan() for this launch
};
// multivariate / patchwise: the sampler stores (triangle, raw weights) per sample, a second kernel reduces
struct UnaryWeightsScratch {
    int *stri;      // one int per sample
    double *sw3;    // three doubles per sample
};
int launch_unary_univariate(msm_ctx *ctx, const UnaryLaunch &u);
int launch_unary_multivariate(msm_ctx *ctx, const UnaryLaunch &u, const UnaryWeightsScratch &w, bool patchwise);
// The plan's sampler and k_unary_fixup behind it; the launchers above call it before their reduction.  w: store (triangle, weights) instead of
// tval.  fused_reduction: k_unary_samples also reduces the control points it settles (DICE) and lists the others in u.redo_list.  prepare_rows: the
// fix-up launch carries the prepare blocks that fill u.mov_a / mov_w / mov_stat (k_unary_reduce_rows follows).
int launch_samples(msm_ctx *ctx, const UnaryLaunch &u, const UnaryPlan &plan, const UnaryWeightsScratch *w, bool fused_reduction, bool prepare_rows = false);

// dynamic LDS beyond the default limit: the kernel's attribute first (the plan has checked that it fits a workgroup)
template <class K>
inline int allow_lds(K kernel, size_t lds) {
    if (lds > kLdsDefault) MSM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MSM_OK;
}

}  // namespace msm
