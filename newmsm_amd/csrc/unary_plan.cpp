// unary_plan.cpp -- the host decisions of a unary-table launch; no kernel lives here.
//
//   unary_plan / unary_plan_refusal   sampler, label split, reduction kernel and their LDS for a largest patch of pmax points, and the refusal
//                                     of what does not fit a workgroup's LDS
//   unary_fix_offsets                 the fix-up list's segments, from the workgroup mapping the samplers use (unary.hpp: unary_workgroup_share)
//   unary_launch_order                the order in which the samplers take the control points
#include <algorithm>

#include "similarity_device.hpp"  // kMvLanes, kMvKeep: the dimensions the eight-lanes-per-point reductions hold
#include "unary.hpp"

namespace msm {

// dynamic LDS of k_unary_samples when the labels are split over nsplit workgroups: patch coordinates and moving feature (4 pmax), rotations, the
// workgroup's sampled target values, pair queue, per-sample counts.  The fifth pmax slice once held a weight row; it is reserved and unread.
static size_t samples_lds(int pmax, int L, int nsplit) {
    const size_t lper = (size_t)unary_labels_per_workgroup(L, nsplit);
    return sizeof(double) * (5 * (size_t)pmax + 9 * (size_t)L + lper * pmax) + sizeof(unsigned) * kQueueCap + sizeof(int) * 2 * kChunk;
}
// dynamic LDS of k_unary_rays: patch coordinates, rotations, and the list of samples the table could not settle
static size_t rays_lds(int pmax, int L, int nsplit) {
    const size_t lper = (size_t)unary_labels_per_workgroup(L, nsplit);
    return sizeof(double) * (3 * (size_t)pmax + 9 * (size_t)L) + sizeof(int) * (lper * pmax + 4) + 16;
}

// Workgroups per control point: enough that one workgroup's samples are about one LDS pass (at most 4 for that
// reason), and more when the patch is so large (coarse control grid under a fine data grid) that the per-label target
// values would not fit in LDS otherwise.
int unary_nsplit(int L, int pmax) {
    int n = std::max(1, std::min(4, (int)(((size_t)L * pmax + kChunk - 1) / kChunk)));
    while (n < L && samples_lds(pmax, L, n) > 64 * 1024) ++n;
    return std::min(n, std::max(L, 1));
}

// Every decision of a unary-table launch that depends on the largest patch, in one place: the launchers act on this plan and on nothing
// else, and msm_unary_launch_plan hands it to the tests.  A plan whose sampler or reduction does not fit is refused before anything is launched.
UnaryPlan unary_plan(int kind, int simmeasure, int D, int L, int pmax, bool ray_table) {
    UnaryPlan p;
    const bool dice = simmeasure == 4 || simmeasure == 5;
    p.nsplit = unary_nsplit(L, pmax);
    p.sampler = ray_table ? MSM_SAMPLER_RAYS : MSM_SAMPLER_SAMPLES;
    p.sampler_lds = ray_table ? rays_lds(pmax, L, p.nsplit) : samples_lds(pmax, L, p.nsplit);
    if (p.sampler_lds + kStaticSampler > kLdsWorkgroup) p.refused = MSM_PLAN_REFUSED_SAMPLER;
    size_t stat = 0;
    if (kind == MSM_COST_UNIVARIATE) {
        // Correlation / SSD: both samplers only fill tval and k_unary_reduce_flat reduces it.  DICE: the wavefront-per-label kernel, over
        // all control points behind the ray sampler, over the redo list behind the complete sampler (which reduces the rest itself)
        p.reduce = dice ? MSM_UNARY_UNIVARIATE : MSM_UNARY_FLAT;
        p.reduce_lds = sizeof(double) * 2 * (size_t)pmax;  // moving feature and weights; DICE reads no weights: its second slice is reserved and unread
        stat = dice ? 0 : kStaticFlat;
    } else if (!dice && D >= 12 && D <= kMvLanes * kMvKeep) {  // few dimensions: a lane per point wastes less
        p.reduce = kind == MSM_COST_MULTIVARIATE ? MSM_UNARY_MV8 : (D <= 32 ? MSM_UNARY_PW8_4 : MSM_UNARY_PW8_8);
    } else {
        p.reduce = MSM_UNARY_FEATURES;
        p.reduce_lds = (dice && kind == MSM_COST_PATCHWISE) ? sizeof(double) * 8 * (size_t)pmax : 0;  // two patches per wavefront
        if (p.reduce_lds > kLdsWorkgroup) {  // one wavefront per control point: a quarter of the LDS
            p.reduce_lds /= 4;
            p.reduce_threads = 64;
        }
    }
    if (!p.refused && p.reduce_lds + stat > kLdsWorkgroup) p.refused = MSM_PLAN_REFUSED_REDUCTION;
    return p;
}

int unary_plan_refusal(const UnaryPlan &p, int pmax) {
    if (!p.refused) return MSM_OK;
    if (p.refused == MSM_PLAN_REFUSED_SAMPLER)
        return fail(MSM_ERR_CAPACITY, "a patch of %d points does not fit in LDS (%s, %zu bytes)", pmax, p.sampler == MSM_SAMPLER_RAYS ? "k_unary_rays" : "k_unary_samples", p.sampler_lds);
    return fail(MSM_ERR_CAPACITY, "a patch of %d points does not fit in LDS (reduction, %zu bytes)", pmax, p.reduce_lds);
}

bool unary_uses_ray_table(const DevTree &t) { return t.simple && t.ray_G > 0 && t.ray_cell && t.ray_tri; }

int unary_fix_segments() { return kFixSegs; }
size_t unary_fix_counter_words() { return (size_t)kCntStride * (1 + kFixSegs); }
// Segment s of the fix-up list holds all samples of the workgroups b with b % kFixSegs == s, so it cannot overflow
void unary_fix_offsets(int N, int L, int pmax, const int32_t *pptr, const int32_t *order, std::vector<uint32_t> &off) {
    const int nsplit = unary_nsplit(L, pmax);
    std::vector<uint64_t> size(kFixSegs, 0);
    for (int b = 0; b < unary_workgroups(N, nsplit); ++b) {
        int at, l_beg, l_end;
        if (!unary_workgroup_share(b, N, L, nsplit, at, l_beg, l_end)) continue;
        const int node = order[at];
        size[b % kFixSegs] += (uint64_t)(l_end - l_beg) * (pptr[node + 1] - pptr[node]);
    }
    off.assign(kFixSegs + 1, 0);
    for (int s = 0; s < kFixSegs; ++s) off[s + 1] = (uint32_t)std::min<uint64_t>(0xffffffffull, off[s] + size[s]);
}

void unary_launch_order(const double *cp, int N, std::vector<int32_t> &order) {
    auto spread = [](uint32_t v) {  // 10 bits -> every third bit
        v &= 0x3ff;
        v = (v | (v << 16)) & 0x030000ff;
        v = (v | (v << 8)) & 0x0300f00f;
        v = (v | (v << 4)) & 0x030c30c3;
        v = (v | (v << 2)) & 0x09249249;
        return v;
    };
    std::vector<std::pair<uint32_t, int32_t>> key(N);
    for (int i = 0; i < N; ++i) {
        uint32_t q[3];
        for (int a = 0; a < 3; ++a) {
            const double u = (cp[(size_t)a * N + i] + kBounds) / (2 * kBounds);
            q[a] = (uint32_t)std::max(0.0, std::min(1023.0, u == u ? u * 1024.0 : 0.0));
        }
        key[i] = {spread(q[0]) << 2 | spread(q[1]) << 1 | spread(q[2]), i};
    }
    std::sort(key.begin(), key.end());
    order.resize(N);
    for (int i = 0; i < N; ++i) order[i] = key[i].second;
}

}  // namespace msm
