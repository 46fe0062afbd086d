// group_internal.hpp -- the group handle and the helpers that the units of the groupwise path share (group.cpp, group_setup.cpp, group_exchange.cpp, group_move.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <numeric>
#include <thread>

#include "devbuf.hpp"
#include "host_parallel.hpp"
#include "kernels.hpp"
#include "resample.hpp"

using namespace msm;

struct msm_group {
    msm_ctx *ctx = nullptr;
    std::atomic<int> patch_cap_hint{0};
    std::atomic<size_t> pidx_hint{0};  // the longest patch index list of a subject so far: the next one's is compacted before the look at its counts
    // a uniform grid over the template's vertices for the range test of a set-up's patch lists (built by group_setup_pipeline, valid while it runs)
    DevBuf<int> d_rg_start, d_rg_cursor, d_rg_ids, d_rg_bad, d_rg_tmp;
    RangeGrid rgrid;
    bool rgrid_valid = false;
    int patch_max = 0;  // largest patch of any subject (msm_group_finalize)
    int pair_lanes = 32;  // lanes per query of k_group_pairwise: 16 when nearly all patches fit a quarter wavefront's registers (msm_group_finalize)
    int64_t npatch = 0, nsmall = 0;  // the patches msm_group_finalize counted, and those of at most kPairSmallPatch entries (msm_group_pair_launch)
    msm_group_params p{};
    int S = 0;
    msm_mesh *tmpl = nullptr;
    std::vector<double> mask;
    DevBuf<double> d_mask;
    int N = 0, Tc = 0;
    std::vector<int32_t> cp_tri;                 // 3 x Tc SoA
    std::vector<msm_mesh *> cpmesh;              // per subject (owned)
    std::vector<msm_mesh *> data;                // per subject (borrowed)
    std::vector<std::vector<double>> feat;       // per subject D x V
    std::vector<std::vector<double>> orig;       // per subject 3 x N: _ORIG_MESHES coords of the control-point ids
    std::vector<char> have_orig;
    int D = 0, L = 0;
    std::vector<double> labels;                  // 3 x L SoA
    // setup products
    bool ready = false, common_ready = false;
    std::vector<char> have_subject;
    std::vector<int32_t> pairs, triplets;
    DevBuf<int32_t> d_pairs, d_triplets;
    std::vector<double> rot, moved;              // (S*N) x 9, (S*N) x L x 3
    DevBuf<double> d_moved, d_cp, d_orig;
    std::vector<std::vector<double>> spacing;
    std::vector<std::unique_ptr<DevBuf<double>>> F;  // S * L: windows into Fslab[subject]
    std::vector<std::unique_ptr<DevBuf<double>>> Fslab;  // per subject: its L resampled feature maps in one allocation (one hipMalloc instead of nineteen per subject
                                                         // and set-up, and large pages under the label steps' gathers)
    std::vector<std::unique_ptr<DevBuf<int32_t>>> pptr, pidx;  // per subject
    // per subject: the D values of every patch entry beside its id (GroupArgs::pval; built by msm_group_finalize, 50 MB per subject at ico6 / ico4, D = 2)
    std::vector<std::unique_ptr<DevBuf<double>>> pval;
    DevBuf<double *> d_pvalp;
    DevBuf<GroupPatchRef> d_patch_dir;  // GroupArgs::dir
    bool pval_ready = false;
    // A group with imported subjects (a rank of a sharded run) evaluates a SLICE of the pair list, which touches a fraction of the patches (an eighth of the
    // control points with eight ranks): the value copies are then written for the nodes of the slice only, when the slice is first asked for
    // (ensure_patch_values); pval_p0 / pval_p1: the slice they cover (the whole list after a set-up without imports)
    bool pval_deferred = false;
    int64_t pval_p0 = -1, pval_p1 = -1;
    DevBuf<int> d_node_flags;
    std::vector<std::vector<int32_t>> h_pptr, h_pidx;  // host copies of the lists: caches, filled when somebody asks (fetch_host_pptr / fetch_host_pidx)
    // What msm_group_finalize and the exports need to know of a subject's lists -- index count, largest patch, patches of at most kPairSmallPatch
    // entries.  Whoever gives a subject its lists writes it: subject_patches from its counts, the host import from the validated offsets, the
    // device imports from the check kernel.
    struct PatchStat {
        int64_t npidx = 0;
        int largest = 0, small = 0;
    };
    std::vector<PatchStat> patch_stat;
    DevBuf<const double *> d_Fp;
    DevBuf<const int *> d_pptrp, d_pidxp;
    DevBuf<int> d_query[4];   // index columns of a batch of evaluations (kept between calls)
    DevBuf<double> d_answer;
    // what the set-up of ONE subject needs before its per-label work can start: the L rotated copies of its data mesh, their trees
    // (a forest), its features.
    static constexpr int kStages = 3;  // of a pipeline: the preparing loop runs this many subjects ahead of the consuming one (run_setup_pipe)
    struct Stage {
        DevBuf<double> d_rot, d_feat, d_rot9;  // d_rot9: the vertices' rotation matrices when they come from the host (rotation_mode 1)
        std::vector<double> rot9;
        Forest forest;
        bool forest_ok = false;
    };
    // the per-label remainder of a subject's set-up with the label as the second grid dimension of every launch (stage_batch)
    struct Batch {
        msm_ctx *ctx = nullptr;  // a stream of its own: runs beside the main stream's preparation of the next subject
        SurgeryScratch surgery;  // of the L problems of one subject
        DevBuf<int> open;
        DevBuf<int2> info[2];
    };
    // One set-up pipeline: a main stream (rotations, forest of the next subject), a batch stream (the per-label work and the patch lists of the
    // current one) and everything they write before a subject's products.  Two pipelines work through alternate subjects side by side (round 4):
    // each is a chain of small dependent launches that leaves most of the GPU idle.
    struct Pipe {
        msm_ctx *main = nullptr;  // pipe 0: the group's context; pipe 1: a context (stream) of its own
        bool own_main = false;
        Stage stage[kStages];
        Batch batch;
        // scratch of subject_patches
        DevBuf<double> d_centres, d_sep;
        DevBuf<double4> d_chunkb;       // k_range: bounding balls of the template's vertices, 64 ids at a time
        DevBuf<int> d_scan_tmp;         // subject_patches: block sums of the row-offset scan
        DevBuf<uint32_t> d_slots;
        DevBuf<int> d_counts;
        msm_mesh *fallback = nullptr;   // on batch.ctx: the data mesh of a subject whose forest outgrew its arrays, one label at a time (stage_fallback)
    };
    static constexpr int kMaxPipes = 2;  // set-up pipelines, both in use from four subjects on (group_setup_pipeline)
    Pipe pipe[kMaxPipes];
    DevBuf<double> d_move_out;           // msm_group_fusion_move: the step's 4 P + 8 T results before they go to the host
    std::vector<int32_t> pair_order;     // the pair list in processing order (control points along a space-filling curve)
    DevBuf<int> d_pair_order;            // ... restricted to the slice [order_p0, order_p1) last asked for
    DevBuf<int4> d_pair_order4;          // the slice's positions with their pairs' nodes (GroupArgs::move_order4): rebuilt when the slice or the pair list changed
    uint64_t pairs_gen = 0, order4_gen = ~0ull;  // pairs_gen: counts estimate_pairs runs (the list's second nodes move with the control grids)
    int64_t order_p0 = -1, order_p1 = -1;
    int order_S = 0, order_N = 0;        // the sizes pair_order was built for
    // msm_group_set_pair_layout: 0 = the reference's list order (subject A, control point, subject B); 1 = control point by control point along the
    // curve -- the list itself in what is otherwise only the processing order, so that a contiguous slice of it is a REGION of the sphere
    int pair_layout = 0;
    // msm_group_set_rotation_mode: who computes estimate_rotation_matrix(centre, vertex) for the data meshes' vertices in get_patch_data.  1 (default): the
    // host's libm, as the reference does -- the rotated meshes are then the reference's to the bit; 0: the device (acos / sincos of the GPU's math library)
    int rotation_mode = 1;
    DevBuf<int> d_pair_perm, d_pairs_tmp;  // layout 1: reference position of every list position (kept with pair_order), and the list as the search wrote it
    Forest cp_forest;                    // the search trees of the S control grids, built together (estimate_pairs)
    DevBuf<double> d_cp_soa, d_rot, d_spacing, d_labels3;  // control points by component; ROT per node; spacing per node; labels 3 x L
    DevBuf<int2> d_forest_info;
    int64_t npairs = 0;                  // N * S * (S - 1) / 2; the host copy of the list (pairs) is fetched when asked for
    bool pval_serves_all() const { return pval_ready && pval_p0 == 0 && pval_p1 == npairs; }  // pval / dir cover every pair: batch evaluations may use them
    bool moved_on_host = false;          // g->moved mirrors d_moved (fetched for the rare host decisions of subject_patches)
    // the (current, current) pair costs of the last label step and the labeling they were computed for (GroupArgs::move_e00)
    DevBuf<double> d_e00;
    DevBuf<int> d_prev_labeling;
    bool e00_valid = false;
    int64_t e00_p0 = -1, e00_p1 = -1;
    // the (proposed, proposed) pair costs per label of the slice [e11_p0, e11_p1): valid from the label's step in the first sweep of
    // Fusion until the next set-up (GroupArgs::move_e11)
    DevBuf<double> d_e11;
    std::vector<unsigned char> e11_have;
    int64_t e11_p0 = -1, e11_p1 = -1;
    void drop_kept() {
        e00_valid = false;
        std::fill(e11_have.begin(), e11_have.end(), (unsigned char)0);
    }
    std::vector<int64_t> order_chunk;    // the slice's order is cut into pieces by OUTPUT range: piece k holds the pairs [order_chunk[k], order_chunk[k+1]) of the slice
    // msm_group_time_moves: HIP events around the kernels of a label step on the context's stream
    hipEvent_t t_ev0 = nullptr, t_ev1 = nullptr;
    bool timing = false, timed = false;
    hipStream_t copy_stream = nullptr;   // the finished pieces of a label step leave for the host while the next ones are computed
    std::vector<hipEvent_t> copy_events;
    // msm_group_mcmc_* (group_mcmc.cpp): the incidence of the pair list of set-up mc_inc_gen, the labelling a block reads, its segment
    // offsets, the pair costs of its queries and its two tables -- one set of buffers, reused by every block; events around a block's phases
    std::vector<int32_t> mc_inc_ptr, mc_inc_idx;
    DevBuf<int32_t> d_mc_inc_ptr, d_mc_inc_idx, d_mc_lab, d_mc_seg;
    DevBuf<double> d_mc_U, d_mc_tc;
    uint64_t mc_inc_gen = ~0ull;
    hipEvent_t mc_ev[4] = {nullptr, nullptr, nullptr, nullptr};
};


namespace msm {

constexpr int kBatchChunk = 1 << 22;  // evaluations per launch of a batch call (84 MB of pinned staging at most)

// the record of a subject's row offsets pptr[0 .. M]
inline msm_group::PatchStat patch_stat_of(const int32_t *pptr, size_t M) {
    msm_group::PatchStat st;
    st.npidx = pptr[M];
    for (size_t k = 0; k < M; ++k) {
        const int n = pptr[k + 1] - pptr[k];
        st.largest = std::max(st.largest, n);
        st.small += n <= kPairSmallPatch;
    }
    return st;
}

// Device room for the n entries (of `per` elements each) of a subject's patches, and one entry of padding: the fast path of k_group_pairwise loads with
// indices clamped to the patch, which for an empty patch in a subject's last row is the element behind the list.
template <class T>
inline hipError_t ensure_patch_entries(DevBuf<T> &buf, size_t n, size_t per = 1) {
    return buf.ensure(per * (n + 1));
}

// group.cpp
int subject_feature_slab(msm_group *g, int s, size_t per);
int group_args(msm_group *g, GroupArgs &a);
int pair_refusal(const msm_group *g);
int fetch_host_pptr(msm_group *g, int s);
int fetch_host_pidx(msm_group *g, int s);
// group_move.cpp
int ensure_patch_values(msm_group *g, int64_t pair0, int64_t pair1);

}  // namespace msm
