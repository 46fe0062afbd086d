// label_step.cpp -- the label step of the optimisers' inner loop: msm_cost_triplet_octets, its hint msm_cost_triplet_octets_prefetch, and the
// single-combination form evaluateTotalCostSum uses (include/msmhip.h).  Three launch forms -- the fused triclique move (move_kernels.hip), the
// strain-only packed move and the general copy route (clique_kernels.hip) -- around which everything else exists once: the pass over the labeling
// (pack_labels), where the costs land (StepDelivery), what follows the kernel (finish_step), a step queued ahead (queue_step / take_pending_move /
// drop_pending_move).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "cost_internal.hpp"
#include "fusion_mplp.hpp"

using namespace msm;

// A label step queued by msm_cost_triplet_octets_prefetch that nobody took: wait for its kernel and discard what it may have raised (its evaluations
// were never asked for).  Called by every entry point of a cost function except the msm_cost_triplet_octets call that matches the prefetch.
int msm::drop_pending_move(msm_cost *c) {
    if (!c->pending.valid) return MSM_OK;
    c->pending.valid = false;
    ++c->prefetch_drops;
    msm_ctx *ctx = c->ctx;
    if (ctx->pending_cost == c) ctx->pending_cost = nullptr;
    MSM_TRY(ctx_sync(ctx));
    volatile int *flags = ctx->h_flag;
    if (flags) {
        flags[1] = 0;
        if (flags[0] != 0) {
            flags[0] = 0;
            (void)check_status(ctx, "a dropped prefetch");  // clears the device status word
        }
    }
    return MSM_OK;
}

// The same from the context's side: whichever cost function holds the context's queued step.  Every entry point that synchronises the stream and reads the
// status word or the mapped flags calls this first (or drop_pending_move on its own object) -- a status raised by a speculative kernel must not be reported
// against another call, a tail request in flags[1] not be consumed by another cost function's move.
int msm::drop_ctx_pending(msm_ctx *ctx) {
    msm_cost *c = ctx->pending_cost;
    if (!c) return MSM_OK;
    ctx->pending_cost = nullptr;
    return drop_pending_move(c);
}

namespace {

// what the caller asked for: the step (labeling, label) into E (8 x T), or, single, combination 000 of the labeling alone (E: T values)
struct StepCall {
    const int32_t *labeling;
    int32_t label;
    double *E;
    bool single;
    // msm_cost_fusion_mplp_step: the costs stay on the device, in dev (8 x T; E is not written), and behind() queues the solve that reads them on the
    // context's stream -- behind the step's kernel, ahead of the step's one synchronisation; again: once more, after a fused move's tail kernel
    double *dev = nullptr;
    const std::function<int(bool again)> *behind = nullptr;
};

// ---- fused fusion move of the HO classes (move_kernels.hip) ----
// bin slots and control triangles per workgroup (at most 64 and 8: the kernel's LDS holds 64 proposed triangles)
constexpr int kMoveSlots = 64, kMoveTriangles = 8;

bool fused_move_applies(const msm_cost *c, const CliqueArgs &a) {
    return cost_is_ho(c) && a.ho_vals && a.tree.simple && a.tree.ray_G > 0 && a.rmode != 4 && a.rmode != 5 && c->pmax <= 128 && a.T > 0;
}

// per get_source_data(): the workgroups' runs of control triangles and the label-independent part of every bin point
int ensure_move(msm_cost *c, const CliqueArgs &a) {
    if (c->move_valid) return MSM_OK;
    msm_ctx *ctx = c->ctx;
    const int T = a.T;
    std::vector<int4> blk;
    // with many features per sample (the eight-lanes-per-sample passes of k_ho_move<., 2>) smaller workgroups do better: 88 against
    // 95 us at D = 32 with 48 slots / 6 triangles; with one feature the two shapes are level in the kernel and the larger is cheaper to launch
    const bool wide = a.kind == MSM_COST_HO_MULTIVARIATE && a.D >= 12;
    int max_slots = wide ? 48 : kMoveSlots, max_tris = wide ? 6 : kMoveTriangles;
    // A workgroup's time is a chain (proposed triangles, sampling rounds, similarity passes, last phase) whose length grows with the
    // triangles it holds, and the whole grid is resident at once up to ~1000 workgroups: on the coarser control grids of a registration's
    // first levels fewer triangles per workgroup shorten every chain at no cost (D = 32: 55 -> 41 us at ico3, 55 -> 34 us at ico2; the
    // ico4 grid keeps 6 / 8).  The smallest run of triangles that still fits the grid into one residency round:
    const int most = max_tris;
    for (int t : {1, 2, 4, 6, 8})
        if ((T + most - 1) / most <= 512 && t <= most && (T + t - 1) / t <= 1024) {  // only when the usual run leaves half the GPU empty
            max_tris = t;
            max_slots = 8 * t;
            break;
        }
    int slots = 0, nt = 0, cap = max_slots, first = 0, most_tris = 0;
    auto close = [&](int t_end) {
        most_tris = std::max(most_tris, nt);
        if (nt > 0) blk.push_back(make_int4(first, nt, c->pptr[first], c->pptr[t_end] - c->pptr[first]));
        first = t_end;
        slots = nt = 0;
    };
    for (int t = 0; t < T; ++t) {
        const int n = c->pptr[t + 1] - c->pptr[t];
        if (nt > 0 && (slots + n > max_slots || nt == max_tris)) close(t);
        slots += n;
        ++nt;
        cap = std::max(cap, slots);
    }
    close(T);
    const size_t ns = std::max<size_t>(c->pidx.size(), 1);
    MSM_TRY(c->d_blk.upload(blk.data(), blk.size(), ctx));
    MSM_HIP(c->d_tri_frame.ensure(5 * (size_t)T));
    MSM_HIP(c->d_tri_stat.ensure(3 * (size_t)T));
    MSM_HIP(c->d_slot_wda.ensure(ns));
    MSM_HIP(c->d_slot_tri.ensure(ns));
    MSM_HIP(c->d_slot_w.ensure(3 * ns));
    MSM_HIP(c->d_slot_sf.ensure(ns));
    if (a.cfw) MSM_HIP(c->d_slot_cw.ensure(ns));
    MSM_HIP(c->d_defer_list.ensure((size_t)8 * T));
    if (!c->d_defer_cnt.p) MSM_HIP(c->d_defer_cnt.zero(2, ctx->stream));
    int st = launch_move_prepare(ctx, a, (int)c->pidx.size(), c->d_slot_tri.p, c->d_slot_w.p, c->d_slot_sf.p, a.cfw ? c->d_slot_cw.p : nullptr, c->d_slot_wda.p,
                                 c->d_tri_frame.p, c->d_tri_stat.p);
    if (st) return st;
    MSM_TRY(ctx_sync(ctx));  // blk is a local
    c->move_nblk = (int)blk.size();
    c->move_cap = cap;
    c->move_maxtri = most_tris;
    c->move_valid = true;
    return MSM_OK;
}

// ---- what exists once around the three launches ----

// the one pass over a step's labeling: every entry checked and, where the labeling fits the kernel arguments (a byte per control point), packed into lab
int pack_labels(const CliqueArgs &a, const int32_t *labeling, MoveLabels &lab, bool &packed) {
    packed = a.N <= 4 * kMoveLabelWords && a.L <= 256;
    if (packed) std::memset(lab.w, 0, sizeof(uint32_t) * (size_t)((a.N + 3) / 4));
    for (int i = 0; i < a.N; ++i) {
        if (labeling[i] < 0 || labeling[i] >= a.L) return fail(MSM_ERR_INVALID, "labeling[%d] out of range", i);
        if (packed) lab.w[i >> 2] |= (uint32_t)labeling[i] << ((i & 3) * 8);
    }
    return MSM_OK;
}

// Fills d for the call's costs (StepDelivery, label_step.hpp).  The pinned io block is taken when the costs travel through it or, pin_anyway, for the
// labeling (pageable copies of these sizes cost more than the kernels); a hint prepares nothing beyond the caller's own array.  staged_copy leaves
// out_dev to label_step.
int deliver(msm_cost *c, const CliqueArgs &a, const StepCall &call, bool hint, bool pin_anyway, StepDelivery &d) {
    msm_ctx *ctx = c->ctx;
    d.in_pad = (sizeof(int32_t) * (size_t)a.N + 255) & ~(size_t)255;
    d.out_bytes = sizeof(double) * (call.single ? 1 : 8) * (size_t)a.T;
    d.out_dev = call.dev ? call.dev : static_cast<double *>(ctx_mapped(ctx, call.E, d.out_bytes));
    d.direct = d.out_dev != nullptr;
    if (hint || (d.direct && !pin_anyway)) return MSM_OK;
    MSM_TRY(ctx_io_pinned(ctx, d.in_pad + d.out_bytes, &d.pin));
    if (d.direct) return MSM_OK;
    d.staged_copy = !ctx->io_dev;  // (the pinned block could not be mapped)
    if (ctx->io_dev) d.out_dev = reinterpret_cast<double *>(static_cast<char *>(ctx->io_dev) + d.in_pad);
    return MSM_OK;
}

// After the kernel of a fused (m) or packed strain (m == nullptr) step has completed -- the stream is synchronised --, in the synchronous call and in the
// call that takes a queued step alike: the tail kernel when the fused move's main kernel asked for it, a raised status, the copy-out.  lab: the packed
// labeling (nullptr: it is in d_labeling)
int finish_step(msm_cost *c, const CliqueArgs &a, const MoveArgs *m, const MoveLabels *lab, const StepDelivery &d, double *E) {
    msm_ctx *ctx = c->ctx;
    volatile int *flags = ctx->h_flag;
    if (m) c->move_deferred = 0;
    if (m && flags[1] != 0) {  // rare: some evaluations need the complete search (sibling leaves, nearest vertex)
        flags[1] = 0;
        MSM_TRY(launch_move_tail(ctx, a, *m, lab));
        if (d.staged_copy) MSM_HIP(hipMemcpyAsync((char *)d.pin + d.in_pad, d.out_dev, d.out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        MSM_TRY(ctx_sync(ctx));
        c->move_tails++;
        unsigned listed = 0;  // how many evaluations the tail kernel took (msm_cost_routes): this move's counter stays until the next move but one clears it
        MSM_TRY(stage_d2h(ctx, &listed, m->defer_cnt + m->parity, sizeof listed));
        MSM_TRY(ctx_sync(ctx));
        c->move_deferred = (int32_t)std::min<unsigned>(listed, (unsigned)INT32_MAX);
    }
    int st = MSM_OK;
    if (flags[0] != 0) {
        flags[0] = 0;
        st = check_status(ctx, "computeTripletCost");
    }
    if (!d.direct) std::memcpy(E, (char *)d.pin + d.in_pad, d.out_bytes);
    return st;
}

// launched for msm_cost_triplet_octets_prefetch: msm_cost_triplet_octets(labeling, label, E) will wait for the step and finish it with what is kept here
// (m == nullptr: the packed strain move, whose finish needs neither a nor lab)
int queue_step(msm_cost *c, const StepCall &call, const CliqueArgs &a, const MoveArgs *m, const MoveLabels &lab, const StepDelivery &d) {
    msm_cost::PendingMove &p = c->pending;
    p.kind = m ? 1 : 2;
    p.label = call.label;
    p.E = call.E;
    p.epoch = c->ctx->epoch;
    c->ctx->pending_cost = c;
    p.labeling.assign(call.labeling, call.labeling + a.N);
    p.d = d;
    if (m) p.a = a, p.m = *m, p.lab = lab;
    c->pending.valid = true;
    return MSM_OK;
}

// the msm_cost_triplet_octets call a prefetch was queued for: wait for the kernel, then what follows a step's kernel in the synchronous call
int take_pending_move(msm_cost *c, double *E) {
    msm_ctx *ctx = c->ctx;
    msm_cost::PendingMove &p = c->pending;
    p.valid = false;
    if (ctx->pending_cost == c) ctx->pending_cost = nullptr;
    ++c->prefetch_hits;
    MSM_TRY(ctx_sync(ctx));
    return finish_step(c, p.a, p.kind == 1 ? &p.m : nullptr, &p.lab, p.d, E);
}

// ---- the three forms: fill the arguments and launch ----

// The fused fusion move of the triclique classes (move_kernels.hip) for one labeling: all eight combinations of every control triangle
// (E: 8 x T, a label step of Fusion) or, single, combination 000 only (E: T values -- the triplet part of evaluateTotalCostSum,
// M/DiscreteCostFunction.cpp:55-77, which used to go through the general on-demand kernel at 143 us per call at ico4 / 32 features).
// lab: the packed labeling, or nullptr: it is in d_labeling.  The timing events go round the main kernel, not the tail.
int fused_move(msm_cost *c, const CliqueArgs &a, const StepCall &call, const MoveLabels *lab, const StepDelivery &d, MoveArgs &m) {
    m.slot_tri = c->d_slot_tri.p;
    m.slot_w = c->d_slot_w.p;
    m.slot_sf = c->d_slot_sf.p;
    m.slot_cw = a.cfw ? c->d_slot_cw.p : nullptr;
    m.slot_wda = c->d_slot_wda.p;
    m.tri_frame = c->d_tri_frame.p;
    m.tri_stat = c->d_tri_stat.p;
    m.blk = c->d_blk.p;
    m.nblk = c->move_nblk;
    m.cap = c->move_cap;
    m.labeling = lab ? nullptr : c->d_labeling.p;
    m.label = call.label;
    m.vals = c->d_ho_vals.p;
    m.defer_list = c->d_defer_list.p;
    m.defer_cnt = c->d_defer_cnt.p;
    m.parity = c->move_parity;
    c->move_parity ^= 1;
    m.out = d.out_dev;
    m.host_flags = c->ctx->d_flag_map;
    m.single = call.single ? 1 : 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    next_timing_slot(c, e0, e1);
    return launch_move(c->ctx, a, m, lab, e0, e1, &c->route_move);
}

// The strain-only label step (--regoption=3 without --triclique: BASELINE config 2) like the triclique move: the labeling rides in
// the kernel arguments, the costs land in mapped pinned memory -- the caller's array when it came from msm_host_alloc --, a raised
// status in the mapped flag: one launch + one synchronisation instead of two copy commands around the kernel and a status read-back
// (57 -> 25 us per call at ico4; MSMHIP_OCTETS=copy: the old way)
int packed_strain_move(msm_cost *c, const CliqueArgs &a, int32_t label, const MoveLabels &lab, const StepDelivery &d) {
    msm_ctx *ctx = c->ctx;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (next_timing_slot(c, e0, e1)) MSM_HIP(hipEventRecord(e0, ctx->stream));  // msm_cost_enable_timing: events around this move's kernel, like the triclique move's
    MSM_TRY(launch_triplet_octets_packed(ctx, a, lab, label, d.out_dev, ctx->d_flag_map));
    c->route_move = MSM_MOVE_STRAIN;  // that launcher has one kernel
    if (e1) MSM_HIP(hipEventRecord(e1, ctx->stream));
    return MSM_OK;
}

// the general route (the on-demand kernels: anatomical strain, large bins, general targets, more labels than a byte holds): labeling and costs travel
// by copy commands through the pinned block, a raised status through the status word
int copied_move(msm_cost *c, const CliqueArgs &a, int32_t label, const StepDelivery &d) {
    msm_ctx *ctx = c->ctx;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (next_timing_slot(c, e0, e1)) MSM_HIP(hipEventRecord(e0, ctx->stream));
    MSM_TRY(launch_triplet_octets(ctx, a, c->d_labeling.p, label, d.out_dev, &c->route_move));
    if (e1) MSM_HIP(hipEventRecord(e1, ctx->stream));
    return MSM_OK;
}

// One step: choose the form, launch it, then wait and finish, or (hint) leave it queued.  The call of the optimisers' inner loop, once per label step:
// in the fused form with a packed labeling into the caller's own array one launch and one synchronisation -- the labeling rides in the kernel arguments,
// the costs are written into mapped pinned memory, a raised status shows up in a mapped flag.
int label_step(msm_cost *c, const CliqueArgs &a, const StepCall &call, bool hint) {
    msm_ctx *ctx = c->ctx;
    const bool fused = fused_move_applies(c, a);
    if (fused) {  // (both ahead of the labeling check)
        MSM_TRY(ensure_move(c, a));
        MSM_TRY(ctx_flag(ctx));
    }
    MoveLabels lab;
    bool packed = false;
    MSM_TRY(pack_labels(a, call.labeling, lab, packed));
    StepDelivery d;
    MSM_TRY(deliver(c, a, call, hint, !(fused && packed), d));
    // the strain-only classes take the packed form where the kernel can write mapped memory, the general route otherwise
    const char *env = fused ? nullptr : std::getenv("MSMHIP_OCTETS");  // "copy": the general route; read per call, the tests run both ways in one process
    const bool strain = !fused && !cost_is_ho(c) && packed && d.out_dev && !(env && std::strcmp(env, "copy") == 0) && ctx_flag(ctx) == MSM_OK;
    // The hint's whole rule: a step is queued ahead only in a one-kernel form (never the general route), with the labeling in the kernel arguments, into
    // the caller's own mapped array, and never in the single form.  Any other hint is silently ignored: the call itself will do everything.
    if (hint && !((fused || strain) && packed && d.direct && !call.single)) return MSM_OK;
    const bool general = !fused && !strain;
    if (general && !call.dev) d.direct = false, d.staged_copy = true;  // whatever E is
    if (d.staged_copy) {
        MSM_HIP(c->d_clique_out.ensure((size_t)8 * a.T));  // (also large enough for the T values of a single-combination call)
        d.out_dev = c->d_clique_out.p;
    }
    if (!packed || general) {  // the labeling goes to d_labeling through the pinned block
        std::memcpy(d.pin, call.labeling, sizeof(int32_t) * (size_t)a.N);
        MSM_HIP(c->d_labeling.ensure(a.N));
        MSM_HIP(hipMemcpyAsync(c->d_labeling.p, d.pin, sizeof(int32_t) * (size_t)a.N, hipMemcpyHostToDevice, ctx->stream));
    }
    MoveArgs m;
    const MoveLabels *labp = packed ? &lab : nullptr;
    MSM_TRY(fused ? fused_move(c, a, call, labp, d, m) : strain ? packed_strain_move(c, a, call.label, lab, d) : copied_move(c, a, call.label, d));
    if (d.staged_copy) MSM_HIP(hipMemcpyAsync((char *)d.pin + d.in_pad, d.out_dev, d.out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    c->counters[2] += (int64_t)(d.out_bytes / sizeof(double));
    if (hint) return queue_step(c, call, a, fused ? &m : nullptr, lab, d);
    if (call.behind) MSM_TRY((*call.behind)(false));
    if (general) {
        const int st = check_status(ctx, "computeTripletCost");  // synchronises
        if (!call.dev) std::memcpy(call.E, (char *)d.pin + d.in_pad, d.out_bytes);
        return st;
    }
    MSM_TRY(ctx_sync(ctx));
    const int64_t tails = c->move_tails;
    MSM_TRY(finish_step(c, a, fused ? &m : nullptr, labp, d, call.E));
    if (call.behind && c->move_tails != tails) {  // rare: the tail kernel completed the octets after the solve had read them -- the solve runs again
        MSM_TRY((*call.behind)(true));
        MSM_TRY(ctx_sync(ctx));
    }
    return MSM_OK;
}

int triplet_octets_impl(msm_cost *c, const int32_t *labeling, int32_t label, double *E, bool hint) {
    CliqueArgs a;
    MSM_TRY(clique_args(c, true, false, a));  // (drops a queued step nobody took)
    if (label < 0 || label >= a.L) return fail(MSM_ERR_INVALID, "label %d out of range", label);
    return label_step(c, a, StepCall{labeling, label, E, false}, hint);
}

}  // namespace

// combination 000 of a fusion move IS computeTripletCost(t, labeling[a], labeling[b], labeling[c]): the fused move kernel with one
// combination per control triangle instead of the general on-demand kernel (143 -> about 20 us at ico4 / 32 features)
int msm::fused_single_costs(msm_cost *c, const int32_t *labeling, double *vals, bool *done) {
    CliqueArgs a;
    MSM_TRY(clique_args(c, true, false, a));
    *done = fused_move_applies(c, a);
    return *done ? label_step(c, a, StepCall{labeling, 0, vals, true}, false) : MSM_OK;
}

extern "C" {

int msm_cost_triplet_octets(msm_cost *c, const int32_t *labeling, int32_t label, double *E) {
    if (!c || !labeling || !E) return fail(MSM_ERR_INVALID, "msm_cost_triplet_octets: null argument");
    if (c->pending.valid && c->pending.label == label && c->pending.E == E && c->pending.epoch == c->ctx->epoch && c->ctx->pending_cost == c && c->cpgrid && (int)c->pending.labeling.size() == c->cpgrid->V &&
        std::memcmp(c->pending.labeling.data(), labeling, sizeof(int32_t) * c->pending.labeling.size()) == 0)
        return take_pending_move(c, E);  // queued ahead by msm_cost_triplet_octets_prefetch: the kernel ran while the host solved
    return triplet_octets_impl(c, labeling, label, E, false);
}

// A hint: queue the label step (labeling, label) into E without waiting -- the optimiser's host-side solve of the step before runs meanwhile, and most
// steps of a converging level leave the labeling as it was (three of four in the MSMAll schedule).  Honoured when E lies in msm_host_alloc memory and the
// step takes the one-kernel form (triclique fused move or strain-only packed move); silently ignored otherwise.  The results do not depend on it.
int msm_cost_triplet_octets_prefetch(msm_cost *c, const int32_t *labeling, int32_t label, double *E) {
    if (!c || !labeling || !E) return fail(MSM_ERR_INVALID, "msm_cost_triplet_octets_prefetch: null argument");
    return triplet_octets_impl(c, labeling, label, E, true);
}

// MPLP over the binary problem of the label step (labeling, label) with nothing but the results leaving the device: the step's kernel
// -- whichever form label_step chooses -- writes its 8 T costs into d_step_octets, k_fusion_mplp gathers theta from the unary table and solves behind it,
// one synchronisation.  A step queued ahead is dropped first (clique_args), by the rule of every entry point but the matching msm_cost_triplet_octets.
int msm_cost_fusion_mplp_step(msm_cost *c, const int32_t *labeling, int32_t label, int32_t sweeps, int32_t polish, int32_t *x, int32_t *sweeps_run,
                              int32_t *passes_run, double *energy, double *bound, double *energies, double *bounds) {
    const char *what = "msm_cost_fusion_mplp_step";
    if (!c || !labeling || !x) return fail(MSM_ERR_INVALID, "%s: null argument", what);
    if (!c->cpgrid || c->L <= 0 || c->triplets.empty()) return fail(MSM_ERR_STATE, "%s: meshes, labels and triplets must be set first", what);
    const int N = c->cpgrid->V, T = (int)(c->triplets.size() / 3);
    MSM_TRY(fusion_mplp_check(what, c->triplets.data(), N, T, sweeps, polish));
    if (label < 0 || label >= c->L) return fail(MSM_ERR_INVALID, "label %d out of range", label);
    msm_ctx *ctx = c->ctx;
    MSM_TRY(drop_pending_move(c));  // a step queued ahead that nobody took
    if (!c->table_valid) {  // computeUnaryCosts as msm_cost_mplp_optimise runs it; an iteration's table serves all its label steps
        MSM_TRY(msm_cost_unary_table_async(c));
        MSM_TRY(check_status(ctx, "computeUnaryCosts"));
    }
    CliqueArgs a;  // (after the table: it recomputes the label rotations the clique kernels read)
    MSM_TRY(clique_args(c, true, false, a));
    if (!c->fusion_plan) {
        std::shared_ptr<FusionMplpPlan> plan = std::make_shared<FusionMplpPlan>();
        MSM_TRY(fusion_mplp_build_plan(ctx, c->triplets.data(), N, T, *plan));
        c->fusion_plan = plan;
    }
    const FusionMplpPlan &plan = *static_cast<const FusionMplpPlan *>(c->fusion_plan.get());
    if (c->d_step_octets.ensure((size_t)8 * T) != hipSuccess) return stage_alloc_failed(sizeof(double) * 8 * (size_t)T);
    MSM_TRY(c->d_step_labeling.upload(labeling, (size_t)N, ctx));
    const std::function<int(bool)> behind = [&](bool again) {
        return fusion_mplp_queue(ctx, what, plan, nullptr, c->d_U.p, c->d_step_labeling.p, label, a.L, c->d_step_octets.p, sweeps, polish, again);
    };
    StepCall call{labeling, label, nullptr, false};
    call.dev = c->d_step_octets.p;
    call.behind = &behind;
    MSM_TRY(label_step(c, a, call, false));
    return fusion_mplp_collect(ctx, what, {x, sweeps_run, passes_run, energy, bound, energies, bounds});
}

int msm_cost_prefetch_stats(msm_cost *c, int64_t *taken, int64_t *dropped) {
    if (!c) return fail(MSM_ERR_INVALID, "null cost");
    if (taken) *taken = c->prefetch_hits;
    if (dropped) *dropped = c->prefetch_drops;
    return MSM_OK;
}

}  // extern "C"
