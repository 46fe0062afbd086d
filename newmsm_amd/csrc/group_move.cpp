// group_move.cpp -- a label step of the groupwise path: its kernels, the order they run in, and the delivery of their results.
#include "group_internal.hpp"

namespace msm {
// The patch entries' values beside their ids and the patch directory (GroupArgs::pval / dir) for the label steps of the pairs [pair0, pair1): the whole list
// writes every patch (3.2 GB at S = 64, ico6 / ico4: 2.3 ms), a rank's slice only the patches of the nodes its pairs touch.
int ensure_patch_values(msm_group *g, int64_t pair0, int64_t pair1) {
    if (g->pval_ready && g->pval_p0 <= pair0 && g->pval_p1 >= pair1) return MSM_OK;
    msm_ctx *ctx = g->ctx;
    const bool ready_before = g->pval_ready;
    g->pval_ready = false;
    GroupArgs a;
    int st = group_args(g, a);
    if (st) return st;
    const bool all = pair0 == 0 && pair1 == g->npairs;
    if (!all) {
        MSM_HIP(g->d_node_flags.zero((size_t)g->S * g->N, ctx->stream));
        st = launch_group_mark_nodes(ctx, g->d_pairs.p, pair0, pair1, g->d_node_flags.p);
        if (st) return st;
    }
    st = launch_group_patch_values(ctx, a, g->d_pvalp.p, all ? nullptr : g->d_node_flags.p);
    if (!st && !ready_before) st = launch_group_patch_dir(ctx, a, g->d_pvalp.p, g->d_patch_dir.p);  // (every patch's record: it does not depend on the slice)
    if (!st) st = ctx_sync(ctx);
    if (st) return st;
    g->pval_ready = true;
    g->pval_p0 = pair0, g->pval_p1 = pair1;
    return MSM_OK;
}
}  // namespace msm

// the slice [pair0, pair1) of the pair list in processing order, on the device.  The order is cut into pieces by output range
// (a quarter of the slice each, for slices worth overlapping): within a piece the pairs run control point by control point, and a
// piece's results are one contiguous range of the output, which can leave for the host while the next piece is computed.
static int slice_pair_order(msm_group *g, int64_t pair0, int64_t pair1, const int **d_order) {
    if (g->order_p0 != pair0 || g->order_p1 != pair1) {
        msm_ctx *ctx = g->ctx;
        MSM_TRY(ctx_sync(ctx));
        const int64_t n = pair1 - pair0;
        const int pieces = n >= (1 << 18) ? 4 : 1;
        // pieces shrink geometrically (ratio 0.5): a piece's results leave for the host while the next piece is
        // computed, so only the LAST piece's copy is not hidden behind kernels -- a fifteenth of the step's results instead of a quarter (S = 64,
        // ico6 / ico4: 9.0 -> 8.4 ms per delivered step; an eighth of a step, as a rank of eight evaluates it: 1.62 -> 1.52 ms)
        constexpr double ratio = 0.5;
        g->order_chunk.assign(pieces + 1, 0);
        {
            double total = 0.0, w = 1.0, acc = 0.0;
            for (int k = 0; k < pieces; ++k, w *= ratio) total += w;
            w = 1.0;
            for (int k = 1; k < pieces; ++k, w *= ratio) {
                acc += w;
                g->order_chunk[k] = std::min<int64_t>(n, std::max<int64_t>(g->order_chunk[k - 1], (int64_t)((double)n * acc / total)));
            }
            g->order_chunk[pieces] = n;
        }
        std::vector<std::vector<int32_t>> part(pieces);
        for (auto &v : part) v.reserve((size_t)(n / pieces + 1));
        for (int32_t p : g->pair_order) {
            if (p < pair0 || p >= pair1) continue;
            int k = (int)((int64_t)(p - pair0) * pieces / std::max<int64_t>(n, 1));
            while (k + 1 < pieces && p - pair0 >= g->order_chunk[k + 1]) ++k;
            while (k > 0 && p - pair0 < g->order_chunk[k]) --k;
            part[k].push_back(p);
        }
        MSM_HIP(g->d_pair_order.ensure(std::max<size_t>((size_t)n, 1)));
        size_t at = 0;
        for (auto &v : part) {
            if (!v.empty()) MSM_TRY(stage_h2d(ctx, g->d_pair_order.p + at, v.data(), sizeof(int32_t) * v.size()));
            at += v.size();
        }
        MSM_TRY(ctx_sync(ctx));
        g->order_p0 = pair0, g->order_p1 = pair1;
        g->order4_gen = ~0ull;
    }
    if (g->order4_gen != g->pairs_gen) {  // the positions with their pairs' nodes, for this slice and this set-up's pair list
        const int64_t n = pair1 - pair0;
        MSM_HIP(g->d_pair_order4.ensure(std::max<size_t>((size_t)n, 1)));
        MSM_TRY(launch_group_expand_order(g->ctx, g->d_pair_order.p, g->d_pairs.p, (int)n, g->d_pair_order4.p));
        g->order4_gen = g->pairs_gen;
    }
    *d_order = g->d_pair_order.p;
    return MSM_OK;
}

// the evaluations of a (slice of a) label step, queued on the stream; results in device memory
// after_piece(k, lo, hi): the kernels of piece k (pairs [pair0 + lo, pair0 + hi) of the output) have been queued; k = -1: the triplets
static int group_move_compute_untimed(msm_group *g, const int32_t *labeling, int32_t label, int64_t pair0, int64_t pair1, int64_t trip0, int64_t trip1,
                              double *quads_dev, double *octets_dev, const char *who, const std::function<int(int, int64_t, int64_t)> *after_piece = nullptr) {
    GroupArgs a;
    int st = group_args(g, a);
    if (!st && pair1 > pair0) st = pair_refusal(g);
    if (st) return st;
    const int nodes = g->S * g->N;
    if (label < 0 || label >= g->L) return fail(MSM_ERR_INVALID, "%s: label %d out of range", who, label);
    for (int i = 0; i < nodes; ++i)
        if (labeling[i] < 0 || labeling[i] >= g->L) return fail(MSM_ERR_INVALID, "%s: label of node %d out of range", who, i);
    msm_ctx *ctx = g->ctx;
    void *pin = nullptr;
    st = ctx_io_pinned(ctx, sizeof(int32_t) * (size_t)nodes, &pin);
    if (st) return st;
    MSM_TRY(ctx_sync(ctx));  // the staging buffer may still be the source of an earlier copy
    std::memcpy(pin, labeling, sizeof(int32_t) * (size_t)nodes);
    MSM_HIP(g->d_query[0].ensure(nodes));
    MSM_HIP(hipMemcpyAsync(g->d_query[0].p, pin, sizeof(int32_t) * (size_t)nodes, hipMemcpyHostToDevice, ctx->stream));
    a.move_labeling = g->d_query[0].p;
    a.move_label = label;
    // Large steps evaluate the triplets (the cheap part: strain only) FIRST, so that their results leave for the host behind the pair kernels
    // instead of after them (S = 64 at ico4: 13.1 -> 12.8 ms per step).  Small steps keep them last: at ico2 (0.3 M pairs, 0.9 ms per step) the
    // early copy command cost 0.85 ms per step, measured both ways in the same run.
    const bool triplets_last = pair1 - pair0 < (1 << 20);
    auto triplets = [&]() -> int {
        a.move_order = nullptr;
        const int64_t first = 8 * trip0, total = 8 * (trip1 - trip0);
        for (int64_t off = 0; off < total; off += kBatchChunk) {
            const int m = (int)std::min<int64_t>(kBatchChunk, total - off);
            if (first + off > 0x7fffffffll - kBatchChunk) return fail(MSM_ERR_CAPACITY, "%s: evaluation index beyond 2^31", who);
            a.move_offset = (int)(first + off);
            st = launch_group_triplet(ctx, a, nullptr, nullptr, nullptr, nullptr, m, octets_dev + off);
            if (st) return st;
        }
        if (after_piece && total > 0) {
            st = (*after_piece)(-1, 0, 0);
            if (st) return st;
        }
        return MSM_OK;
    };
    if (!triplets_last) {
        st = triplets();
        if (st) return st;
    }
    if (pair1 > pair0) {
        st = slice_pair_order(g, pair0, pair1, &a.move_order);
        if (st) return st;
        a.move_order4 = g->d_pair_order4.p;
        if (g->pval_deferred || g->pval_ready) {  // the value copies of this slice's patches (a rank of a sharded run builds them here, once per set-up and slice)
            st = ensure_patch_values(g, pair0, pair1);
            if (st) return st;
            a.pval = const_cast<const double *const *>(g->d_pvalp.p);
            a.dir = g->d_patch_dir.p;
        }
        a.move_base = (int)pair0;
        // The (current, current) combination of a pair does not depend on the proposed label: it is evaluated in a pass of its own
        // (whole wavefronts of pairs whose two nodes kept their labels since the last step leave at once with the kept cost), the
        // three combinations with the proposed label in a second pass.  DICE: all four together, nothing kept.
        const bool two_pass = g->p.simmeasure != 4 && g->p.simmeasure != 5;
        if (two_pass) {
            const int64_t P = g->npairs;
            MSM_HIP(g->d_e00.ensure((size_t)std::max<int64_t>(P, 1)));
            MSM_HIP(g->d_prev_labeling.ensure(nodes));
            a.move_e00 = g->d_e00.p;
            a.move_prev = (g->e00_valid && g->e00_p0 == pair0 && g->e00_p1 == pair1) ? g->d_prev_labeling.p : nullptr;
            g->e00_valid = false;  // until this step has gone through: a failure half way leaves nothing to rely on
        }
        // The (proposed, proposed) combination depends on the label alone: the second sweep of Fusion over the labels (I/Fusion/Fusion.h:136-138)
        // takes it from the first (kept per label for this slice until the next set-up; 8 bytes x pairs x labels: 0.8 GB for 64 subjects at
        // ico4).  A slice whose table would pass kE11CapMB: evaluated every time.
        constexpr double kE11CapMB = 16384.0;
        const int64_t nslice = pair1 - pair0;
        bool have11 = false;
        if (two_pass && 8.0 * (double)nslice * g->L <= kE11CapMB * 1048576.0) {
            if (g->e11_p0 != pair0 || g->e11_p1 != pair1 || (int)g->e11_have.size() != g->L) {
                g->e11_have.assign((size_t)g->L, 0);
                g->e11_p0 = pair0, g->e11_p1 = pair1;
            }
            MSM_HIP(g->d_e11.ensure((size_t)nslice * g->L));
            a.move_e11 = g->d_e11.p + (size_t)label * nslice;
            have11 = g->e11_have[(size_t)label] != 0;
            g->e11_have[(size_t)label] = 0;  // until this step has gone through
        }
        for (size_t k = 0; k + 1 < g->order_chunk.size(); ++k) {
            const int64_t n0 = g->order_chunk[k], n1 = g->order_chunk[k + 1];  // pairs of the piece, in processing order
            if (have11) {
                st = launch_group_kept(ctx, a.move_order + n0, (int)pair0, a.move_e11, (int)(n1 - n0), quads_dev);
                if (st) return st;
            }
            a.move_first = (int)n0, a.move_count = (int)(n1 - n0);
            for (int pass = two_pass ? 1 : 0; pass <= (two_pass ? 2 : 0); ++pass) {
                const int64_t mult = pass == 0 ? 4 : (pass == 1 ? 1 : (have11 ? 2 : 3)), q0 = mult * n0, q1 = mult * n1;
                a.move_combos = pass == 2 && have11 ? 3 : pass;
                for (int64_t off = q0; off < q1; off += kBatchChunk) {
                    const int m = (int)std::min<int64_t>(kBatchChunk, q1 - off);
                    if (off > 0x7fffffffll - kBatchChunk) return fail(MSM_ERR_CAPACITY, "%s: evaluation index beyond 2^31", who);
                    a.move_offset = (int)off;
                    st = launch_group_pairwise(ctx, a, nullptr, nullptr, nullptr, m, quads_dev);
                    if (st) return st;
                }
            }
            if (after_piece) {
                st = (*after_piece)((int)k, n0, n1);
                if (st) return st;
            }
        }
        if (two_pass) {  // what the next step compares with
            MSM_HIP(hipMemcpyAsync(g->d_prev_labeling.p, g->d_query[0].p, sizeof(int32_t) * (size_t)nodes, hipMemcpyDeviceToDevice, ctx->stream));
            g->e00_valid = true;
            g->e00_p0 = pair0, g->e00_p1 = pair1;
        }
        if (a.move_e11) g->e11_have[(size_t)label] = 1;
        a.move_combos = 0;
        a.move_first = a.move_count = 0;
        a.move_prev = nullptr;
        a.move_e00 = nullptr;
        a.move_e11 = nullptr;
    }
    return triplets_last ? triplets() : MSM_OK;
}

// the same between two events when the caller asked for the kernels' time (msm_group_time_moves; bench.py's gmsm roofline)
static int group_move_compute(msm_group *g, const int32_t *labeling, int32_t label, int64_t pair0, int64_t pair1, int64_t trip0, int64_t trip1,
                              double *quads_dev, double *octets_dev, const char *who, const std::function<int(int, int64_t, int64_t)> *after_piece = nullptr) {
    if (!g->timing) return group_move_compute_untimed(g, labeling, label, pair0, pair1, trip0, trip1, quads_dev, octets_dev, who, after_piece);
    MSM_HIP(hipEventRecord(g->t_ev0, g->ctx->stream));
    const int st = group_move_compute_untimed(g, labeling, label, pair0, pair1, trip0, trip1, quads_dev, octets_dev, who, after_piece);
    if (st) return st;
    MSM_HIP(hipEventRecord(g->t_ev1, g->ctx->stream));
    g->timed = true;
    return MSM_OK;
}

// the copy stream and its events (one per piece + one for the triplets)
static int ensure_copy_stream(msm_group *g) {
    if (!g->copy_stream) MSM_HIP(hipStreamCreateWithFlags(&g->copy_stream, hipStreamNonBlocking));
    while (g->copy_events.size() < 8) {
        hipEvent_t e;
        MSM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        g->copy_events.push_back(e);
    }
    return MSM_OK;
}
// finished results leave for pinned host memory on the copy stream while the compute stream goes on
static int copy_behind(msm_group *g, int slot, double *host_dst, const double *dev_src, size_t n) {
    msm_ctx *ctx = g->ctx;
    hipEvent_t e = g->copy_events[(size_t)slot % g->copy_events.size()];
    MSM_HIP(hipEventRecord(e, ctx->stream));
    MSM_HIP(hipStreamWaitEvent(g->copy_stream, e, 0));
    MSM_HIP(hipMemcpyAsync(host_dst, dev_src, sizeof(double) * n, hipMemcpyDeviceToHost, g->copy_stream));
    return MSM_OK;
}

// One label step from its kernels to its status: the evaluations into cq / ct (device memory), and each finished piece handed to the copy stream for
// host_q / host_t (pinned host memory at the position of cq / ct; null: the results stay on the device).
// The kept (current, current) and (label, label) pair costs are marked valid when their kernels are queued; a step that then fails -- a status
// raised by a kernel (e.g. MSM_ERR_CAPACITY), a failed copy -- must not leave them behind for later steps to deliver: every failure here drops
// everything kept.  And however the step ends, the copy engine has finished with the caller's arrays when this returns.
static int group_move_run(msm_group *g, const int32_t *labeling, int32_t label, int64_t pair0, int64_t pair1, int64_t trip0, int64_t trip1, double *cq, double *ct,
                          double *host_q, double *host_t, const char *who) {
    const bool copies = host_q || host_t;
    struct Guard {
        msm_group *g;
        bool done = false;
        ~Guard() {
            if (done) return;
            if (g->copy_stream) (void)hipStreamSynchronize(g->copy_stream);
            g->drop_kept();
        }
    } guard{g};
    int st = copies ? ensure_copy_stream(g) : MSM_OK;
    if (st) return st;
    const std::function<int(int, int64_t, int64_t)> deliver = [&](int k, int64_t lo, int64_t hi) -> int {
        if (k < 0) return host_t ? copy_behind(g, 7, host_t, ct, 8 * (size_t)(trip1 - trip0)) : MSM_OK;
        return host_q ? copy_behind(g, k, host_q + 4 * lo, cq + 4 * lo, 4 * (size_t)(hi - lo)) : MSM_OK;
    };
    st = group_move_compute(g, labeling, label, pair0, pair1, trip0, trip1, cq, ct, who, copies ? &deliver : nullptr);
    if (st) return st;
    st = check_status(g->ctx, "DiscreteGroupCostFunction (fusion move)");  // synchronises: device buffers may go into a collective on another stream
    if (copies) MSM_HIP(hipStreamSynchronize(g->copy_stream));
    if (st) return st;
    guard.done = true;
    return MSM_OK;
}

// A slice of a label step with the results left in DEVICE memory (the caller's buffers, e.g. torch tensors that go into an
// RCCL gather, or the device address of mapped host memory): pairs [pair0, pair1) -> quads_dev[4 * (pair1 - pair0)],
// triplets [trip0, trip1) -> octets_dev[8 * (trip1 - trip0)].
static int group_fusion_move_dev_impl(msm_group *g, const int32_t *labeling, int32_t label, int64_t pair0, int64_t pair1, int64_t trip0, int64_t trip1,
                                      double *quads_dev, double *octets_dev, const char *who) {
    if (!g || !labeling) return fail(MSM_ERR_INVALID, "%s: null argument", who);
    if (!g->ready) return fail(MSM_ERR_STATE, "msm_group: msm_group_setup() must be called first");
    const int64_t P = g->npairs, T = (int64_t)g->S * g->Tc;
    if (pair0 < 0 || pair1 < pair0 || pair1 > P || trip0 < 0 || trip1 < trip0 || trip1 > T) return fail(MSM_ERR_INVALID, "%s: range out of bounds", who);
    if ((pair1 > pair0 && !quads_dev) || (trip1 > trip0 && !octets_dev)) return fail(MSM_ERR_INVALID, "%s: missing output buffer", who);
    // an output inside a msm_host_alloc / msm_host_register block (pinned host memory, possibly shared with other processes): the kernels' scattered
    // 8-byte results are gathered in HBM first, and the results of each piece of the pair list (and of the triplets) are copied out by the DMA engine
    // while the kernels of the next piece run -- 186 MB at S = 64, 3.7 ms that used to follow the kernels
    msm_ctx *ctx = g->ctx;
    const size_t nq = (size_t)(4 * (pair1 - pair0)), nt = (size_t)(8 * (trip1 - trip0));
    const bool host_q = nq && ctx_mapped(ctx, quads_dev, sizeof(double) * nq), host_t = nt && ctx_mapped(ctx, octets_dev, sizeof(double) * nt);
    double *cq = quads_dev, *ct = octets_dev;
    if (host_q || host_t) {
        MSM_HIP(g->d_move_out.ensure(nq + nt + 2));
        if (host_q) cq = g->d_move_out.p;
        if (host_t) ct = g->d_move_out.p + ((nq + 1) & ~(size_t)1);  // both 16-byte aligned
    }
    return group_move_run(g, labeling, label, pair0, pair1, trip0, trip1, cq, ct, host_q ? quads_dev : nullptr, host_t ? octets_dev : nullptr, who);
}

extern "C" {

int msm_group_fusion_move_dev(msm_group *g, const int32_t *labeling, int32_t label, int64_t pair0, int64_t pair1, int64_t trip0, int64_t trip1,
                              double *quads_dev, double *octets_dev) {
    return group_fusion_move_dev_impl(g, labeling, label, pair0, pair1, trip0, trip1, quads_dev, octets_dev, "msm_group_fusion_move_dev");
}

int msm_group_fusion_move(msm_group *g, const int32_t *labeling, int32_t label, double *pair_quads, double *triplet_octets) {
    const char *who = "msm_group_fusion_move";
    if (!g || !labeling) return fail(MSM_ERR_INVALID, "%s: null argument", who);
    if (!g->ready) return fail(MSM_ERR_STATE, "msm_group: msm_group_setup() must be called first");
    msm_ctx *ctx = g->ctx;
    const int64_t P = pair_quads ? g->npairs : 0, T = triplet_octets ? (int64_t)g->S * g->Tc : 0;
    // both arrays in msm_host_alloc / msm_host_register blocks: the device entry point's step over the whole lists
    if ((P == 0 || ctx_mapped(ctx, pair_quads, sizeof(double) * 4 * (size_t)P)) && (T == 0 || ctx_mapped(ctx, triplet_octets, sizeof(double) * 8 * (size_t)T)))
        return group_fusion_move_dev_impl(g, labeling, label, 0, P, 0, T, pair_quads, triplet_octets, who);
    MSM_HIP(g->d_move_out.ensure((size_t)(4 * P + 8 * T) + 2));
    double *dq = g->d_move_out.p, *dt = dq + ((4 * P + 1) & ~1ll);  // both 16-byte aligned
    int st = group_move_run(g, labeling, label, 0, P, 0, T, dq, dt, nullptr, nullptr, who);
    if (st) return st;
    // delivery: arrays inside a msm_host_alloc / msm_host_register block are written by a copy kernel (full-width stores over
    // PCIe, no staging); others go through the pinned staging buffer in chunks
    bool flagged = false;
    for (int pass = 0; pass < 2; ++pass) {
        double *out = pass == 0 ? pair_quads : triplet_octets;
        const double *src = pass == 0 ? dq : dt;
        const size_t total = (size_t)(pass == 0 ? 4 * P : 8 * T);
        if (!out || total == 0) continue;
        double *mapped = static_cast<double *>(ctx_mapped(ctx, out, sizeof(double) * total));
        if (mapped && reinterpret_cast<uintptr_t>(mapped) % 16 == 0) {
            st = ctx_flag(ctx);
            if (st) return st;
            st = launch_copy_to_mapped(ctx, src, mapped, total, ctx->d_flag_map);
            if (st) return st;
            flagged = true;
            continue;
        }
        for (size_t off = 0; off < total; off += kBatchChunk) {
            const size_t m = std::min<size_t>(kBatchChunk, total - off);
            void *pin = nullptr;
            st = ctx_io_pinned(ctx, sizeof(double) * m, &pin);
            if (st) return st;
            MSM_HIP(hipMemcpyAsync(pin, src + off, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
            MSM_TRY(ctx_sync(ctx));
            std::memcpy(out + off, pin, sizeof(double) * m);
        }
    }
    st = check_status(ctx, "DiscreteGroupCostFunction (fusion move)");
    if (flagged) ctx->h_flag[0] = 0;
    return st;
}

int msm_group_time_moves(msm_group *g, int enable) {
    if (!g) return fail(MSM_ERR_INVALID, "null group");
    (void)hipSetDevice(g->ctx->device);
    if (enable && !g->t_ev0) {
        MSM_HIP(hipEventCreate(&g->t_ev0));
        MSM_HIP(hipEventCreate(&g->t_ev1));
    }
    g->timing = enable != 0;
    g->timed = false;
    return MSM_OK;
}

int msm_group_move_kernels_ms(msm_group *g, double *ms) {
    if (!g || !ms) return fail(MSM_ERR_INVALID, "msm_group_move_kernels_ms: null argument");
    *ms = -1.0;
    if (!g->timed) return MSM_OK;
    MSM_HIP(hipEventSynchronize(g->t_ev1));
    float f = 0.f;
    MSM_HIP(hipEventElapsedTime(&f, g->t_ev0, g->t_ev1));
    *ms = f;
    return MSM_OK;
}

}  // extern "C"
