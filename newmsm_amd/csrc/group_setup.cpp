// group_setup.cpp -- the set-up of a group: what is common to all subjects, and the pipelines that give a subject its resampled maps and patch lists.
#include "group_internal.hpp"

namespace {

inline V3 pt(const double *xyz, int V, int i) { return mk(xyz[i], xyz[V + i], xyz[2 * V + i]); }

// patch lists of one subject: template vertices within range*spacing of each rotated control point
// (get_patch_data, M/DiscreteGroupModel.cpp:109-117), via the range kernel + host tie resolution (see k_range)
// deferred: work queued on the stream before this call whose status has not been looked at yet (stage_batch) -- named in the error should it have failed;
// the first synchronisation here covers it
int subject_patches(msm_group *g, int s, msm_ctx *ctx, msm_group::Pipe *pipe, const char *deferred) {  // ctx: the context (stream) to work on, pipe: whose scratch
    const int N = g->N, L = g->L, M = N * L, Vt = g->tmpl->V;
    const bool timing = std::getenv("MSMHIP_TIMING") != nullptr;
    auto tick = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "      patches: %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(now - tick).count());
        tick = now;
    };
    DevBuf<double> &d_c = pipe->d_centres, &d_sep = pipe->d_sep;
    DevBuf<uint32_t> &d_slots = pipe->d_slots;
    DevBuf<int> &d_counts = pipe->d_counts;
    MSM_HIP(d_c.ensure(3 * (size_t)M));
    MSM_HIP(d_sep.ensure(M));
    {
        int st = launch_group_centres(ctx, g->d_moved.p + 3 * (size_t)s * M, g->d_spacing.p + (size_t)s * N, N, L, d_c.p, d_sep.p);
        if (st) return st;
    }
    MSM_HIP(d_counts.ensure((size_t)M + 1));  // + the number of undecided entries
    MSM_HIP(pipe->d_chunkb.ensure((size_t)(Vt + 63) / 64 + 1));
    int cap = std::max(256, g->patch_cap_hint.load());  // the previous call's largest patch: one k_range pass instead of two
    std::vector<int> counts((size_t)M + 1);
    auto first_sync = [&]() -> int {
        if (!deferred) return ctx_sync(ctx);
        const char *what = deferred;
        deferred = nullptr;
        return check_status(ctx, what);
    };
    // Round 5: from a set-up's second subject on the row offsets are summed and the list compacted on the device BEFORE the host has seen the counts (the list
    // sized from the longest one so far, the kernel guarded), so that a subject's batch stream synchronises once -- it was three round trips (after the
    // resampling, after the counts, after the compaction), each followed by launches onto an idle stream: a quarter of the stream's time was gaps.
    const size_t list_hint = g->pidx_hint.load();
    bool early = false;
    for (int attempt = 0; attempt < 3; ++attempt) {
        MSM_HIP(d_slots.ensure((size_t)M * cap));
        int st = launch_range(ctx, d_c.p, M, g->tmpl->d_xyz.p, Vt, d_sep.p, g->p.range, cap, d_slots.p, d_counts.p, pipe->d_chunkb.p, d_counts.p + M, L,
                              g->rgrid_valid ? &g->rgrid : nullptr);
        if (st) return st;
        early = attempt == 0 && list_hint > 0;
        if (early) {
            MSM_HIP(g->pptr[s]->ensure((size_t)M + 1));
            MSM_HIP(pipe->d_scan_tmp.ensure((size_t)M / 4096 + 2));
            MSM_HIP(g->pidx[s]->ensure(list_hint + list_hint / 8 + 1024));
            MSM_HIP(hipMemcpyAsync(g->pptr[s]->p, d_counts.p, sizeof(int) * (size_t)M, hipMemcpyDeviceToDevice, ctx->stream));
            st = launch_scan_exclusive(ctx, g->pptr[s]->p, M, pipe->d_scan_tmp.p);
            if (st) return st;
            st = launch_patch_compact(ctx, d_slots.p, cap, g->pptr[s]->p, M, g->pidx[s]->p, g->pidx[s]->cap);
            if (st) return st;
        }
        MSM_TRY(d_counts.download(counts.data(), (size_t)M + 1, ctx));
        MSM_TRY(first_sync());
        const int mx = *std::max_element(counts.begin(), counts.begin() + M);
        if (mx + 16 > g->patch_cap_hint.load()) g->patch_cap_hint.store(mx + 16);
        if (mx <= cap) break;
        if (attempt == 2) return fail(MSM_ERR_CAPACITY, "group patch capacity");
        cap = mx + 16;
        early = false;
    }
    lap("range kernel");
    if (counts[M] == 0) {
        // nothing sits on the threshold: the rows are final.  The list is compacted where it is used; the host keeps the row
        // offsets and fetches the 12.7 MB of indices only if msm_group_patch / msm_group_export_subject ask for them.
        auto &pp = g->h_pptr[s];
        pp.assign((size_t)M + 1, 0);
        for (int k = 0; k < M; ++k) pp[k + 1] = pp[k] + counts[k];
        g->h_pidx[s].clear();
        g->patch_stat[s] = patch_stat_of(pp.data(), (size_t)M);
        if ((size_t)pp[M] > g->pidx_hint.load()) g->pidx_hint.store((size_t)pp[M]);
        if (early && (size_t)pp[M] < g->pidx[s]->cap) {  // (the list and its padding element fit the hinted allocation)
            lap("lists (device, no second look)");
            return MSM_OK;
        }
        MSM_TRY(g->pptr[s]->upload(pp.data(), pp.size(), ctx));
        MSM_HIP(ensure_patch_entries(*g->pidx[s], (size_t)pp[M]));
        int st = launch_patch_compact(ctx, d_slots.p, cap, g->pptr[s]->p, M, g->pidx[s]->p);
        if (st) return st;
        MSM_TRY(ctx_sync(ctx));
        lap("lists (device)");
        return MSM_OK;
    }
    // 50 MB at ico6 / 19 labels: through pinned memory (a pageable copy of this size took most of this function's time)
    void *pin = nullptr;
    {
        int st = ctx_io_pinned(ctx, sizeof(uint32_t) * (size_t)M * cap, &pin);
        if (st) return st;
    }
    const uint32_t *slots = static_cast<const uint32_t *>(pin);
    MSM_HIP(hipMemcpyAsync(pin, d_slots.p, sizeof(uint32_t) * (size_t)M * cap, hipMemcpyDeviceToHost, ctx->stream));
    MSM_TRY(ctx_sync(ctx));
    lap("slots to the host");
    auto &pp = g->h_pptr[s];
    auto &pi = g->h_pidx[s];
    pp.assign(M + 1, 0);
    const double *tx = g->tmpl->xyz.data();
    // the centres and spacings the kernel used, for the host's decisions (this branch is rare: exact ties)
    std::vector<double> centres(3 * (size_t)M), sep(M);
    MSM_TRY(d_c.download(centres.data(), centres.size(), ctx));
    MSM_TRY(d_sep.download(sep.data(), sep.size(), ctx));
    MSM_TRY(ctx_sync(ctx));
    // an entry flagged by the kernel sits within 1e-11 of the threshold: decided with the host libm, as the reference does
    auto keeps = [&](int k, uint32_t e) {
        if (!(e & 0x80000000u)) return true;
        const V3 c = mk(centres[k], centres[M + k], centres[2 * (size_t)M + k]);
        const double arc = chord_to_arc(norm(sub(c, pt(tx, Vt, (int)(e & 0x7fffffffu)))));
        return arc < g->p.range * sep[k];
    };
    const int workers = host_workers();
    parallel_chunks(M, workers, [&](int, int k0, int k1) {  // rows are independent: count, then (below) fill at the prefix sums
        for (int k = k0; k < k1; ++k) {
            int n = 0;
            for (int j = 0; j < counts[k]; ++j) n += keeps(k, slots[(size_t)k * cap + j]) ? 1 : 0;
            pp[k + 1] = n;
        }
    });
    for (int k = 0; k < M; ++k) pp[k + 1] += pp[k];
    pi.resize((size_t)pp[M]);
    parallel_chunks(M, workers, [&](int, int k0, int k1) {
        for (int k = k0; k < k1; ++k) {
            int32_t *dst = pi.data() + pp[k];
            for (int j = 0; j < counts[k]; ++j) {
                const uint32_t e = slots[(size_t)k * cap + j];
                if (keeps(k, e)) *dst++ = (int32_t)(e & 0x7fffffffu);
            }
        }
    });
    lap("lists");
    g->patch_stat[s] = patch_stat_of(pp.data(), (size_t)M);
    MSM_TRY(g->pptr[s]->upload(pp.data(), pp.size(), ctx));
    MSM_HIP(ensure_patch_entries(*g->pidx[s], pi.size()));
    {
        int st = upload_staged(ctx, g->pidx[s]->p, pi.data(), pi.size() * sizeof(int32_t));  // 12.7 MB at ico6 / 19 labels
        if (st) return st;
    }
    MSM_TRY(ctx_sync(ctx));
    lap("uploads");
    return MSM_OK;
}

// estimate_pairs, spacings, rotations: cheap, needs every subject's control grid, identical on every rank
int group_common_setup(msm_group *g) {
    if (!g->tmpl || g->N <= 0 || g->L <= 0) return fail(MSM_ERR_STATE, "msm_group: template, control grid and labels must be set first");
    msm_ctx *ctx = g->ctx;
    const int S = g->S, N = g->N, L = g->L;
    const double centre[3] = {g->labels[0], g->labels[L], g->labels[2 * (size_t)L]};
    const bool timing = std::getenv("MSMHIP_TIMING") != nullptr;
    auto tick = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "  group set-up, common: %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(now - tick).count());
        tick = now;
    };
    // estimate_pairs, M/DiscreteGroupModel.cpp:37-55: closest control point of subject B for every control point of A.  The S
    // control grids share their triangle list, so their search trees are built together as a forest and one kernel writes the
    // whole list (N S (S - 1) / 2 pairs: 5.2 M at S = 64) where the cost kernels read it.  Round 1 / the first half of round 2:
    // S - 1 search calls with host trees and host loops, 67 ms at S = 64 on every rank.
    // get_spacings :123-139 and get_rotations :77-86 on the host (their asin / acos decide patch membership to the last bit, so they use the host's libm as
    // the reference does), subjects spread over the host threads -- started here, beside the GPU's estimate_pairs below (round 5: they used to follow it,
    // 2 ms that every rank of a sharded run repeats)
    g->rot.resize(9 * (size_t)S * N);
    g->moved.clear();
    g->moved_on_host = false;
    std::vector<double> cp_all(3 * (size_t)S * N), orig_all(3 * (size_t)S * N, 0.0), spacing_all((size_t)S * N);
    std::vector<int> sub_status(S, MSM_OK);
    std::thread host_side([&] {
        parallel_for(S, host_workers(), [&](int s) {
            msm_mesh *cm = g->cpmesh[s];
            g->spacing[s].resize(N);
            double mvd;
            int st = msm_cp_spacings(cm->xyz.data(), cm->tri.data(), N, g->Tc, g->spacing[s].data(), &mvd);
            if (!st) st = msm_cp_rotations(centre, cm->xyz.data(), N, &g->rot[9 * (size_t)s * N]);
            sub_status[s] = st;
            std::copy(g->spacing[s].begin(), g->spacing[s].end(), spacing_all.begin() + (size_t)s * N);
            std::copy(cm->xyz.begin(), cm->xyz.end(), cp_all.begin() + 3 * (size_t)s * N);
            if (g->have_orig[s]) std::copy(g->orig[s].begin(), g->orig[s].end(), orig_all.begin() + 3 * (size_t)s * N);
        });
    });
    struct Joiner {  // every return below leaves with the thread joined
        std::thread &t;
        ~Joiner() {
            if (t.joinable()) t.join();
        }
    } joiner{host_side};
    g->npairs = (int64_t)N * S * (S - 1) / 2;
    g->pairs.clear();
    ++g->pairs_gen;
    std::vector<double> cp_soa(3 * (size_t)S * N);
    for (int s = 0; s < S; ++s)
        for (int ax = 0; ax < 3; ++ax)
            std::copy(g->cpmesh[s]->xyz.begin() + (size_t)ax * N, g->cpmesh[s]->xyz.begin() + (size_t)(ax + 1) * N, cp_soa.begin() + (size_t)ax * S * N + (size_t)s * N);
    MSM_HIP(g->d_cp_soa.ensure(cp_soa.size()));
    {
        int st = upload_staged(ctx, g->d_cp_soa.p, cp_soa.data(), sizeof(double) * cp_soa.size());
        if (st) return st;
    }
    MSM_HIP(g->d_pairs.ensure(std::max<size_t>(2 * (size_t)g->npairs, 1)));
    bool pairs_done = false;
    if (S >= 2) {
        int st = gpu_build_forest(ctx, g->cp_forest, g->d_cp_soa.p, (size_t)S * N, (size_t)N, N, g->cpmesh[0]->d_tri.p, g->Tc, S);
        if (st == MSM_OK) {
            std::vector<int2> info(S);
            for (int b = 0; b < S; ++b) info[b] = make_int2(g->cp_forest.info[b].nnodes, g->cp_forest.info[b].grid_depth);
            MSM_TRY(g->d_forest_info.upload(info.data(), info.size(), ctx));
            ForestDev fd;
            fd.node = g->cp_forest.node.p, fd.parent = g->cp_forest.parent.p, fd.leaf_tri = g->cp_forest.leaf_tri.p, fd.grid = g->cp_forest.grid.p;
            fd.cone = g->cp_forest.cone.p, fd.rec = g->cp_forest.rec.p;
            fd.s_node = g->cp_forest.s_node, fd.s_leaf = g->cp_forest.s_leaf, fd.s_rec = g->cp_forest.s_rec, fd.s_grid = g->cp_forest.s_grid;
            fd.info = g->d_forest_info.p;
            st = launch_group_pairs(ctx, fd, g->d_cp_soa.p, S, N, g->d_pairs.p);
            if (st) return st;
            st = check_status(ctx, "estimate_pairs");  // synchronises (info is a local)
            if (st) return st;
            pairs_done = true;
        } else if (st != MSM_ERR_CAPACITY) {
            return st;
        }
    }
    if (!pairs_done && S >= 2) {  // a control grid whose tree outgrew the forest's arrays: one search per target subject, as before
        g->pairs.resize(2 * (size_t)g->npairs);
        std::vector<std::vector<int32_t>> closest((size_t)S * S);
        std::vector<double> q;
        std::vector<int32_t> found;
        for (int b = 1; b < S; ++b) {
            const size_t Mq = (size_t)b * N;
            q.resize(3 * Mq);
            for (int a = 0; a < b; ++a)
                for (int ax = 0; ax < 3; ++ax)
                    std::copy(g->cpmesh[a]->xyz.begin() + (size_t)ax * N, g->cpmesh[a]->xyz.begin() + (size_t)(ax + 1) * N, q.begin() + ax * Mq + (size_t)a * N);
            found.resize(Mq);
            int st = msm_closest_vertex(g->cpmesh[b], q.data(), (int32_t)Mq, found.data());
            if (st) return st;
            for (int a = 0; a < b; ++a) closest[(size_t)a * S + b].assign(found.begin() + (size_t)a * N, found.begin() + (size_t)(a + 1) * N);
        }
        size_t pair = 0;
        for (int a = 0; a < S; ++a)
            for (int v = 0; v < N; ++v)
                for (int b = a + 1; b < S; ++b) {
                    g->pairs[2 * pair] = a * N + v;
                    g->pairs[2 * pair + 1] = b * N + closest[(size_t)a * S + b][v];
                    ++pair;
                }
        MSM_TRY(g->d_pairs.upload_vec(g->pairs, ctx));
    }
    lap("estimate_pairs");
    {
        // Processing order of a label step's pairs.  The list above runs subject A, control point, subject B: neighbours in it
        // share A's patch, but consecutive control-point ids are not neighbours on the sphere and every pair pulls another
        // subject's patch in, so at S = 16 a step fetched 2.9 GB through an L2 hit rate of 69 %.  Processed control point by
        // control point along a space-filling curve -- all S (S - 1) / 2 subject pairs of one, then the next -- the patches of a
        // neighbourhood (S subjects x 2 labels x a few KB) stay in the L2 while every pair that needs them runs.  Results keep
        // the list's positions (GroupArgs::move_order).
        // The order only serves locality: any permutation is correct, and the control grids move little from one iteration to the
        // next, so the order of the first set-up with these sizes is kept (with it the slice on the device and its four pieces).
        if (g->pair_order.size() != (size_t)g->npairs || g->order_S != S || g->order_N != N) {
            const double *c0 = g->cpmesh[0]->xyz.data();
            auto spread = [](uint32_t v) {
                v &= 0x3ff;
                v = (v | (v << 16)) & 0x030000ff;
                v = (v | (v << 8)) & 0x0300f00f;
                v = (v | (v << 4)) & 0x030c30c3;
                v = (v | (v << 2)) & 0x09249249;
                return v;
            };
            std::vector<std::pair<uint32_t, int>> key(N);
            for (int v = 0; v < N; ++v) {
                uint32_t q[3];
                for (int ax = 0; ax < 3; ++ax) {
                    const double u = (c0[(size_t)ax * N + v] + kBounds) / (2 * kBounds);
                    q[ax] = (uint32_t)std::max(0.0, std::min(1023.0, u == u ? u * 1024.0 : 0.0));
                }
                key[v] = {spread(q[0]) << 2 | spread(q[1]) << 1 | spread(q[2]), v};
            }
            std::sort(key.begin(), key.end());
            std::vector<int64_t> base(S, 0);
            for (int a = 1; a < S; ++a) base[a] = base[a - 1] + (int64_t)N * (S - a);
            g->pair_order.resize((size_t)g->npairs);
            size_t at = 0;
            for (int i = 0; i < N; ++i) {
                const int v = key[i].second;
                for (int a = 0; a + 1 < S; ++a)
                    for (int b = a + 1; b < S; ++b) g->pair_order[at++] = (int32_t)(base[a] + (int64_t)v * (S - 1 - a) + (b - a - 1));
            }
            g->order_S = S, g->order_N = N;
            g->order_p0 = g->order_p1 = -1;
            if (g->pair_layout == 1) {  // the curve order becomes the list's own: kept on the device for every set-up's permutation, the processing order is the identity
                MSM_HIP(g->d_pair_perm.ensure(std::max<size_t>(g->pair_order.size(), 1)));
                int st = upload_staged(ctx, g->d_pair_perm.p, g->pair_order.data(), sizeof(int32_t) * g->pair_order.size());
                if (st) return st;
                MSM_TRY(ctx_sync(ctx));
                std::iota(g->pair_order.begin(), g->pair_order.end(), 0);
            }
        }
        if (g->pair_layout == 1 && g->npairs > 0) {
            MSM_HIP(g->d_pairs_tmp.ensure(2 * (size_t)g->npairs));
            std::swap(g->d_pairs.p, g->d_pairs_tmp.p);  // d_pairs_tmp: the list in the reference's order, as written above
            std::swap(g->d_pairs.cap, g->d_pairs_tmp.cap);
            std::swap(g->d_pairs.owned, g->d_pairs_tmp.owned);
            int st = launch_group_permute_pairs(ctx, g->d_pairs_tmp.p, g->d_pair_perm.p, (int)g->npairs, g->d_pairs.p);
            if (st) return st;
            if (!g->pairs.empty()) {  // the fallback above filled the host copy and queued its upload: in the other order now -- fetched again when asked for
                MSM_TRY(ctx_sync(ctx));  // (the upload reads the vector)
                g->pairs.clear();
            }
        }
    }
    lap("pair order");
    // ROT * label for every (node, label) -- 3.1 M products at S = 64, 75 MB -- on the device from the uploaded rotations (multiplications and additions
    // only, in the host's order: the same bits)
    host_side.join();
    for (int s = 0; s < S; ++s)
        if (sub_status[s]) return fail(sub_status[s], "msm_group: spacings / rotations of subject %d's control grid failed", s);
    MSM_HIP(g->d_rot.ensure(g->rot.size()));
    MSM_HIP(g->d_moved.ensure(3 * (size_t)S * N * L));
    {
        int st = upload_staged(ctx, g->d_rot.p, g->rot.data(), sizeof(double) * g->rot.size());
        if (st) return st;
    }
    // through the pinned staging block: asynchronous copies out of freshly allocated pageable vectors (these are locals) left a stall of 10-30 ms
    // behind them that the NEXT work on the stream paid for -- the first subject's rotations (tools/time_group_rank.py; DESIGN 5.4b has the same
    // finding for the mesh uploads)
    MSM_HIP(g->d_labels3.ensure(3 * (size_t)L));
    MSM_HIP(g->d_spacing.ensure(spacing_all.size()));
    MSM_HIP(g->d_cp.ensure(cp_all.size()));
    MSM_HIP(g->d_orig.ensure(orig_all.size()));
    {
        int st = upload_staged(ctx, g->d_labels3.p, g->labels.data(), sizeof(double) * 3 * (size_t)L);
        if (!st) st = upload_staged(ctx, g->d_spacing.p, spacing_all.data(), sizeof(double) * spacing_all.size());
        if (!st) st = upload_staged(ctx, g->d_cp.p, cp_all.data(), sizeof(double) * cp_all.size());
        if (!st) st = upload_staged(ctx, g->d_orig.p, orig_all.data(), sizeof(double) * orig_all.size());
        if (st) return st;
    }
    {
        int st = launch_group_moved(ctx, g->d_rot.p, S * N, g->d_labels3.p, L, g->d_moved.p);
        if (st) return st;
    }
    MSM_TRY(ctx_sync(ctx));
    g->F.resize((size_t)S * L);
    g->Fslab.resize(S);
    g->have_subject.assign(S, 0);
    g->common_ready = true;
    lap("spacings, rotations, uploads");
    return MSM_OK;
}

// get_patch_data of one subject with everything in HBM, in three stages (msm_group_setup_subjects runs them as a pipeline):
//   prepare   main stream: the L rotated copies of the data mesh side by side in one 3 x (L * V) array (x of label 0, x of label
//             1, ..., y of label 0, ...), the subject's features, the L trees built together as a forest; ends synchronised
//   batch     batch stream: queries, weight-list surgery (resample_kernels.hip) and the weighted sums into F[s][l] for all L labels
//             in every launch (stage_batch; stage_fallback label by label when the forest could not be built)
//   patches   batch stream: subject_patches
// the L rotated copies of subject s's data mesh into d_out (3 x (L * V)), on ctx's stream: one launch; with rotation_mode 1 the V rotation matrices are
// computed here on the host workers first (libm's acos / sincos: 0.15 us each) and uploaded (72 V bytes)
static int rotate_subject(msm_group *g, msm_mesh *dm, msm_ctx *ctx, std::vector<double> &rot9, DevBuf<double> &d_rot9, double *d_out) {
    const int L = g->L, V = dm->V;
    const double centre[3] = {g->labels[0], g->labels[L], g->labels[2 * (size_t)L]};
    const double *d_mats = nullptr;
    if (g->rotation_mode == 1) {
        MSM_TRY(refresh_host_xyz(dm, ctx));  // (through the pipeline's context, not the mesh's)
        rot9.resize(9 * (size_t)V);
        std::atomic<int> bad{0};
        const double *xyz = dm->xyz.data();
        parallel_chunks(V, host_workers(), [&](int, int v0, int v1) {
            for (int v = v0; v < v1; ++v)
                if (!rotation_matrix(mk(centre[0], centre[1], centre[2]), pt(xyz, V, v), rot9.data() + 9 * (size_t)v)) bad.store(1);
        });
        if (bad.load()) return fail(MSM_ERR_ROTATION, "rotation angle is greater than 90 degrees");
        MSM_HIP(d_rot9.ensure(rot9.size()));
        int st = upload_staged(ctx, d_rot9.p, rot9.data(), sizeof(double) * rot9.size());
        if (st) return st;
        d_mats = d_rot9.p;
    }
    return launch_rotate_to_labels(ctx, dm->d_xyz.p, V, centre, g->d_labels3.p, L, d_mats, d_out, (size_t)L * V);
}

static int stage_prepare(msm_group *g, int s, msm_group::Stage &b, msm_ctx *ctx) {
    if (!g->data[s]) return fail(MSM_ERR_STATE, "msm_group: subject %d has no data", s);
    const int L = g->L, D = g->D, Vt = g->tmpl->V;
    msm_mesh *dm = g->data[s];
    const int V = dm->V, T = dm->T;
    const size_t LV = (size_t)L * V;
    static const bool timing = std::getenv("MSMHIP_TIMING") != nullptr && std::getenv("MSMHIP_TIMING")[0] == '2';
    auto tick = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        (void)hipStreamSynchronize(ctx->stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "      prepare subject %d: %s %.2f ms\n", s, what, std::chrono::duration<double, std::milli>(now - tick).count());
        tick = now;
    };
    MSM_HIP(b.d_rot.ensure(3 * LV));
    MSM_HIP(b.d_feat.ensure((size_t)D * V));
    int st = upload_staged(ctx, b.d_feat.p, g->feat[s].data(), sizeof(double) * (size_t)D * V);  // (first: the host's copy into the staging block is not between two launches then)
    if (st) return st;
    lap("feature upload");
    st = rotate_subject(g, dm, ctx, b.rot9, b.d_rot9, b.d_rot.p);  // one launch for the L labels (round 4: L - 1 launches that each computed the matrices again, and 3 copies)
    if (st) return st;
    lap("rotations");
    st = subject_feature_slab(g, s, (size_t)D * Vt);
    if (st) return st;
    lap("slab");
    // the L trees, built together (one chain of launches per subject instead of one per label); a tree that outgrows its arrays
    // (a degenerate mesh) sends the subject down the per-label builds of stage_fallback
    st = gpu_build_forest(ctx, b.forest, b.d_rot.p, LV, (size_t)V, V, dm->d_tri.p, T, L);
    b.forest_ok = st != MSM_ERR_CAPACITY;
    if (st && b.forest_ok) return st;
    lap("forest");
    st = check_status(ctx, "get_patch_data (rotation)");  // synchronises: rotations, features and trees are where the batch stream will read them
    return st;
}

// The per-label remainder with all L labels in every launch (the trees came from the forest): forward queries of the template's
// vertices in every tree, reverse queries of all rotated vertices in the template's tree (one launch over the L * V points of
// d_rot), vertex areas, weight-list surgery and the weighted sums into the subject's slab -- some forty launches per SUBJECT
// instead of thirty per label.  On a stream of its own (batch.ctx), beside the main stream's work on the next subject.
static int stage_batch(msm_group *g, int s, msm_group::Stage &b, int which, msm_group::Batch &w, bool defer_status = false) {
    if (!w.ctx) {
        w.ctx = msm_ctx_create(g->ctx->device);
        if (!w.ctx) return MSM_ERR_HIP;
    }
    msm_ctx *ctx = w.ctx;  // (created by group_setup_pipeline)
    const int L = g->L, D = g->D;
    msm_mesh *dm = g->data[s], *tm = g->tmpl;
    const int V = dm->V, T = dm->T, Vt = tm->V, Tt = tm->T;
    const size_t LV = (size_t)L * V, LVt = (size_t)L * Vt;
    int st = MSM_OK;  // (the data mesh's adjacency lists are on the device: group_setup_pipeline saw to it before the pipelines started)
    SurgeryScratch &sc = w.surgery;
    MSM_TRY(sc.ensure(V, Vt, T, Tt, L));
    std::vector<int2> info(L);
    for (int l = 0; l < L; ++l) info[l] = make_int2(b.forest.info[l].nnodes, b.forest.info[l].grid_depth);
    MSM_HIP(w.info[which].ensure(L));
    MSM_TRY(stage_h2d(ctx, w.info[which].p, info.data(), sizeof(int2) * (size_t)L));
    MSM_TRY(ctx_sync(ctx));  // the previous subject's batch has finished with the scratch
    ForestDev fd;
    fd.node = b.forest.node.p, fd.parent = b.forest.parent.p, fd.leaf_tri = b.forest.leaf_tri.p, fd.grid = b.forest.grid.p;
    fd.cone = b.forest.cone.p, fd.rec = b.forest.rec.p;
    fd.s_node = b.forest.s_node, fd.s_leaf = b.forest.s_leaf, fd.s_rec = b.forest.s_rec, fd.s_grid = b.forest.s_grid;
    fd.info = w.info[which].p;
    // forward: the template's vertices in every label's tree; reverse: every label's vertices in the template's tree (:74-78)
    st = launch_query_forest(ctx, fd, L, tm->d_xyz.p, Vt, sc.fvid.p, sc.fw.p, LVt);
    if (st) return st;
    MSM_HIP(w.open.ensure(LV + 1));
    st = launch_query_rays(ctx, dev_tree(tm), b.d_rot.p, (int)LV, nullptr, sc.rvid.p, sc.rw.p, MSM_WEIGHTS_PROJECTED, w.open.p);  // (the template's direction table: group_setup_pipeline)
    if (st) return st;
    st = launch_vertex_areas_batch(ctx, b.d_rot.p, LV, (size_t)V, V, dm->d_tri.p, T, dm->d_tid_ptr.p, dm->d_tid.p, L, sc.ta.p, sc.oldA.p);
    if (st) return st;
    st = launch_vertex_areas_batch(ctx, tm->d_xyz.p, (size_t)Vt, 0, Vt, tm->d_tri.p, Tt, tm->d_tid_ptr.p, tm->d_tid.p, 1, sc.ta.p, sc.newA.p);
    if (st) return st;
    const AdaptiveDevArgs a = sc.args(V, Vt, L);
    st = launch_adaptive_surgery(ctx, a);
    if (st) return st;
    st = launch_apply_rows_batch(ctx, a, D, b.d_feat.p, g->Fslab[s]->p, (size_t)D * Vt);
    if (st) return st;
    if (defer_status) return MSM_OK;  // the caller queues the subject's patch lists behind this and looks once (subject_patches)
    return check_status(ctx, "get_patch_data (resampling)");  // synchronises the batch stream
}

// A subject whose forest outgrew its arrays (a degenerate mesh), label by label on the batch stream: the label's rotated coordinates become those of the
// pipeline's scratch mesh, which builds a tree of its own (on the GPU, or on the host when that overflows too), and its weights resample into F[s][l]
static int stage_fallback(msm_group *g, int s, msm_group::Stage &b, msm_group::Pipe &P) {
    msm_ctx *ctx = P.batch.ctx;
    const int L = g->L, D = g->D;
    msm_mesh *dm = g->data[s];
    const int V = dm->V;
    const size_t LV = (size_t)L * V;
    msm_mesh *&m = P.fallback;
    if (m && (m->V != V || m->T != dm->T || m->tri != dm->tri)) {
        MSM_TRY(ctx_sync(ctx));
        msm_mesh_destroy(m);
        m = nullptr;
    }
    if (!m) {
        m = msm_mesh_create(ctx, dm->xyz.data(), V, dm->tri.data(), dm->T);
        if (!m) return MSM_ERR_HIP;
        m->gpu_tree_always = true;
    }
    for (int l = 0; l < L; ++l) {
        for (int a = 0; a < 3; ++a)
            MSM_HIP(hipMemcpyAsync(m->d_xyz.p + (size_t)a * V, b.d_rot.p + a * LV + (size_t)l * V, sizeof(double) * (size_t)V, hipMemcpyDeviceToDevice, ctx->stream));
        m->tree_valid = false;
        m->host_xyz_stale = true;
        AdaptiveDev w;
        int st = adaptive_weights_dev(m, g->tmpl, w, false);
        if (!st) st = apply_weights_dev(ctx, w, b.d_feat.p, D, g->F[(size_t)s * L + l]->p);
        if (st) return st;
    }
    return check_status(ctx, "get_patch_data (resampling)");  // synchronises the batch stream
}

// one pipeline over its share of the subjects: while the batch stream works through subject i, the main stream prepares subject i + 1
static int run_setup_pipe(msm_group *g, msm_group::Pipe &P, int pipe_no, const std::vector<int> &subjects) {
    const int n = (int)subjects.size();
    if (n == 0) return MSM_OK;
    msm_ctx *ctx = P.main;
    (void)hipSetDevice(ctx->device);
    const bool timing = std::getenv("MSMHIP_TIMING") != nullptr;
    // Two loops over a ring of kStages stages (round 5; until then one iteration = a thread for subject i's per-label work beside the preparation of subject
    // i + 1, joined: either stream idled 0.4 - 0.55 ms per subject for the other one, thread start and join included).  The preparing loop (this thread,
    // the main stream) runs up to kStages subjects ahead of the consuming one (a thread of its own for the whole pipeline, the batch stream).
    constexpr int K = msm_group::kStages;
    std::mutex mu;
    std::condition_variable cv;
    int prepared = 0, consumed = 0;  // subjects whose stage is ready / whose stage is free again
    bool stop = false;
    int st_batch = MSM_OK, st_main = MSM_OK;
    std::string msg_batch;
    std::thread consumer([&] {
        (void)hipSetDevice(ctx->device);
        for (int i = 0; i < n; ++i) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return prepared > i || stop; });
                if (prepared <= i) return;  // the preparing side failed
            }
            const int s = subjects[i];
            msm_group::Stage &cur = P.stage[i % K];
            const auto l0 = std::chrono::steady_clock::now();
            // the subject's patch lists (the range kernel) follow its per-label work on the batch stream, one look at the outcome of both
            int st = cur.forest_ok ? stage_batch(g, s, cur, i & 1, P.batch, true) : stage_fallback(g, s, cur, P);
            if (!st) st = subject_patches(g, s, P.batch.ctx, &P, cur.forest_ok ? "get_patch_data (resampling)" : nullptr);
            if (timing && i < 4)
                fprintf(stderr, "  group set-up, pipeline %d, subject %d: per-label work + patches %.2f ms\n", pipe_no, s,
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - l0).count());
            std::lock_guard<std::mutex> lk(mu);
            if (st) {
                st_batch = st, msg_batch = msm_last_error(), stop = true;
                cv.notify_all();
                return;
            }
            g->have_subject[s] = 1;
            consumed = i + 1;
            cv.notify_all();
        }
    });
    for (int i = 0; i < n && !st_main; ++i) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return i - consumed < K || stop; });
            if (stop) break;
        }
        const auto m0 = std::chrono::steady_clock::now();
        st_main = stage_prepare(g, subjects[i], P.stage[i % K], ctx);
        if (timing && i < 4)
            fprintf(stderr, "  group set-up, pipeline %d, subject %d: rotations + forest %.2f ms\n", pipe_no, subjects[i],
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - m0).count());
        std::lock_guard<std::mutex> lk(mu);
        if (st_main) stop = true;
        else prepared = i + 1;
        cv.notify_all();
    }
    consumer.join();
    if (st_batch) return fail(st_batch, "%s", msg_batch.c_str());
    return st_main;
}

// The subjects of this rank, pipelined.  Within a pipeline the batch stream works through subject i while the main stream prepares subject i + 1
// (rotations, forest); round 4: TWO pipelines take alternate subjects (streams, forests and scratch of their own, a host thread each): either is a
// chain of small dependent launches that leaves the GPU mostly idle (2.35 -> 1.5 ms per ico6 subject).
static int group_setup_pipeline(msm_group *g, const int32_t *subjects, int n) {
    if (n <= 0) return MSM_OK;
    msm_ctx *ctx = g->ctx;
    // the template's search structure and adjacency, and the data meshes' adjacency lists, are read by every pipeline: complete before they start
    int st = ensure_tree(g->tmpl);
    if (st) return st;
    // the template's direction table (a simple surface has one; built once per template content and kept, api.cpp: ensure_rays): the reverse queries of every
    // subject and label run through it (stage_batch)
    st = ensure_rays(g->tmpl, true);
    if (st) return st;
    st = ensure_adjacency_dev(g->tmpl);
    if (st) return st;
    {   // the grid the subjects' range tests take their candidates from (subject_patches): cells of about a sixteenth of the sphere's diameter
        const int G = g->tmpl->V > 60000 ? 64 : 32;
        const size_t cells = (size_t)G * G * G;
        MSM_HIP(g->d_rg_start.ensure(cells + 1));
        MSM_HIP(g->d_rg_cursor.ensure(cells));
        MSM_HIP(g->d_rg_ids.ensure((size_t)g->tmpl->V));
        MSM_HIP(g->d_rg_bad.ensure(1));
        MSM_HIP(g->d_rg_tmp.ensure(cells / 4096 + 2));
        const double origin = -1.01 * kRad, inv_h = (double)G / (2.02 * kRad);
        st = launch_range_grid_build(ctx, g->tmpl->d_xyz.p, g->tmpl->V, G, origin, inv_h, g->d_rg_start.p, g->d_rg_cursor.p, g->d_rg_ids.p, g->d_rg_bad.p, g->d_rg_tmp.p);
        if (st) return st;
        g->rgrid.start = g->d_rg_start.p, g->rgrid.ids = g->d_rg_ids.p, g->rgrid.bad = g->d_rg_bad.p, g->rgrid.G = G, g->rgrid.origin = origin, g->rgrid.inv_h = inv_h;
        g->rgrid_valid = true;
    }
    struct GridScope {  // the template may move before anybody else asks for patch lists
        msm_group *g;
        ~GridScope() { g->rgrid_valid = false; }
    } grid_scope{g};
    for (int i = 0; i < n; ++i) {
        if (!g->data[subjects[i]]) return fail(MSM_ERR_STATE, "msm_group: subject %d has no data", subjects[i]);
        st = ensure_adjacency_dev(g->data[subjects[i]]);
        if (st) return st;
    }
    MSM_TRY(ctx_sync(ctx));
    const int npipes = std::max(1, std::min(msm_group::kMaxPipes, n / 2));
    g->pipe[0].main = ctx;
    for (int k = 1; k < npipes; ++k)
        if (!g->pipe[k].main) {
            g->pipe[k].main = msm_ctx_create(ctx->device);
            if (!g->pipe[k].main) return MSM_ERR_HIP;
            g->pipe[k].own_main = true;
        }
    for (int k = 0; k < npipes; ++k)
        if (!g->pipe[k].batch.ctx) {
            g->pipe[k].batch.ctx = msm_ctx_create(ctx->device);
            if (!g->pipe[k].batch.ctx) return MSM_ERR_HIP;
        }
    std::vector<int> share[msm_group::kMaxPipes];
    for (int i = 0; i < n; ++i) share[i % npipes].push_back(subjects[i]);
    if (npipes == 1) return run_setup_pipe(g, g->pipe[0], 0, share[0]);
    int stk[msm_group::kMaxPipes] = {MSM_OK, MSM_OK};
    std::string msgk[msm_group::kMaxPipes];
    std::vector<std::thread> others;
    for (int k = 1; k < npipes; ++k)
        others.emplace_back([&, k] {
            stk[k] = run_setup_pipe(g, g->pipe[k], k, share[k]);
            if (stk[k]) msgk[k] = msm_last_error();
        });
    stk[0] = run_setup_pipe(g, g->pipe[0], 0, share[0]);
    if (stk[0]) msgk[0] = msm_last_error();
    for (auto &t : others) t.join();
    for (int k = 0; k < npipes; ++k)
        if (stk[k]) return fail(stk[k], "%s", msgk[k].c_str());
    return MSM_OK;
}

}  // namespace

extern "C" {

int msm_group_setup_subjects(msm_group *g, const int32_t *subjects, int32_t n) {
    if (!g || (n > 0 && !subjects) || n < 0) return fail(MSM_ERR_INVALID, "msm_group_setup_subjects: bad arguments");
    g->ready = false;
    g->common_ready = false;
    g->drop_kept();
    int st = group_common_setup(g);
    if (st) return st;
    for (int i = 0; i < n; ++i)
        if (subjects[i] < 0 || subjects[i] >= g->S) return fail(MSM_ERR_INVALID, "subject %d out of range", subjects[i]);
    return group_setup_pipeline(g, subjects, n);
}

// further subjects of this rank after msm_group_setup_subjects (same control grids, labels and data): the set-up in chunks, so that the exchange of
// one chunk (an all-gather on another stream) runs while the next is set up
int msm_group_setup_more_subjects(msm_group *g, const int32_t *subjects, int32_t n) {
    if (!g || (n > 0 && !subjects) || n < 0) return fail(MSM_ERR_INVALID, "msm_group_setup_more_subjects: bad arguments");
    if (!g->common_ready) return fail(MSM_ERR_STATE, "msm_group: msm_group_setup_subjects() must be called first (an empty list is fine)");
    g->ready = false;
    for (int i = 0; i < n; ++i)
        if (subjects[i] < 0 || subjects[i] >= g->S) return fail(MSM_ERR_INVALID, "subject %d out of range", subjects[i]);
    return group_setup_pipeline(g, subjects, n);
}

}  // extern "C"
