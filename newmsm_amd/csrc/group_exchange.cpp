// group_exchange.cpp -- a subject's resampled maps and patch lists leave one group and enter another (the ranks of a sharded run): the host and the
// device entry points of msm_group_export_subject* / msm_group_import_subject*, over one core each way.
#include "group_internal.hpp"

namespace {

// The core of every export.  n subjects into the caller's arrays, host memory or device memory of this context's GPU: subject subjects[k]'s maps at
// F + k * F_stride (doubles), its row offsets at pptr + k * pptr_stride, its ids at pidx + k * pidx_stride (room for pidx_stride of them), its index
// count in npidx[k]; a null array is not wanted.  Everything is checked before the first copy, and the copies are complete on return.
int export_subjects(msm_group *g, const char *who, const int32_t *subjects, int n, double *F, int64_t F_stride, int32_t *pptr, int64_t pptr_stride, int32_t *pidx,
                    int64_t pidx_stride, int64_t *npidx, bool device) {
    msm_ctx *ctx = g->ctx;
    for (int k = 0; k < n; ++k) {
        const int s = subjects[k];
        if (s < 0 || s >= g->S) return fail(MSM_ERR_INVALID, "%s: subject %d out of range", who, s);
        if (!g->common_ready || !g->have_subject[s]) return fail(MSM_ERR_STATE, "msm_group: subject %d has not been set up on this rank", s);
        if (npidx) npidx[k] = g->patch_stat[s].npidx;
        if (pidx && g->patch_stat[s].npidx > pidx_stride) return fail(MSM_ERR_CAPACITY, "patch index buffer too small");
    }
    const size_t per = (size_t)g->D * g->tmpl->V, M = (size_t)g->N * g->L;
    auto copy = [&](void *dst, const void *src, size_t bytes) -> int {
        if (!device) return stage_d2h(ctx, dst, src, bytes);
        if (bytes) MSM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return MSM_OK;
    };
    const int parts = device ? 1 : g->L;  // (a host copy goes through a pinned block of its size: a map at a time)
    for (int k = 0; k < n; ++k) {
        const int s = subjects[k];
        for (int l = 0; F && l < parts; ++l) MSM_TRY(copy(F + (size_t)k * F_stride + per * l, g->Fslab[s]->p + per * l, sizeof(double) * per * (g->L / parts)));
        if (pptr) MSM_TRY(copy(pptr + (size_t)k * pptr_stride, g->pptr[s]->p, sizeof(int32_t) * (M + 1)));
        if (pidx) MSM_TRY(copy(pidx + (size_t)k * pidx_stride, g->pidx[s]->p, sizeof(int32_t) * (size_t)g->patch_stat[s].npidx));
    }
    return ctx_sync(ctx);  // a device buffer may go straight into a collective on another stream
}

// The core of every import, after the caller's validation: n subjects adopt the arrays of src (laid out as for export_subjects, npidx[k] ids each), which
// are host memory or device memory of this context's GPU; stat[k]: what the validation found in subject k's row offsets.
int adopt_subjects(msm_group *g, const int32_t *subjects, int n, const double *F, int64_t F_stride, const int32_t *pptr, int64_t pptr_stride, const int32_t *pidx,
                   int64_t pidx_stride, const int64_t *npidx, const msm_group::PatchStat *stat, bool device) {
    msm_ctx *ctx = g->ctx;
    const size_t per = (size_t)g->D * g->tmpl->V, M = (size_t)g->N * g->L;
    auto copy = [&](void *dst, const void *src, size_t bytes) -> int {
        if (!device) return upload_staged(ctx, dst, src, bytes);
        if (bytes) MSM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return MSM_OK;
    };
    const int parts = device ? 1 : g->L;
    for (int k = 0; k < n; ++k) {
        const int s = subjects[k];
        const int32_t *pp = pptr + (size_t)k * pptr_stride, *pi = pidx + (size_t)k * pidx_stride;
        MSM_TRY(subject_feature_slab(g, s, per));
        for (int l = 0; l < parts; ++l) MSM_TRY(copy(g->Fslab[s]->p + per * l, F + (size_t)k * F_stride + per * l, sizeof(double) * per * (g->L / parts)));
        MSM_HIP(g->pptr[s]->ensure(M + 1));
        MSM_TRY(copy(g->pptr[s]->p, pp, sizeof(int32_t) * (M + 1)));
        MSM_HIP(ensure_patch_entries(*g->pidx[s], (size_t)npidx[k]));
        MSM_TRY(copy(g->pidx[s]->p, pi, sizeof(int32_t) * (size_t)npidx[k]));
        g->patch_stat[s] = stat[k];
        // the host's copies: what the caller handed over, or nothing until somebody asks (msm_group_patch)
        g->h_pptr[s].clear();
        g->h_pidx[s].clear();
        if (!device) {
            g->h_pptr[s].assign(pp, pp + M + 1);
            g->h_pidx[s].assign(pi, pi + npidx[k]);
        }
    }
    MSM_TRY(ctx_sync(ctx));  // the caller may reuse its buffers
    for (int k = 0; k < n; ++k) g->have_subject[subjects[k]] = 2;  // (2: imported)
    return MSM_OK;
}

// Lists in device memory come from other ranks: checked where they are before any kernel indexes with them, then adopted
int import_from_device(msm_group *g, const char *who, const int32_t *subjects, int n, const double *F, int64_t F_stride, const int32_t *pptr, int64_t pptr_stride,
                       const int32_t *pidx, int64_t pidx_stride, const int64_t *npidx) {
    if (!g->common_ready) return fail(MSM_ERR_STATE, "msm_group: msm_group_setup_subjects() must be called first (an empty list is fine)");
    if (n == 0) return MSM_OK;
    msm_ctx *ctx = g->ctx;
    const size_t per = (size_t)g->D * g->tmpl->V, M = (size_t)g->N * g->L;
    if ((int64_t)(per * g->L) > F_stride || (int64_t)(M + 1) > pptr_stride) return fail(MSM_ERR_INVALID, "%s: strides too small", who);
    int64_t most = (int64_t)M + 1;
    for (int k = 0; k < n; ++k) {
        if (subjects[k] < 0 || subjects[k] >= g->S) return fail(MSM_ERR_INVALID, "%s: subject %d out of range", who, subjects[k]);
        if (npidx[k] < 0 || npidx[k] > pidx_stride) return fail(MSM_ERR_INVALID, "patch CSR of subject %d: %lld entries do not fit the buffer", subjects[k], (long long)npidx[k]);
        most = std::max(most, npidx[k]);
    }
    DevBuf<int64_t> d_np;
    DevBuf<int> d_out;
    MSM_TRY(d_np.upload(npidx, (size_t)n, ctx));
    MSM_HIP(d_out.zero(4 * (size_t)n, ctx->stream));
    MSM_TRY(launch_group_check_csr(ctx, pptr, pptr_stride, M, pidx, pidx_stride, d_np.p, most, n, g->tmpl->V, d_out.p));
    std::vector<int> out(4 * (size_t)n);
    MSM_TRY(d_out.download(out.data(), out.size(), ctx));
    MSM_TRY(ctx_sync(ctx));
    std::vector<msm_group::PatchStat> stat((size_t)n);
    for (int k = 0; k < n; ++k) {
        if (out[4 * (size_t)k])
            return fail(MSM_ERR_INVALID, "patch CSR of subject %d is inconsistent (code %d: 1 ends, 2 row lengths, 4 vertex ids)", subjects[k], out[4 * (size_t)k]);
        stat[(size_t)k].npidx = npidx[k];
        stat[(size_t)k].largest = out[4 * (size_t)k + 1];
        stat[(size_t)k].small = out[4 * (size_t)k + 2];
    }
    return adopt_subjects(g, subjects, n, F, F_stride, pptr, pptr_stride, pidx, pidx_stride, npidx, stat.data(), true);
}

}  // namespace

extern "C" {

int msm_group_export_subject(msm_group *g, int32_t s, double *F, int32_t *pptr, int32_t *pidx, int64_t cap, int64_t *npidx) {
    if (!g) return fail(MSM_ERR_INVALID, "msm_group_export_subject: bad arguments");
    return export_subjects(g, "msm_group_export_subject", &s, 1, F, 0, pptr, 0, pidx, cap, npidx, false);
}

// The same exchange without the host in between: the caller's buffers are DEVICE memory on this context's GPU (e.g. torch
// tensors about to go through an RCCL all-gather, or just out of one).  With null arrays: the subject's index count.
int msm_group_export_subject_dev(msm_group *g, int32_t s, double *F_dev, int32_t *pptr_dev, int32_t *pidx_dev, int64_t cap, int64_t *npidx) {
    if (!g) return fail(MSM_ERR_INVALID, "msm_group_export_subject_dev: bad arguments");
    return export_subjects(g, "msm_group_export_subject_dev", &s, 1, F_dev, 0, pptr_dev, 0, pidx_dev, cap, npidx, true);
}

// n subjects at once into / out of strided device buffers -- the send and receive buffers of ONE all-gather: subject subjects[k]'s arrays start at
// F_dev + k * F_stride (doubles), pptr_dev + k * pptr_stride and pidx_dev + k * pidx_stride (int32).  One synchronisation per call instead of two per
// subject (56 imports of an 8-rank, 64-subject group: 9.2 -> under 1 ms, tools/time_group_rank.py).
int msm_group_export_subjects_dev(msm_group *g, const int32_t *subjects, int32_t n, double *F_dev, int64_t F_stride, int32_t *pptr_dev, int64_t pptr_stride,
                                  int32_t *pidx_dev, int64_t pidx_stride, int64_t *npidx) {
    if (!g || (n > 0 && (!subjects || !F_dev || !pptr_dev || !pidx_dev)) || n < 0) return fail(MSM_ERR_INVALID, "msm_group_export_subjects_dev: bad arguments");
    if (g->tmpl && ((int64_t)g->D * g->tmpl->V * g->L > F_stride || (int64_t)g->N * g->L + 1 > pptr_stride))
        return fail(MSM_ERR_CAPACITY, "msm_group_export_subjects_dev: strides too small");
    return export_subjects(g, "msm_group_export_subjects_dev", subjects, n, F_dev, F_stride, pptr_dev, pptr_stride, pidx_dev, pidx_stride, npidx, true);
}

int msm_group_import_subject(msm_group *g, int32_t s, const double *F, const int32_t *pptr, const int32_t *pidx, int64_t npidx) {
    if (!g || !F || !pptr || (!pidx && npidx > 0) || s < 0 || s >= g->S || npidx < 0) return fail(MSM_ERR_INVALID, "msm_group_import_subject: bad arguments");
    if (!g->common_ready) return fail(MSM_ERR_STATE, "msm_group: msm_group_setup_subjects() must be called first (an empty list is fine)");
    const size_t M = (size_t)g->N * g->L;
    // the arrays come from another rank: nothing of them is trusted before it indexes device or host memory
    if (pptr[0] != 0 || pptr[M] != npidx) return fail(MSM_ERR_INVALID, "patch CSR of subject %d is inconsistent", s);
    for (size_t r = 0; r < M; ++r)
        if (pptr[r + 1] < pptr[r]) return fail(MSM_ERR_INVALID, "patch CSR of subject %d: row %zu has a negative length", s, r);
    const int32_t Vt = g->tmpl->V;
    for (int64_t j = 0; j < npidx; ++j)
        if (pidx[j] < 0 || pidx[j] >= Vt) return fail(MSM_ERR_INVALID, "patch CSR of subject %d: template vertex id %d out of range [0,%d)", s, pidx[j], Vt);
    const msm_group::PatchStat stat = patch_stat_of(pptr, M);
    return adopt_subjects(g, &s, 1, F, 0, pptr, 0, pidx, 0, &npidx, &stat, false);
}

int msm_group_import_subject_dev(msm_group *g, int32_t s, const double *F_dev, const int32_t *pptr_dev, const int32_t *pidx_dev, int64_t npidx) {
    if (!g || !F_dev || !pptr_dev || (!pidx_dev && npidx > 0) || npidx < 0) return fail(MSM_ERR_INVALID, "msm_group_import_subject_dev: bad arguments");
    constexpr int64_t whole = INT64_MAX;  // one subject is a batch of one: no second subject follows at any stride
    return import_from_device(g, "msm_group_import_subject_dev", &s, 1, F_dev, whole, pptr_dev, whole, pidx_dev, npidx, &npidx);
}

int msm_group_import_subjects_dev(msm_group *g, const int32_t *subjects, int32_t n, const double *F_dev, int64_t F_stride, const int32_t *pptr_dev,
                                  int64_t pptr_stride, const int32_t *pidx_dev, int64_t pidx_stride, const int64_t *npidx) {
    if (!g || n < 0 || (n > 0 && (!subjects || !F_dev || !pptr_dev || !pidx_dev || !npidx))) return fail(MSM_ERR_INVALID, "msm_group_import_subjects_dev: bad arguments");
    return import_from_device(g, "msm_group_import_subjects_dev", subjects, n, F_dev, F_stride, pptr_dev, pptr_stride, pidx_dev, pidx_stride, npidx);
}

}  // extern "C"
