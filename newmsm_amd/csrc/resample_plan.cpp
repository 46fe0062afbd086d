// resample_plan.cpp -- msm_resample_plan_*: the rows of one (in_mesh -> new_mesh) resampling built once, kept in HBM and applied to any number of maps.
// The rows come from the paths the library already has (adaptive_weights_dev / adaptive_weights, launch_query, launch_closest_vertex: resample.cpp,
// kernels.hip); what is new is the ownership (a snapshot: nothing here points back into a mesh or into context scratch) and the apply
// (resample_plan_kernels.hip).  Host arrays travel in slabs through the context's pinned staging blocks (stager.cpp): the device never holds more than
// the slab budget of maps, whatever D is.
// A smoothing plan (msm_resample_plan_create_smooth) is the fourth kind of row: smooth_data's neighbourhoods, built on the device and never seen by the
// host (smooth_plan_kernels.hip), with a divisor per row that the apply divides by.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "kernels.hpp"
#include "resample.hpp"
#include "resample_plan.hpp"

using namespace msm;

struct msm_resample_plan {
    msm_ctx *ctx = nullptr;
    int nOld = 0, nNew = 0, method = 0, longest = 0;
    int64_t nnz = 0;
    bool masked = false;
    DevBuf<int32_t> row_ptr, col;   // nNew + 1, nnz
    DevBuf<double> val, excl;       // nnz, nOld (masked plans)
    DevBuf<double> div;             // nNew (smoothing plans): the sum of a row's weights, 0.0 where the row is not divided
    std::vector<double> excl_out;   // masked plans: the resampled / smoothed mask (it depends on the rows and the mask only)
    DevBuf<char> in, out, tin, tout;  // grow-only scratch of the applies: a slab of maps in and out, one tile in vertex-major order in and out
    hipEvent_t ev = nullptr;        // behind a slab's download: its delivery waits for this, not for the stream

    PlanRows rows() const {
        PlanRows r;
        r.nOld = nOld, r.nNew = nNew, r.row_ptr = row_ptr.p, r.col = col.p, r.val = val.p, r.excl = masked ? excl.p : nullptr;
        r.row_div = method == MSM_RESAMPLE_SMOOTH ? div.p : nullptr;
        return r;
    }
};

namespace {

// The slab budget: bytes of maps (input and result together) the device holds at a time.  Two tiles of kPlanTile maps in vertex-major order come on top.
constexpr size_t kPlanBudgetDefault = (size_t)64 << 20;
size_t plan_budget() {
    const char *e = std::getenv("MSMHIP_PLAN_CHUNK_KB");
    const long long kb = e ? std::atoll(e) : 0;
    return kb > 0 ? (size_t)kb << 10 : kPlanBudgetDefault;
}
// maps per slab for elements of es bytes: what the budget holds, whole tiles when it holds more than one
int64_t slab_maps(const msm_resample_plan *p, size_t es, int64_t D) {
    const size_t per_map = ((size_t)p->nOld + (size_t)p->nNew) * es;
    int64_t s = per_map ? (int64_t)(plan_budget() / per_map) : D;
    s = std::max<int64_t>(1, std::min(s, D));
    if (s > kPlanTile) s -= s % kPlanTile;
    return s;
}

int upload_rows(msm_resample_plan *p, const std::vector<int32_t> &rp, const std::vector<int32_t> &c, const std::vector<double> &v) {
    msm_ctx *ctx = p->ctx;
    p->nnz = (int64_t)c.size();
    if (p->row_ptr.ensure(rp.size(), true) || p->col.ensure(std::max<size_t>(c.size(), 1), true) || p->val.ensure(std::max<size_t>(v.size(), 1), true))
        return stage_alloc_failed(12 * c.size());
    MSM_TRY(stage_h2d(ctx, p->row_ptr.p, rp.data(), sizeof(int32_t) * rp.size()));
    MSM_TRY(stage_h2d(ctx, p->col.p, c.data(), sizeof(int32_t) * c.size()));
    MSM_TRY(stage_h2d(ctx, p->val.p, v.data(), sizeof(double) * v.size()));
    for (size_t k = 0; k + 1 < rp.size(); ++k) p->longest = std::max(p->longest, rp[k + 1] - rp[k]);
    return MSM_OK;
}

int build(msm_resample_plan *p, msm_mesh *in_mesh, msm_mesh *new_mesh, const double *excl) {
    msm_ctx *ctx = p->ctx;
    const int nOld = p->nOld, nNew = p->nNew;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MSM_HIP(hipEventCreateWithFlags(&p->ev, hipEventDisableTiming));
    std::vector<int32_t> rp, c;
    std::vector<double> v;
    if (p->method == MSM_RESAMPLE_ADAP_BARY && !excl) {
        // searches and list surgery on the device; the rows leave the context's scratch with three device-to-device copies
        AdaptiveDev w;
        MSM_TRY(adaptive_weights_dev(in_mesh, new_mesh, w));
        size_t nnz = 0;
        MSM_TRY(fetch_row_ptr(ctx, w, rp, nnz));
        p->nnz = (int64_t)nnz;
        if (p->row_ptr.ensure(rp.size(), true) || p->col.ensure(std::max<size_t>(nnz, 1), true) || p->val.ensure(std::max<size_t>(nnz, 1), true))
            return stage_alloc_failed(12 * nnz);
        MSM_HIP(hipMemcpyAsync(p->row_ptr.p, w.row_ptr, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToDevice, ctx->stream));
        if (nnz) {
            MSM_HIP(hipMemcpyAsync(p->col.p, w.col, sizeof(int32_t) * nnz, hipMemcpyDeviceToDevice, ctx->stream));
            MSM_HIP(hipMemcpyAsync(p->val.p, w.val, sizeof(double) * nnz, hipMemcpyDeviceToDevice, ctx->stream));
        }
        for (int k = 0; k < nNew; ++k) p->longest = std::max(p->longest, rp[(size_t)k + 1] - rp[(size_t)k]);
        return ctx_sync(ctx);
    }
    if (p->method == MSM_RESAMPLE_ADAP_BARY) {
        MSM_TRY(adaptive_weights(in_mesh, new_mesh, excl, rp, c, v));  // the searches on the GPU, the surgery with its mask on the host
    } else {
        MSM_TRY(ensure_tree(in_mesh));
        rp.resize((size_t)nNew + 1);
        if (p->method == MSM_RESAMPLE_BARYCENTRIC) {
            DevBuf<int> dvid;
            DevBuf<double> dw;
            std::vector<int> vid(3 * (size_t)nNew);
            std::vector<double> w(3 * (size_t)nNew);
            if (dvid.ensure(vid.size() + 1) || dw.ensure(w.size() + 1)) return stage_alloc_failed(36 * (size_t)nNew);
            MSM_TRY(launch_query(ctx, dev_tree(in_mesh), new_mesh->d_xyz.p, nNew, nullptr, dvid.p, dw.p, MSM_WEIGHTS_PROJECTED));
            MSM_TRY(dvid.download(vid.data(), vid.size(), ctx));
            MSM_TRY(dw.download(w.data(), w.size(), ctx));
            MSM_TRY(check_status(ctx, "msm_resample_plan_create (barycentric)"));
            for (int k = 0; k < nNew; ++k) {
                WeightEntry e[3];  // R/resampler.cpp:150-166 read at :296-297
                const int n = small_map(vid.data(), w.data(), nNew, k, e);
                rp[(size_t)k] = (int32_t)c.size();
                for (int j = 0; j < n; ++j) c.push_back(e[j].key), v.push_back(e[j].w);
            }
        } else {
            DevBuf<int> dcv;
            std::vector<int> cv((size_t)nNew);
            if (dcv.ensure(cv.size() + 1)) return stage_alloc_failed(4 * (size_t)nNew);
            MSM_TRY(launch_closest_vertex(ctx, dev_tree(in_mesh), new_mesh->d_xyz.p, nNew, dcv.p));
            MSM_TRY(dcv.download(cv.data(), cv.size(), ctx));
            MSM_TRY(check_status(ctx, "msm_resample_plan_create (nearest)"));
            for (int k = 0; k < nNew; ++k) rp[(size_t)k] = k;
            c.assign(cv.begin(), cv.end());
            v.assign((size_t)nNew, 1.0);
        }
        rp[(size_t)nNew] = (int32_t)c.size();
    }
    MSM_TRY(upload_rows(p, rp, c, v));
    if (excl) {
        p->masked = true;
        MSM_TRY(p->excl.upload(excl, (size_t)nOld, ctx));
        p->excl_out.assign((size_t)nNew, 0.0);
        resampled_mask(rp, c, v, excl, p->excl_out.data());
    }
    return ctx_sync(ctx);
}

// The rows of smooth_data(orig, sphlow, sigma, excl), R/resampler.cpp:168-230, with msm_smooth_data's indexing (api.cpp).  The mask is part of the stored
// weights, so the plan keeps none for its applies (masked stays false) and only hands out the smoothed mask.
int build_smooth(msm_resample_plan *p, msm_mesh *orig, msm_mesh *sphlow, double sigma, const double *excl) {
    msm_ctx *ctx = p->ctx;
    const int N = p->nNew;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MSM_HIP(hipEventCreateWithFlags(&p->ev, hipEventDisableTiming));
    MSM_TRY(ensure_tree(orig));
    DevBuf<int> dcv, dtmp;
    DevBuf<double> dunit, dexcl, dexo;
    if (dcv.ensure((size_t)N + 1) || dunit.ensure(smooth_scratch_doubles(N)) || dtmp.ensure((size_t)N / 4096 + 2) || p->row_ptr.ensure((size_t)N + 1, true) ||
        p->div.ensure(std::max<size_t>((size_t)N, 1), true) || (excl && dexo.ensure(std::max<size_t>((size_t)N, 1))))
        return stage_alloc_failed(sizeof(double) * smooth_scratch_doubles(N) + 16 * (size_t)N);
    MSM_TRY(launch_closest_vertex(ctx, dev_tree(orig), sphlow->d_xyz.p, N, dcv.p));  // Octree(orig).get_closest_vertex_ID(ci), :182
    MSM_TRY(launch_smooth_prepare(ctx, sphlow->d_xyz.p, N, dunit.p));
    if (excl) MSM_TRY(dexcl.upload(excl, (size_t)p->nOld, ctx));
    const double ang = 4 * asin(sigma / (2 * kRad));  // :175, with the host's libm like the reference
    const SmoothRows s{dunit.p, reinterpret_cast<const double4 *>(dunit.p + smooth_bounds_offset(N)), dcv.p, excl ? dexcl.p : nullptr, N, sigma, cos(ang)};
    MSM_TRY(launch_smooth_plan_count(ctx, s, p->row_ptr.p));
    // the lengths come down once; their sum is taken in 64 bits before anything is sized by it
    std::vector<int32_t> len((size_t)N);
    MSM_TRY(p->row_ptr.download(len.data(), (size_t)N, ctx));
    MSM_TRY(check_status(ctx, "msm_resample_plan_create_smooth"));
    int64_t nnz = 0;
    for (int32_t l : len) nnz += l, p->longest = std::max(p->longest, (int)l);
    if (nnz > (int64_t)INT32_MAX)
        return fail(MSM_ERR_INVALID, "msm_resample_plan_create_smooth: nnz = %lld entries (%d rows, the longest of %d) do not fit the plan's 32-bit row offsets", (long long)nnz,
                    N, p->longest);
    p->nnz = nnz;
    if (p->col.ensure(std::max<size_t>((size_t)nnz, 1), true) || p->val.ensure(std::max<size_t>((size_t)nnz, 1), true)) return stage_alloc_failed(12 * (size_t)nnz);
    MSM_TRY(launch_scan_exclusive(ctx, p->row_ptr.p, N, dtmp.p));
    MSM_TRY(launch_smooth_plan_fill(ctx, s, p->row_ptr.p, p->col.p, p->val.p, p->div.p, excl ? dexo.p : nullptr));
    if (excl) {
        p->excl_out.assign((size_t)N, 0.0);
        MSM_TRY(dexo.download(p->excl_out.data(), (size_t)N, ctx));
    }
    return check_status(ctx, "msm_resample_plan_create_smooth");
}

template <typename T>
int tiles(msm_resample_plan *p, const T *d_data, int64_t D, T *d_out) {
    const PlanRows r = p->rows();
    for (int64_t d0 = 0; d0 < D; d0 += kPlanTile) {
        const int nd = (int)std::min<int64_t>(kPlanTile, D - d0);
        MSM_TRY(launch_plan_tile<T>(p->ctx, r, d_data + (size_t)d0 * (size_t)p->nOld, nd, (T *)p->tin.p, (T *)p->tout.p, d_out + (size_t)d0 * (size_t)p->nNew));
    }
    return MSM_OK;
}

int ensure_tiles(msm_resample_plan *p, size_t es) {
    if (p->tin.ensure(std::max<size_t>((size_t)p->nOld, 1) * kPlanTile * es) || p->tout.ensure(std::max<size_t>((size_t)p->nNew, 1) * kPlanTile * es))
        return stage_alloc_failed(((size_t)p->nOld + (size_t)p->nNew) * kPlanTile * es);
    return MSM_OK;
}

int check_apply(const msm_resample_plan *p, const void *data, int dtype, int64_t D, const void *out, const char *what) {
    if (!p) return fail(MSM_ERR_INVALID, "%s: null plan", what);
    if (dtype != MSM_F64 && dtype != MSM_F32) return fail(MSM_ERR_INVALID, "%s: unknown dtype %d (MSM_F64 = 0, MSM_F32 = 1)", what, dtype);
    if (D < 0) return fail(MSM_ERR_INVALID, "%s: D = %lld maps", what, (long long)D);
    if (D > 0 && (!data || !out)) return fail(MSM_ERR_INVALID, "%s: null array with D = %lld", what, (long long)D);
    return MSM_OK;
}

// host arrays, slab by slab.  While the GPU works on slab i the host fills the staging block of slab i + 1 and hands slab i - 1's result to the caller;
// the copies and kernels themselves run in order on the context's one stream (a staged download is delivered from the thread that queued it, after an
// event behind it: stager.cpp).
template <typename T>
int apply_host(msm_resample_plan *p, const T *data, int64_t D, T *out) {
    msm_ctx *ctx = p->ctx;
    const size_t nOld = (size_t)p->nOld, nNew = (size_t)p->nNew;
    const int64_t S = slab_maps(p, sizeof(T), D);
    MSM_TRY(ensure_tiles(p, sizeof(T)));
    if (p->in.ensure(std::max<size_t>((size_t)S * nOld, 1) * sizeof(T)) || p->out.ensure(std::max<size_t>((size_t)S * nNew, 1) * sizeof(T)))
        return stage_alloc_failed((size_t)S * (nOld + nNew) * sizeof(T));
    bool pending = false;
    for (int64_t d0 = 0; d0 < D; d0 += S) {
        const int64_t n = std::min(S, D - d0);
        MSM_TRY(stage_h2d(ctx, p->in.p, data + (size_t)d0 * nOld, (size_t)n * nOld * sizeof(T)));
        MSM_TRY(tiles<T>(p, (const T *)p->in.p, n, (T *)p->out.p));
        if (pending) {  // the previous slab's download has been queued before this slab's kernels
            MSM_HIP(hipEventSynchronize(p->ev));
            stage_deliver(ctx);
        }
        MSM_TRY(stage_d2h(ctx, out + (size_t)d0 * nNew, p->out.p, (size_t)n * nNew * sizeof(T)));
        MSM_HIP(hipEventRecord(p->ev, ctx->stream));
        pending = true;
    }
    return ctx_sync(ctx);
}

}  // namespace

extern "C" {

msm_resample_plan *msm_resample_plan_create(msm_mesh *in_mesh, msm_mesh *new_mesh, int method, const double *excl) {
    if (!in_mesh || !new_mesh) {
        fail(MSM_ERR_INVALID, "msm_resample_plan_create: null mesh");
        return nullptr;
    }
    if (in_mesh->ctx != new_mesh->ctx) {
        fail(MSM_ERR_INVALID, "msm_resample_plan_create: the two meshes belong to different contexts");
        return nullptr;
    }
    if (method != MSM_RESAMPLE_ADAP_BARY && method != MSM_RESAMPLE_BARYCENTRIC && method != MSM_RESAMPLE_NEAREST) {
        fail(MSM_ERR_INVALID, "msm_resample_plan_create: unknown method %d (ADAP_BARY = 0, BARYCENTRIC = 1, NEAREST = 2)", method);
        return nullptr;
    }
    msm_resample_plan *p = new (std::nothrow) msm_resample_plan();
    if (!p) {
        fail(MSM_ERR_INVALID, "msm_resample_plan_create: out of memory");
        return nullptr;
    }
    p->ctx = in_mesh->ctx;
    p->nOld = in_mesh->V, p->nNew = new_mesh->V, p->method = method;
    int st;
    try {
        st = build(p, in_mesh, new_mesh, excl);
    } catch (const std::exception &e) {
        st = fail(MSM_ERR_INVALID, "msm_resample_plan_create: %s", e.what());
    }
    if (st) {
        msm_resample_plan_destroy(p);
        return nullptr;
    }
    return p;
}

msm_resample_plan *msm_resample_plan_create_smooth(msm_mesh *orig, msm_mesh *sphlow, double sigma, const double *excl) {
    if (!orig || !sphlow) {
        fail(MSM_ERR_INVALID, "msm_resample_plan_create_smooth: null mesh");
        return nullptr;
    }
    if (orig->ctx != sphlow->ctx) {
        fail(MSM_ERR_INVALID, "msm_resample_plan_create_smooth: the two meshes belong to different contexts");
        return nullptr;
    }
    if (!(sigma > 0)) {
        fail(MSM_ERR_INVALID, "msm_resample_plan_create_smooth: sigma = %g, a positive width is needed", sigma);
        return nullptr;
    }
    // the reference reads orig's data and the exclusion mask with sphLow's vertex ids (R/resampler.cpp:193-210)
    if (orig->V < sphlow->V) {
        fail(MSM_ERR_INVALID, "msm_resample_plan_create_smooth: the data mesh has %d vertices, the sphere %d", orig->V, sphlow->V);
        return nullptr;
    }
    msm_resample_plan *p = new (std::nothrow) msm_resample_plan();
    if (!p) {
        fail(MSM_ERR_INVALID, "msm_resample_plan_create_smooth: out of memory");
        return nullptr;
    }
    p->ctx = orig->ctx;
    p->nOld = orig->V, p->nNew = sphlow->V, p->method = MSM_RESAMPLE_SMOOTH;
    int st;
    try {
        st = build_smooth(p, orig, sphlow, sigma, excl);
    } catch (const std::exception &e) {
        st = fail(MSM_ERR_INVALID, "msm_resample_plan_create_smooth: %s", e.what());
    }
    if (st) {
        msm_resample_plan_destroy(p);
        return nullptr;
    }
    return p;
}

void msm_resample_plan_destroy(msm_resample_plan *p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    if (p->ev) (void)hipEventDestroy(p->ev);
    delete p;  // the buffers go back to the pool, which waits for work that may still use them
}

int msm_resample_plan_sizes(const msm_resample_plan *p, int32_t *V_in, int32_t *V_out, int64_t *nnz, int32_t *longest_row) {
    if (!p) return fail(MSM_ERR_INVALID, "msm_resample_plan_sizes: null plan");
    if (V_in) *V_in = p->nOld;
    if (V_out) *V_out = p->nNew;
    if (nnz) *nnz = p->nnz;
    if (longest_row) *longest_row = p->longest;
    return MSM_OK;
}

int msm_resample_plan_weights(msm_resample_plan *p, int32_t *row_ptr, int32_t *col, double *val, int64_t cap) {
    if (!p) return fail(MSM_ERR_INVALID, "msm_resample_plan_weights: null plan");
    if ((col || val) && cap < p->nnz) return fail(MSM_ERR_INVALID, "msm_resample_plan_weights: the plan has %lld entries, the arrays hold %lld", (long long)p->nnz, (long long)cap);
    msm_ctx *ctx = p->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    if (row_ptr) MSM_TRY(p->row_ptr.download(row_ptr, (size_t)p->nNew + 1, ctx));
    if (col) MSM_TRY(p->col.download(col, (size_t)p->nnz, ctx));
    if (val) MSM_TRY(p->val.download(val, (size_t)p->nnz, ctx));
    return ctx_sync(ctx);
}

int msm_resample_plan_divisors(msm_resample_plan *p, double *div) {
    if (!p || !div) return fail(MSM_ERR_INVALID, "msm_resample_plan_divisors: null %s", p ? "array" : "plan");
    if (p->method != MSM_RESAMPLE_SMOOTH) {  // the other methods' rows are not divided
        std::fill(div, div + p->nNew, 0.0);
        return MSM_OK;
    }
    msm_ctx *ctx = p->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MSM_TRY(p->div.download(div, (size_t)p->nNew, ctx));
    return ctx_sync(ctx);
}

int msm_resample_plan_apply(msm_resample_plan *p, const void *data, int dtype, int64_t D, void *out, double *excl_out) {
    MSM_TRY(check_apply(p, data, dtype, D, out, "msm_resample_plan_apply"));
    if (excl_out) {
        if (!p->excl_out.empty()) std::copy(p->excl_out.begin(), p->excl_out.end(), excl_out);
        else std::fill(excl_out, excl_out + p->nNew, 0.0);
    }
    if (D == 0) return MSM_OK;
    MSM_HIP(hipSetDevice(p->ctx->device));
    MSM_TRY(drop_ctx_pending(p->ctx));
    return dtype == MSM_F32 ? apply_host<float>(p, (const float *)data, D, (float *)out) : apply_host<double>(p, (const double *)data, D, (double *)out);
}

int msm_resample_plan_apply_dev(msm_resample_plan *p, const void *data_dev, int dtype, int64_t D, void *out_dev) {
    MSM_TRY(check_apply(p, data_dev, dtype, D, out_dev, "msm_resample_plan_apply_dev"));
    if (D == 0) return MSM_OK;
    MSM_HIP(hipSetDevice(p->ctx->device));
    MSM_TRY(drop_ctx_pending(p->ctx));
    MSM_TRY(ensure_tiles(p, dtype == MSM_F32 ? sizeof(float) : sizeof(double)));
    if (dtype == MSM_F32) MSM_TRY(tiles<float>(p, (const float *)data_dev, D, (float *)out_dev));
    else MSM_TRY(tiles<double>(p, (const double *)data_dev, D, (double *)out_dev));
    return ctx_sync(p->ctx);  // the caller's buffers are free for any stream on return (the stream contract, msmhip.h)
}

int msm_resample_plan_apply_labels(msm_resample_plan *p, const int32_t *labels, int64_t D, int32_t unassigned, int32_t *out) {
    if (!p) return fail(MSM_ERR_INVALID, "msm_resample_plan_apply_labels: null plan");
    if (D < 0) return fail(MSM_ERR_INVALID, "msm_resample_plan_apply_labels: D = %lld rows", (long long)D);
    if (p->method == MSM_RESAMPLE_SMOOTH) return fail(MSM_ERR_INVALID, "msm_resample_plan_apply_labels: a smoothing plan takes no labels (a Gaussian vote is not defined)");
    if (D > 0 && (!labels || !out)) return fail(MSM_ERR_INVALID, "msm_resample_plan_apply_labels: null array with D = %lld", (long long)D);
    if (D == 0) return MSM_OK;
    msm_ctx *ctx = p->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    const size_t nOld = (size_t)p->nOld, nNew = (size_t)p->nNew;
    int64_t S = slab_maps(p, sizeof(int32_t), D);
    S = std::max<int64_t>(1, std::min<int64_t>(S, ((int64_t)1 << 33) / std::max<int64_t>(p->nNew, 1)));  // 16 lanes per (row, vertex): a launch's grid stays inside 31 bits
    if (p->in.ensure(std::max<size_t>((size_t)S * nOld, 1) * sizeof(int32_t)) || p->out.ensure(std::max<size_t>((size_t)S * nNew, 1) * sizeof(int32_t)))
        return stage_alloc_failed((size_t)S * (nOld + nNew) * sizeof(int32_t));
    for (int64_t d0 = 0; d0 < D; d0 += S) {
        const int64_t n = std::min(S, D - d0);
        MSM_TRY(stage_h2d(ctx, p->in.p, labels + (size_t)d0 * nOld, (size_t)n * nOld * sizeof(int32_t)));
        MSM_TRY(launch_plan_labels(ctx, p->rows(), (const int32_t *)p->in.p, (int)n, unassigned, (int32_t *)p->out.p));
        MSM_TRY(stage_d2h(ctx, out + (size_t)d0 * nNew, p->out.p, (size_t)n * nNew * sizeof(int32_t)));
        MSM_TRY(ctx_sync(ctx));
    }
    return MSM_OK;
}

}  // extern "C"
