// resample.cpp -- the host side of the adaptive-barycentric resampler (resample.hpp): the scratch of the device surgery, the weights of a mesh pair on
// the device or (with an exclusion mask) through the host surgery, and the entry points msm_adaptive_barycentric_weights / msm_metric_resample.
// adaptive_weights_dev_masked queues the masked surgery on the device for msm_level_features (features.cpp); the two entry points keep the host surgery.
#include <algorithm>
#include <cstring>
#include <memory>

#include "devbuf.hpp"
#include "kernels.hpp"
#include "resample.hpp"

using namespace msm;

namespace msm {

namespace {

// entries a problem's result (and its columns, and the long-list sort's copy) can have: a row is the forward list, at most 3, or the transposed reverse
// list, whose lengths add up to at most 3 nOld
size_t row_cap(int nOld, int nNew) { return 3 * (size_t)nNew + 3 * (size_t)nOld; }
size_t scan_len(int nOld, int nNew) { return (size_t)std::max(nNew, nOld) / 4096 + 2; }

}  // namespace

int SurgeryScratch::ensure(int nOld, int nNew, int Told, int Tnew, int B) {
    const size_t b = (size_t)B, bOld = b * nOld, bNew = b * nNew, cap = b * row_cap(nOld, nNew);
    MSM_HIP(fvid.ensure(3 * bNew));
    MSM_HIP(fw.ensure(3 * bNew));
    MSM_HIP(rvid.ensure(3 * bOld));
    MSM_HIP(rw.ensure(3 * bOld));
    MSM_HIP(oldA.ensure(bOld));
    MSM_HIP(newA.ensure(nNew));
    MSM_HIP(ta.ensure(b * std::max(Told, Tnew)));
    MSM_HIP(counters.ensure(2 * bNew + 2 * bOld + 4 * b));
    MSM_HIP(rkey.ensure(3 * bOld));
    MSM_HIP(rwt.ensure(3 * bOld));
    MSM_HIP(ckey.ensure(cap));
    MSM_HIP(cval.ensure(cap));
    MSM_HIP(correction.ensure(bOld));
    MSM_HIP(row_ptr.ensure(bNew + b));
    MSM_HIP(col.ensure(cap));
    MSM_HIP(val.ensure(cap));
    MSM_HIP(tkey.ensure(cap));
    MSM_HIP(tval.ensure(cap));
    MSM_HIP(scan_tmp.ensure(b * scan_len(nOld, nNew)));
    return MSM_OK;
}

AdaptiveDevArgs SurgeryScratch::args(int nOld, int nNew, int B) const {
    const size_t b = (size_t)B, o = (size_t)nOld, n = (size_t)nNew;
    AdaptiveDevArgs a;
    a.nOld = nOld, a.nNew = nNew, a.B = B;
    a.fvid = fvid.p, a.fw = fw.p, a.rvid = rvid.p, a.rw = rw.p, a.oldA = oldA.p, a.newA = newA.p;
    a.roff = counters.p, a.rfill = a.roff + b * (n + 1), a.coff = a.rfill + b * n, a.cfill = a.coff + b * (o + 1), a.long_flag = a.cfill + b * o;
    a.rkey = rkey.p, a.rwt = rwt.p;
    a.ckey = ckey.p, a.cval = cval.p, a.correction = correction.p;
    a.row_ptr = row_ptr.p, a.col = col.p, a.val = val.p, a.tkey = tkey.p, a.tval = tval.p, a.scan_tmp = scan_tmp.p;
    a.fstride = b * n, a.rstride = b * o;
    a.s_f = n, a.s_r = o, a.s_oldA = o, a.s_newA = 0;  // (the new mesh's areas are shared)
    a.s_roff = n + 1, a.s_rfill = n, a.s_r3 = 3 * o;
    a.s_coff = o + 1, a.s_cfill = o, a.s_cap = row_cap(nOld, nNew), a.s_corr = o, a.s_rowptr = n + 1, a.s_scan = scan_len(nOld, nNew);
    return a;
}

namespace {

// compute_vertex_area for every vertex (R/mesh.cpp:1275-1283): mean area of the adjacent faces, in trID order
void vertex_areas_of(const double *xyz, const int32_t *tri, int V, int T, const Adjacency &a, std::vector<double> &area) {
    std::vector<double> ta(T);
    auto pt = [&](int i) { return mk(xyz[i], xyz[V + i], xyz[2 * V + i]); };
    for (int t = 0; t < T; ++t) ta[t] = tri_area(pt(tri[t]), pt(tri[T + t]), pt(tri[2 * T + t]));
    area.resize(V);
    for (int v = 0; v < V; ++v) {
        double sum = 0;
        for (int j = a.tid_ptr[v]; j < a.tid_ptr[v + 1]; ++j) sum += ta[a.tid[j]];
        area[v] = sum / (a.tid_ptr[v + 1] - a.tid_ptr[v]);
    }
}

int vertex_areas(msm_mesh *m, std::vector<double> &area) {
    vertex_areas_of(m->xyz.data(), m->tri.data(), m->V, m->T, mesh_adjacency(m), area);
    return MSM_OK;
}

// Resampler::get_adaptive_barycentric_weights, R/resampler.cpp:72-140, the variant with an exclusion mask (or meshes of two
// contexts), in two halves: the 2 x N nearest-triangle queries run on the GPU (adaptive_queries); the list
// surgery (transpose, pick, area correction) is done on the host in the reference's serial order so that every sum has the
// same operand order (adaptive_surgery: touches no handle).  Without a mask everything runs on the device: adaptive_weights_dev below.
struct AdaptiveQueries {
    std::vector<int> fvid, rvid, closest;  // forward (new -> old) and reverse (old -> new) hit-triangle vertex ids, 3 x N SoA
    std::vector<double> fw, rw;            // and their projected barycentric weights
};
int adaptive_queries(msm_mesh *in_mesh, msm_mesh *new_mesh, bool with_closest, AdaptiveQueries &q) {
    const int nOld = in_mesh->V, nNew = new_mesh->V;
    q.fvid.resize(3 * (size_t)nNew);
    q.rvid.resize(3 * (size_t)nOld);
    q.fw.resize(3 * (size_t)nNew);
    q.rw.resize(3 * (size_t)nOld);
    // the query points are the other mesh's vertices, which its handle keeps in HBM (same context, same stream)
    const bool same_ctx = in_mesh->ctx == new_mesh->ctx;
    int st = query_host(in_mesh, new_mesh->xyz.data(), nNew, nullptr, q.fvid.data(), q.fw.data(), MSM_WEIGHTS_PROJECTED, "adaptive weights (forward)",
                        same_ctx ? new_mesh->d_xyz.p : nullptr);
    if (st) return st;
    st = query_host(new_mesh, in_mesh->xyz.data(), nOld, nullptr, q.rvid.data(), q.rw.data(), MSM_WEIGHTS_PROJECTED, "adaptive weights (reverse)",
                        same_ctx ? in_mesh->d_xyz.p : nullptr);
    if (st) return st;
    q.closest.clear();
    if (with_closest) {
        q.closest.resize(nNew);
        msm_ctx *ctx = in_mesh->ctx;
        DevBuf<double> dq;
        DevBuf<int> dout;
        MSM_TRY(dq.upload(new_mesh->xyz.data(), 3 * (size_t)nNew, ctx));
        MSM_HIP(dout.ensure(nNew));
        st = launch_closest_vertex(ctx, dev_tree(in_mesh), dq.p, nNew, dout.p);
        if (st) return st;
        MSM_TRY(dout.download(q.closest.data(), nNew, ctx));
        st = check_status(ctx, "adaptive weights (exclusion)");
        if (st) return st;
    }
    return MSM_OK;
}

void adaptive_surgery(const AdaptiveQueries &q, int nOld, int nNew, const std::vector<double> &oldA, const std::vector<double> &newA,
                      const double *excl, std::vector<int32_t> &row_ptr, std::vector<int32_t> &col, std::vector<double> &val) {
    const std::vector<int> &fvid = q.fvid, &rvid = q.rvid, &closest = q.closest;
    const std::vector<double> &fw = q.fw, &rw = q.rw;
    // reverse lists transposed: for each new vertex the old vertices whose triangle contains it (:91-97);
    // old vertices are visited in ascending order, so each list is already sorted by key
    std::vector<int32_t> rcount(nNew + 1, 0);
    for (int o = 0; o < nOld; ++o) {
        WeightEntry e[3];
        const int n = small_map(rvid.data(), rw.data(), nOld, o, e);
        for (int j = 0; j < n; ++j) rcount[e[j].key + 1]++;
    }
    for (int k = 0; k < nNew; ++k) rcount[k + 1] += rcount[k];
    std::vector<WeightEntry> rlist(rcount[nNew]);
    {
        std::vector<int32_t> fill(rcount.begin(), rcount.end() - 1);
        for (int o = 0; o < nOld; ++o) {
            WeightEntry e[3];
            const int n = small_map(rvid.data(), rw.data(), nOld, o, e);
            for (int j = 0; j < n; ++j) rlist[fill[e[j].key]++] = WeightEntry{o, e[j].w};
        }
    }
    row_ptr.assign(nNew + 1, 0);
    col.clear();
    val.clear();
    std::vector<double> correction(nOld, 0.0);
    std::vector<char> active(nNew, 0);
    for (int k = 0; k < nNew; ++k) {  // :99-118
        row_ptr[k] = (int32_t)col.size();
        if (excl && !(closest[k] >= 0 && excl[closest[k]] != 0)) continue;
        active[k] = 1;
        WeightEntry f[3];
        const int nf = small_map(fvid.data(), fw.data(), nNew, k, f);
        const int nr = rcount[k + 1] - rcount[k];
        const WeightEntry *src = (nr <= nf) ? f : &rlist[rcount[k]];
        const int n = (nr <= nf) ? nf : nr;
        for (int j = 0; j < n; ++j) {
            const double wgt = src[j].w * newA[k];
            col.push_back(src[j].key);
            val.push_back(wgt);
            correction[src[j].key] += wgt;
        }
    }
    row_ptr[nNew] = (int32_t)col.size();
    for (int k = 0; k < nNew; ++k) {  // :120-137
        if (!active[k]) continue;
        double wsum = 0.0;
        for (int e = row_ptr[k]; e < row_ptr[k + 1]; ++e) {
            val[e] *= oldA[col[e]] / correction[col[e]];
            wsum += val[e];
        }
        if (wsum != 0.0)
            for (int e = row_ptr[k]; e < row_ptr[k + 1]; ++e) val[e] /= wsum;
    }
}

// per context, kept between calls (msm_ctx::resample_scratch)
struct ResampleScratch {
    SurgeryScratch surgery;
    DevBuf<double> data, out;  // msm_metric_resample: the maps in and out
    DevBuf<int> closest;       // the masked device surgery: the old vertex closest to every new vertex
};
ResampleScratch &resample_scratch(msm_ctx *ctx) {
    if (!ctx->resample_scratch) ctx->resample_scratch = std::shared_ptr<void>(new ResampleScratch(), [](void *p) { delete static_cast<ResampleScratch *>(p); });
    return *static_cast<ResampleScratch *>(ctx->resample_scratch.get());
}

}  // namespace

// d_excl: nullptr, or the mask of adaptive_weights_dev_masked
static int adaptive_weights_queue(msm_mesh *in_mesh, msm_mesh *new_mesh, const double *d_excl, AdaptiveDev &out, bool check) {
    // Everything is queued on in_mesh's context.  new_mesh may belong to another context of the same GPU (the fallback mesh of the
    // gMSM set-up against the group's template) if its tree and adjacency are complete and synchronised: they are only read.
    const bool foreign = in_mesh->ctx != new_mesh->ctx;
    if (foreign && (in_mesh->ctx->device != new_mesh->ctx->device || !new_mesh->tree_valid || !new_mesh->d_tid_ptr.p))
        return fail(MSM_ERR_INVALID, "adaptive weights: the two meshes belong to different contexts");
    msm_ctx *ctx = in_mesh->ctx;
    const int nOld = in_mesh->V, nNew = new_mesh->V;
    int st = foreign ? ensure_tree(in_mesh) : ensure_tree_pair(in_mesh, new_mesh);
    if (st) return st;
    if ((st = ensure_adjacency_dev(in_mesh)) || (st = ensure_adjacency_dev(new_mesh))) return st;
    SurgeryScratch &s = resample_scratch(ctx).surgery;
    MSM_TRY(s.ensure(nOld, nNew, in_mesh->T, new_mesh->T, 1));
    // forward: the new mesh's vertices in the old mesh's tree; reverse: the old vertices in the new mesh's tree (:74-78)
    st = launch_query(ctx, dev_tree(in_mesh), new_mesh->d_xyz.p, nNew, nullptr, s.fvid.p, s.fw.p, MSM_WEIGHTS_PROJECTED);
    if (st) return st;
    st = launch_query(ctx, dev_tree(new_mesh), in_mesh->d_xyz.p, nOld, nullptr, s.rvid.p, s.rw.p, MSM_WEIGHTS_PROJECTED);
    if (st) return st;
    st = launch_vertex_areas(ctx, in_mesh->d_xyz.p, nOld, in_mesh->d_tri.p, in_mesh->T, in_mesh->d_tid_ptr.p, in_mesh->d_tid.p, s.ta.p, s.oldA.p);
    if (st) return st;
    st = launch_vertex_areas(ctx, new_mesh->d_xyz.p, nNew, new_mesh->d_tri.p, new_mesh->T, new_mesh->d_tid_ptr.p, new_mesh->d_tid.p, s.ta.p, s.newA.p);
    if (st) return st;
    AdaptiveDevArgs args = s.args(nOld, nNew, 1);
    if (d_excl) {  // :101: the old vertex closest to every new vertex decides whether its row takes part
        DevBuf<int> &closest = resample_scratch(ctx).closest;
        MSM_HIP(closest.ensure(nNew));
        st = launch_closest_vertex(ctx, dev_tree(in_mesh), new_mesh->d_xyz.p, nNew, closest.p);
        if (st) return st;
        args.closest = closest.p, args.excl = d_excl;
    }
    st = launch_adaptive_surgery(ctx, args);
    if (st) return st;
    if (check) {
        st = check_status(ctx, "adaptive weights");  // a failed search in either direction (synchronises)
        if (st) return st;
    }
    out.nOld = nOld, out.nNew = nNew, out.row_ptr = s.row_ptr.p, out.col = s.col.p, out.val = s.val.p;
    return MSM_OK;
}

int adaptive_weights_dev(msm_mesh *in_mesh, msm_mesh *new_mesh, AdaptiveDev &out, bool check) { return adaptive_weights_queue(in_mesh, new_mesh, nullptr, out, check); }

int adaptive_weights_dev_masked(msm_mesh *in_mesh, msm_mesh *new_mesh, const double *d_excl, AdaptiveDev &out) {
    if (!d_excl) return fail(MSM_ERR_INVALID, "adaptive weights: the masked surgery needs a mask");
    if (in_mesh->ctx != new_mesh->ctx) return fail(MSM_ERR_INVALID, "adaptive weights: the two meshes belong to different contexts");
    return adaptive_weights_queue(in_mesh, new_mesh, d_excl, out, false);
}

int reserve_surgery_scratch(msm_ctx *ctx, int nOld, int nNew, int Told, int Tnew) {
    ResampleScratch &s = resample_scratch(ctx);
    MSM_TRY(s.surgery.ensure(nOld, nNew, Told, Tnew, 1));
    MSM_HIP(s.closest.ensure(nNew));
    return MSM_OK;
}

int apply_weights_dev(msm_ctx *ctx, const AdaptiveDev &w, const double *d_data, int D, double *d_out) {
    return launch_apply_rows(ctx, w.nNew, w.nOld, D, w.row_ptr, w.col, w.val, d_data, d_out);
}

// the first half of every fetch of device rows: their offsets to the host, synchronised, so that the caller knows how many entries follow
int fetch_row_ptr(msm_ctx *ctx, const AdaptiveDev &w, std::vector<int32_t> &row_ptr, size_t &nnz) {
    row_ptr.resize((size_t)w.nNew + 1);
    MSM_TRY(stage_d2h(ctx, row_ptr.data(), w.row_ptr, sizeof(int32_t) * row_ptr.size()));
    MSM_TRY(ctx_sync(ctx));
    nnz = (size_t)row_ptr.back();
    return MSM_OK;
}

// weights as host CSR through the device surgery (no exclusion mask)
static int adaptive_weights_via_device(msm_mesh *in_mesh, msm_mesh *new_mesh, std::vector<int32_t> &row_ptr, std::vector<int32_t> &col, std::vector<double> &val) {
    AdaptiveDev w;
    int st = adaptive_weights_dev(in_mesh, new_mesh, w);
    if (st) return st;
    msm_ctx *ctx = in_mesh->ctx;
    size_t nnz = 0;
    MSM_TRY(fetch_row_ptr(ctx, w, row_ptr, nnz));
    col.resize(nnz);
    val.resize(nnz);
    if (nnz) {
        MSM_TRY(stage_d2h(ctx, col.data(), w.col, sizeof(int32_t) * nnz));
        MSM_TRY(stage_d2h(ctx, val.data(), w.val, sizeof(double) * nnz));
        MSM_TRY(ctx_sync(ctx));
    }
    return MSM_OK;
}

int adaptive_weights(msm_mesh *in_mesh, msm_mesh *new_mesh, const double *excl, std::vector<int32_t> &row_ptr,
                     std::vector<int32_t> &col, std::vector<double> &val) {
    if (!excl && in_mesh->ctx == new_mesh->ctx) return adaptive_weights_via_device(in_mesh, new_mesh, row_ptr, col, val);
    AdaptiveQueries q;
    int st = adaptive_queries(in_mesh, new_mesh, excl != nullptr, q);
    if (st) return st;
    std::vector<double> oldA, newA;
    vertex_areas(in_mesh, oldA);
    vertex_areas(new_mesh, newA);
    adaptive_surgery(q, in_mesh->V, new_mesh->V, oldA, newA, excl, row_ptr, col, val);
    return MSM_OK;
}

// barycentric_data_interpolation on the mask itself, R/resampler.cpp:54-67; a failed search (col < 0, the plan's unmasked-surgery rows) takes no part
void resampled_mask(const std::vector<int32_t> &row_ptr, const std::vector<int32_t> &col, const std::vector<double> &val, const double *excl, double *excl_out) {
    for (size_t k = 0; k + 1 < row_ptr.size(); ++k) {
        double acc = 0.0;
        for (int e = row_ptr[k]; e < row_ptr[k + 1]; ++e)
            if (col[e] >= 0 && excl[col[e]] != 0) acc += excl[col[e]] * val[e];
        excl_out[k] = acc;
    }
}

// barycentric_data_interpolation on the host, R/resampler.cpp:40-52: out (D x nNew) = the rows applied to data (D x nOld), masked columns left out
static void apply_rows_host(const std::vector<int32_t> &row_ptr, const std::vector<int32_t> &col, const std::vector<double> &val, const double *excl, const double *data,
                            int D, int nOld, double *out) {
    const int nNew = (int)row_ptr.size() - 1;
    for (int d = 0; d < D; ++d)
        for (int k = 0; k < nNew; ++k) {
            double acc = 0.0;
            for (int e = row_ptr[k]; e < row_ptr[k + 1]; ++e)
                if (!excl || excl[col[e]] != 0) acc += data[(size_t)d * nOld + col[e]] * val[e];
            out[(size_t)d * nNew + k] = acc;
        }
}

}  // namespace msm

extern "C" {

int msm_adaptive_barycentric_weights(msm_mesh *in_mesh, msm_mesh *new_mesh, const double *excl, int32_t *row_ptr, int32_t *col, double *val,
                                     int64_t cap, int64_t *nnz) {
    if (!in_mesh || !new_mesh) return fail(MSM_ERR_INVALID, "msm_adaptive_barycentric_weights: null mesh");
    std::vector<int32_t> rp, c;
    std::vector<double> v;
    int st = adaptive_weights(in_mesh, new_mesh, excl, rp, c, v);
    if (st) return st;
    if (nnz) *nnz = (int64_t)c.size();
    if (!col) return MSM_OK;
    if ((int64_t)c.size() > cap) return fail(MSM_ERR_CAPACITY, "weights need %zu entries, buffer holds %lld", c.size(), (long long)cap);
    if (row_ptr) std::copy(rp.begin(), rp.end(), row_ptr);
    std::copy(c.begin(), c.end(), col);
    if (val) std::copy(v.begin(), v.end(), val);
    return MSM_OK;
}

int msm_metric_resample(msm_mesh *in_mesh, const double *data, int32_t D, msm_mesh *new_mesh, const double *excl, double *out, double *excl_out) {
    if (!in_mesh || !new_mesh || !data || !out || D <= 0) return fail(MSM_ERR_INVALID, "msm_metric_resample: bad arguments");
    if (!excl && !excl_out && in_mesh->ctx == new_mesh->ctx) {
        // queries, list surgery and the weighted sums on the device; only the data go up and the resampled data come back
        msm_ctx *ctx = in_mesh->ctx;
        AdaptiveDev w;
        int st = adaptive_weights_dev(in_mesh, new_mesh, w);
        if (st) return st;
        ResampleScratch &s = resample_scratch(ctx);
        const size_t nin = (size_t)D * in_mesh->V, nout = (size_t)D * new_mesh->V;
        MSM_HIP(s.data.ensure(nin));
        MSM_HIP(s.out.ensure(nout));
        st = upload_staged(ctx, s.data.p, data, sizeof(double) * nin);
        if (st) return st;
        st = apply_weights_dev(ctx, w, s.data.p, D, s.out.p);
        if (st) return st;
        if (ctx_mapped(ctx, out, sizeof(double) * nout)) {  // the caller's array is pinned for this context: one copy command, no memcpy
            MSM_HIP(hipMemcpyAsync(out, s.out.p, sizeof(double) * nout, hipMemcpyDeviceToHost, ctx->stream));
            MSM_TRY(ctx_sync(ctx));
            return MSM_OK;
        }
        void *pin = nullptr;
        st = ctx_io_pinned(ctx, sizeof(double) * nout, &pin);
        if (st) return st;
        MSM_HIP(hipMemcpyAsync(pin, s.out.p, sizeof(double) * nout, hipMemcpyDeviceToHost, ctx->stream));
        MSM_TRY(ctx_sync(ctx));
        std::memcpy(out, pin, sizeof(double) * nout);
        return MSM_OK;
    }
    std::vector<int32_t> rp, c;
    std::vector<double> v;
    int st = adaptive_weights(in_mesh, new_mesh, excl, rp, c, v);
    if (st) return st;
    apply_rows_host(rp, c, v, excl, data, D, in_mesh->V, out);
    if (excl && excl_out) resampled_mask(rp, c, v, excl, excl_out);
    return MSM_OK;
}

int msm_create_exclusion(const double *data, int32_t D, int32_t V, double thrl, double thru, double *excl) {
    if (!data || !excl || D < 0 || V < 0) return fail(MSM_ERR_INVALID, "msm_create_exclusion: bad arguments");
    for (int i = 0; i < V; ++i) {
        excl[i] = 0.0;
        for (int d = 0; d < D; ++d) {
            const double x = data[(size_t)d * V + i];
            if (!(x >= (thrl - kEps) && x <= (thru + kEps))) {
                excl[i] = 1.0;
                break;
            }
        }
    }
    return MSM_OK;
}

}  // extern "C"
