// rigid.cpp -- the rigid level (Rigid_cost_function, M/rigid_costfunction.cpp) behind the C ABI: set-up, the cost launches and the
// optimiser's control flow (run, :164-228), which stays on the host and reads back B doubles per launch.
//
// What the reference keeps and this does not: the per-vertex Neighbourhood (an O(V^2) build at initialise, M/reg_tools.cpp:31-57) and the
// sparse similarity matrix rewritten on every evaluation.  Neither changes a result: SOURCE equals TARGET at initialise, so every vertex has
// neighbours (nrows(i) > 0); Evaluate_SIMGradient replaces the list with get_all_neighbours of the closest triangle every time, which depends
// on that triangle only; and sim(q, i) depends only on the data.  So the query lists are built once per target triangle and the similarities
// are computed where they are used (rigid_kernels.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.hpp"
#include "rigid.hpp"

using namespace msm;

struct msm_rigid {
    msm_ctx *ctx = nullptr;
    msm_mesh *target = nullptr;
    int V = 0, Ts = 0, Vt = 0, D = 0, sim = 0;
    double min_sigma = 0.0;
    DevBuf<double> src, saved, rot, val, sums, fin, fref, mean_in, mean_ref;
    DevBuf<int32_t> stri, stid_ptr, stid, qptr, qidx;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double kernel_ms = 0.0;
    int launches = 0;
};

namespace {

// meanvector (M/similarities.cpp:100-120) of a D x n matrix: one global mean for a single row, the per-column mean otherwise
std::vector<double> mean_vector(const double *f, int D, int n) {
    std::vector<double> m((size_t)n, 0.0);
    if (D == 1) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += f[i];
        for (int i = 0; i < n; ++i) m[i] = sum / n;
    } else {
        for (int i = 0; i < n; ++i) {
            double sum = 0.0;
            for (int d = 0; d < D; ++d) sum += f[(size_t)d * n + i];
            m[i] = sum / D;
        }
    }
    return m;
}

std::vector<double> vertex_major(const double *f, int D, int n) {
    std::vector<double> out((size_t)D * n);
    for (int d = 0; d < D; ++d)
        for (int i = 0; i < n; ++i) out[(size_t)i * D + d] = f[(size_t)d * n + i];
    return out;
}

// euler_rotate's matrix (R/point.cpp:154-165), row-major, from libm sin / cos
void euler_matrix(double w1, double w2, double w3, double *R) {
    R[0] = std::cos(w2) * std::cos(w3);
    R[1] = -std::cos(w1) * std::sin(w3) + std::sin(w1) * std::sin(w2) * std::cos(w3);
    R[2] = std::sin(w1) * std::sin(w3) + std::cos(w1) * std::sin(w2) * std::cos(w3);
    R[3] = std::cos(w2) * std::sin(w3);
    R[4] = std::cos(w1) * std::cos(w3) + std::sin(w1) * std::sin(w2) * std::sin(w3);
    R[5] = -std::sin(w1) * std::cos(w3) + std::cos(w1) * std::sin(w2) * std::sin(w3);
    R[6] = -std::sin(w2);
    R[7] = std::sin(w1) * std::cos(w2);
    R[8] = std::cos(w1) * std::cos(w2);
}

RigidEvalArgs eval_args(msm_rigid *r) {
    RigidEvalArgs a;
    a.tree = dev_tree(r->target);
    if (!a.tree.simple) a.tree.ray_G = 0;  // the direction table vouches for simple surfaces only
    a.src = r->src.p;
    a.rot = r->rot.p;
    a.V = r->V;
    a.stri = r->stri.p;
    a.Ts = r->Ts;
    a.stid_ptr = r->stid_ptr.p;
    a.stid = r->stid.p;
    a.txyz = r->target->d_xyz.p;
    a.Vt = r->Vt;
    a.qptr = r->qptr.p;
    a.qidx = r->qidx.p;
    a.fin = r->fin.p;
    a.fref = r->fref.p;
    a.mean_in = r->mean_in.p;
    a.mean_ref = r->mean_ref.p;
    a.D = r->D;
    a.sim = r->sim;
    a.two_sig2 = 2 * r->min_sigma * r->min_sigma;
    a.val = r->val.p;
    a.status = r->ctx->d_status;
    return a;
}

// B <= kRigidMaxProbes cost evaluations of the current SOURCE in one launch; sums (host) complete on return, per_vertex (B x V) when given
int eval_probes(msm_rigid *r, const double *euler, int B, double *sums, double *per_vertex) {
    msm_ctx *ctx = r->ctx;
    MSM_TRY(ensure_tree(r->target));
    RigidRot R;
    for (int b = 0; b < B; ++b) euler_matrix(euler[3 * b], euler[3 * b + 1], euler[3 * b + 2], R.r[b]);
    void *pin = nullptr;
    MSM_TRY(ctx_io_pinned(ctx, sizeof(double) * kRigidMaxProbes, &pin));
    MSM_HIP(hipEventRecord(r->ev0, ctx->stream));
    MSM_TRY(launch_rigid_eval(ctx, eval_args(r), R, B, r->sums.p));
    MSM_HIP(hipEventRecord(r->ev1, ctx->stream));
    MSM_HIP(hipMemcpyAsync(pin, r->sums.p, sizeof(double) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (per_vertex) MSM_TRY(r->val.download(per_vertex, (size_t)B * r->V, ctx));
    MSM_TRY(check_status(ctx, "rigid_cost_mesh"));
    std::memcpy(sums, pin, sizeof(double) * B);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r->ev0, r->ev1) == hipSuccess) r->kernel_ms += ms;
    ++r->launches;
    return MSM_OK;
}

int rotate_source(msm_rigid *r, double w1, double w2, double w3) {
    RigidRot R;
    euler_matrix(w1, w2, w3, R.r[0]);
    return launch_rigid_rotate(r->ctx, r->src.p, r->saved.p, r->V, R);
}

int restore_source(msm_rigid *r) {
    MSM_HIP(hipMemcpyAsync(r->src.p, r->saved.p, sizeof(double) * 3 * (size_t)r->V, hipMemcpyDeviceToDevice, r->ctx->stream));
    return MSM_OK;
}

int rigid_create(msm_rigid *r, msm_mesh *target, msm_mesh *source, const double *in_feat, const double *ref_feat) {
    msm_ctx *ctx = r->ctx;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MSM_HIP(hipEventCreate(&r->ev0));
    MSM_HIP(hipEventCreate(&r->ev1));
    // calculate_MeanVD of SOURCE (R/mesh.cpp:276-293): every vertex's neighbours in the mesh's order
    Adjacency sa;
    build_adjacency(source->tri.data(), r->V, r->Ts, sa);
    const double *x = source->xyz.data();
    const int V = r->V;
    int k = 0;
    double kr = 0.0;
    for (int i = 0; i < V; ++i) {
        const V3 sp = mk(x[i], x[V + i], x[2 * V + i]);
        for (int j = sa.nbr_ptr[i]; j < sa.nbr_ptr[i + 1]; ++j) {
            const int n = sa.nbr[j];
            ++k;
            kr += norm(sub(mk(x[n], x[V + n], x[2 * V + n]), sp));
        }
    }
    if (k == 0) return fail(MSM_ERR_INVALID, "msm_rigid_create: the source mesh has no edges");
    r->min_sigma = kr / k;
    // get_all_neighbours (M/rigid_costfunction.cpp:141-162) of every TARGET triangle: its corners in order, each corner's triangles in trID
    // order, the three vertices of each, every vertex once
    Adjacency ta;
    const int Tt = target->T;
    build_adjacency(target->tri.data(), r->Vt, Tt, ta);
    std::vector<int32_t> qptr((size_t)Tt + 1, 0), qidx, seen((size_t)r->Vt, -1);
    qidx.reserve((size_t)Tt * 12);
    for (int t = 0; t < Tt; ++t) {
        for (int c = 0; c < 3; ++c) {
            const int corner = target->tri[(size_t)c * Tt + t];
            for (int j = ta.tid_ptr[corner]; j < ta.tid_ptr[corner + 1]; ++j) {
                const int tt = ta.tid[j];
                for (int v = 0; v < 3; ++v) {
                    const int q = target->tri[(size_t)v * Tt + tt];
                    if (seen[q] != t) {
                        seen[q] = t;
                        qidx.push_back(q);
                    }
                }
            }
        }
        qptr[t + 1] = (int32_t)qidx.size();
    }
    MSM_TRY(r->qptr.upload_vec(qptr, ctx));
    MSM_TRY(r->qidx.upload_vec(qidx, ctx));
    MSM_TRY(r->stri.upload_vec(source->tri, ctx));
    MSM_TRY(r->stid_ptr.upload_vec(sa.tid_ptr, ctx));
    MSM_TRY(r->stid.upload_vec(sa.tid, ctx));
    MSM_TRY(r->src.upload_vec(source->xyz, ctx));
    if (r->saved.ensure(3 * (size_t)V) != hipSuccess) return stage_alloc_failed(sizeof(double) * 3 * (size_t)V);
    if (r->rot.ensure((size_t)kRigidMaxProbes * 3 * V) != hipSuccess) return stage_alloc_failed(sizeof(double) * kRigidMaxProbes * 3 * (size_t)V);
    if (r->val.ensure((size_t)kRigidMaxProbes * V) != hipSuccess) return stage_alloc_failed(sizeof(double) * kRigidMaxProbes * (size_t)V);
    if (r->sums.ensure(kRigidMaxProbes) != hipSuccess) return stage_alloc_failed(sizeof(double) * kRigidMaxProbes);
    MSM_TRY(r->fin.upload_vec(vertex_major(in_feat, r->D, V), ctx));
    MSM_TRY(r->fref.upload_vec(vertex_major(ref_feat, r->D, r->Vt), ctx));
    MSM_TRY(r->mean_in.upload_vec(mean_vector(in_feat, r->D, V), ctx));
    MSM_TRY(r->mean_ref.upload_vec(mean_vector(ref_feat, r->D, r->Vt), ctx));
    MSM_TRY(ensure_tree(target));
    MSM_TRY(ensure_rays(target, true));
    return check_status(ctx, "msm_rigid_create");
}

}  // namespace

extern "C" {

msm_rigid *msm_rigid_create(msm_ctx *ctx, msm_mesh *target, msm_mesh *source, const double *in_feat, const double *ref_feat, int32_t D,
                            int32_t simmeasure) {
    if (!ctx || !target || !source || !in_feat || !ref_feat || D <= 0) {
        fail(MSM_ERR_INVALID, "msm_rigid_create: bad arguments");
        return nullptr;
    }
    if (target->ctx != ctx || source->ctx != ctx) {
        fail(MSM_ERR_INVALID, "msm_rigid_create: meshes belong to another context");
        return nullptr;
    }
    if (simmeasure != 1 && simmeasure != 2) {
        fail(MSM_ERR_INVALID, "msm_rigid_create: simmeasure %d (the rigid level computes 1 SSD or 2 correlation)", simmeasure);
        return nullptr;
    }
    if (source->V <= 0 || source->T <= 0 || target->V <= 0 || target->T <= 0) {
        fail(MSM_ERR_INVALID, "msm_rigid_create: empty mesh");
        return nullptr;
    }
    msm_rigid *r = new msm_rigid();
    r->ctx = ctx;
    r->target = target;
    r->V = source->V;
    r->Ts = source->T;
    r->Vt = target->V;
    r->D = D;
    r->sim = simmeasure;
    if (rigid_create(r, target, source, in_feat, ref_feat) != MSM_OK) {
        const std::string msg = msm_last_error();
        msm_rigid_destroy(r);
        set_error("%s", msg.c_str());
        return nullptr;
    }
    return r;
}

void msm_rigid_destroy(msm_rigid *r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    (void)hipStreamSynchronize(r->ctx->stream);
    if (r->ev0) (void)hipEventDestroy(r->ev0);
    if (r->ev1) (void)hipEventDestroy(r->ev1);
    delete r;
}

int msm_rigid_set_source(msm_rigid *r, const double *xyz) {
    if (!r || !xyz) return fail(MSM_ERR_INVALID, "msm_rigid_set_source: null argument");
    MSM_HIP(hipSetDevice(r->ctx->device));
    MSM_TRY(drop_ctx_pending(r->ctx));
    MSM_TRY(r->src.upload(xyz, 3 * (size_t)r->V, r->ctx));
    return ctx_sync(r->ctx);
}

int msm_rigid_get_source(msm_rigid *r, double *xyz) {
    if (!r || !xyz) return fail(MSM_ERR_INVALID, "msm_rigid_get_source: null argument");
    MSM_HIP(hipSetDevice(r->ctx->device));
    MSM_TRY(drop_ctx_pending(r->ctx));
    MSM_TRY(r->src.download(xyz, 3 * (size_t)r->V, r->ctx));
    return check_status(r->ctx, "msm_rigid_get_source");
}

int msm_rigid_cost(msm_rigid *r, const double *euler, int32_t n, double *sums, double *per_vertex) {
    if (!r || !euler || !sums || n < 0) return fail(MSM_ERR_INVALID, "msm_rigid_cost: bad arguments");
    MSM_HIP(hipSetDevice(r->ctx->device));
    MSM_TRY(drop_ctx_pending(r->ctx));
    r->kernel_ms = 0.0;
    r->launches = 0;
    for (int k0 = 0; k0 < n; k0 += kRigidMaxProbes) {
        const int B = std::min(kRigidMaxProbes, n - k0);
        MSM_TRY(eval_probes(r, euler + 3 * (size_t)k0, B, sums + k0, per_vertex ? per_vertex + (size_t)k0 * r->V : nullptr));
    }
    return MSM_OK;
}

int msm_rigid_rotate(msm_rigid *r, const double euler[3]) {
    if (!r || !euler) return fail(MSM_ERR_INVALID, "msm_rigid_rotate: bad arguments");
    MSM_HIP(hipSetDevice(r->ctx->device));
    MSM_TRY(drop_ctx_pending(r->ctx));
    MSM_TRY(rotate_source(r, euler[0], euler[1], euler[2]));
    return check_status(r->ctx, "msm_rigid_rotate");
}

int msm_rigid_run(msm_rigid *r, int32_t iters, double stepsize, double gradsampling, double *trace, int32_t cap, int32_t *n, double summary[3]) {
    if (!r || iters < 0 || cap < 0 || (cap > 0 && !trace)) return fail(MSM_ERR_INVALID, "msm_rigid_run: bad arguments");
    MSM_HIP(hipSetDevice(r->ctx->device));
    MSM_TRY(drop_ctx_pending(r->ctx));
    r->kernel_ms = 0.0;
    r->launches = 0;
    double Euler1 = 0.0, Euler2 = 0.0, Euler3 = 0.0, RECfinal = 0.0;
    int min_iter = 0, loop = 0, rows = 0;
    long long evals = 0;
    double spacing = gradsampling;
    double zero[3] = {Euler1, Euler2, Euler3};
    double grad_zero;
    MSM_TRY(eval_probes(r, zero, 1, &grad_zero, nullptr));
    ++evals;
    double mingrad_zero = grad_zero;
    const double RECinit = grad_zero;
    while (spacing > 0.05) {
        double step = stepsize;
        const double per = spacing;
        for (int it = 1; it <= iters; ++it) {
            Euler1 = 0.0, Euler2 = 0.0, Euler3 = 0.0;
            const double probes[9] = {Euler1 + per, Euler2, Euler3, Euler1, Euler2 + per, Euler3, Euler1, Euler2, Euler3 + per};
            double s[3];
            MSM_TRY(eval_probes(r, probes, 3, s, nullptr));
            evals += 3;
            V3 grad = mk((s[0] - grad_zero) / per, (s[1] - grad_zero) / per, (s[2] - grad_zero) / per);
            grad = normalized(grad);
            Euler1 += step * grad.x;
            Euler2 += step * grad.y;
            Euler3 += step * grad.z;
            const double step_taken = step;
            MSM_TRY(rotate_source(r, Euler1, Euler2, Euler3));  // the previous SOURCE stays in `saved` for the restore
            const double e[3] = {Euler1, Euler2, Euler3};
            MSM_TRY(eval_probes(r, e, 1, &grad_zero, nullptr));  // evaluated at the doubly rotated mesh, as the reference does
            ++evals;
            if (grad_zero > mingrad_zero) {
                mingrad_zero = grad_zero;
                min_iter = loop * iters + it;
                RECfinal = mingrad_zero;
            }
            const bool rejected = loop * iters + it - min_iter > 0;
            if (rejected) {
                step *= 0.5;
                MSM_TRY(restore_source(r));  // grad_zero keeps the rejected value
            }
            if (rows < cap) {
                double *row = trace + 6 * (size_t)rows;
                row[0] = loop, row[1] = it, row[2] = per, row[3] = step_taken, row[4] = grad_zero, row[5] = rejected ? 0.0 : 1.0;
            }
            ++rows;
            if (step < 1e-3) break;
        }
        ++loop;
        spacing *= 0.5;
    }
    MSM_TRY(check_status(r->ctx, "msm_rigid_run"));
    if (n) *n = rows;
    if (summary) summary[0] = RECinit, summary[1] = RECfinal, summary[2] = (double)evals;
    return MSM_OK;
}

int msm_rigid_kernel_ms(msm_rigid *r, double ms[2]) {
    if (!r || !ms) return fail(MSM_ERR_INVALID, "msm_rigid_kernel_ms: bad arguments");
    ms[0] = r->kernel_ms;
    ms[1] = r->launches;
    return MSM_OK;
}

}  // extern "C"
