// vertex_strains.cpp -- calculate_strains (M/reg_tools.cpp:498-549) behind the C ABI: the per-vertex principal stretches of an aMSM run's
// anatomy (save_transformed_data, M/mesh_registration.cpp:397-407).  Validation, the grid's shape and the copies are here; everything per
// vertex is on the device (vertex_strain_kernels.hip).
//
// What the reference does and this does not: the O(V^2) scan of every vertex against every vertex, repeated each time the fit radius grows.  A
// uniform grid built on the device picks the candidates, and one pass per vertex finds the radius at which the repeated scan would stop; the
// members are then those of the reference's exact tests at that radius (vertex_strain_kernels.hip).
#include <algorithm>
#include <cmath>
#include <vector>

#include "vertex_strains.hpp"

using namespace msm;

namespace {

constexpr double kRadiusStep = 0.5;         // fit_temp += 0.5 (M/reg_tools.cpp:541)
constexpr double kMaxRadiusSteps = 1e7;     // a mesh whose extent would need more of them is refused (the per-vertex loop stays short)

struct StrainBufs {
    DevBuf<double> fin, nrm, sxyz, snrm, sfin, radius, strains;
    DevBuf<int32_t> cell, cnt, start, cursor, svid, kept;
};

// the grid's shape: cells of the fit radius' size, coarsened until there are at most 4 V + 1024 of them
StrainGrid grid_of(const double *xyz, int V, double fit_radius, int *C) {
    double lo[3], hi[3];
    for (int d = 0; d < 3; ++d) {
        lo[d] = hi[d] = xyz[(size_t)d * V];
        for (int i = 1; i < V; ++i) {
            lo[d] = std::min(lo[d], xyz[(size_t)d * V + i]);
            hi[d] = std::max(hi[d], xyz[(size_t)d * V + i]);
        }
    }
    const double cap = 4.0 * V + 1024.0;
    double h = fit_radius;
    double n[3];
    for (;;) {
        for (int d = 0; d < 3; ++d) n[d] = std::floor((hi[d] - lo[d]) / h) + 1;
        if (n[0] * n[1] * n[2] <= cap) break;
        h *= 1.5;
    }
    StrainGrid g;
    g.x0 = lo[0], g.y0 = lo[1], g.z0 = lo[2];
    g.inv_h = 1.0 / h;
    g.nx = (int)n[0], g.ny = (int)n[1], g.nz = (int)n[2];
    *C = g.nx * g.ny * g.nz;
    return g;
}

int calculate_strains(msm_mesh *orig, const double *final_xyz, double fit_radius, double *strains, int32_t *kept, double *radius) {
    msm_ctx *ctx = orig->ctx;
    const int V = orig->V;
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    MSM_TRY(refresh_host_xyz(orig, ctx));
    const double *x = orig->xyz.data();
    double extent = 0.0;
    for (int d = 0; d < 3; ++d) {
        double lo = x[(size_t)d * V], hi = lo;
        for (int i = 0; i < V; ++i) {
            const double v = x[(size_t)d * V + i];
            if (!std::isfinite(v)) return fail(MSM_ERR_INVALID, "msm_calculate_strains: vertex %d of the original mesh is not finite", i);
            lo = std::min(lo, v), hi = std::max(hi, v);
        }
        extent += hi - lo;
    }
    if (extent / kRadiusStep > kMaxRadiusSteps)
        return fail(MSM_ERR_INVALID, "msm_calculate_strains: the original mesh spans %g, too far for fit-radius steps of %g", extent, kRadiusStep);
    for (size_t k = 0; k < 3 * (size_t)V; ++k)
        if (!std::isfinite(final_xyz[k])) return fail(MSM_ERR_INVALID, "msm_calculate_strains: vertex %d of the final mesh is not finite", (int)(k % V));
    MSM_TRY(ensure_adjacency_dev(orig));

    int C = 0;
    StrainBufs b;
    StrainArgs a;
    a.g = grid_of(x, V, fit_radius, &C);
    a.V = V;
    a.T = orig->T;
    a.orig = orig->d_xyz.p;
    a.tri = orig->d_tri.p;
    a.tid_ptr = orig->d_tid_ptr.p;
    a.tid = orig->d_tid.p;
    a.fit_radius = fit_radius;
    MSM_TRY(b.fin.upload(final_xyz, 3 * (size_t)V, ctx));
    const size_t v3 = 3 * (size_t)V;
    if (b.nrm.ensure(v3) || b.sxyz.ensure(v3) || b.snrm.ensure(v3) || b.sfin.ensure(v3) || b.radius.ensure(V) || b.strains.ensure(4 * (size_t)V) ||
        b.cell.ensure(V) || b.svid.ensure(V) || b.kept.ensure(V) || b.cnt.ensure(C) || b.start.ensure((size_t)C + 1) || b.cursor.ensure(C))
        return stage_alloc_failed(sizeof(double) * (13 * (size_t)V) + sizeof(int32_t) * (3 * (size_t)V + 3 * (size_t)C));
    a.fin = b.fin.p;
    a.nrm = b.nrm.p;
    a.cell = b.cell.p;
    a.cnt = b.cnt.p;
    a.start = b.start.p;
    a.cursor = b.cursor.p;
    a.svid = b.svid.p;
    a.sxyz = b.sxyz.p;
    a.snrm = b.snrm.p;
    a.sfin = b.sfin.p;
    a.radius = b.radius.p;
    a.kept = b.kept.p;
    a.strains = b.strains.p;
    MSM_TRY(launch_vertex_strains(ctx, a, C));

    std::vector<int32_t> k_host;
    std::vector<double> r_host;
    int32_t *k_out = kept;
    double *r_out = radius;
    if (!k_out) k_host.resize(V), k_out = k_host.data();
    if (!r_out) r_host.resize(V), r_out = r_host.data();
    MSM_TRY(b.strains.download(strains, 4 * (size_t)V, ctx));
    MSM_TRY(b.kept.download(k_out, V, ctx));
    MSM_TRY(b.radius.download(r_out, V, ctx));
    MSM_TRY(check_status(ctx, "msm_calculate_strains"));
    for (int i = 0; i < V; ++i)
        if (r_out[i] < 0)
            return fail(MSM_ERR_INVALID,
                        "msm_calculate_strains: vertex %d has %d vertices whose normals face its own, never the 9 a local fit needs (the reference's "
                        "radius would grow forever)",
                        i, k_out[i]);
    return MSM_OK;
}

}  // namespace

extern "C" {

int msm_calculate_strains(msm_mesh *orig, const double *final_xyz, int32_t V, double fit_radius, double *strains, int32_t *kept, double *radius) {
    if (!orig || !final_xyz || !strains) return fail(MSM_ERR_INVALID, "msm_calculate_strains: null argument");
    if (V != orig->V) return fail(MSM_ERR_INVALID, "msm_calculate_strains: the final mesh has %d vertices, the original %d", V, orig->V);
    if (!(fit_radius > 0) || !std::isfinite(fit_radius)) return fail(MSM_ERR_INVALID, "msm_calculate_strains: fit radius %g (must be > 0)", fit_radius);
    return calculate_strains(orig, final_xyz, fit_radius, strains, kept, radius);
}

}  // extern "C"
