// frame_device.hpp -- the per-vertex frame of the reference's local fits as device functions shared by the rigid level (rigid_kernels.hip)
// and the strain maps (vertex_strain_kernels.hip): Mesh::local_normal (R/mesh.cpp:133-141) and calculate_tangs (M/reg_tools.cpp:205-262).
#pragma once

#include "geom.hpp"

namespace msm {

__device__ __forceinline__ V3 soa_vertex(const double *xyz, int V, int i) { return mk(xyz[i], xyz[V + i], xyz[2 * (size_t)V + i]); }

// Mesh::local_normal (R/mesh.cpp:133-141): the normals (Triangle::normal) of vertex i's triangles summed in trID order, then normalised.
// xyz 3 x V SoA, tri 3 x T SoA, tid_ptr / tid the Mpoint::trID lists as CSR over vertices.
__device__ __forceinline__ V3 local_normal(const double *xyz, int V, const int32_t *tri, int T, const int32_t *tid_ptr, const int32_t *tid, int i) {
    V3 nsum = mk(0.0, 0.0, 0.0);
    for (int k = tid_ptr[i]; k < tid_ptr[i + 1]; ++k) {
        const int t = tid[k];
        const V3 v0 = soa_vertex(xyz, V, tri[t]);
        const V3 v1 = soa_vertex(xyz, V, tri[T + t]);
        const V3 v2 = soa_vertex(xyz, V, tri[2 * (size_t)T + t]);
        const V3 n = tri_normal(v0, v1, v2);
        nsum.x += n.x;
        nsum.y += n.y;
        nsum.z += n.z;
    }
    return normalized(nsum);
}

// calculate_tangs (M/reg_tools.cpp:205-262) from the local normal a (already flipped towards the point)
__device__ __forceinline__ void tangs_of(const V3 &a, V3 &e1, V3 &e2) {
    double mag;
    if (fabs(a.x) >= fabs(a.y) && fabs(a.x) >= fabs(a.z)) {
        mag = sqrt(a.z * a.z + a.y * a.y);
        e1 = mag == 0 ? mk(0.0, 0.0, 1.0) : mk(0.0, -a.z / mag, a.y / mag);
    } else if (fabs(a.y) >= fabs(a.x) && fabs(a.y) >= fabs(a.z)) {
        mag = sqrt(a.z * a.z + a.x * a.x);
        e1 = mag == 0 ? mk(0.0, 0.0, 1.0) : mk(-a.z / mag, 0.0, a.x / mag);
    } else {
        mag = sqrt(a.y * a.y + a.x * a.x);
        e1 = mag == 0 ? mk(1.0, 0.0, 0.0) : mk(-a.y / mag, a.x / mag, 0.0);
    }
    e2 = normalized(cross(a, e1));
}

}  // namespace msm
