// vertex_strains.hpp -- the strain maps of an aMSM run (calculate_strains, M/reg_tools.cpp:365-549) on the device (vertex_strain_kernels.hip),
// used by vertex_strains.cpp.
#pragma once

#include "internal.hpp"

namespace msm {

// a uniform grid over ORIG's bounding box: cell (x, y, z) of a point is floor((p - lo) / h) per axis, clamped to the grid; cell id (z ny + y) nx + x
struct StrainGrid {
    double x0, y0, z0, inv_h;
    int nx, ny, nz;
};

struct StrainArgs {
    StrainGrid g;
    int V, T;
    const double *orig, *fin;            // ORIG and FINAL, 3 x V SoA
    const int32_t *tri, *tid_ptr, *tid;  // ORIG's triangles (3 x T SoA) and its Mpoint::trID lists (CSR over vertices)
    double *nrm;                         // ORIG's normals (estimate_normals), 3 x V SoA
    int32_t *cell;                       // per vertex: its cell
    int32_t *cnt, *start, *cursor;       // per cell: count, first sorted position (C + 1), scatter cursor
    int32_t *svid;                       // the vertices sorted by cell, ascending id within a cell
    double *sxyz, *snrm, *sfin;          // ORIG, its normals and FINAL in that order, 3 x V SoA each
    double fit_radius;
    double *radius;                      // per vertex: the radius the reference's loop stops at (-1: never 9 members)
    int32_t *kept;                       // per vertex: the member count at that radius (the candidates found when it is -1)
    double *strains;                     // 4 x V
};

// normals, the grid (a counting sort on the device), each vertex's final radius, then the local fits and the stretches
int launch_vertex_strains(msm_ctx *ctx, const StrainArgs &a, int C);

}  // namespace msm
