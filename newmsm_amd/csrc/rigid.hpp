// rigid.hpp -- the rigid level's device side (rigid_kernels.hip), used by rigid.cpp.
#pragma once

#include "internal.hpp"

namespace msm {

constexpr int kRigidMaxProbes = 4;  // Euler triples of one k_rigid_eval launch: the three finite-difference probes of an iteration, or one

// R(w1, w2, w3) of euler_rotate (R/point.cpp:154-171), row-major; the vertices move by R^T
struct RigidRot {
    double r[kRigidMaxProbes][9];
};

struct RigidEvalArgs {
    DevTree tree;                        // TARGET's search structure
    const double *src;                   // SOURCE, 3 x V SoA
    double *rot;                         // scratch, B x 3 x V: SOURCE rotated by each probe (k_rigid_probe)
    int V;
    const int32_t *stri;                 // SOURCE's triangles, 3 x Ts SoA
    int Ts;
    const int32_t *stid_ptr, *stid;      // SOURCE's Mpoint::trID lists (CSR over vertices)
    const double *txyz;                  // TARGET, 3 x Vt SoA
    int Vt;
    const int32_t *qptr, *qidx;          // per TARGET triangle: the query list of get_all_neighbours (CSR over triangles)
    const double *fin, *fref;            // input (V x D) and reference (Vt x D) features, vertex-major
    const double *mean_in, *mean_ref;    // meanvector of both (simmeasure 2)
    int D, sim;
    double two_sig2;                     // 2 * min_sigma * min_sigma, in that order
    double *val;                         // B x V: the per-vertex values (current_sim)
    int *status;
};

// val[b * V + i] for the B rotations of R (B <= kRigidMaxProbes), each on its own rotated copy of SOURCE in a.rot; sums[b] = their sum in a fixed order
int launch_rigid_eval(msm_ctx *ctx, const RigidEvalArgs &a, const RigidRot &R, int B, double *d_sums);
// saved = src; src = R.r[0]^T src (rotate_in_mesh)
int launch_rigid_rotate(msm_ctx *ctx, double *d_src, double *d_saved, int V, const RigidRot &R);

}  // namespace msm
