// vertex_strain_kernels.hip -- calculate_strains (M/reg_tools.cpp:365-549) on gfx950: the strain map of an aMSM run.
//
//   k_strain_normals     one lane per vertex: ORIG's normals as estimate_normals leaves them (Mesh::local_normal, R/mesh.cpp:133-150).
//   k_grid_count         one lane per vertex: its cell of a uniform grid over ORIG's bounding box, counted with integer atomics.
//   k_grid_scan          one workgroup: the cells' first positions (exclusive prefix sum of the counts).
//   k_grid_scatter       one lane per vertex: its position within its cell's range (the order within a cell is put right by k_grid_sort).
//   k_grid_sort          one lane per cell: the cell's vertices sorted by id, then ORIG, the normals and FINAL gathered into that order.
//   k_strain_radius      one lane per vertex: the radius the reference's `fit_temp += 0.5` loop stops at.  The 9th smallest distance d9 over the
//                        members of growing boxes (every vertex within distance R of the vertex lies in the box of R, so once 9 members lie within
//                        R, d9 is exact); the radius is then fit_radius + 0.5 + 0.5 ... by the reference's own additions, the first that is >= d9.
//   k_strain_fit         one lane per vertex: the members at that radius, in a fixed order (cells z, y, x ascending, ids ascending within a
//                        cell), streamed row by row into a Givens QR of the 5-column least-squares problem (the reference's 6-column alpha has an
//                        identically zero first column, to which its pseudo-inverse gives coefficient 0); then get_coordinate_transformation
//                        (:179-203), F = g G_cont^T, C = F^T F, its eigenpairs by cyclic Jacobi, and the two stretches of the eigenvectors that
//                        are not the one most aligned with G3.
//
// Membership is decided only by the reference's tests (|x_i - x_j| <= r with Point::norm, n_j . n_i >= 0) on FP64 values computed as it
// computes them (-ffp-contract=off); the grid only decides which vertices are tested, with a margin that keeps it conservative.  No
// floating-point atomics: two calls give the same bits.
#include "frame_device.hpp"
#include "vertex_strains.hpp"

namespace msm {

namespace {

constexpr int kBlock = 256;
constexpr int kScanThreads = 1024;

__device__ __forceinline__ int axis_cell(double x, double x0, double inv_h, int n) {
    const double f = floor((x - x0) * inv_h);
    if (!(f > 0.0)) return 0;
    if (f >= (double)(n - 1)) return n - 1;
    return (int)f;
}

// the cells that hold every point within R of p (per axis [p - R, p + R], widened by far more than the rounding of the distance test)
__device__ __forceinline__ void box_of(const StrainGrid &g, const V3 &p, double R, int lo[3], int hi[3]) {
    const double px[3] = {p.x, p.y, p.z}, x0[3] = {g.x0, g.y0, g.z0};
    const int n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double w = R + 1e-9 * (fabs(px[k]) + R);
        lo[k] = axis_cell(px[k] - w, x0[k], g.inv_h, n[k]);
        hi[k] = axis_cell(px[k] + w, x0[k], g.inv_h, n[k]);
    }
}

__global__ __launch_bounds__(kBlock) void k_strain_normals(StrainArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.V) return;
    const V3 n = local_normal(a.orig, a.V, a.tri, a.T, a.tid_ptr, a.tid, i);
    a.nrm[i] = n.x;
    a.nrm[a.V + i] = n.y;
    a.nrm[2 * (size_t)a.V + i] = n.z;
}

__global__ __launch_bounds__(kBlock) void k_grid_count(StrainArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.V) return;
    const V3 p = soa_vertex(a.orig, a.V, i);
    const int c = (axis_cell(p.z, a.g.z0, a.g.inv_h, a.g.nz) * a.g.ny + axis_cell(p.y, a.g.y0, a.g.inv_h, a.g.ny)) * a.g.nx +
                  axis_cell(p.x, a.g.x0, a.g.inv_h, a.g.nx);
    a.cell[i] = c;
    atomicAdd(&a.cnt[c], 1);
}

__global__ __launch_bounds__(kScanThreads) void k_grid_scan(const int32_t *__restrict__ cnt, int C, int32_t *__restrict__ start, int32_t *__restrict__ cursor) {
    __shared__ int32_t part[kScanThreads];
    const int t = threadIdx.x;
    const int per = (C + kScanThreads - 1) / kScanThreads;
    const int b = t * per, e = min(b + per, C);
    int32_t s = 0;
    for (int k = b; k < e; ++k) s += cnt[k];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int32_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int32_t run = t > 0 ? part[t - 1] : 0;
    for (int k = b; k < e; ++k) {
        start[k] = run;
        cursor[k] = run;
        run += cnt[k];
    }
    if (t == kScanThreads - 1) start[C] = part[t];
}

__global__ __launch_bounds__(kBlock) void k_grid_scatter(StrainArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.V) return;
    a.svid[atomicAdd(&a.cursor[a.cell[i]], 1)] = i;
}

__global__ __launch_bounds__(kBlock) void k_grid_sort(StrainArgs a, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int b = a.start[c], e = a.start[c + 1];
    for (int k = b + 1; k < e; ++k) {
        const int v = a.svid[k];
        int m = k - 1;
        while (m >= b && a.svid[m] > v) {
            a.svid[m + 1] = a.svid[m];
            --m;
        }
        a.svid[m + 1] = v;
    }
    const size_t V = a.V;
    for (int k = b; k < e; ++k) {
        const int v = a.svid[k];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a.sxyz[d * V + k] = a.orig[d * V + v];
            a.snrm[d * V + k] = a.nrm[d * V + v];
            a.sfin[d * V + k] = a.fin[d * V + v];
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_strain_radius(StrainArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.V) return;
    const V3 p = soa_vertex(a.orig, a.V, i);
    const V3 ni = soa_vertex(a.nrm, a.V, i);
    double R = a.fit_radius, d9 = 0.0;
    int found = 0;
    for (;;) {
        int lo[3], hi[3];
        box_of(a.g, p, R, lo, hi);
        const bool full = lo[0] == 0 && lo[1] == 0 && lo[2] == 0 && hi[0] == a.g.nx - 1 && hi[1] == a.g.ny - 1 && hi[2] == a.g.nz - 1;
        double best[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) best[k] = INFINITY;
        found = 0;
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y) {
                const int row = (z * a.g.ny + y) * a.g.nx;
                for (int k = a.start[row + lo[0]]; k < a.start[row + hi[0] + 1]; ++k) {
                    const V3 q = soa_vertex(a.sxyz, a.V, k);
                    const double d = norm(sub(p, q));
                    if ((full || d <= R) && dot(soa_vertex(a.snrm, a.V, k), ni) >= 0) {
                        ++found;
                        if (d < best[8]) {  // keep the nine smallest, sorted
                            best[8] = d;
#pragma unroll
                            for (int m = 8; m > 0; --m)
                                if (best[m] < best[m - 1]) {
                                    const double t = best[m];
                                    best[m] = best[m - 1];
                                    best[m - 1] = t;
                                }
                        }
                    }
                }
            }
        if (found >= 9) {
            d9 = best[8];
            break;
        }
        if (full) {  // fewer than 9 vertices face the same way: the reference's loop never ends
            a.radius[i] = -1.0;
            a.kept[i] = found;
            return;
        }
        R *= 2.0;
    }
    double r = a.fit_radius;
    while (!(d9 <= r)) r += 0.5;
    a.radius[i] = r;
}

// one row (a | b) of the least-squares problem rotated into the triangular factor R and the rotated right-hand sides Q
__device__ __forceinline__ void givens_row(double (&R)[5][5], double (&Q)[5][4], double (&a)[5], double (&b)[4]) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        if (a[k] != 0.0) {
            const double x = R[k][k], y = a[k];
            const double h = sqrt(x * x + y * y);
            const double c = x / h, s = y / h;
            R[k][k] = h;
            a[k] = 0.0;
#pragma unroll
            for (int l = k + 1; l < 5; ++l) {
                const double u = R[k][l], v = a[l];
                R[k][l] = c * u + s * v;
                a[l] = c * v - s * u;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double u = Q[k][q], v = b[q];
                Q[k][q] = c * u + s * v;
                b[q] = c * v - s * u;
            }
        }
    }
}

// one Jacobi rotation of the symmetric A (3 x 3) in the plane (p, q), accumulated into the columns of U
template <int p, int q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&U)[3][3]) {
    constexpr int r = 3 - p - q;
    const double apq = A[p][q];
    if (fabs(apq) <= 1e-300 || fabs(apq) <= 1e-18 * (fabs(A[p][p]) + fabs(A[q][q]))) {
        A[p][q] = A[q][p] = 0.0;
        return;
    }
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    double t;
    if (fabs(theta) > 1e150) t = 0.5 / theta;
    else t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[p][p] -= t * apq;
    A[q][q] += t * apq;
    A[p][q] = A[q][p] = 0.0;
    const double arp = A[r][p], arq = A[r][q];
    A[r][p] = A[p][r] = c * arp - s * arq;
    A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ukp = U[k][p], ukq = U[k][q];
        U[k][p] = c * ukp - s * ukq;
        U[k][q] = s * ukp + c * ukq;
    }
}

__device__ __forceinline__ void swap_pair(double (&w)[3], double (&U)[3][3], int i, int j) {
    const double t = w[i];
    w[i] = w[j];
    w[j] = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double u = U[k][i];
        U[k][i] = U[k][j];
        U[k][j] = u;
    }
}

__global__ __launch_bounds__(kBlock) void k_strain_fit(StrainArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.V) return;
    const double r = a.radius[i];
    if (!(r >= 0)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a.strains[(size_t)k * a.V + i] = 0.0;
        return;
    }
    const V3 p = soa_vertex(a.orig, a.V, i);
    const V3 ni = soa_vertex(a.nrm, a.V, i);  // Normal_O: unflipped
    const V3 fi = soa_vertex(a.fin, a.V, i);
    V3 nf = ni;  // calculate_tangs flips the local normal towards the point
    if (dot(nf, p) < 0) nf = scale(nf, -1.0);
    V3 e1, e2;
    tangs_of(nf, e1, e2);

    double R[5][5], Q[5][4];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int l = 0; l < 5; ++l) R[k][l] = 0.0;
#pragma unroll
        for (int l = 0; l < 4; ++l) Q[k][l] = 0.0;
    }
    int members = 0;
    int lo[3], hi[3];
    box_of(a.g, p, r, lo, hi);
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y) {
            const int row = (z * a.g.ny + y) * a.g.nx;
            for (int k = a.start[row + lo[0]]; k < a.start[row + hi[0] + 1]; ++k) {
                const V3 q = soa_vertex(a.sxyz, a.V, k);
                if (!(norm(sub(p, q)) <= r && dot(soa_vertex(a.snrm, a.V, k), ni) >= 0)) continue;
                ++members;
                const V3 tmp = sub(q, p);
                const double T1 = dot(tmp, e1), T2 = dot(tmp, e2);
                const V3 tf = sub(soa_vertex(a.sfin, a.V, k), fi);
                double row5[5] = {T1, T2, 0.5 * T1 * T1, 0.5 * T2 * T2, T1 * T2};
                double rhs[4] = {dot(tmp, ni), dot(tf, e1), dot(tf, e2), dot(tf, ni)};  // N, t1, t2, n
                givens_row(R, Q, row5, rhs);
            }
        }
    // back substitution for the four right-hand sides; a zero pivot (a rank-deficient neighbourhood) gives its coefficient 0
    double X[5][4];
#pragma unroll
    for (int k = 4; k >= 0; --k) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double s = Q[k][q];
#pragma unroll
            for (int l = k + 1; l < 5; ++l) s -= R[k][l] * X[l][q];
            X[k][q] = R[k][k] != 0.0 ? s / R[k][k] : 0.0;
        }
    }
    const double dNdT1 = X[0][0], dNdT2 = X[1][0], dt1dT1 = X[0][1], dt1dT2 = X[1][1], dt2dT1 = X[0][2], dt2dT2 = X[1][2], dndT1 = X[0][3],
                 dndT2 = X[1][3];

    // get_coordinate_transformation (:179-203): G = [G1 G2 G3], G_cont = (G^-1)^T
    const V3 G1 = mk(1.0, 0.0, dNdT1), G2 = mk(0.0, 1.0, dNdT2);
    V3 G3 = cross(G1, G2);
    const double g3n = sqrt(dot(G3, G3));
    G3 = mk(G3.x / g3n, G3.y / g3n, G3.z / g3n);
    const double G[3][3] = {{G1.x, G2.x, G3.x}, {G1.y, G2.y, G3.y}, {G1.z, G2.z, G3.z}};
    const double det = G[0][0] * (G[1][1] * G[2][2] - G[1][2] * G[2][1]) - G[0][1] * (G[1][0] * G[2][2] - G[1][2] * G[2][0]) +
                       G[0][2] * (G[1][0] * G[2][1] - G[1][1] * G[2][0]);
    double Gi[3][3];  // G^-1 by its adjugate
    Gi[0][0] = (G[1][1] * G[2][2] - G[1][2] * G[2][1]) / det;
    Gi[0][1] = (G[0][2] * G[2][1] - G[0][1] * G[2][2]) / det;
    Gi[0][2] = (G[0][1] * G[1][2] - G[0][2] * G[1][1]) / det;
    Gi[1][0] = (G[1][2] * G[2][0] - G[1][0] * G[2][2]) / det;
    Gi[1][1] = (G[0][0] * G[2][2] - G[0][2] * G[2][0]) / det;
    Gi[1][2] = (G[0][2] * G[1][0] - G[0][0] * G[1][2]) / det;
    Gi[2][0] = (G[1][0] * G[2][1] - G[1][1] * G[2][0]) / det;
    Gi[2][1] = (G[0][1] * G[2][0] - G[0][0] * G[2][1]) / det;
    Gi[2][2] = (G[0][0] * G[1][1] - G[0][1] * G[1][0]) / det;

    const V3 g1 = mk(dt1dT1, dt2dT1, dndT1), g2 = mk(dt1dT2, dt2dT2, dndT2);
    V3 g3 = cross(g1, g2);
    const double g3m = sqrt(dot(g3, g3));
    g3 = mk(g3.x / g3m, g3.y / g3m, g3.z / g3m);
    const double g[3][3] = {{g1.x, g2.x, g3.x}, {g1.y, g2.y, g3.y}, {g1.z, g2.z, g3.z}};
    double F[3][3], A[3][3], U[3][3];  // F = g G_cont^T = g G^-1, A = C = F^T F
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int l = 0; l < 3; ++l) F[k][l] = g[k][0] * Gi[0][l] + g[k][1] * Gi[1][l] + g[k][2] * Gi[2][l];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            A[k][l] = F[0][k] * F[0][l] + F[1][k] * F[1][l] + F[2][k] * F[2][l];
            U[k][l] = k == l ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 32; ++sweep) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
        jacobi_rotate<0, 1>(A, U);
        jacobi_rotate<0, 2>(A, U);
        jacobi_rotate<1, 2>(A, U);
    }
    // SVD(C, Omega, U): the singular values of the symmetric C, in decreasing order with their vectors
    double w[3] = {fabs(A[0][0]), fabs(A[1][1]), fabs(A[2][2])};
    if (w[0] < w[1]) swap_pair(w, U, 0, 1);
    if (w[1] < w[2]) swap_pair(w, U, 1, 2);
    if (w[0] < w[1]) swap_pair(w, U, 0, 1);
    const double m0 = fabs(G3.x * U[0][0] + G3.y * U[1][0] + G3.z * U[2][0]);
    const double m1 = fabs(G3.x * U[0][1] + G3.y * U[1][1] + G3.z * U[2][1]);
    const double m2 = fabs(G3.x * U[0][2] + G3.y * U[1][2] + G3.z * U[2][2]);
    int maxind, minind;
    if (m0 >= m1 && m0 >= m2) {
        if (sqrt(w[1]) > sqrt(w[2])) maxind = 1, minind = 2;
        else maxind = 2, minind = 1;
    } else if (m1 >= m0 && m1 >= m2) {
        if (sqrt(w[0]) > sqrt(w[2])) maxind = 0, minind = 2;
        else maxind = 2, minind = 0;
    } else {
        if (sqrt(w[0]) > sqrt(w[1])) maxind = 0, minind = 1;
        else maxind = 1, minind = 0;
    }
    const double s1 = sqrt(maxind == 0 ? w[0] : (maxind == 1 ? w[1] : w[2]));
    const double s2 = sqrt(minind == 0 ? w[0] : (minind == 1 ? w[1] : w[2]));
    a.strains[i] = s1;
    a.strains[(size_t)a.V + i] = s2;
    a.strains[2 * (size_t)a.V + i] = 0.5 * (s1 * s1 - 1);
    a.strains[3 * (size_t)a.V + i] = 0.5 * (s2 * s2 - 1);
    a.kept[i] = members;
}

}  // namespace

int launch_vertex_strains(msm_ctx *ctx, const StrainArgs &a, int C) {
    if (a.V <= 0 || C <= 0) return fail(MSM_ERR_INVALID, "launch_vertex_strains: V %d, %d cells", a.V, C);
    const dim3 gv((a.V + kBlock - 1) / kBlock), gc((C + kBlock - 1) / kBlock);
    MSM_HIP(hipMemsetAsync(a.cnt, 0, sizeof(int32_t) * (size_t)C, ctx->stream));
    hipLaunchKernelGGL(k_strain_normals, gv, dim3(kBlock), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_grid_count, gv, dim3(kBlock), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_grid_scan, dim3(1), dim3(kScanThreads), 0, ctx->stream, a.cnt, C, a.start, a.cursor);
    hipLaunchKernelGGL(k_grid_scatter, gv, dim3(kBlock), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_grid_sort, gc, dim3(kBlock), 0, ctx->stream, a, C);
    hipLaunchKernelGGL(k_strain_radius, gv, dim3(kBlock), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_strain_fit, gv, dim3(kBlock), 0, ctx->stream, a);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
