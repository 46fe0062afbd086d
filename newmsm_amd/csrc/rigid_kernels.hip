// rigid_kernels.hip -- the cost of the rigid level (Rigid_cost_function, M/rigid_costfunction.cpp) on gfx950.
//
//   k_rigid_probe   one lane per (probe b, SOURCE vertex i): the vertex rotated by R_b^T (euler_rotate, R/point.cpp:154-171) into the probe's
//                   B x 3 x V scratch copy of SOURCE (rigid_cost_mesh rotates a copy, :123-139).
//   k_rigid_eval    one lane per (probe b, SOURCE vertex i), on that copy: rigid_cost_mesh for B Euler triples at once.  The lane forms the local
//                   normal of the rotated mesh and the tangent pair of calculate_tangs (M/reg_tools.cpp:205-262), finds the closest TARGET triangle (search_device.hpp:
//                   the direction table where the target has one, the complete octree search otherwise) and evaluates WLS_simgradient (:60-85)
//                   over that triangle's query list (get_all_neighbours, :141-162, precomputed per target triangle) with the similarity of
//                   calculate_sim_column_nbh (M/similarities.cpp:37-52) computed inline.  val[b * V + i] = current_sim(i + 1).
//   k_rigid_sum     one workgroup per probe: the V values summed in a fixed order (strided per lane, then a tree in LDS) -- two runs give the
//                   same bits; no floating-point atomics.
//   k_rigid_rotate  rotate_in_mesh (:110-121) of SOURCE in place, keeping the previous coordinates for a restore.
//
// The rotation matrices are built on the host with libm (device sin / cos may differ in the last bit).  Every decision and every value uses
// the reference's FP64 operations in the reference's order (-ffp-contract=off); the weight's exp() is the device's.
#include "frame_device.hpp"
#include "kernels.hpp"
#include "rigid.hpp"
#include "search_device.hpp"

namespace msm {

namespace {

// R^T v with R row-major: component k = R(0,k) x + R(1,k) y + R(2,k) z, summed left to right (NEWMAT's product)
__device__ __forceinline__ V3 rot_t(const double *R, const V3 &v) {
    return mk(R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z, R[2] * v.x + R[5] * v.y + R[8] * v.z);
}

__device__ __forceinline__ V3 src_vertex(const double *src, int V, int i) { return mk(src[i], src[V + i], src[2 * (size_t)V + i]); }

// sim(q, i) of sparsesimkernel: -SSD (M/similarities.cpp:98-112) or corr (:54-96) between input column i and reference column q (dense data)
__device__ __forceinline__ double sim_of(const RigidEvalArgs &a, int i, int q) {
    const double *x = a.fin + (size_t)i * a.D;
    const double *y = a.fref + (size_t)q * a.D;
    if (a.sim == 1) {
        double prod = 0.0;
        for (int d = 0; d < a.D; ++d) prod += (x[d] - y[d]) * (x[d] - y[d]);
        return -(sqrt(prod) / a.D);
    }
    const double ma = a.mean_in[i], mb = a.mean_ref[q];
    double prod = 0.0, varA = 0.0, varB = 0.0;
    for (int d = 0; d < a.D; ++d) {
        prod += (x[d] - ma) * (y[d] - mb);
        varA += (x[d] - ma) * (x[d] - ma);
        varB += (y[d] - mb) * (y[d] - mb);
    }
    if (varA == 0.0 || varB == 0.0) return 0.0;
    return prod / (sqrt(varA) * sqrt(varB));
}

__global__ __launch_bounds__(256) void k_rigid_probe(const double *__restrict__ src, int V, RigidRot Rs, double *__restrict__ rot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= V) return;
    const V3 r = rot_t(Rs.r[b], src_vertex(src, V, i));
    double *out = rot + (size_t)b * 3 * V;
    out[i] = r.x;
    out[V + i] = r.y;
    out[2 * (size_t)V + i] = r.z;
}

__global__ __launch_bounds__(256) void k_rigid_eval(RigidEvalArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= a.V) return;
    const double *rs = a.rot + (size_t)b * 3 * a.V;  // SOURCE rotated by probe b
    const V3 p = src_vertex(rs, a.V, i);
    // Mesh::local_normal (R/mesh.cpp:133-141) of the rotated mesh: the incident triangles' normals summed in trID order
    V3 nrm = local_normal(rs, a.V, a.stri, a.Ts, a.stid_ptr, a.stid, i);
    if (dot(nrm, p) < 0) nrm = scale(nrm, -1.0);
    V3 e1, e2;
    tangs_of(nrm, e1, e2);
    const V3 origin = scale(normalized(cross(e1, e2)), kRad);
    const V3 po = sub(p, origin);
    const double y1 = dot(po, e1), y2 = dot(po, e2);

    int t = ray_find(a.tree, p);
    if (t < 0) t = find_closest_triangle(a.tree, p);
    double val = 0.0;
    if (t < 0) {
        atomicMin(a.status, t);
    } else {
        double sum = 0.0, jp = 0.0;
        for (int k = a.qptr[t]; k < a.qptr[t + 1]; ++k) {
            const int q = a.qidx[k];
            const V3 co = sub(src_vertex(a.txyz, a.Vt, q), origin);
            const double d1 = dot(co, e1) - y1, d2 = dot(co, e2) - y2;
            const double dd = d1 * d1 + d2 * d2;
            if (dd > 0) {
                const double w = exp(-dd / a.two_sig2);
                sum += w;
                jp += (q != 0 ? sim_of(a, i, q) : 0.0) * w;  // target vertex 0 never gets a similarity (M/similarities.cpp:40): 0, its weight counts
            }
        }
        if (sum > 0) jp /= sum;
        val = jp;
    }
    a.val[(size_t)b * a.V + i] = val;
}

constexpr int kSumThreads = 1024;  // lanes per probe

__global__ __launch_bounds__(kSumThreads) void k_rigid_sum(const double *__restrict__ val, int V, double *__restrict__ sums) {
    __shared__ double part[kSumThreads];
    const double *v = val + (size_t)blockIdx.x * V;
    double acc = 0.0;
    for (int i = threadIdx.x; i < V; i += kSumThreads) acc += v[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kSumThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(256) void k_rigid_rotate(double *__restrict__ src, double *__restrict__ saved, int V, RigidRot Rs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const V3 v = src_vertex(src, V, i);
    saved[i] = v.x;
    saved[V + i] = v.y;
    saved[2 * (size_t)V + i] = v.z;
    const V3 r = rot_t(Rs.r[0], v);
    src[i] = r.x;
    src[V + i] = r.y;
    src[2 * (size_t)V + i] = r.z;
}

}  // namespace

int launch_rigid_eval(msm_ctx *ctx, const RigidEvalArgs &a, const RigidRot &R, int B, double *d_sums) {
    if (a.V <= 0 || B <= 0 || B > kRigidMaxProbes) return fail(MSM_ERR_INVALID, "launch_rigid_eval: V %d, B %d", a.V, B);
    hipLaunchKernelGGL(k_rigid_probe, dim3((a.V + 255) / 256, B), dim3(256), 0, ctx->stream, a.src, a.V, R, a.rot);
    hipLaunchKernelGGL(k_rigid_eval, dim3((a.V + 255) / 256, B), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_rigid_sum, dim3(B), dim3(kSumThreads), 0, ctx->stream, a.val, a.V, d_sums);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

int launch_rigid_rotate(msm_ctx *ctx, double *d_src, double *d_saved, int V, const RigidRot &R) {
    if (V <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_rigid_rotate, dim3((V + 255) / 256), dim3(256), 0, ctx->stream, d_src, d_saved, V, R);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
