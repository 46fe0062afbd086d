// internal.hpp -- shared declarations of libmsmhip (not part of the C ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/msmhip.h"
#include "devbuf.hpp"
#include "geom.hpp"

namespace msm {

// ---------------------------------------------------------------- errors
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);
// pool.cpp: device memory of the handles (size-classed free lists over hipMalloc / hipFree; taken and given back through DevBuf, devbuf.hpp)
void pool_trim();
size_t pool_idle_bytes();

#define MSM_HIP(call)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return msm::fail(MSM_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define MSM_TRY(call)               \
    do {                            \
        const int st_ = (call);     \
        if (st_) return st_;        \
    } while (0)

// ---------------------------------------------------------------- host mesh helpers (host_mesh.cpp)
struct Adjacency {
    std::vector<int32_t> nbr_ptr, nbr, tid_ptr, tid;
};
void build_adjacency(const int32_t *tri /*3 x T SoA*/, int V, int T, Adjacency &adj);
void icosphere_unit(int order, std::vector<double> &xyz_aos, std::vector<int32_t> &tri_aos);

// ---------------------------------------------------------------- octree (octree.cpp)
// Per-triangle record used by the exact test: vertices, the triangle-only half of project_point, ids.
struct alignas(128) TriRec {
    double v0[3], v1[3], v2[3];
    double s3[3];
    double d;
    int32_t id[3];
    int32_t tri;
    double reserved;
};
static_assert(sizeof(TriRec) == 128, "TriRec must be 128 bytes");

// Per-triangle record of the ray-table path, nine 16-byte pieces (144 bytes, two cache lines):
//   pieces 0-2  the three edge planes (float4: inward unit normal, acceptance threshold)      -- ray_table.cpp
//   pieces 3-8  the vertices v0,v1,v2 (9 doubles) and, on single-feature meshes, the feature at them (3 doubles)
// so that a wavefront can fetch the records of its 64 samples with 9 load instructions that touch ~2 lines per
// record (lanes of one instruction read neighbouring pieces) instead of 9 x 64 lines.  k_unary_rays reads pieces 3-8 that way by lane
// pairs (two neighbouring lanes take two adjacent pieces of one record in each instruction, at 32-bit byte offsets from the table's base:
// 16 * kRayPieces * kRayMaxTris fits 32 bits), pieces 0-2 lane by lane.  Built on the GPU (kernels.hip: k_build_raytri).
constexpr int kRayPieces = 9;

// First-candidate hints of a direction cell.  A cell is cut into kRayHintK x kRayHintK sub-cells, and two bits per sub-cell
// say which of the candidates stored in the cell itself (x, y, z, and w when it is an id) to try first: the one whose
// gnomonic triangle holds the sub-cell's centre, 0 = the stored order.  They ride in the top 6 bits of x, y, z -- word
// su (x, y, z for su = 0, 1, 2), bits 26 + 2 sv -- above a 26-bit two's-complement id (-1 = none; w holds an id, -1 or the
// ray_more reference in its low 23 bits, see the certificates below). The order of trial cannot change a result: at most one listed candidate
// passes the acceptance test (ray_table.cpp).  The cut is 3 x 3 and no parameter: the certificates below give the same nine sub-cells
// a bit each, at 3 su + sv.
constexpr int kRayHintK = 3;
constexpr int kRayIdBits = 26;
static_assert(kRayHintK == 3 && kRayIdBits + 2 * kRayHintK == 32, "3 x 3 sub-cells: a hint word per su (x, y, z), three two-bit fields above its id");
// Certificates.  The fourth word gives its top nine bits to one bit per sub-cell, bit kRayWBits + 3 su + sv: "the candidate this
// sub-cell's hint names passes the acceptance test for every direction of the sub-cell, and needs no vouching" (ray_table.cpp:
// build_ray_table has the proof), so a kernel may take that candidate without loading its edge planes.  Below them w keeps what it held
// as a 23-bit two's-complement field: an id, -1, or the ray_more reference -2 - index.  So an id has 22 bits (the unary path's own
// kTriBits): a mesh with more than kRayMaxTris = 2^22 triangles gets no table, and a table whose ray_more list would pass
// kRayMaxMore = 2^22 - 2 entries (its references would leave the field) gets none either -- with four candidates listed per entry
// no mesh below the first limit comes near the second.  MSMHIP_RAY_CERTS=off writes all nine bits as zero.
constexpr int kRayWBits = 23;
static_assert(kRayWBits + kRayHintK * kRayHintK == 32 && kRayWBits <= kRayIdBits, "nine certificate bits, one per sub-cell, above the fourth word's field");
constexpr int kRayMaxTris = 1 << (kRayWBits - 1);  // a mesh with more triangles gets no table (build_ray_table)
constexpr int kRayMaxMore = (1 << (kRayWBits - 1)) - 2;

// Direction (ray) table of a simple surface (ray_table.cpp: build_ray_table), the host side; G == 0 when absent.
struct RayTable {
    // closed, consistently oriented, star-shaped about the origin, covering the sphere exactly once: every ray from
    // the origin meets exactly one triangle (true for the icosphere targets; false for folded meshes)
    bool simple = false;
    int G = 0;                   // cube-map cells per face axis
    std::vector<int4> cell;      // 6 x G x G: up to four candidate triangles per direction cell, -1 padded
    std::vector<float4> edge;    // 3 per triangle: inward unit normal of the plane (origin, edge k); .w: see ray_table.cpp
    std::vector<int4> more;      // candidates 4..7 of the cells that have more than four
    std::vector<int4> excl;      // up to seven leaf boxes a query must not lie in for its triangle to be vouched for: {b0, b1, b2, count} and, for count > 3, {b3 .. b6} in the next record
    double r2lo = 0, r2hi = 0;   // squared radius range of the query points the table is valid for
    bool certs = true;           // built with certificates in the cells (MSMHIP_RAY_CERTS); false: all nine bits of every cell are zero
};

struct FlatOctree {
    // node[n].x >= 0: internal node, children are node[n].x .. +7 in (i,j,k) order.
    // node[n].x <  0: leaf with (-x - 1) entries starting at node[n].y (a multiple of 8) in leaf_tri / cone;
    //                 each leaf's entries are padded to a multiple of 8 (leaf_tri -1).
    // node[n].z: leaves with 1..64 entries own 64 sub-cell masks at mask[64 * z ..]; -1 otherwise.
    // node[n].w: depth of the node (root 0); its box has edge 202 / 2^w.
    std::vector<int4> node;
    std::vector<double4> nodebox;  // per node: lower corner (x,y,z) and edge length (w), all exact dyadics
    int nmask_blocks = 0;
    std::vector<int32_t> parent;
    std::vector<int32_t> leaf_tri;
    // Dense top of the tree: the node reached after grid_depth levels of descent (or the leaf met earlier),
    // indexed [ix][iy][iz] with G = 2^grid_depth cells per axis over (-101, 101).  Child boxes are exact
    // halvings, so the cell of a point is found arithmetically and the descent starts there.
    std::vector<int32_t> grid;
    int grid_depth = 0;
    RayTable rays;  // see there; filled by build_ray_table
    int64_t stats[5] = {0, 0, 0, 0, 0};
    // a tree built on the GPU (octree_kernels.hip) has no host arrays: `node` etc. stay empty and these describe it
    int dev_nnodes = 0, dev_entries = 0;
    int nnodes() const { return node.empty() ? dev_nnodes : (int)node.size(); }
    int nentries() const { return node.empty() ? dev_entries : (int)leaf_tri.size(); }
};
// builds the tree exactly as Octree::initialize_tree / add_triangle do (R/octree.cpp:42-141)
void build_octree(const double *xyz /*3 x V SoA*/, const int32_t *tri /*3 x T SoA*/, int V, int T, FlatOctree &out);
// decides RayTable::simple and, for a simple surface, fills the ray table (tree.rays) of an already built tree (ray_table.cpp)
void build_ray_table(const double *xyz, const int32_t *tri, int V, int T, FlatOctree &tree);
// MSMHIP_RAY_CERTS is not "off": build_ray_table writes certificates (read per call; the content cache of tables keys on it, api.cpp)
bool ray_certs_enabled();

// device view of a mesh's search structure
struct DevTree {
    const int4 *node;
    const int32_t *parent;
    const int32_t *leaf_tri;
    const float4 *cone;
    const TriRec *rec;
    const int32_t *grid;
    int grid_depth;  // G = 1 << grid_depth cells per axis
    int simple;  // see RayTable::simple
    const unsigned long long *mask;  // 64 per mask block (see FlatOctree::node), or nullptr before the masks are built
    int nnodes;
    // ray table (RayTable); ray_G == 0: none
    int ray_G;
    const int4 *ray_cell;
    const float4 *ray_tri;   // kRayPieces float4 per triangle
    const int4 *ray_more, *ray_excl;
    double ray_r2lo, ray_r2hi;
};

}  // namespace msm

namespace msm {
struct Stager;
}

// ---------------------------------------------------------------- handles
struct msm_ctx {
    int device = 0;
    int num_cus = 256;  // hipDeviceAttributeMultiprocessorCount (MI355X: 256; a partitioned or smaller device has fewer): sizes the launches whose workgroups wait for one another
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int *d_status = nullptr;  // first error code raised by a kernel (atomicMin), 0 when clean
    int *h_status = nullptr;  // pinned
    // grow-only scratch of the host-array query entry points (hipMalloc / hipFree per call cost more than the queries)
    msm::DevBuf<char> q_buf[5];  // queries, triangle ids, vertex ids, weights, the list of queries the direction table left open
    // pinned staging blocks of every host <-> device copy whose host side is not pinned memory of this library (stager.cpp): grow only, event fenced,
    // never moved; created and destroyed with the context
    msm::Stager *stager = nullptr;
    hipEvent_t wait_ev = nullptr;  // msm_ctx_wait_stream
    // A label step queued ahead (msm_cost_triplet_octets_prefetch) shares the stream, the status word and the mapped flags with every other call on the context:
    // the cost function that holds one (at most one per context), resolved -- taken by its matching call, or waited for and discarded -- before any other
    // entry point synchronises the stream or reads the flags (label_step.cpp: drop_ctx_pending)
    struct msm_cost *pending_cost = nullptr;
    // bumped by everything a queued label step's inputs or destination depend on and that the cost function cannot see: a mesh's coordinates or features
    // changed, a pinned block released (a new block may get the old one's address).  A queued step is only taken when the epoch is the one it was queued under.
    uint64_t epoch = 0;
    // small pinned buffers for the per-label-step calls (labeling in, fusion-move energies out)
    void *io_pin = nullptr;
    void *io_dev = nullptr;  // its device address (the block is mapped), or nullptr
    size_t io_cap = 0;
    // a mapped pinned word kernels of the per-label-step calls store a raised status into (no status copy on their fast path)
    int *h_flag = nullptr;
    int *d_flag_map = nullptr;  // its device address
    std::shared_ptr<void> resample_scratch;  // resample.cpp: device buffers of adaptive_weights_dev and msm_metric_resample, kept between calls
    std::shared_ptr<void> histmatch_scratch;  // histmatch.cpp: device buffers of msm_histogram_match, kept between calls
    std::shared_ptr<void> cohort_scratch;     // cohort.cpp: device buffers of msm_surface_distortion and msm_abs_summary, kept between calls
    std::shared_ptr<void> mcmc_scratch;       // mcmc.cpp: device buffers, events and counters of the Monte Carlo sweeps, kept between calls
    std::shared_ptr<void> mplp_scratch;       // mplp.cpp: device buffers, events and counters of the MPLP sweeps, kept between calls
    std::shared_ptr<void> mplp_pairs_scratch;  // mplp_pairs.cpp: the same for MPLP over the pair tables
    std::shared_ptr<void> fusion_mplp_scratch;  // fusion_mplp.cpp: device buffers, events and counters of MPLP over a label step, kept between calls
    int mcmc_draw = 0;                   // msm_ctx_set_mcmc_draw: 0 the GPU sweeps take their proposals from the host's stream, 1 they are drawn on the device
    std::shared_ptr<void> features_scratch;  // features.cpp: device buffers of msm_level_features, kept between calls
    // msm_ctx_time_queries: events around the search kernel of the host-array query entry points
    hipEvent_t q_ev0 = nullptr, q_ev1 = nullptr;
    bool q_timing = false, q_timed = false;
    // scratch of the GPU octree build (octree_kernels.hip), grow only
    msm::DevBuf<double> oct_box;
    msm::DevBuf<int> oct_ints, oct_counters;
    int *oct_hcounters = nullptr;  // pinned
    // msm_host_alloc blocks: pinned host memory the GPU writes results into directly
    struct HostBlock {
        char *host;
        char *dev;
        size_t bytes;
        bool registered = false;  // msm_host_register: the caller's memory, unregistered (not freed) on release
    };
    std::vector<HostBlock> host_blocks;
};

namespace msm {
struct RayJob;
}

struct msm_mesh {
    msm_ctx *ctx = nullptr;
    int V = 0, T = 0, D = 0;
    std::vector<double> xyz;   // 3 x V SoA (host copy)
    std::vector<int32_t> tri;  // 3 x T SoA
    std::vector<double> feat;  // D x V host copy
    bool tree_valid = false;
    bool gpu_tree_always = false;   // build the tree on the GPU whatever the size (the fallback mesh of the gMSM set-up: the host never sees its coordinates)
    bool host_xyz_stale = false;    // the coordinates were last written on the device only (group.cpp): fetched before any host-side use
    std::shared_ptr<void> oct_job;  // a GPU build that has been queued but not looked at yet (octree_kernels.hip)
    msm::FlatOctree tree;
    bool masks_valid = false;
    bool rays_valid = false;
    bool rayrec_valid = false;  // d_ray_tri matches the current coordinates and features
    msm::Adjacency adj;
    bool adj_valid = false;
    // device: every array is owned here and goes back to the pool with the mesh
    msm::DevBuf<double> d_xyz;    // 3 x V SoA
    msm::DevBuf<int32_t> d_tri;   // 3 x T SoA
    msm::DevBuf<float4> d_tcone;  // per-triangle bounding cone (scratch of the record kernel)
    msm::DevBuf<double> d_feat;   // V x D (vertex-major: one row per vertex for gathers)
    msm::DevBuf<int4> d_node;
    msm::DevBuf<double4> d_nodebox;
    msm::DevBuf<unsigned long long> d_mask;
    msm::DevBuf<int32_t> d_parent, d_leaf_tri;
    msm::DevBuf<float4> d_cone;
    msm::DevBuf<msm::TriRec> d_rec;
    msm::DevBuf<int32_t> d_grid;
    msm::DevBuf<int4> d_ray_cell;
    msm::DevBuf<float4> d_ray_edge;
    msm::DevBuf<float4> d_ray_tri;  // kRayPieces per triangle
    msm::DevBuf<int4> d_ray_more, d_ray_excl;
    msm::DevBuf<int32_t> d_tid_ptr, d_tid;  // Mpoint::trID lists as CSR (unfold's fold test)
    msm::DevBuf<int32_t> d_fold;            // [0] folded count, [1] vertices without a triangle, then V flags
    // background build of the ray table (api.cpp: ensure_rays): the job of the current tree, and finished-with jobs of
    // earlier trees that are joined when the mesh goes.  Declared after `tri`, which the job's thread reads: members are
    // destroyed in reverse order, so the jobs are joined before the triangles go.
    uint64_t tree_gen = 0;
    std::shared_ptr<msm::RayJob> ray_job;
    std::vector<std::shared_ptr<msm::RayJob>> stale_jobs;
};

namespace msm {
int ensure_adjacency_dev(msm_mesh *m);  // Mpoint::trID lists as CSR in HBM (d_tid_ptr / d_tid), and d_fold
const Adjacency &mesh_adjacency(msm_mesh *m);  // the host's lists, built on first use
// the host copy of the coordinates follows the device when they were last written there (msm_mesh::host_xyz_stale); fetched on via's stream
int refresh_host_xyz(msm_mesh *m, msm_ctx *via);
int ensure_tree_pair(msm_mesh *a, msm_mesh *b);  // both trees; a host build of one runs while the GPU builds the other
// get_barycentric_weights on the device for host-resident query points; q_on_device (optional): the same 3 x N points already in HBM (the vertices
// of a mesh handle of this context); the host copy then stays where it is
int query_host(msm_mesh *target, const double *q, int N, int *tri_id, int *vid, double *w, int mode, const char *what, const double *q_on_device = nullptr);
int ensure_tree(msm_mesh *m);  // build + upload the search structure if stale
// octree_kernels.hip: the same tree built in HBM from the mesh's device coordinates (MSM_ERR_CAPACITY: use the host build)
int gpu_build_octree(msm_mesh *m, const std::function<void()> *overlap = nullptr);
// B trees over one triangle list and B coordinate sets, built together (octree_kernels.hip: gpu_build_forest); the arrays of tree b
// start b * s_* elements into the shared buffers
struct Forest {
    int B = 0, T = 0, V = 0;
    size_t s_node = 0, s_leaf = 0, s_rec = 0, s_grid = 0;
    DevBuf<int4> node;
    DevBuf<int32_t> parent, leaf_tri, grid;
    DevBuf<double4> nodebox;
    DevBuf<float4> cone, tcone;
    DevBuf<TriRec> rec;
    DevBuf<double> box;
    DevBuf<int> ints, counters;
    int *h_counters = nullptr;  // pinned
    size_t h_counters_cap = 0;
    struct Info {
        int nnodes = 0, entries = 0, grid_depth = 0;
    };
    std::vector<Info> info;
    int last_levels = 0;  // the levels the deepest tree of the previous build needed: queued up front by the next one (no look in between)
    ~Forest() {
        if (h_counters) (void)hipHostFree(h_counters);
    }
};
// component a of vertex i of tree b at d_xyz[a * comp_stride + b * tree_stride + i]; MSM_ERR_CAPACITY: a tree outgrew its arrays
int gpu_build_forest(msm_ctx *ctx, Forest &f, const double *d_xyz, size_t comp_stride, size_t tree_stride, int V, const int32_t *d_tri, int T, int B);
int gpu_build_octree_begin(msm_mesh *m);   // the same in two halves: queue the build ... 
int gpu_build_octree_finish(msm_mesh *m);  // ... wait for it (one build at a time per context)
int ensure_tree_begin(msm_mesh *m);        // api.cpp: starts the GPU build of an invalid tree (no-op otherwise); ensure_tree() completes it
bool mesh_tree_on_gpu(const msm_mesh *m);  // api.cpp: is this mesh's tree built by the GPU kernels (large meshes) or on the host
int finish_tree(msm_mesh *m);       // what follows either build: validity flags, generation
int ensure_masks(msm_mesh *m);  // + the per-leaf sub-cell masks the cost kernels use (built on the GPU)
int ensure_rays(msm_mesh *m, bool wait = false);   // + the ray table of a simple surface (unary table kernels); see api.cpp
DevTree dev_tree(const msm_mesh *m);
int check_status(msm_ctx *ctx, const char *what);  // sync + read kernel status
int ctx_io_pinned(msm_ctx *ctx, size_t bytes, void **out);  // grow-only pinned scratch for small per-call transfers
// device address of [p, p + bytes) when it lies in a msm_host_alloc block of this context, else nullptr
void *ctx_mapped(msm_ctx *ctx, const void *p, size_t bytes);
int ctx_flag(msm_ctx *ctx);  // makes ctx->h_flag / d_flag_map available
int drop_ctx_pending(msm_ctx *ctx);  // label_step.cpp: the label step queued ahead on this context, if any, is waited for and discarded (see msm_ctx::pending_cost)
// host -> device on the context's stream: from where it lies when src is pinned memory of this context (msm_host_alloc / msm_host_register; complete on
// return, the caller may write the array again), through the staging blocks otherwise (src consumed on return, the copy queued; nothing waits)
int upload_staged(msm_ctx *ctx, void *dst, const void *src, size_t bytes);
// stager.cpp (stage_h2d / stage_d2h are declared in devbuf.hpp)
void stager_create(msm_ctx *ctx);
void stager_destroy(msm_ctx *ctx);  // the device is idle
void stager_stats(msm_ctx *ctx, int64_t out[4]);  // blocks, bytes, blocks ever allocated, waits for a busy block
int ctx_sync(msm_ctx *ctx);         // hipStreamSynchronize(ctx->stream) + what stage_d2h fetched goes to its destinations
void stage_deliver(msm_ctx *ctx);   // the second half alone (the stream has been synchronised by other means)
void stage_forget(msm_ctx *ctx);     // drops them instead
// An entry point that fails between a device -> host copy and its synchronisation must not leave the delivery behind: a later synchronisation would write
// into a local that is gone, or into an array the caller freed after the failed call.  Every error return starts at fail() on the thread that queued the
// copy, which calls this: the deliveries still pending on the context this thread last fetched through are dropped.
void stage_on_failure();
}  // namespace msm
