/*
 * msmhip.h -- C ABI of libmsmhip: the MI355X (gfx950) implementation of newMSM's data-parallel hot
 * path (octree nearest-triangle search + barycentric / adaptive-barycentric resampling, and the
 * discrete unary / pairwise / triplet label-cost evaluation).
 *
 * Every entry point names the reference interface it replaces (paths under
 * /root/reference/libraries/: R/ = msm-newresampler/src, M/ = msm-newmeshreg/src,
 * I/ = msm-newmeshreg/include).  INTEGRATION.md shows the binding a newMSM maintainer would add.
 *
 * Conventions
 *  - plain C types only; all arrays are caller-owned HOST memory unless a name ends in _dev;
 *  - point sets are SoA: xyz = x[0..N) y[0..N) z[0..N) (3 x N doubles); triangle lists are
 *    3 x T int32 (first, second, third vertex rows); feature matrices are D x V row-major doubles
 *    (the reference's pvalues[dim][vertex], R/mesh.h:45);
 *  - every function returning int returns MSM_OK (0) or a negative MSM_ERR_* code; the message is
 *    available from msm_last_error() (thread-local).  No exception crosses this boundary;
 *  - handles are opaque; a handle belongs to one context (one GPU, one HIP stream); calls on one
 *    context must be serialised by the caller (the reference's OpenMP loops become one launch);
 *  - lifetimes: a cost function / group keeps plain pointers to the meshes handed to it (target, source,
 *    control grid, anatomical sphere, template, subjects' data meshes): they must outlive it, and all of
 *    them must belong to its context (checked: MSM_ERR_INVALID).  Destroy cost functions and groups
 *    first, then meshes, then the context;
 *  - functions marked [host] need no GPU and may be called on a machine without one.  Everything
 *    else fails with MSM_ERR_NOGPU when no device is present: there is no CPU fallback.
 */
#ifndef MSMHIP_H
#define MSMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM_ABI_VERSION 12  /* 12: msm_ctx_set_mcmc_draw / msm_ctx_get_mcmc_draw / msm_mcmc_draw_thresholds / msm_mcmc_draw_block_bound / msm_mcmc_proposals_mirror / msm_mcmc_proposals_mirror_counted / msm_mcmc_draw_gpu / msm_mcmc_draw_stats added (the Monte Carlo optimiser's proposals drawn on the device; additive, the version stays).  12: msm_group_pair_route / msm_group_pair_launch added (which path of the pair-cost kernel a query takes, and what the group's launch was decided to be; additive, the version stays).  12: msm_mcmc_optimise_gpu / msm_cost_mcmc_optimise / msm_mcmc_gpu_stats / msm_mcmc_proposals / msm_mcmc_schedule added (the Monte Carlo optimiser's sweeps on the GPU; additive, the version stays).  12: msm_resample_plan_create_smooth / msm_resample_plan_divisors added (Gaussian smoothing as a fourth kind of plan row; additive, the version stays).  12: msm_cost_routes added (which kernel the last unary table and the last triclique label step ran); routes[MSM_ROUTE_MOVE_DEFERRED] fills a slot that was reserved and 0 (additive, the version stays).  11: msm_resample_plan_* added (weights built once, applied to many maps; additive, the version stays).  11: msm_dedrift_set_warp / msm_dedrift_group_stats_select added (merging registered groups up a hierarchy: a given warp, statistics over a list of subjects and a vertex mask; additive, the version stays).  11: msm_dedrift_create / _destroy / _reset / _accumulate / _finish / _correct / _set_map / _group_stats added (dedrifting and the statistics of a groupwise run; additive, the version stays).  11: msm_calculate_strains added (the strain map of an aMSM run; additive, the version stays).  11: msm_rigid_create / _destroy / _set_source / _get_source / _cost / _rotate / _run / _kernel_ms added (the rigid level; additive, the version stays).  11 (round 5): msm_ctx_wait_stream, msm_ctx_staging_stats, msm_group_context; msm_host_register takes whole pages only.  10 (round 4): msm_group_set_rotation_mode.  9 (round 4): msm_group_set_pair_layout.  8 (round 4): msm_query_lanes, msm_resample_anatomy_grid, msm_cost_triplet_octets_prefetch / msm_cost_prefetch_stats, msm_group_export_subjects_dev / msm_group_import_subjects_dev / msm_group_setup_more_subjects added.  6 (round 3): msm_pairwise_icm, msm_ctx_time_queries / msm_ctx_query_kernel_ms, msm_group_time_moves / msm_group_move_kernels_ms,
                             * msm_store_release_i64 / msm_load_acquire_i64 / msm_min_acquire_i64, msm_mesh_sphere_project_warp added; nothing removed or changed */

#define MSM_OK 0
#define MSM_ERR_INVALID (-1)  /* bad argument / inconsistent sizes */
#define MSM_ERR_HIP (-2)      /* HIP runtime failure */
#define MSM_ERR_OUTSIDE (-3)  /* "Point is not in the bounding box of the mesh", R/octree.cpp:158 */
#define MSM_ERR_NOTFOUND (-4) /* "Error in octree. ... too distorted mesh face", R/octree.cpp:210 */
#define MSM_ERR_NOGPU (-5)    /* no gfx950 device / extension unusable */
#define MSM_ERR_STATE (-6)    /* call order violated (e.g. cost evaluated before get_source_data) */
#define MSM_ERR_CAPACITY (-7) /* caller buffer too small */
#define MSM_ERR_ROTATION (-8) /* "rotation angle is greater than 90 degrees", R/point.cpp:112 */

#define MSM_RAD 100.0    /* R/point.h:32 */
#define MSM_FOLDING 1e7  /* M/reg_tools.h:30 */

typedef struct msm_ctx msm_ctx;
typedef struct msm_mesh msm_mesh;
typedef struct msm_cost msm_cost;

/* ------------------------------------------------------------------------------------------------
 * library
 * ---------------------------------------------------------------------------------------------- */
int         msm_abi_version(void);                 /* [host] */
const char *msm_last_error(void);                  /* [host] message of the last failing call on this thread */
int         msm_device_count(void);                /* [host] number of visible HIP devices (0 when none) */

/* ------------------------------------------------------------------------------------------------
 * [host] mesh utilities the reference keeps in R/mesh.cpp and M/DiscreteModel.cpp.  They produce
 * the inputs of the device path (numbering is observable in outputs, so they reproduce the
 * reference's vertex / triangle / neighbour order exactly).
 * ---------------------------------------------------------------------------------------------- */
/* vertex and triangle count of make_mesh_from_icosa(order); Mesh::get_resolution R/mesh.cpp:810-830 */
int msm_icosphere_counts(int order, int32_t *V, int32_t *T);
/* make_mesh_from_icosa(order) R/mesh.cpp:1111-1196 followed by true_rescale(radius) :1210-1219
 * (radius <= 0: keep the unit sphere).  Same vertex and triangle numbering as the reference. */
int msm_icosphere(int order, double radius, double *xyz, int32_t *tri);
/* Mpoint::nID / trID lists in Mesh::push_triangle order, R/mesh.cpp:115-134, as CSR.
 * nbr / tid may be NULL to size: nbr_ptr[V] / tid_ptr[V] give the lengths. */
int msm_mesh_adjacency(const int32_t *tri, int32_t V, int32_t T, int32_t *nbr_ptr, int32_t *nbr, int32_t *tid_ptr, int32_t *tid);
/* per-vertex mean adjacent triangle area: compute_vertex_area R/mesh.cpp:1275-1283 with the
 * triangle areas taken from the given coordinates (Triangle::calc_area R/triangle.cpp:52-55) */
int msm_vertex_areas(const double *xyz, const int32_t *tri, int32_t V, int32_t T, double *area);
/* Mesh_registration::resample_anatomy, M/mesh_registration.cpp:250-332, without its surface_resample call (msm_barycentric_coords_resample does that):
 * what a --regoption=5 (aMSM) level prepares for msm_cost_set_anatomical.  The control grid (3 x N SoA, 3 x Tc SoA) is retessellated `levels` (=
 * --anatgrid minus --CPgrid, >= 0) times as retessellate(mesh, old_tr_nbours) does it (R/mesh.cpp:1007-1109: children of triangle t numbered 4t .. 4t+3,
 * every vertex re-normalised) and rescaled to `rad` (true_rescale) -> ANAT_ico (axyz 3 x Va SoA, atri 3 x Ta SoA); face_ptr (Tc + 1) / face_idx (Ta):
 * NEARESTFACES, the faces of ANAT_ico under every control triangle IN THE REFERENCE'S ORDER (each pass after the first puts an entry's children in
 * front of the list, :268-283; the order is the summation order of the mean anatomical strain); w_ptr (Va + 1) / w_cp / w_val (3 Va each):
 * _ANATbaryweights, calc_barycentric_weights (R/triangle.cpp:124-143) of every ANAT_ico vertex in the control triangle that names it LAST in the loop
 * :303-321, control point ids ascending within a row (std::map order).  With every output pointer NULL the call only returns the sizes *Va, *Ta. */
int msm_resample_anatomy_grid(const double *cp_xyz, int32_t N, const int32_t *cp_tri, int32_t Tc, int32_t levels, double rad, int32_t *Va, int32_t *Ta,
                              double *axyz, int32_t *atri, int32_t *w_ptr, int32_t *w_cp, double *w_val, int32_t *face_ptr, int32_t *face_idx);
/* NonLinearSRegDiscreteModel::Initialize M/DiscreteModel.cpp:72-89: per control point the largest
 * geodesic distance to a neighbour, and Mesh::calculate_MaxVD R/mesh.cpp:263-277 */
int msm_cp_spacings(const double *xyz, const int32_t *tri, int32_t V, int32_t T, double *maxsep, double *mvdmax);
/* Initialize_sampling_grid + label_sampling_grid M/DiscreteModel.cpp:110-190 on the icosphere of
 * order sg_order (radius 100).  samples / barycentres: 3 x cap SoA, entry 0 is the centre.
 * abs_is_int != 0 selects the int abs() overload the reference may bind at :170 (SURVEY hard parts). */
int msm_label_sampling_grid(int sg_order, double max_dist, int abs_is_int, int32_t cap,
                            double *samples, int32_t *nsamples, double *barycentres, int32_t *nbarycentres);
/* rescale_sampling_grid M/DiscreteModel.cpp:192-214; *scale is read and updated (x0.8) */
int msm_rescale_sampling_grid(const double *samples, int32_t n, double *scale, double *labels);
/* estimate_rotation_matrix R/point.cpp:97-152, row-major 3x3 */
int msm_rotation_matrix(const double ci[3], const double index[3], double R[9]);
/* get_rotations M/DiscreteModel.cpp:310-319: rot[9*k..] = R(centre -> cp[k]) row-major */
int msm_cp_rotations(const double centre[3], const double *cp_xyz, int32_t N, double *rot);
/* estimate_triplets M/DiscreteModel.cpp:291-308 (triplets: 3 per triangle, ascending, AoS T x 3 as
 * the optimisers expect) and estimate_pairs :271-289 (pairs may be NULL to count; returns count) */
int msm_estimate_triplets(const int32_t *tri, int32_t T, int32_t *triplets);
int msm_estimate_pairs(const int32_t *tri, int32_t V, int32_t T, int32_t *pairs);
/* testing hook: the search tree (newresampler::Octree, R/octree.cpp:31-141) of a mesh, built on the host without a GPU:
 * stats as msm_mesh_octree_stats, and a signature of the leaves (box + triangle list in stored order of every leaf) */
int msm_octree_signature(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int64_t stats[5], uint64_t *signature);
/* testing hook, host only: the guarantee of the direction table that the cost kernels search simple-surface targets with (csrc/ray_table.cpp:
 * build_ray_table), checked at nsamples points (random directions; points next to random edges and vertices) against the first pass of
 * Octree::get_closest_triangle (R/octree.cpp:156-178) over the host-built tree: whatever a kernel may accept must be the one listed triangle
 * that passes the inside test.  report: [0] points [1] accepted by the float test [2] only by the FP64 re-test [3] left to the complete search
 * [4] violations (must be 0) [5] triangles the table cannot use [6] triangles with exclusion boxes [7] simple surface [8] exclusion boxes
 * checked one by one (the centre of the leaf a box stands for must be refused) [9] sampled points refused by the boxes alone */
int msm_ray_table_check(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int32_t nsamples, uint64_t seed, int64_t report[10]);
/* testing hook, host only: the first-candidate hints of the direction table's cells (which of a cell's candidates a kernel tries first, by sub-cell),
 * at nsamples random directions on the radius shell; a point's triangle is the one the first pass of Octree::get_closest_triangle returns, found as
 * msm_ray_table_check finds it.  report: [0] points [1] points whose triangle is the hinted first candidate [2] points whose triangle is the first
 * stored candidate, hints ignored [3] points whose triangle is anywhere in the cell's list [4] cells whose decoded candidates differ from the stored
 * ones (must be 0) [5] cells [6] cells with more than four candidates [7] sub-cells per cell axis.  cells: NULL, or room for cells_cap words
 * (4 x [5] are needed) that receive the cell array as stored. */
int msm_ray_hint_check(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int32_t nsamples, uint64_t seed, int64_t report[8], int32_t *cells,
                       int64_t cells_cap);
/* testing hook, host only: how deep in its cell's candidate list a point's triangle sits, in the order a kernel tries the candidates (the hinted first
 * candidate, the other two of the cell, then the fourth or the four of the cell's further-candidate entry), at msm_ray_hint_check's points and with its
 * notion of a point's triangle.  report: [0] points [1..5] points whose triangle is at position 0, 1, 2, 3, 4 [6] at position 5 or beyond [7] not listed
 * (a point without a triangle counts in [0] only). */
int msm_ray_depth_check(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int32_t nsamples, uint64_t seed, int64_t report[8]);
/* testing hook, host only: the certificates of the direction table's cells (one bit per sub-cell: the hinted first candidate is the answer for every
 * direction of the sub-cell, and a kernel takes it without its acceptance test), at nsamples random directions and some 10 000 placed ones: next to
 * sub-cell and cell borders and corners, cube-face edges and corners, through mesh vertices, and next to edge midpoints.  report: [0] points [1] points in a
 * certified sub-cell [2] of those, points whose first candidate fails the FP64 edge-plane test at the threshold the table's proof asks for (must be 0)
 * [3] of those, points for which the first pass of Octree::get_closest_triangle does not return it (must be 0) [4] sub-cells [5] certified sub-cells
 * [6] cells [7] placed points.  cells: as msm_ray_hint_check.  MSMHIP_RAY_CERTS=off (read when a table is built) writes no certificates. */
int msm_ray_cert_check(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int32_t nsamples, uint64_t seed, int64_t report[8], int32_t *cells,
                       int64_t cells_cap);
/* testing hook, host only: a signature of the whole direction table of a mesh, as the host builds it.  out: [0] cells per face axis (0: no table, and
 * every count is zero) [1] simple surface [2] built with certificates [3..6] elements of the cell, edge-plane, further-candidate and exclusion arrays
 * [7] [8] the bit patterns of the squared radius range [9..12] 64-bit FNV-1a over the raw bytes of those four arrays. */
int msm_ray_table_signature(const double *xyz, const int32_t *tri, int32_t V, int32_t T, uint64_t out[13]);

/* ------------------------------------------------------------------------------------------------
 * context: one per GPU
 * ---------------------------------------------------------------------------------------------- */
msm_ctx *msm_ctx_create(int device);                         /* owns a new non-blocking HIP stream */
msm_ctx *msm_ctx_create_on_stream(int device, void *hip_stream); /* launches on the caller's stream */
void     msm_ctx_destroy(msm_ctx *ctx);
int      msm_ctx_synchronize(msm_ctx *ctx);
void    *msm_ctx_stream(msm_ctx *ctx);                        /* hipStream_t, for event timing */
/* Optional HIP-event timing of the search kernel of msm_query_triangles / msm_closest_vertex (bench.py's `resample` object): with
 * enable != 0 every such call records two events around its kernel on the context's stream; msm_ctx_query_kernel_ms returns the
 * duration of the most recent one in milliseconds (-1 when none was timed). */
/* [host] Release / acquire accesses to 64-bit counters in memory shared between the ranks of a node (newmsm_amd/dist.py:
 * SharedStepBuffer: a producer's slice of a label step must be visible before its progress counter, the consumer's reads must not
 * move before its look at the counters).  __atomic_store_n(.., __ATOMIC_RELEASE) / __atomic_load_n(.., __ATOMIC_ACQUIRE). */
void     msm_store_release_i64(int64_t *addr, int64_t value);
int64_t  msm_load_acquire_i64(const int64_t *addr);
int64_t  msm_min_acquire_i64(const int64_t *addr, int32_t n);   /* the smallest of n counters, each read with acquire semantics */
/* Stream contract.  A context from msm_ctx_create owns a NON-BLOCKING stream: nothing it runs orders against the caller's streams (not even the
 * default stream), and every entry point that takes HOST arrays is complete when it returns.  The entry points that take DEVICE pointers of the
 * caller (msm_group_export_subject(s)_dev, msm_group_import_subject(s)_dev, msm_group_fusion_move_dev, ...) read and write them on the context's
 * stream, therefore:
 *   before the call   the caller's pending work on those buffers (a memset, a collective that fills them, a kernel) must be complete -- or ordered
 *                     by msm_ctx_wait_stream(ctx, your_stream): everything the library queues after it waits for what your_stream held when it
 *                     was called (one event, no host wait; your_stream = NULL names the default stream).  Without either, a late fill of yours
 *                     lands on top of what the library wrote (the race DESIGN.md section 6 describes).
 *   after the call    the library's work on the buffers is complete: every such entry point synchronises the context's stream before it returns,
 *                     so any stream may use them.
 * A context from msm_ctx_create_on_stream runs on the caller's stream and orders with the rest of that stream as usual. */
int      msm_ctx_wait_stream(msm_ctx *ctx, void *hip_stream);
/* [diagnostics] the pinned staging blocks of the context's host <-> device copies (csrc/stager.cpp): out[0] blocks, out[1] their bytes, out[2] blocks ever
 * allocated, out[3] times a copy waited for a busy block.  Blocks are never moved or freed before the context goes. */
int      msm_ctx_staging_stats(msm_ctx *ctx, int64_t out[4]);
int      msm_ctx_time_queries(msm_ctx *ctx, int enable);
int      msm_ctx_query_kernel_ms(msm_ctx *ctx, double *ms);
int      msm_query_lanes(int64_t n_queries);                 /* [host] lanes per query (4 or 8) the search kernels use for a launch of n_queries: names the instantiation a profile shows */
/* Pinned host memory mapped into the GPU's address space.  An output array that lies inside such a block is written by the
 * kernels directly (no staging copy, no copy-engine command): use it for the arrays of the optimisers' inner loop --
 * msm_cost_triplet_octets' E, msm_group_fusion_move's pair_quads / triplet_octets -- the counterpart of the buffers
 * Fusion::optimize keeps per label step (I/Fusion/Fusion.h:142-146).  Plain malloc'ed arrays keep working everywhere.
 * The block belongs to the context and is released with it at the latest. */
void    *msm_host_alloc(msm_ctx *ctx, size_t bytes);
void     msm_host_free(msm_ctx *ctx, void *p);
/* The same for memory the caller owns -- e.g. a POSIX shared-memory segment that the processes of one node (one per GPU) map, so
 * that every rank's kernels deliver their slice of a label step into the optimiser rank's address space without a collective.
 * msm_host_free(ctx, p) undoes the registration (the memory stays the caller's).  p must be page aligned and bytes a multiple of the page
 * size (4096; MSM_ERR_INVALID otherwise): page-locking works on whole pages and the device address of the block is its host address, so a
 * range that shares a page with other data would share that page's GPU mapping with whatever else gets locked there -- the HIP runtime
 * page-locks pageable buffers of asynchronous copies on its own -- and the first of the two to be released unmaps it under the other. */
int      msm_host_register(msm_ctx *ctx, void *p, size_t bytes);

/* ------------------------------------------------------------------------------------------------
 * mesh + search structure.  Replaces newresampler::Mesh (coords/triangles/pvalues) as seen by the
 * hot path and newresampler::Octree(const Mesh&) R/octree.h:48-52, R/octree.cpp:31-141.  The
 * octree is built on first use and rebuilt after msm_mesh_update_coords (the reference constructs a
 * new Octree per call site).
 * ---------------------------------------------------------------------------------------------- */
msm_mesh *msm_mesh_create(msm_ctx *ctx, const double *xyz, int32_t V, const int32_t *tri, int32_t T);
void      msm_mesh_destroy(msm_mesh *m);
int       msm_mesh_update_coords(msm_mesh *m, const double *xyz);   /* Mesh::set_coord for all vertices */
int       msm_mesh_get_coords(msm_mesh *m, double *xyz);
int       msm_mesh_set_features(msm_mesh *m, const double *feat, int32_t D); /* Mesh::set_pvalues */
int       msm_mesh_sizes(const msm_mesh *m, int32_t *V, int32_t *T, int32_t *D);
/* [host part] stats[0]=nodes [1]=leaves [2]=max depth (root 0) [3]=triangle references [4]=largest leaf */
int       msm_mesh_octree_stats(msm_mesh *m, int64_t stats[5]);
/* testing hook: stats + the leaf signature of msm_octree_signature, computed from the tree as it sits in HBM.  Trees of
 * meshes with >= 8192 triangles are built on the GPU (level by level, the same leaves in the same order); MSMHIP_OCTREE=host|gpu
 * forces one of the two builds. */
int       msm_mesh_octree_signature(msm_mesh *m, int64_t stats[5], uint64_t *signature);
/* The same signature for B coordinate sets (xyz: B consecutive 3 x V SoA blocks) over one triangle list, the B trees built together
 * as one forest -- how the gMSM set-up builds the trees of a subject's data mesh rotated to every label (testing aid). */
int       msm_octree_forest_signatures(msm_ctx *ctx, const double *xyz, int32_t V, const int32_t *tri, int32_t T, int32_t B, uint64_t *signatures);
/* Builds the search structures a cost function uses on this mesh as its target (octree, and for a closed star-shaped
 * surface the direction table that settles most searches with one lookup).  The direction table takes tens of ms of
 * host time, so by default it is built on a background thread when a cost function first evaluates against the mesh,
 * and the complete octree search serves until it is ready -- with bit-identical results.  wait != 0 blocks until
 * everything is in place (benchmarks, many evaluations against one target); wait == 0 only starts the work.
 * *ready (optional) = 1 when nothing is pending.  MSMHIP_RAYTABLE=sync|off changes the default for all meshes. */
int       msm_mesh_prepare_search(msm_mesh *m, int wait, int32_t *ready);

/* ------------------------------------------------------------------------------------------------
 * resampler (R/resampler.h:38-53)
 * ---------------------------------------------------------------------------------------------- */
#define MSM_WEIGHTS_PROJECTED 0 /* calc_barycentric_weights R/triangle.cpp:124-143 (query ray-projected) */
#define MSM_WEIGHTS_RAW 1       /* the area ratios inside barycentric_interpolation :145-157 (query as given) */
/* Octree::get_closest_triangle R/octree.cpp:156-214 for N points + Resampler::get_barycentric_weights
 * R/resampler.cpp:142-167.  tri_id[N]; v_id 3 x N (triangle vertex order); w 3 x N.  Any output may be NULL.
 * A failing query yields tri_id < 0 (MSM_ERR_OUTSIDE / MSM_ERR_NOTFOUND) and the call returns the first such code. */
int msm_query_triangles(msm_mesh *target, const double *q_xyz, int32_t N, int32_t *tri_id, int32_t *v_id, double *w, int weight_mode);
/* Octree::get_closest_vertex_ID R/octree.cpp:216-233 */
int msm_closest_vertex(msm_mesh *target, const double *q_xyz, int32_t N, int32_t *v_id);
/* Resampler::get_adaptive_barycentric_weights R/resampler.cpp:72-140 as CSR (rows = vertices of new_mesh,
 * columns ascending = std::map order).  excl (length V of in_mesh) may be NULL.  Vertex areas are taken
 * from the meshes' current coordinates.  Call with col == NULL to obtain *nnz only. */
int msm_adaptive_barycentric_weights(msm_mesh *in_mesh, msm_mesh *new_mesh, const double *excl,
                                     int32_t *row_ptr, int32_t *col, double *val, int64_t cap, int64_t *nnz);
/* metric_resample R/resampler.cpp:304-309 (= barycentric_data_interpolation :30-70): data D x V(in_mesh) -> out D x V(new_mesh).
 * excl (optional, V(in_mesh) values: the EXCL mesh's data, 0 = excluded) masks the weights and the sums as in :38-52;
 * excl_out (optional, V(new_mesh)) is the resampled mask the reference writes back into EXCL (:54-67). */
int msm_metric_resample(msm_mesh *in_mesh, const double *data, int32_t D, msm_mesh *new_mesh, const double *excl, double *out, double *excl_out);
/* sphere_project_warp R/resampler.cpp:311-328: sphere (3 x N, in/out) is carried through from -> to_xyz (3 x V(from)) */
int msm_sphere_project_warp(msm_mesh *from, const double *to_xyz, double *sphere_xyz, int32_t N);
/* The same for the coordinates a mesh handle already holds: `sphere`'s vertices are located on `from` and moved through (from -> to_xyz) in place on
 * the device, its host copy follows -- SPH_reg of Mesh_registration::run_discrete_opt (M/mesh_registration.cpp:224) without three host round trips.
 * to_xyz: 3 x V(from) SoA.  Same context for both meshes.  Bit-identical to msm_sphere_project_warp on the same inputs. */
int msm_mesh_sphere_project_warp(msm_mesh *sphere, msm_mesh *from, const double *to_xyz);
/* surface_resample :284-302 / project_anatomical_mesh :260-282 core: out = sum_j w_j * coords[v_j] for the
 * barycentric weights of q against `from` (no renormalisation); coords 3 x V(from), out 3 x N */
int msm_barycentric_coords_resample(msm_mesh *from, const double *coords_xyz, const double *q_xyz, int32_t N, double *out_xyz);
/* smooth_data R/resampler.cpp:168-230: Gaussian smoothing (std sigma, geodesic) of D x V(orig) data rows onto the vertices
 * of sphlow, with the reference's indexing (orig's octree finds the centre, whose id then indexes sphlow; neighbours
 * run over sphlow's vertices and read orig's data by the same id -- i.e. meant for orig and sphlow being the same
 * sphere).  excl (optional, V(orig) values) is the EXCL mesh's data and excl_out (optional, V(sphlow)) the smoothed
 * mask the reference writes back.  check_scale (R/mesh.cpp:1198-1208) is left to the caller.  out: D x V(sphlow). */
int msm_smooth_data(msm_mesh *orig, const double *data, int32_t D, msm_mesh *sphlow, double sigma, const double *excl, double *out, double *excl_out);
/* nearest_neighbour_interpolation R/resampler.cpp:232-258: data D x V(orig) -> out D x N.  With excl (optional, V(orig)) a
 * query whose closest vertex is excluded (0) gets zeros, and excl_out (optional, N) receives the mask at the queries. */
int msm_nearest_neighbour(msm_mesh *orig, const double *data, int32_t D, const double *q_xyz, int32_t N, const double *excl, double *out, double *excl_out);
/* [host] create_exclusion R/mesh.cpp:1257-1273: excl[i] = 1 when some feature of vertex i lies outside [thrl - EPSILON,
 * thru + EPSILON], else 0 (as written in the reference: the mask marks the vertices to cut with 1).  data D x V. */
int msm_create_exclusion(const double *data, int32_t D, int32_t V, double thrl, double thru, double *excl);

/* ------------------------------------------------------------------------------------------------
 * resampling plan: the weights of one (in_mesh -> new_mesh) pair built once and applied to any number of maps.  Replaces the bodies of the
 * reference's resampler programs (R/../demo: metric-resample, NN-resample, surface-resample) and of `wb_command -metric-resample` /
 * `-label-resample` in its scripts (gMSM_scripts/run_gMSM.sh:95), which rebuild two octrees and the weights for every file.
 * A plan is a SNAPSHOT: it owns device copies of its rows (and of excl), so later calls on the context, msm_mesh_update_coords on either mesh or
 * destroying either mesh do not change what it does.  It belongs to in_mesh's context: destroy it before that context.
 * Data and results are D x V row-major (one map after another); D is 64-bit.
 * Arithmetic of an apply, for row k and map d: acc = 0.0; for the row's entries in stored order, skipping col < 0 and, with a mask, excl[col] == 0:
 * acc += (double)data[d][col] * val (FP64, product and sum rounded separately).  MSM_F64 stores acc, MSM_F32 stores (float)acc (one rounding to nearest
 * even); a row without kept entries gives 0.  Two runs give the same bits.
 * ---------------------------------------------------------------------------------------------- */
typedef struct msm_resample_plan msm_resample_plan;
#define MSM_RESAMPLE_ADAP_BARY   0  /* Resampler::get_adaptive_barycentric_weights, R/resampler.cpp:72-140: metric_resample's rows */
#define MSM_RESAMPLE_BARYCENTRIC 1  /* get_barycentric_weights :142-167 of new_mesh's vertices on in_mesh, ascending ids: surface_resample's rows (:284-302) */
#define MSM_RESAMPLE_NEAREST     2  /* nearest_neighbour_interpolation :232-258: one entry of weight 1 per row */
#define MSM_RESAMPLE_SMOOTH      3  /* smooth_data R/resampler.cpp:168-230: only through msm_resample_plan_create_smooth */
#define MSM_F64 0
#define MSM_F32 1
/* excl: V(in_mesh) values (the EXCL mesh's data, 0 = excluded) or NULL.  NULL on failure (msm_last_error): meshes of different contexts, an unknown
 * method, a failed search (MSM_ERR_OUTSIDE / MSM_ERR_NOTFOUND, as msm_metric_resample fails). */
msm_resample_plan *msm_resample_plan_create(msm_mesh *in_mesh, msm_mesh *new_mesh, int method, const double *excl);
/* Gaussian smoothing (msm_smooth_data above, with its arguments and its indexing) as a plan: the neighbourhood sweep runs once, on the device, and the
 * rows stay in HBM.  V_in = V(orig), V_out = V(sphlow).  Row i: c = the vertex of orig closest to sphlow's vertex i; the entries are the vertices n of
 * sphlow with (unit[n] | unit[c]) >= cos(4 asin(sigma / 2R)) in ascending n, val = gain * exp(-(g * g) / (2 sigma^2)) with
 * g = 2R asin(|unit[c] - unit[n]| / 2R), gain = 1 / sqrt(2 pi sigma^2), multiplied by excl[n] when excl (V(orig) values) is given: the mask is part of
 * the stored weights, an apply skips nothing.  Per row, summed in stored order from 0.0: the divisor SUM of the stored weights, and with a mask
 * excl_out = SUM / (the sum of the unmasked weights), 0 where that is 0.  A centre with excl[c] <= 0 gives an empty row, divisor 0, excl_out 0.
 * An apply sums acc += (double)data[d][col] * val in stored order as every plan does and then, where the row's divisor is not 0.0, stores
 * acc / divisor (one FP64 division): msm_smooth_data's arithmetic -- an MSM_F64 apply gives its bits, a NaN that meets a zero weight included.
 * msm_resample_plan_apply hands out excl_out for a plan with excl; msm_resample_plan_apply_labels refuses a smoothing plan (MSM_ERR_INVALID).
 * NULL on failure: sigma <= 0, V(orig) < V(sphlow), meshes of different contexts, more than INT32_MAX entries (a large sigma on ico7).
 * msm_resample_plan_create refuses MSM_RESAMPLE_SMOOTH as an unknown method: it has no sigma. */
msm_resample_plan *msm_resample_plan_create_smooth(msm_mesh *orig, msm_mesh *sphlow, double sigma, const double *excl);
void msm_resample_plan_destroy(msm_resample_plan *p);
/* [host] any pointer may be NULL */
int  msm_resample_plan_sizes(const msm_resample_plan *p, int32_t *V_in, int32_t *V_out, int64_t *nnz, int32_t *longest_row);
/* the rows as CSR (row_ptr: V_out + 1; col / val: nnz entries, cap = their capacity; any of the three may be NULL), read back from the device */
int  msm_resample_plan_weights(msm_resample_plan *p, int32_t *row_ptr, int32_t *col, double *val, int64_t cap);
/* div: V_out values, the divisor of every row.  0.0 means "not divided": every row of the three resampling methods, and the rows of a smoothing plan
 * whose weights sum to 0 */
int  msm_resample_plan_divisors(msm_resample_plan *p, double *div);
/* data: D x V_in host array of dtype (MSM_F64: double, MSM_F32: float); out: D x V_out of the same type.  excl_out (optional, V_out): the resampled
 * mask of a plan with excl (:54-67; NEAREST: the mask at the closest vertex, :244-249), zeros for a plan without.  The maps travel through the context's
 * pinned staging blocks in slabs of a fixed device budget (64 MiB of maps; MSMHIP_PLAN_CHUNK_KB overrides), whatever D is.  D == 0: nothing is done. */
int  msm_resample_plan_apply(msm_resample_plan *p, const void *data, int dtype, int64_t D, void *out, double *excl_out);
/* the same for the caller's DEVICE arrays, read and written on the context's stream under the stream contract above (msm_ctx_wait_stream orders the
 * caller's pending work before the call; the context's stream is synchronised before it returns).  No mask output. */
int  msm_resample_plan_apply_dev(msm_resample_plan *p, const void *data_dev, int dtype, int64_t D, void *out_dev);
/* Integer keys (a parcellation) through the plan's rows: the largest-summed-weight vote `wb_command -label-resample ADAP_BARY_AREA` stands for (the
 * reference itself has nearest-vertex only).  For row k and every distinct key among its kept entries: the sum of val over the entries holding that
 * key, in stored order from 0.0; the largest sum wins, an exact tie goes to the smallest key, a row without kept entries gets `unassigned`
 * (tests/resample_literal.py).  labels: D x V_in, out: D x V_out. */
int  msm_resample_plan_apply_labels(msm_resample_plan *p, const int32_t *labels, int64_t D, int32_t unassigned, int32_t *out);

/* ------------------------------------------------------------------------------------------------
 * the callers' side of one iteration (run_discrete_opt, M/mesh_registration.cpp:164-232): what sits between two
 * evaluations of the cost tables besides the optimiser's own data structures
 * ---------------------------------------------------------------------------------------------- */
/* unfold M/reg_tools.cpp:131-178 on the mesh's current coordinates (sphere of the given radius; the reference uses RAD = 100):
 * the fold test check_for_intersections :118-129 runs on the GPU for all vertices; when some are folded (rare) their
 * gradients and the step-halving moves are applied on the host in the reference's serial order, and the test repeats
 * (at most 1000 passes).  *passes = passes that moved vertices (0: nothing folded, coordinates untouched),
 * *first_folded = folded vertices found by the first pass; both optional.  Read the result with msm_mesh_get_coords. */
int msm_mesh_unfold(msm_mesh *m, double radius, int32_t *passes, int32_t *first_folded);
/* [host] variance_normalise M/reg_tools.cpp:804-843: data D x V in place; excl (V values, > 0 keeps the vertex) or NULL.
 * The running mean / variance recurrence of the reference is serial per feature row, so it stays on the host. */
int msm_variance_normalise(double *data, int32_t D, int32_t V, const double *excl);
/* multivariate_histogram_normalization M/reg_tools.cpp:745-802 (--IN / --INc) on the GPU: every feature row of n_src source matrices (src: n_src x D x Vs)
 * is matched to the same row of ONE target matrix (ref: D x Vt) through 256-bin histograms, whose statistics are computed once.  The reference
 * hands the matching itself to FSL's MISCMATHS::Histogram (generate / generateCDF / match), which is not in its tree: the definition followed here is
 * written down in DESIGN.md section 5.11 and restated in tests/histmatch_literal.py; agreement with FSL itself is unpinned.  A value is counted when it
 * is finite and its mask is > 0; src_excl (optional: n_src x src_excl_rows x Vs) and ref_excl (optional: ref_excl_rows x Vt) are the EXCL meshes' data,
 * row d of a mask serves feature row d when the mask has that many rows, row 0 otherwise (:764-767).  Counted source values become the target value at
 * their quantile; the others, and rows without counted values or without a range on either side, stay as they are.  out: n_src x D x Vs (may be src). */
int msm_histogram_match(msm_ctx *ctx, int32_t n_src, int32_t D, int32_t Vs, const double *src, const double *src_excl, int32_t src_excl_rows,
                        int32_t Vt, const double *ref, const double *ref_excl, int32_t ref_excl_rows, double *out);
typedef struct msm_level_features_params {
    int32_t exclude;    /* masks exist: --excl, or the cut of --INc (M/featurespace.cpp:61) */
    int32_t intensity;  /* --IN / --INc: data set i >= 1 matched to data set 0 (:76-78) */
    int32_t varnorm;    /* --VN (:81-83) */
    int32_t reserved;
    double  thrl, thru; /* --cutthr */
} msm_level_features_params;
/* featurespace::initialise (M/featurespace.cpp:39-86) for n data sets on one level grid, in one call: per data set msm_create_exclusion (with
 * p->exclude), msm_metric_resample onto the grid and msm_smooth_data on the grid (sigma[i] > 0), then over all of them msm_histogram_match of data
 * sets 1 .. n-1 against data set 0 with the masks as they stand after smoothing (p->intensity, n > 1) and msm_variance_normalise (p->varnorm) -- the
 * bytes that sequence of entry points gives, with everything but the variance recurrence queued on the device behind one upload per data set and
 * in front of one download; the masked list surgery runs on the device too.  All meshes belong to one context.
 * data[i]: D x V(in_mesh[i]) host rows.  sigma[i]: <= 0 means no smoothing.
 * feat: n x D x V(grid).  mask: n x V(grid), required when p->exclude, else NULL.  A failed search fails the call as msm_metric_resample fails it. */
int msm_level_features(msm_mesh *grid, int32_t n, msm_mesh *const *in_mesh, const double *const *data, int32_t D, const double *sigma,
                       const msm_level_features_params *p, double *feat, double *mask);
/* [host] MCMC::optimise M/mcmc_opt.h:31-134 over the tables of msm_cost_unary_table (L x N) and msm_cost_triplet_table
 * (T x L x L x L): `iters` sweeps over the triplets, each proposing one label drawn from std::geometric_distribution(mcparam)
 * (std::mt19937 seeded with `seed`; the reference seeds from std::random_device) and keeping the cheapest of the eight
 * combinations.  labeling (N) is read and updated.  The energy the reference returns is msm_cost_total(labeling). */
int msm_mcmc_optimise(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, double mcparam,
                      int32_t iters, uint64_t seed, int32_t *labeling);
/* MCMC::optimise M/mcmc_opt.h:31-134 with the sweeps on the GPU: the labelling msm_mcmc_optimise gives for the same arguments, bit for bit.  The host
 * tables are uploaded through the context's staging blocks; one workgroup walks the triplets level by level (a triplet's level is one above the highest
 * level of the earlier triplets that share a node with it, so the triplets of a level are independent) with the labelling in LDS, and takes its
 * proposals from the host's own stream (std::mt19937 + std::geometric_distribution, drawn chunk by chunk while the device works on the chunk before;
 * MSMHIP_MCMC_CHUNK_SWEEPS sets the sweeps per chunk).  Argument checks and messages are msm_mcmc_optimise's; additionally L > 65535 is refused
 * (MSM_ERR_INVALID) and N > 80000 (the labelling does not fit a workgroup's LDS: MSM_ERR_CAPACITY).  iters == 0 or T == 0 leave the labelling as it is. */
int msm_mcmc_optimise_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T,
                          double mcparam, int32_t iters, uint64_t seed, int32_t *labeling);
/* What the last msm_mcmc_optimise_gpu / msm_cost_mcmc_optimise on the context did: stats[0] ms in the sweep kernels (HIP events), [1] levels walked,
 * [2] ms the host spent drawing proposals, [3] chunks, [4] levels of one sweep, [5] the widest level. */
int msm_mcmc_gpu_stats(msm_ctx *ctx, double stats[6]);
/* K chains of msm_mcmc_optimise_gpu from one start, side by side in one launch per chunk (a workgroup per chain over the same two tables): chain k is
 * msm_mcmc_optimise(..., seeds[k], ...) bit for bit.  labelings: K x N out (may be NULL); energies: K out (may be NULL); labeling (N): the start in,
 * chain *best's labelling out (best may be NULL).  The energy of a chain is msm_mcmc_energy of its labelling, *best is msm_mcmc_best of the energies.
 * 1 <= K <= 256 and seeds given, else MSM_ERR_INVALID; the other checks and messages are msm_mcmc_optimise_gpu's.  iters == 0 or T == 0: every chain
 * is the start, *best = 0.  The K proposal streams are drawn on up to min(MSMHIP_HOST_THREADS, 16, K) host threads; MSMHIP_MCMC_CHUNK_SWEEPS counts
 * sweeps per chain (default: half a million proposals per chain, at most 16 MB over all chains).  Afterwards msm_mcmc_gpu_stats gives [0] kernel ms,
 * [1] levels walked by one chain, [2] wall ms of the threaded draw, [3] chunks, [4] and [5] as before. */
int msm_mcmc_optimise_chains_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T,
                                 double mcparam, int32_t iters, const uint64_t *seeds, int32_t K, int32_t *labeling, int32_t *labelings, double *energies,
                                 int32_t *best);
/* [host] The same over host tables: K runs of msm_mcmc_optimise from the one start (on the host worker threads), msm_mcmc_energy, msm_mcmc_best. */
int msm_mcmc_optimise_chains(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, double mcparam,
                             int32_t iters, const uint64_t *seeds, int32_t K, int32_t *labeling, int32_t *labelings, double *energies, int32_t *best);
/* [host] The table form of evaluateTotalCostSum (M/DiscreteCostFunction.cpp:55-77): (sum over i < N ascending, from 0.0, of unary[labeling[i] * N + i])
 * + 0.0 + (sum over t < T ascending, from 0.0, of tcosts[t][la][lb][lc]). */
int msm_mcmc_energy(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const int32_t *labeling,
                    double *energy);
/* [host] std::min_element's rule over K >= 1 energies: the first index no later energy is strictly smaller than (ties go to the lower index, a NaN never
 * beats anything, nothing beats a NaN in slot 0). */
int msm_mcmc_best(const double *energies, int32_t K, int32_t *best);
/* Chains and host draw threads of the last msm_mcmc_optimise*_gpu / msm_cost_mcmc_optimise* call on the context (1 and 1 after a single-chain call). */
int msm_mcmc_chains_info(msm_ctx *ctx, int32_t *K, int32_t *draw_threads);
/* [host] The proposal stream both optimisers consume: out[s * T + t] is the label proposed to triplet t in sweep s (sweeps x T values), drawn in chunks of
 * chunk_sweeps whole sweeps (<= 0: one chunk); the stream does not depend on the chunking.  L > 65535: MSM_ERR_INVALID. */
int msm_mcmc_proposals(int32_t L, double mcparam, uint64_t seed, int32_t T, int32_t sweeps, int32_t chunk_sweeps, uint16_t *out);
/* [host] Where the GPU entry points of the Monte Carlo optimiser (msm_mcmc_optimise_gpu, msm_mcmc_optimise_chains_gpu, msm_cost_mcmc_optimise,
 * msm_cost_mcmc_optimise_chains) get their proposals on this context.  mode 0 (the default): from the host's stream, as described above.  mode 1: a
 * kernel draws them, a workgroup per chain with the chain's std::mt19937 state in LDS, the labels taken from thresholds the host locates once per call
 * with its own log (msm_mcmc_draw_thresholds) -- the same proposals, labellings, energies and bytes.  The draw of chunk c + 1 runs on a side stream the
 * context owns beside the sweeps of chunk c; it starts behind what the context's stream held at the call and is joined to that stream before the
 * downloads, so the stream contract above describes these entry points in either mode.  After a mode 1 call msm_mcmc_gpu_stats[2] is 0 and
 * msm_mcmc_chains_info's draw threads are 0.  Any other mode: MSM_ERR_INVALID.  The host optimisers ignore the mode. */
int msm_ctx_set_mcmc_draw(msm_ctx *ctx, int32_t mode);
int msm_ctx_get_mcmc_draw(msm_ctx *ctx, int32_t *mode);
/* [host] The steps of the host's label function floor(log(x) / log(1 - mcparam)) over x = 1 - u in [2^-53, 1]: thr[k - 1], k = 1 .. L, is the bit pattern
 * of the smallest such double whose label is at most k - 1 (2^-53's pattern where even that one's is), found by bisection on bit patterns with the
 * host's log.  Non-increasing in k; the label of x is the number of k with bits(x) < thr[k - 1], and L means "drawn again". */
int msm_mcmc_draw_thresholds(int32_t L, double mcparam, uint64_t *thr /* L */);
/* [host] The 312-candidate blocks the draw kernel may generate for `need` accepted proposals of one chain: with a = 1 - (1 - mcparam)^L,
 * ceil((need / a + 16 sqrt(need (1 - a)) / a + 624) / 312) + 1. */
int msm_mcmc_draw_block_bound(int64_t need, int32_t L, double mcparam, int64_t *blocks);
/* [host] msm_mcmc_proposals' stream (one chunk) from the hand-written pieces the draw kernel is made of -- the mt19937 recurrence and tempering, two
 * words to a double, 1 - u, the thresholds -- without std::mt19937 or std::geometric_distribution: (sweeps x T values in visit order).  _counted also
 * gives the candidates the stream consumed (candidates may be NULL). */
int msm_mcmc_proposals_mirror(int32_t L, double mcparam, uint64_t seed, int32_t T, int32_t sweeps, uint16_t *out);
int msm_mcmc_proposals_mirror_counted(int32_t L, double mcparam, uint64_t seed, int32_t T, int32_t sweeps, uint16_t *out, uint64_t *candidates);
/* The device's streams alone: out[(k * sweeps + s) * T + pos[t]] is the label proposed to triplet t in sweep s of chain k (seeds[k]; 1 <= K <= 256), drawn
 * chunk_sweeps sweeps per launch (<= 0: one launch) through the kernel and the per-chain record the optimiser's entry points use, then downloaded.  pos:
 * a permutation of 0 .. T - 1, or NULL for the identity.  At most 2^30 proposals per call (MSM_ERR_CAPACITY).  Runs on the context's side stream and is
 * joined to the context's stream before the download; complete on return.  `out` is written only when the call succeeds. */
int msm_mcmc_draw_gpu(msm_ctx *ctx, int32_t L, double mcparam, const uint64_t *seeds, int32_t K, int32_t T, int32_t sweeps, int32_t chunk_sweeps,
                      const int32_t *pos, uint16_t *out);
/* [host] What the draw kernel did in the last msm_mcmc_draw_gpu or mode 1 optimiser call on the context: stats[0] ms in the draw kernels (HIP events),
 * [1] candidates generated, [2] proposals accepted (both over all chains), [3] the block bound of the last chunk.  MSMHIP_MCMC_DRAW_BLOCKS=n (testing)
 * replaces the bound; a chain that reaches it before its chunk is complete fails the call with MSM_ERR_CAPACITY and a message that names the draw. */
int msm_mcmc_draw_stats(msm_ctx *ctx, double stats[4]);
/* [host] The level schedule of a triplet list (any list with nodes in [0, N)): level[t] (0-based), order (the T triplets by level, ascending within a
 * level), level_off (offsets into order; room for T + 1), *levels.  level / order / level_off may be NULL. */
int msm_mcmc_schedule(const int32_t *triplets, int32_t N, int32_t T, int32_t *level, int32_t *order, int32_t *level_off, int32_t *levels);
/* [host] AN EXTENSION (not newMSM's): max-product linear programming (MPLP; Globerson & Jaakkola 2007, Sontag et al. 2011 Fig. 1.4) over the tables
 * msm_mcmc_optimise reads -- block-coordinate ascent on the dual of the labelling LP, deterministic, written from the published update rule; DESIGN.md
 * 5.19 has the definition this serial literal and the GPU entry points follow bit for bit.  Messages m[t][s][x] (T x 3 x L doubles) start at 0.0; a
 * sweep updates the factors t = 0 .. T - 1 in order; after every sweep the beliefs are decoded (argmin, lowest label on ties).  Candidate 0 is the start
 * (labeling, N, in), candidate k the decode after sweep k; labeling receives the candidate of the first lowest msm_mcmc_energy (msm_mcmc_best's rule),
 * so the result is never worse than the start.  The run ends after `sweeps` sweeps, or after the first sweep that leaves every message's bits as they
 * were; *sweeps_run says how many ran.  Outputs, all optional (NULL): *energy the winner's energy; *bound the dual value D after the last sweep, which
 * no labelling's energy lies below (up to rounding) and which never falls from sweep to sweep; energies / bounds (`sweeps` values each): the decode's
 * energy and D after every sweep (the sweeps a fixed point spares repeat its values; untouched when no sweep ran); messages (T x 3 x L).  Asking for
 * bounds costs a second pass over the triplet table per sweep, asking for bound alone one pass.  sweeps == 0 or T == 0: the labelling stays, *sweeps_run
 * = 0.  Refused before anything is written: what msm_mcmc_optimise refuses, with its messages; a triplet that names a node twice (MSM_ERR_INVALID); a
 * non-finite table entry (MSM_ERR_INVALID, the message names the table and --fixnan); L > 1024 (MSM_ERR_CAPACITY). */
int msm_mplp_optimise(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, int32_t sweeps, int32_t *labeling,
                      int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds, double *messages);
/* msm_mplp_optimise with the sweeps on the GPU: the same labelling, sweeps_run, energies, bounds and messages, bit for bit.  The host tables are
 * uploaded as msm_mcmc_optimise_gpu uploads them; a sweep is one launch per level of msm_mcmc_schedule, a workgroup per factor; the terms of the
 * energies and bounds are evaluated on the device and summed on the host in the literal's order; the finiteness check is one device pass.  Everything
 * runs on the context's stream and the call is complete on return. */
int msm_mplp_optimise_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, int32_t sweeps,
                          int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds, double *messages);
/* What the last msm_mplp_optimise_gpu / msm_cost_mplp_optimise on the context did: stats[0] ms in the sweeps' kernels (HIP events around every chunk
 * of sweeps: updates, decodes, energy and bound terms), [1] levels per sweep, [2] sweeps run, [3] the widest level. */
int msm_mplp_gpu_stats(msm_ctx *ctx, double stats[4]);
/* [host] The colouring the rounding walks (DESIGN.md 5.19 "Rounding"): nodes in ascending order, colour[i] (N, out) the smallest colour no lower-index
 * node that shares a triplet with i holds; a node in no triplet has colour 0; nodes of one colour share no triplet.  *classes (may be NULL): the number
 * of colours.  Refuses a node out of range and a triplet that names a node twice. */
int msm_mplp_colouring(const int32_t *triplets, int32_t N, int32_t T, int32_t *colour, int32_t *classes);
/* [host] Rounds MPLP's messages (T x 3 x L as msm_mplp_optimise returns them; NULL: all zero) to a labelling, by the definition of DESIGN.md 5.19
 * "Rounding", which this serial literal and the GPU entry points follow bit for bit.  The conditioned decode walks the colour classes k = 0, 1, ...:
 * every node of class k takes the first argmin of theta_i(x) + sum over its slots of g(x), where g minimises the factor's table, less the messages of
 * the other two slots, over those of the two other nodes that lie in a class >= k, the ones in a lower class held at the label they have just taken.
 * A polish pass is the same walk with every other node held: iterated conditional modes class by class, the current label kept unless another is
 * strictly lower; a pass that changes no label ends the run.  Candidate 0 is the labelling handed in (labeling, N); mode 0 adds the conditioned decode
 * and every polish pass of it, mode 1 every polish pass of the labelling handed in (messages are not read).  labeling receives the candidate of the
 * first lowest msm_mcmc_energy, never worse than what was handed in.  Optional outputs (NULL): *passes_run the polish passes run; *energy the winner's;
 * energies, 2 + polish values in mode 0 and 1 + polish in mode 1, one per candidate (the passes a fixed point spares repeat the last value).  Refused
 * before anything is written: what msm_mplp_optimise refuses, with its messages; a non-finite message (mode 0); a mode other than 0 / 1; polish < 0 or
 * > 1024. */
int msm_mplp_round(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const double *messages, int32_t mode,
                   int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies);
/* msm_mplp_round on the GPU, bit for bit: the tables and the messages are uploaded; a pass is one launch per colour class on the context's stream (the
 * conditioned decode a workgroup per node, a polish pass a wavefront per node); the energy terms are evaluated on the device and summed on the host.
 * Complete on return. */
int msm_mplp_round_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const double *messages,
                       int32_t mode, int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies);
/* What the last rounding on the context's GPU did: stats[0] ms in the conditioned decode's launches, [1] ms in the polish passes (with their energy
 * terms), [2] colour classes, [3] polish passes run. */
int msm_mplp_round_gpu_stats(msm_ctx *ctx, double stats[4]);
/* FORBIDDEN ENTRIES (opt-in; DESIGN.md 5.19 "Forbidden entries").  The entry points above refuse every table with a NaN or an infinity.  The ones below
 * read a triplet entry that is NaN or +infinity as a forbidden label combination: theta^(a,b,c) = theta(a,b,c) where that is below +infinity and
 * +infinity otherwise.  A message of +infinity says that label of that node is proved infeasible; messages are never NaN or -infinity.  The bound's
 * factor term is the minimum over the combinations whose entry and three messages are all below +infinity (+infinity where there is none): D lies
 * below the energy of every labelling that uses no forbidden entry, up to rounding, and D = +infinity says there is none.  Energies are E^: every term
 * passed through the same mapping, so finite or +infinity and never NaN; the winner is the first strictly lower E^, never worse than the start in E^,
 * and a start on a forbidden entry loses to any feasible candidate.  In the rounding a combination is +infinity when its entry or a message it would
 * subtract is.  Still refused (MSM_ERR_INVALID, nothing written, the message names the table and the class of value): -infinity in the triplet table,
 * any non-finite unary entry, and for the rounding a message that is NaN or -infinity.  On tables without a forbidden entry every output equals the
 * plain entry point's, bit for bit: the host decides the route from the counts and runs the plain code there.
 * [host] msm_mplp_classify counts: counts[0] the non-finite unary entries, counts[1..3] the NaN, +infinity and -infinity triplet entries. */
int msm_mplp_classify(const double *unary, const double *tcosts, int32_t N, int32_t L, int32_t T, int64_t counts[4]);
/* [host] msm_mplp_optimise under that reading; counts (may be NULL) receives msm_mplp_classify's four values */
int msm_mplp_optimise_forbid(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, int32_t sweeps,
                             int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds, double *messages,
                             int64_t counts[4]);
/* the same on the GPU, bit for bit: one device pass counts both tables (counts, may be NULL), then the forbidden-aware kernels run where the table
 * holds a forbidden entry and the plain ones where it does not */
int msm_mplp_optimise_forbid_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T,
                                 int32_t sweeps, int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds,
                                 double *messages, int64_t counts[4]);
/* [host] msm_mplp_round under that reading (messages may hold +infinity); counts as above */
int msm_mplp_round_forbid(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const double *messages,
                          int32_t mode, int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies, int64_t counts[4]);
/* the same on the GPU, bit for bit */
int msm_mplp_round_forbid_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T,
                              const double *messages, int32_t mode, int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies,
                              int64_t counts[4]);
/* MPLP OVER THE PAIR TABLES (an extension): the optimiser above for the pairwise model of a --regoption=1 level, whose factors are the
 * P pairs of msm_cost_set_pairs.  unary: L x N as above; pairs: 2 P nodes, pair p on A = pairs[2p] (slot 0) and B = pairs[2p+1] (slot 1), A not
 * required to be below B, two pairs may name the same two nodes; paircosts: P x L x L as msm_cost_pairwise_table writes them, theta_p(a, b) at
 * (p L + b) L + a.  Messages m[p][s][x] are P x 2 x L doubles.  The plain reading only: the forbidden-entry reading above does not apply.
 * [host] The two colourings 5.20 walks.  pair_colour[p] (P): the smallest colour no pair q < p that shares a node with p holds -- a sweep walks the
 * colours ascending and a colour's pairs ascending, and pairs of one colour share no node.  node_colour[i] (N): the smallest colour no lower-index node
 * that shares a pair with i holds (a node in no pair: 0) -- what a polish pass walks.  Every output may be NULL.  Refuses a node out of range and a
 * pair that names one node twice. */
int msm_mplp_pairs_colouring(const int32_t *pairs, int32_t N, int32_t P, int32_t *pair_colour, int32_t *pair_classes, int32_t *node_colour,
                             int32_t *node_classes);
/* [host] The energy of a labelling over these tables: the unary terms summed over i ascending from 0.0, `+ 0.0`, plus the pair terms
 * theta_p(x_A, x_B) summed over p ascending from 0.0 (msm_mcmc_energy's shape with the pair terms in the triplet terms' place). */
int msm_mplp_pairs_energy(const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P, const int32_t *labeling,
                          double *energy);
/* [host] The serial literal of DESIGN.md 5.20.  Candidates, winner, stop and the optional outputs are msm_mplp_optimise's: labeling (N) is the start
 * in and the first lowest energy among the start and the decode after every sweep out; *sweeps_run; *energy; *bound (the dual value after the last
 * sweep); energies / bounds (`sweeps` values, the sweeps a fixed point spares repeat the last; untouched when no sweep ran); messages (P x 2 x L).
 * sweeps == 0 or P == 0: the labelling stays, *sweeps_run = 0.  Refused before anything is written: a node or a start label out of range and negative
 * counts (msm_mcmc_optimise's wording where it applies); a pair that names one node twice (MSM_ERR_INVALID); a non-finite entry in either table
 * (MSM_ERR_INVALID, the message names the table, the unary one first); L > 1024 (MSM_ERR_CAPACITY). */
int msm_mplp_pairs_optimise(const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P, int32_t sweeps,
                            int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds, double *messages);
/* msm_mplp_pairs_optimise with the sweeps on the GPU, bit for bit: the tables are uploaded, a sweep is one launch per pair colour (a wavefront per pair
 * up to 64 labels, a workgroup per pair above), the terms of the energies and bounds are evaluated on the device and summed on the host in the
 * literal's order, the finiteness check is one device pass.  Everything runs on the context's stream; complete on return. */
int msm_mplp_pairs_optimise_gpu(msm_ctx *ctx, const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P,
                                int32_t sweeps, int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies, double *bounds,
                                double *messages);
/* [host] The polish of 5.20: `polish` passes (0 to 1024) of iterated conditional modes over the node colours, every other node held at its label, the
 * current label kept unless the first argmin is strictly lower; a pass that changes no label ends the run.  Candidate 0 is the labelling handed in,
 * candidate k the labelling after pass k; labeling receives the first lowest energy.  Optional: *passes_run, *energy, energies (1 + polish values,
 * the passes a fixed point spares repeat the last).  Refuses what msm_mplp_pairs_optimise refuses. */
int msm_mplp_pairs_polish(const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P, int32_t polish,
                          int32_t *labeling, int32_t *passes_run, double *energy, double *energies);
/* msm_mplp_pairs_polish on the GPU, bit for bit: a launch per node colour and pass, a wavefront per node */
int msm_mplp_pairs_polish_gpu(msm_ctx *ctx, const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P,
                              int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies);
/* What the last sweeps and the last polish over pair tables on the context's GPU did: stats[0] ms in the sweeps' kernels (HIP events around every
 * chunk), [1] pair colours per sweep, [2] sweeps run, [3] the widest colour class, [4] ms in the polish passes, [5] passes run (the sweeps reset [4]
 * and [5] to 0). */
int msm_mplp_pairs_gpu_stats(msm_ctx *ctx, double stats[6]);
/* [host] A STAND-IN for the binary solve of one label step of Fusion::optimize (I/Fusion/Fusion.h:198-229 hands the step to ELC's
 * reduction + FastPD, which are licence-restricted and FSL-bound: not reproduced).  Iterated conditional modes over x in {0,1}^N
 * (0: the node keeps its label, 1: it takes the proposed one) for
 *     E(x) = sum_i unary2[2 i + x_i] + sum_p quads[4 p + 2 x_a + x_b] + sum_t octets[8 t + 4 x_a + 2 x_b + x_c]
 * (quads / octets as msm_group_fusion_move and msm_cost_triplet_octets write them; unary2 NULL: no unary costs; P or T may be 0) from
 * x = 0, nodes in ascending order, a node flips only when that lowers E strictly, at most max_passes passes.  Deterministic; it exists
 * so that the fusion-move path can be driven end to end (tools, tests, bench) the way the HCP configurations drive it -- a registration
 * run with it is NOT the reference's optimisation result. */
int msm_fusion_icm_step(const double *unary2 /* N x 2 or NULL */, const double *quads /* P x 4 */, const int32_t *pairs /* P x 2 */, int32_t P,
                        const double *octets /* T x 8 */, const int32_t *triplets /* T x 3 */, int32_t T, int32_t N, int32_t max_passes,
                        int32_t *x /* N, out */);
/* [host] AN EXTENSION (not newMSM's), in place of the binary solve of one label step of Fusion::optimize (I/Fusion/Fusion.h:198-229: ELC + FastPD, not
 * reproduced): MPLP over the step's binary problem, by the definitions of msm_mplp_optimise and msm_mplp_round at L = 2.  With
 * theta_i(x) = unary2[2 i + x] (U[x N + i] in msm_mplp_optimise's layout; NULL: all zero) and the octets as the triplet table (octets[8 t + 4 x_a + 2 x_b
 * + x_c] is tcosts[((t L + a) L + b) L + c] at L = 2): msm_mplp_optimise from x = 0 for `sweeps` sweeps, then, polish > 0, msm_mplp_round mode 0 over the
 * final messages with the sweeps' winner handed in.  x (N values 0 / 1) is never worse than x = 0; *bound, the bound after the last sweep run, never
 * lies above the step's optimum.  Optional: *sweeps_run, *passes_run, *energy (of x), *bound, energies -- 1 + sweeps values (the start, then every
 * sweep's decode; sweeps a fixed point spares repeat the last) followed, polish > 0, by 1 + polish values (the conditioned decode, then the polish
 * passes) --, bounds (one per sweep).  Refused before anything is written: what msm_mplp_optimise and msm_mplp_round refuse (a non-finite entry names
 * its table, the unary one first), sweeps outside 0 .. 1024, polish outside 0 .. 1024.  Only the plain reading: no forbidden entries.  Pair factors
 * (msm_group_fusion_move's quads) are not taken. */
int msm_fusion_mplp_step(const double *unary2 /* N x 2 or NULL */, const double *octets /* T x 8 */, const int32_t *triplets /* T x 3 */, int32_t T, int32_t N,
                         int32_t sweeps, int32_t polish, int32_t *x /* N, out */, int32_t *sweeps_run, int32_t *passes_run, double *energy, double *bound,
                         double *energies, double *bounds);
/* msm_fusion_mplp_step on the GPU (an extension), bit for bit in every output: the tables are uploaded, and the sweeps, their decodes, the rounding and
 * the polish run in one launch of one workgroup with one synchronisation.  MSMHIP_FUSION_MSG=lds|global (for tests) forces where the messages live;
 * results do not depend on it. */
int msm_fusion_mplp_step_gpu(msm_ctx *ctx, const double *unary2, const double *octets, const int32_t *triplets, int32_t T, int32_t N, int32_t sweeps,
                             int32_t polish, int32_t *x, int32_t *sweeps_run, int32_t *passes_run, double *energy, double *bound, double *energies,
                             double *bounds);
/* The last msm_fusion_mplp_step_gpu / msm_cost_fusion_mplp_step on the context (an extension): stats[0] ms in the solve launch (HIP events), [1] levels
 * per sweep, [2] sweeps run, [3] launches the solve took (1; 2 where a fused move's tail kernel completed the octets after the first) */
int msm_fusion_mplp_gpu_stats(msm_ctx *ctx, double stats[4]);
/* [host] A STAND-IN for FPD::FastPD on the multi-label pairwise MRF of --regoption=1 (M/mesh_registration.cpp:182-188: computeUnaryCosts,
 * computePairwiseCosts, FastPD): iterated conditional modes over unary[label * N + node] and paircosts[(pair * L + labelB) * L + labelA]
 * (the layouts FastPD reads, I/FastPD/FastPD.h:126,213,224), nodes in ascending order, lowest label on ties, at most max_passes passes.
 * labeling: the start (resetLabeling gives zeros) in, the result out.  Not FastPD's optimum: it lets the regoption-1 caller loop run. */
int msm_pairwise_icm(const double *unary, const double *paircosts, const int32_t *pairs, int32_t N, int32_t L, int32_t P, int32_t max_passes, int32_t *labeling);

/* ------------------------------------------------------------------------------------------------
 * discrete cost function.  Replaces NonLinearSRegDiscreteCostFunction and its five subclasses
 * (M/DiscreteCostFunction.h:83-283) behind the DiscreteCostFunction evaluator interface
 * (M/DiscreteCostFunction.h:41-59) the optimisers call.
 * ---------------------------------------------------------------------------------------------- */
#define MSM_COST_UNIVARIATE 0      /* UnivariateNonLinearSRegDiscreteCostFunction */
#define MSM_COST_MULTIVARIATE 1    /* MultivariateNonLinearSRegDiscreteCostFunction */
#define MSM_COST_PATCHWISE 2       /* PatchwiseMultivariateNonLinearSRegDiscreteCostFunction */
#define MSM_COST_HO_UNIVARIATE 3   /* HOUnivariateNonLinearSRegDiscreteCostFunction (--triclique) */
#define MSM_COST_HO_MULTIVARIATE 4 /* HOMultivariateNonLinearSRegDiscreteCostFunction */

typedef struct msm_cost_params { /* set_parameters M/DiscreteCostFunction.cpp:119-133 */
    int32_t kind;        /* MSM_COST_* (chosen in initialize_cost_function M/DiscreteModel.cpp:43-61) */
    int32_t simmeasure;  /* "simmeasure": 1 SSD, 2 correlation, 4 DICE, 5 genDICE (get_sim_for_min M/similarities.h:48-58) */
    int32_t rmode;       /* "regularisermode": 1 pairwise angle, 2/3 triangle strain, 4/5 anatomical strain (msm_cost_set_anatomical) */
    int32_t reserved;
    double  lambda;      /* "lambda" */
    double  mu;          /* "shearmodulus" */
    double  kappa;       /* "bulkmodulus" */
    double  k_exp;       /* "kexponent" */
    double  rexp;        /* "exponent" */
    double  range;       /* "range" (_controlptrange) */
    double  percentile;  /* "percentile" (DICE measures; M/similarities.h:68 default 0.75, must lie in (0,1)) */
} msm_cost_params;

msm_cost *msm_cost_create(msm_ctx *ctx, const msm_cost_params *params);
void      msm_cost_destroy(msm_cost *c);
/* set_anatomical + set_anatomical_neighbourhood (M/DiscreteCostFunction.h:160-170), for regularisermode 4/5 (aMSM:
 * computeTripletCost :169-182 with deform_anatomy :255-301).  sphere = _TARGEThi, the anatomical-resolution sphere
 * (its octree is the reference's `anattree`); atarget_xyz = _aTARGET coordinates, 3 x (vertices of sphere) SoA;
 * asource_* = _aSOURCE (3 x Vs SoA, 3 x Ts SoA); w_* = _ANATbaryweights as CSR over the Vs vertices, control point
 * ids ascending within a row (std::map order); face_* = NEARESTFACES as CSR over the triplets (set_triplets first). */
int msm_cost_set_anatomical(msm_cost *c, msm_mesh *sphere, const double *atarget_xyz, const double *asource_xyz, int32_t Vs,
                            const int32_t *asource_tri, int32_t Ts, const int32_t *w_ptr, const int32_t *w_cp, const double *w_val,
                            const int32_t *face_ptr, const int32_t *face_idx);
/* set_meshes M/DiscreteCostFunction.h:196-198: captures _ORIG (source coords) and _oCPgrid */
int msm_cost_set_meshes(msm_cost *c, msm_mesh *target, msm_mesh *source, msm_mesh *cpgrid);
/* reset_source :208 / reset_CPgrid :209: pick up the meshes' current coordinates */
int msm_cost_reset_source(msm_cost *c, msm_mesh *source);
int msm_cost_reset_cpgrid(msm_cost *c, msm_mesh *cpgrid);
/* set_featurespace :203-205: input (moving) features D x V(source); reference features are the
 * target mesh's features (msm_mesh_set_features) */
int msm_cost_set_source_features(msm_cost *c, const double *feat, int32_t D);
/* set_dataaffintyweighting :165: rows x V(source), rows == 1 or D; NULL = all ones (M/mesh_registration.cpp:234-238) */
int msm_cost_set_cfweight(msm_cost *c, const double *w, int32_t rows);
/* set_spacings :207 */
int msm_cost_set_spacings(msm_cost *c, const double *maxsep, double mvdmax);
/* set_labels :199-202: labels 3 x L SoA, rot 9 per control point (row-major) */
int msm_cost_set_labels(msm_cost *c, const double *labels, int32_t L, const double *rot);
/* setTriplets / setPairs M/DiscreteCostFunction.h:44-45 (AoS, node ids ascending within a clique) */
int msm_cost_set_triplets(msm_cost *c, const int32_t *triplets, int32_t T);
int msm_cost_set_pairs(msm_cost *c, const int32_t *pairs, int32_t P);
/* initialize() + get_source_data(): Univariate M/DiscreteCostFunction.cpp:334-351, Multivariate :393-416,
 * Patchwise :629-650 (range test per control point), HO :468-485 / :541-563 (bin by closest CP triangle),
 * then resample_weights :303-323 */
int msm_cost_get_source_data(msm_cost *c);
/* _sourceinrange as CSR: ptr[groups+1], idx[ptr[groups]]; idx may be NULL to size */
int msm_cost_patches(msm_cost *c, int32_t *ngroups, int32_t *ptr, int32_t *idx, int64_t cap);
int msm_cost_absolute_weights(msm_cost *c, double *absw /* N */);
/* computeUnaryCosts M/DiscreteCostFunction.cpp:236-243: U[label * N + node] (the layout FastPD and MCMC read,
 * I/FastPD/FastPD.h:126, M/mcmc_opt.h:59).  _async only enqueues on the context's stream; _fetch copies back. */
int msm_cost_unary_table(msm_cost *c, double *U);
int msm_cost_unary_table_async(msm_cost *c);
int msm_cost_unary_table_fetch(msm_cost *c, double *U);
/* computeUnaryCost(node,label) :378 for a list of (node,label) queries (Fusion's per-label sweep, I/Fusion/Fusion.h:148-155) */
int msm_cost_unary_batch(msm_cost *c, const int32_t *nodes, const int32_t *labels, int32_t n, double *out);
/* computeTripletCost M/DiscreteCostFunction.cpp:135-188 for n (triplet, labelA, labelB, labelC) queries */
int msm_cost_triplet_batch(msm_cost *c, const int32_t *triplet, const int32_t *la, const int32_t *lb, const int32_t *lc, int32_t n, double *out);
/* the 8 costs per triplet of one fusion move, I/Fusion/Fusion.h:181-196: E[8*t + k], k = 000..111 with bit
 * order (A,B,C) and 0 = current labeling, 1 = `label` */
int msm_cost_triplet_octets(msm_cost *c, const int32_t *labeling, int32_t label, double *E);
/* A hint that costs nothing to ignore: queue the label step (labeling, label) into E and return without waiting.  Between two label steps of
 * Fusion::optimize the host solves a binary problem (ELC + FastPD, I/Fusion/Fusion.h:204-221) while the GPU idles, and most steps of a converging level
 * change no label (three of four in the HCP MSMAll schedule): the next step's evaluations can run meanwhile.  The next msm_cost_triplet_octets on this
 * cost function with the same labeling, label and E only waits for the queued kernel; any other call drops the queued step (its evaluations were never
 * asked for: a status they raised is discarded).  Honoured when E lies in msm_host_alloc memory and the step has its one-kernel form (the fused triclique
 * move, or the strain-only move with the labeling in the kernel arguments); silently ignored otherwise.  Results do not depend on it.
 * msm_cost_prefetch_stats: steps taken from a prefetch / prefetches dropped, since creation. */
int msm_cost_triplet_octets_prefetch(msm_cost *c, const int32_t *labeling, int32_t label, double *E);
int msm_cost_prefetch_stats(msm_cost *c, int64_t *taken, int64_t *dropped);
/* computePairwiseCost :190-226 for n (pair, labelA, labelB) queries, and the full table of
 * computePairwiseCosts :228-234: paircosts[(pair*L + labelB)*L + labelA] */
int msm_cost_pairwise_batch(msm_cost *c, const int32_t *pair, const int32_t *la, const int32_t *lb, int32_t n, double *out);
int msm_cost_pairwise_table(msm_cost *c, double *paircosts);
/* computeTripletCosts M/DiscreteCostFunction.cpp:245-253 (the MCMC optimiser's table, M/mcmc_opt.h:58): tcosts[((t - t0)*L + a)*L*L + b*L + c]
 * for the triplets t0 <= t < t1 (the whole table is T * L^3 doubles, 281 MB at ico4 / 19 labels: fetch it in ranges) */
int msm_cost_triplet_table(msm_cost *c, int32_t t0, int32_t t1, double *tcosts);
/* computeUnaryCosts + computeTripletCosts + MCMC::optimise (M/mcmc_opt.h:31-134) over the cost function's own tables, which never leave the device: the
 * unary table's kernels and the triplet-table kernels fill device buffers (T * L^3 doubles for the latter), then the sweeps of msm_mcmc_optimise_gpu run
 * there.  The labelling (N, read and updated) is the one msm_cost_unary_table + msm_cost_triplet_table(0, T) + msm_mcmc_optimise give, bit for bit. */
int msm_cost_mcmc_optimise(msm_cost *c, double mcparam, int32_t iters, uint64_t seed, int32_t *labeling);
/* msm_mcmc_optimise_chains_gpu over the cost function's own device tables, as msm_cost_mcmc_optimise: what msm_cost_unary_table +
 * msm_cost_triplet_table(0, T) + msm_mcmc_optimise_chains give, bit for bit. */
int msm_cost_mcmc_optimise_chains(msm_cost *c, double mcparam, int32_t iters, const uint64_t *seeds, int32_t K, int32_t *labeling, int32_t *labelings,
                                  double *energies, int32_t *best);
/* msm_mplp_optimise_gpu over the cost function's own device tables, filled as msm_cost_mcmc_optimise fills them: what msm_cost_unary_table +
 * msm_cost_triplet_table(0, T) + msm_mplp_optimise give, bit for bit (labelling, sweeps_run, energies, bounds, messages). */
int msm_cost_mplp_optimise(msm_cost *c, int32_t sweeps, int32_t *labeling, int32_t *sweeps_run, double *energy, double *bound, double *energies,
                           double *bounds, double *messages);
/* MPLP's sweeps and the rounding over the cost function's own device tables; the messages never leave the device.  What msm_cost_mplp_optimise(messages)
 * followed by msm_mplp_round(mode 0) on those messages with that winner handed in give, bit for bit: labeling, *sweeps_run, *passes_run, *energy,
 * *bound (after the last sweep), energies (2 + polish).  then_polish != 0: one msm_mplp_round(mode 1) call on that result follows over the same tables
 * (labeling and *energy are its; a no-op where the polish reached its fixed point, it matters when the labelling handed in won). */
int msm_cost_mplp_round(msm_cost *c, int32_t sweeps, int32_t polish, int32_t then_polish, int32_t *labeling, int32_t *sweeps_run, int32_t *passes_run,
                        double *energy, double *bound, double *energies);
/* msm_mplp_round(mode 1) over the cost function's own device tables, filled as msm_cost_mplp_optimise fills them; energies: 1 + polish values */
int msm_cost_mplp_polish(msm_cost *c, int32_t polish, int32_t *labeling, int32_t *passes_run, double *energy, double *energies);
/* msm_fusion_mplp_step (an extension, in place of I/Fusion/Fusion.h:198-229's binary solve) over the label step (labeling, label) with the tables staying
 * on the device: the step's 8 T costs are evaluated as msm_cost_triplet_octets evaluates them (fused triclique move, packed strain move or the copied
 * route) into a device buffer, unary2 is gathered on the device from the cost function's unary table -- filled as msm_cost_mplp_optimise fills it where
 * the iteration's table is not valid, reused otherwise --, the solve runs behind the step's kernel, one synchronisation.  What msm_fusion_mplp_step
 * gives over msm_cost_unary_table (unary2[2 i] = U[labeling[i] N + i], unary2[2 i + 1] = U[label N + i]) and msm_cost_triplet_octets, bit for bit.  A
 * step queued by msm_cost_triplet_octets_prefetch is dropped first.  msm_cost_set_mplp_forbid is ignored: non-finite values are refused. */
int msm_cost_fusion_mplp_step(msm_cost *c, const int32_t *labeling, int32_t label, int32_t sweeps, int32_t polish, int32_t *x, int32_t *sweeps_run,
                              int32_t *passes_run, double *energy, double *bound, double *energies, double *bounds);
/* [host] on != 0: msm_cost_mplp_optimise / _round / _polish read the device triplet table's NaN and +infinity entries as forbidden combinations, as
 * msm_mplp_optimise_forbid_gpu / msm_mplp_round_forbid_gpu do (the strain regulariser produces such entries where a label set lets control points
 * meet); 0, the default: they refuse such a table. */
int msm_cost_set_mplp_forbid(msm_cost *c, int32_t on);
/* [host] what the last of those calls counted over the two device tables while the switch was on (msm_mplp_classify's four values) */
int msm_cost_mplp_forbidden(msm_cost *c, int64_t counts[4]);
/* MPLP over the pair tables with both tables staying on the device: the unary table and the pair table are filled as
 * msm_cost_mcmc_optimise fills its two (the pair table by the kernel of msm_cost_pairwise_table, never downloaded), the sweeps run from `labeling`, and
 * with polish > 0 the sweeps' winner is polished over the same tables.  What msm_cost_unary_table + msm_cost_pairwise_table + msm_mplp_pairs_optimise
 * (+ msm_mplp_pairs_polish of its result) give, bit for bit: labeling, *sweeps_run, *passes_run (0 without polish), *energy (the final labelling's),
 * *bound (after the last sweep), energies / bounds (`sweeps` values), polish_energies (1 + polish values, written when polish > 0).  All but labeling
 * may be NULL.  Needs msm_cost_set_pairs (MSM_ERR_STATE without).  msm_cost_set_mplp_forbid is ignored here: computePairwiseCost returns a finite cost
 * or the folding value. */
int msm_cost_mplp_pairs_optimise(msm_cost *c, int32_t sweeps, int32_t polish, int32_t *labeling, int32_t *sweeps_run, int32_t *passes_run, double *energy,
                                 double *bound, double *energies, double *bounds, double *polish_energies);
/* evaluateTotalCostSum :55-77: parts = {unary, pairwise, triplet} sums in the reference's serial order */
int msm_cost_total(msm_cost *c, const int32_t *labeling, double *total, double parts[3]);
/* Optional HIP-event timing of the sampling kernel (k_unary_rays or k_unary_samples) of each unary-table launch, recorded on the
 * context's stream.  msm_cost_kernel_times returns the durations (ms) of the last launches (most recent last; at most
 * 64 are kept) after synchronising the stream. */
int msm_cost_enable_timing(msm_cost *c, int enable);
int msm_cost_kernel_times(msm_cost *c, double *ms, int32_t cap, int32_t *n);
/* counters since creation: [0] point samples (rotate + nearest triangle + interpolate), [1] unary evals,
 * [2] triplet evals, [3] pairwise evals */
int msm_cost_counters(msm_cost *c, int64_t counters[4]);
/* Which kernels this cost function ran, as its launchers recorded them where they chose (host bookkeeping only: no synchronisation, nothing on the
 * device).  routes[MSM_ROUTE_UNARY]: the reduction kernel of the last unary table; routes[MSM_ROUTE_MOVE]: the route of the last triclique label step
 * (msm_cost_triplet_octets, or the single-combination move of msm_cost_total); routes[MSM_ROUTE_MOVE_NBLK / _CAP / _MAXTRI]: workgroups of the fused
 * move, bin slots one of them holds at most, and the largest number of control triangles in one (0 until a fused move has run);
 * routes[MSM_ROUTE_MOVE_TAILS]: moves that needed the tail kernel since creation (saturating); routes[MSM_ROUTE_MOVE_DEFERRED]: evaluations (of the
 * move's 8 x T, or T in msm_cost_total) that the last fused move handed to the tail kernel, 0 when it launched none -- read back (four bytes) behind the
 * tail kernel only, so a move that needs no tail pays nothing; samples settled by the leaf search inside the main kernel are not counted.
 * routes[MSM_ROUTE_UNARY_FORM]: the form of the last table's MSM_UNARY_FLAT reduction, MSM_UNARY_FORM_ROWS where k_unary_reduce_rows ran (univariate
 * correlation / SSD, no patch above 96 points: a row per 8-lane group, the moving patches prepared beside the fix-up), MSM_UNARY_FORM_STAGED where
 * k_unary_reduce_flat staged them per workgroup and for every other reduction. */
#define MSM_ROUTE_UNARY 0
#define MSM_ROUTE_MOVE 1
#define MSM_ROUTE_MOVE_NBLK 2
#define MSM_ROUTE_MOVE_CAP 3
#define MSM_ROUTE_MOVE_MAXTRI 4
#define MSM_ROUTE_MOVE_TAILS 5
#define MSM_ROUTE_MOVE_DEFERRED 6
#define MSM_ROUTE_UNARY_FORM 7
#define MSM_UNARY_NONE 0        /* no unary table yet (the triclique classes' table is all zeros: no kernel) */
#define MSM_UNARY_UNIVARIATE 1  /* k_unary_reduce_univariate (DICE measures of the univariate class) */
#define MSM_UNARY_FLAT 2        /* k_unary_reduce_flat */
#define MSM_UNARY_FEATURES 3    /* k_unary_reduce_features */
#define MSM_UNARY_MV8 4         /* k_unary_reduce_mv8 */
#define MSM_UNARY_PW8_4 5       /* k_unary_reduce_pw8<4> */
#define MSM_UNARY_PW8_8 6       /* k_unary_reduce_pw8<8> */
#define MSM_UNARY_FORM_STAGED 0
#define MSM_UNARY_FORM_ROWS 1
#define MSM_MOVE_NONE 0
#define MSM_MOVE_FUSED_0 1      /* k_ho_move<., 0>: the univariate triclique class */
#define MSM_MOVE_FUSED_1 2      /* k_ho_move<., 1>: one lane per sample */
#define MSM_MOVE_FUSED_2 3      /* k_ho_move<., 2>: eight lanes per sample, four dimension pairs per lane */
#define MSM_MOVE_FUSED_3 4      /* k_ho_move<., 3>: eight lanes per sample, two dimension pairs per lane */
#define MSM_MOVE_OCTETS_SAMPLE 5      /* three-kernel path with k_ho_octets_sample */
#define MSM_MOVE_OCTETS_SAMPLE_MV8 6  /* three-kernel path with k_ho_octets_sample_mv8 */
#define MSM_MOVE_OCTETS_HO 7          /* k_triplet_octets_ho: the general on-demand kernel */
#define MSM_MOVE_STRAIN 8             /* the strain-only classes: k_triplet_octets / k_triplet_octets_packed */
int msm_cost_routes(msm_cost *c, int32_t routes[8]);
/* The launch plan of a unary table: every decision of the launch that depends on the largest patch pmax (a coarse control grid under a fine data
 * grid gives patches of thousands of points), taken by one host function that the launchers act on.  plan[MSM_PLAN_NSPLIT]: workgroups (label
 * ranges) per control point, 1 <= nsplit <= L; plan[MSM_PLAN_SAMPLER]: MSM_SAMPLER_RAYS (k_unary_rays, targets with a direction table) or
 * MSM_SAMPLER_SAMPLES (k_unary_samples, the complete search); plan[MSM_PLAN_SAMPLER_LDS]: its dynamic LDS in bytes; plan[MSM_PLAN_REDUCE]: the
 * reduction kernel, MSM_UNARY_*; plan[MSM_PLAN_REDUCE_LDS] / [MSM_PLAN_REDUCE_THREADS]: its dynamic LDS in bytes and its workgroup size;
 * plan[MSM_PLAN_REFUSED]: 0, or which kernel's LDS exceeds the 160 KB of a workgroup (MSM_PLAN_REFUSED_*) -- such a table fails with
 * MSM_ERR_CAPACITY and a message that names the patch size before anything is launched, and the cost function stays usable;
 * plan[MSM_PLAN_PMAX]: the pmax the plan was made for.  Byte counts saturate at INT32_MAX.
 *   msm_unary_launch_plan   the plan for (kind MSM_COST_UNIVARIATE / _MULTIVARIATE / _PATCHWISE, simmeasure, D, L, pmax, ray_table != 0): pure host
 *                           arithmetic, no context, no device.
 *   msm_cost_unary_launch   the plan of this cost function's last unary table, refused ones included (all zero but nsplit = 1, threads = 256
 *                           before the first); host bookkeeping only, as msm_cost_routes.
 *   msm_unary_launch_order  the order in which the unary kernels take the control points (cp_xyz: 3 x N): Morton order of their positions.
 *   msm_unary_fix_offsets   the MSM_UNARY_FIX_SEGMENTS + 1 offsets of the fix-up list's segments for patches pptr (N + 1) and that order: workgroup b of
 *                           the sampling kernel appends to segment b % MSM_UNARY_FIX_SEGMENTS, which holds all samples of its workgroups; the last
 *                           offset is L * pptr[N] (saturating at 2^32 - 1).
 *   msm_cost_unary_fix_counters  counts[0]: the redo counter, counts[1 + s]: the fill of fix-up segment s, read back from the device after the
 *                           queued work (a synchronising call for tests: every unary table leaves all MSM_UNARY_FIX_SEGMENTS + 1 of them zero). */
#define MSM_PLAN_NSPLIT 0
#define MSM_PLAN_SAMPLER 1
#define MSM_PLAN_SAMPLER_LDS 2
#define MSM_PLAN_REDUCE 3
#define MSM_PLAN_REDUCE_LDS 4
#define MSM_PLAN_REDUCE_THREADS 5
#define MSM_PLAN_REFUSED 6
#define MSM_PLAN_PMAX 7
#define MSM_SAMPLER_NONE 0
#define MSM_SAMPLER_SAMPLES 1
#define MSM_SAMPLER_RAYS 2
#define MSM_PLAN_REFUSED_SAMPLER 1
#define MSM_PLAN_REFUSED_REDUCTION 2
#define MSM_UNARY_FIX_SEGMENTS 64
int msm_unary_launch_plan(int32_t kind, int32_t simmeasure, int32_t D, int32_t L, int32_t pmax, int32_t ray_table, int32_t plan[8]);
int msm_cost_unary_launch(msm_cost *c, int32_t plan[8]);
int msm_cost_unary_fix_counters(msm_cost *c, uint32_t *counts);
int msm_unary_launch_order(const double *cp_xyz, int32_t N, int32_t *order);
int msm_unary_fix_offsets(int32_t N, int32_t L, int32_t pmax, const int32_t *pptr, const int32_t *order, uint32_t *off);

/* ------------------------------------------------------------------------------------------------
 * groupwise registration (gMSM).  Replaces DiscreteGroupModel::setupCostFunction and its helpers
 * (M/DiscreteGroupModel.cpp:37-196) and DiscreteGroupCostFunction's evaluators
 * (M/DiscreteGroupCostFunction.cpp:26-98).  Node ids are subject * N + control point, as in the reference.
 * Subjects are independent until the pairwise costs, so a multi-GPU run shards them.
 * ---------------------------------------------------------------------------------------------- */
typedef struct msm_group msm_group;
typedef struct msm_group_params { /* set_parameters M/DiscreteCostFunction.cpp:119-133 */
    int32_t simmeasure;  /* 1 SSD, 2 correlation, 4 DICE, 5 genDICE (get_sim_for_min, M/similarities.h:48-58) */
    int32_t fixnan;      /* "fixnan": NaN cost -> FIX_NAN = 1e7 (M/reg_tools.h:31) */
    double  lambda, mu, kappa, k_exp, rexp, range;
    double  percentile;  /* "percentile" (M/DiscreteCostFunction.cpp:129): DICE threshold rank; 0 means the default 0.75 */
} msm_group_params;
msm_group *msm_group_create(msm_ctx *ctx, const msm_group_params *params, int32_t num_subjects);
msm_ctx   *msm_group_context(msm_group *g);   /* [host] the context the group was created on (its stream: msm_ctx_stream / msm_ctx_wait_stream) */
void       msm_group_destroy(msm_group *g);
/* DiscreteGroupModel::set_meshspace target_space M/DiscreteGroupModel.h:56-61, set_masks :54 (mask: V(template) or NULL) */
int msm_group_set_template(msm_group *g, msm_mesh *template_mesh, const double *mask);
/* Initialize(controlgrid) M/DiscreteGroupModel.cpp:141-161: every subject starts from this grid; builds the triplets */
int msm_group_set_controlgrid(msm_group *g, const double *xyz, const int32_t *tri, int32_t N, int32_t Tc);
/* m_datameshes[s] (reset_meshspace M/DiscreteGroupModel.h:63-65) and FEAT->get_data_matrix(s) (D x V).  The first call
 * for a subject also captures _ORIG_MESHES[s] (set_meshes M/DiscreteGroupCostFunction.h:40-46). */
int msm_group_set_subject(msm_group *g, int32_t subject, msm_mesh *data_mesh, const double *feat, int32_t D);
/* reset_CPgrid M/DiscreteGroupModel.h:67-70 */
int msm_group_reset_cpgrid(msm_group *g, int32_t subject, const double *xyz);
/* m_labels = m_samples (M/DiscreteGroupModel.cpp:177); labels[0] is the sampling-grid centre */
int msm_group_set_labels(msm_group *g, const double *labels, int32_t L);
/* The order of the pair list -- of msm_group_get_pairs and of every pair index and pair range of this interface.  0 (default): estimate_pairs' own
 * (subject A, control point, subject B: M/DiscreteGroupModel.cpp:37-55).  1: control point by control point along a space-filling curve, so that a
 * contiguous range of the list is a region of the sphere: the layout for runs that shard the list over ranks (msm_group_fusion_move_dev), whose
 * slices then read a part of every resampled map instead of whole maps.  Same set of pairs; the optimiser reads pairs[i] beside the i-th costs
 * (I/Fusion/Fusion.h:157-196).  Takes effect at the next set-up. */
int msm_group_set_pair_layout(msm_group *g, int32_t layout);
/* Who computes estimate_rotation_matrix(centre, vertex) (R/point.cpp:97-152) for the data meshes' vertices in get_patch_data (M/DiscreteGroupModel.cpp:97-105):
 * 1 (default) the host's libm as the reference calls it (the matrices are applied on the device in the reference's operation order): the rotated meshes are then
 * the reference's to the bit -- which decides the resampled values where a label carries data vertices exactly onto template vertices (a regular icosphere as the
 * template under regular data grids: the last bits of the rotation pick the triangle that "contains" such a vertex); V x 0.15 us of host time per subject and
 * set-up, beside the GPU's work.  0: the device (its own acos / sincos: the rotated meshes agree with the reference's to 1e-13). */
int msm_group_set_rotation_mode(msm_group *g, int32_t mode);
/* setupCostFunction M/DiscreteGroupModel.cpp:163-196: estimate_pairs :37-55, get_spacings :123-139, get_rotations :77-86,
 * get_patch_data :88-121 */
int msm_group_setup(msm_group *g);
/* Sharded set-up (one process per GPU, subjects split over ranks): every rank runs msm_group_setup_subjects on ITS
 * subjects (the pair list, spacings and rotations are computed for all subjects -- they only need the control grids),
 * exports them, imports the other ranks' subjects (the exchange itself is the caller's all-gather / broadcast over
 * RCCL, see newmsm_amd/dist.py), then msm_group_finalize.  msm_group_setup = all subjects + finalize.
 * F: L x D x V(template) doubles; pptr: N*L + 1; pidx: pptr[N*L] entries (query *npidx with pidx == NULL). */
int msm_group_setup_subjects(msm_group *g, const int32_t *subjects, int32_t n);
int msm_group_export_subject(msm_group *g, int32_t subject, double *F, int32_t *pptr, int32_t *pidx, int64_t cap, int64_t *npidx);
int msm_group_import_subject(msm_group *g, int32_t subject, const double *F, const int32_t *pptr, const int32_t *pidx, int64_t npidx);
/* the same exchange with the caller's buffers in DEVICE memory of this context's GPU (what an RCCL all-gather reads and writes):
 * no host copy in between.  F_dev / pptr_dev / pidx_dev as above; any of them may be NULL on export. */
int msm_group_export_subject_dev(msm_group *g, int32_t subject, double *F_dev, int32_t *pptr_dev, int32_t *pidx_dev, int64_t cap, int64_t *npidx);
int msm_group_import_subject_dev(msm_group *g, int32_t subject, const double *F_dev, const int32_t *pptr_dev, const int32_t *pidx_dev, int64_t npidx);
/* n subjects at once out of / into strided device buffers -- the send and receive buffers of ONE all-gather: subject subjects[k]'s arrays start at
 * F_dev + k * F_stride (doubles), pptr_dev + k * pptr_stride, pidx_dev + k * pidx_stride (int32 entries); npidx[k] = its index count (written on
 * export, read on import).  One range-check launch and one synchronisation per call; the imported row offsets stay on the device (the host copy is
 * fetched if msm_group_patch asks).  msm_group_setup_more_subjects: further subjects of this rank after msm_group_setup_subjects, so that a rank can
 * set up and exchange its shard in chunks (the exchange of one chunk overlapping the set-up of the next, newmsm_amd/dist.py). */
int msm_group_export_subjects_dev(msm_group *g, const int32_t *subjects, int32_t n, double *F_dev, int64_t F_stride, int32_t *pptr_dev, int64_t pptr_stride,
                                  int32_t *pidx_dev, int64_t pidx_stride, int64_t *npidx);
int msm_group_import_subjects_dev(msm_group *g, const int32_t *subjects, int32_t n, const double *F_dev, int64_t F_stride, const int32_t *pptr_dev,
                                  int64_t pptr_stride, const int32_t *pidx_dev, int64_t pidx_stride, const int64_t *npidx);
int msm_group_setup_more_subjects(msm_group *g, const int32_t *subjects, int32_t n);
int msm_group_finalize(msm_group *g);
int msm_group_sizes(msm_group *g, int32_t *nodes, int32_t *pairs, int32_t *triplets);
/* S subjects, N control points each, L labels, D feature rows, V(template): the sizes of the exchange buffers above (any pointer may be NULL) */
int msm_group_dims(msm_group *g, int32_t *S, int32_t *N, int32_t *L, int32_t *D, int32_t *Vt);
int msm_group_get_pairs(msm_group *g, int32_t *pairs /* P x 2 */);
int msm_group_get_triplets(msm_group *g, int32_t *triplets /* T x 3 */);
/* one patch (subject, control point, label): ascending template vertex ids and their D values (cap entries); *n = size */
int msm_group_patch(msm_group *g, int32_t subject, int32_t cp, int32_t label, int32_t *ids, double *data, int32_t cap, int32_t *n);
/* computePairwiseCost M/DiscreteGroupCostFunction.cpp:54-98 / computeTripletCost :26-52 for n queries */
int msm_group_pairwise_batch(msm_group *g, const int32_t *pair, const int32_t *la, const int32_t *lb, int32_t n, double *out);
int msm_group_triplet_batch(msm_group *g, const int32_t *triplet, const int32_t *la, const int32_t *lb, const int32_t *lc, int32_t n, double *out);
/* One label step of Fusion::optimize (I/Fusion/Fusion.h:157-196) in one call: labeling (S * N, by global node id) is the
 * current labeling, label the proposed one.  pair_quads[4 * p + k] = pair_data[p].buffer[k] (k = 2 * [A takes the label] +
 * [B takes it]) and triplet_octets[8 * t + k] = triplet_data[t].buffer[k] (k = 000..111); either output may be NULL.
 * Nothing but the labeling travels to the GPU. */
int msm_group_fusion_move(msm_group *g, const int32_t *labeling, int32_t label, double *pair_quads, double *triplet_octets);

/* A slice of one label step for a multi-GPU run: every rank evaluates ITS slice of the pair list and of the triplet list
 * (the loop of M/DiscreteGroupCostFunction.cpp:54-98 over N_cp * S (S - 1) / 2 pairs is what a 64-subject iteration spends its
 * time in) and leaves the results in DEVICE memory, from where the caller gathers them to the optimiser's rank (RCCL gather).
 * pairs [pair0, pair1) -> quads_dev[4 * (pair1 - pair0)], triplets [trip0, trip1) -> octets_dev[8 * (trip1 - trip0)], both in
 * the buffer order of msm_group_fusion_move. */
int msm_group_fusion_move_dev(msm_group *g, const int32_t *labeling, int32_t label, int64_t pair0, int64_t pair1, int64_t trip0, int64_t trip1,
                              double *quads_dev, double *octets_dev);
/* Optional HIP-event timing of a label step's kernels (everything msm_group_fusion_move / _dev queue on the context's stream for one
 * step: the pair passes, the kept-cost copies, the triplets), for bench.py's gmsm roofline: msm_group_move_kernels_ms returns the most recent
 * step's GPU time in milliseconds (-1 when none was timed). */
int msm_group_time_moves(msm_group *g, int enable);
int msm_group_move_kernels_ms(msm_group *g, double *ms);
/* What the pair-cost kernel (k_group_pairwise) does with a query, for the tests that steer it.
 *   msm_group_pair_route   the code path of ONE query whose patches hold cntA and cntB entries, with D feature rows, the measure and `lanes` lanes per query
 *                          (16 or 32 for SSD / correlation, 64 for DICE / genDICE) -- the function the kernel itself calls; pure host arithmetic, no
 *                          context, no device.  route[MSM_PAIR_ROUTE_FAST]: everything in registers, else the general path; [_PADDED]: the length B's
 *                          list is padded to in LDS (64 / 128 / 256; 0 when it is not staged); [_STAGED]: B's ids in LDS, else read from memory;
 *                          [_BEYOND]: general path with entries of A past the 64 rounds x lanes membership bits, looked up again in every pass.
 *   msm_group_pair_launch  what msm_group_finalize decided for this group and what a pair evaluation would be handed NOW; host bookkeeping, no kernel and
 *                          no synchronisation.  out[MSM_PAIR_LAUNCH_LANES]: lanes per query; [_PATCH_MAX]: the largest patch; [_NPATCH] / [_NSMALL]: the
 *                          patches counted and those of at most 80 entries (16 lanes when 10 nsmall >= 9 npatch, unless MSMHIP_GROUP_PAIR_LANES says
 *                          otherwise); [_DICE_LDS]: static plus dynamic LDS bytes of the DICE launch (0 for the other measures); [_DICE_FIT]: 0 it runs
 *                          as it is, 1 the kernel's attribute is raised first (more than 64 KB), 2 refused (more than 160 KB: every pair evaluation fails
 *                          with MSM_ERR_CAPACITY before anything is queued, the group stays usable otherwise); [_PVAL] / [_DIR]: whether the value copies
 *                          and the patch directory serve the WHOLE pair list (a group with imported subjects builds them at its first label step). */
#define MSM_PAIR_ROUTE_FAST 0
#define MSM_PAIR_ROUTE_PADDED 1
#define MSM_PAIR_ROUTE_STAGED 2
#define MSM_PAIR_ROUTE_BEYOND 3
#define MSM_PAIR_LAUNCH_LANES 0
#define MSM_PAIR_LAUNCH_PATCH_MAX 1
#define MSM_PAIR_LAUNCH_NPATCH 2
#define MSM_PAIR_LAUNCH_NSMALL 3
#define MSM_PAIR_LAUNCH_DICE_LDS 4
#define MSM_PAIR_LAUNCH_DICE_FIT 5
#define MSM_PAIR_LAUNCH_PVAL 6
#define MSM_PAIR_LAUNCH_DIR 7
int msm_group_pair_route(int32_t cntA, int32_t cntB, int32_t D, int32_t simmeasure, int32_t lanes, int32_t route[4]);
int msm_group_pair_launch(msm_group *g, int64_t out[8]);

/* ------------------------------------------------------------------------------------------------
 * groupwise MCMC: gMSM with the Monte Carlo optimiser (MCMC::optimise, M/mcmc_opt.h:31-134), subject by subject.
 * AN EXTENSION, opt-in: the reference refuses anything but HOCR in groupwise mode (M/group_mesh_registration.cpp:87).  The group energy restricted to
 * one subject s, the other subjects' labels held fixed, has the form MCMC::optimise reads, so block-coordinate descent over the subjects solves each
 * block with the reference's own optimiser through the unchanged chain kernels; no cost table leaves the device.  Nodes are s * N + v, the pair list
 * is the group's current one (msm_group_get_pairs, whatever layout is set), labeling is over S * N nodes; every pair joins two different subjects
 * (estimate_pairs, M/DiscreteGroupModel.cpp:37-55).
 *   incidence          for node n the pair indices p with pairs[2p] == n or pairs[2p + 1] == n, ascending.
 *   conditional unary  U_s[l * N + v] = the sum, from 0.0, over the incident pairs of s * N + v in ascending pair index of computePairwiseCost(p, la, lb)
 *                      (M/DiscreteGroupCostFunction.cpp:54-98), the node's own slot taking l and the partner's slot labeling[partner]; sequential FP64,
 *                      each addition rounded, no contraction; a node without incident pairs gives exactly 0.0.  Each term is the value
 *                      msm_group_pairwise_batch returns for that query (the same kernel through the same launcher): --fixnan, masks and all four
 *                      measures are as they are there.
 *   triplet table      tc_s[t][a][b][c] = computeTripletCost (:26-52) of the subject's t-th triplet in list order (msm_group_triplet_batch's value for
 *                      (s * Tc + t, a, b, c)); node ids are made local by subtracting s * N.
 *   block              msm_mcmc_optimise_chains' semantics on (U_s, tc_s, local triplets, N, L, Tc, mcparam, iters, seeds[K]) from the subject's current
 *                      labels: every chain is bit for bit the host optimiser on its seed, energies are msm_mcmc_energy, best is msm_mcmc_best.  The best
 *                      chain's labelling replaces the subject's labels only when its energy is strictly below the start's energy in the same table
 *                      arithmetic; a NaN energy is never accepted.  Otherwise the subject keeps its labels.
 *   pass               the subjects in ascending order, each block seeing the labels the earlier blocks wrote.
 *   seeds              chain k of subject s in pass p of iteration it: seed + it + 1000003 k + 15485863 (p S + s) (chain 0 of subject 0 in pass 0 is the
 *                      pairwise loops' seed).
 * The group energy is E_s plus terms that do not involve subject s (each incident pair appears once in U_s), so with the acceptance rule a pass never
 * raises the table energy.  That is the whole claim: nothing is promised about the quality of the minimum.
 *
 * The device entry points refuse, before anything is queued: a group that is not finalised (MSM_ERR_STATE); a group with imported subjects (a rank of a
 * sharded run: MSM_ERR_STATE, "one rank only"); a subject, label or K (1 ... 256) out of range, mcparam outside (0, 1], more than 65535 labels or more
 * than 80000 control points (msm_mcmc_optimise_chains_gpu's messages); a DICE group whose patches do not fit (msm_group_pairwise_batch's message).
 *   msm_group_mcmc_incidence [host]   pairs (P x 2, nodes in [0, nodes)) -> CSR: ptr[nodes + 1], idx[ptr[nodes]] (room for 2 P entries).  O(P).
 *   msm_group_mcmc_seeds [host]       the K seeds of one block by the rule above.
 *   msm_group_mcmc_accept [host]      the acceptance rule: *accepted = best < start.
 *   msm_group_conditional_unary       U_s of `labeling` on the device; U (L x N, may be NULL) receives it.
 *   msm_group_subject_triplet_table   tc_s on the device (filled in triplet ranges, so a table beyond 2^31 values is no special case); tc
 *                                     (Tc x L^3, may be NULL) receives it.
 *   msm_group_mcmc_subject            one block: labeling (S * N, in and out), energies[0] the start's and [1] the kept energy, *accepted 0 or 1
 *                                     (either may be NULL).  The proposals are drawn as msm_ctx_set_mcmc_draw says.
 *   msm_group_mcmc_pass               `passes` passes over the subjects with the seed rule.  per_block (passes * S records of 8 doubles, may be NULL):
 *                                     start energy, kept energy, accepted, best chain, then the block's GPU milliseconds by HIP events: query build plus
 *                                     pair costs, segment sums, triplet table, and the sweep kernels (msm_mcmc_gpu_stats).
 * ---------------------------------------------------------------------------------------------- */
int msm_group_mcmc_incidence(const int32_t *pairs, int32_t P, int32_t nodes, int32_t *ptr, int32_t *idx);
int msm_group_mcmc_seeds(uint64_t seed, int32_t it, int32_t pass, int32_t S, int32_t subject, int32_t K, uint64_t *seeds);
int msm_group_mcmc_accept(double start, double best, int32_t *accepted);
int msm_group_conditional_unary(msm_group *g, int32_t subject, const int32_t *labeling, double *U);
int msm_group_subject_triplet_table(msm_group *g, int32_t subject, double *tc);
int msm_group_mcmc_subject(msm_group *g, int32_t subject, int32_t *labeling, double mcparam, int32_t iters, const uint64_t *seeds, int32_t K,
                           double energies[2], int32_t *accepted);
int msm_group_mcmc_pass(msm_group *g, int32_t *labeling, double mcparam, int32_t iters, uint64_t seed, int32_t it, int32_t K, int32_t passes,
                        double *per_block);


/* ------------------------------------------------------------------------------------------------
 * rigid level (--opt=RIGID / AFFINE).  Replaces Rigid_cost_function (M/rigid_costfunction.cpp): the rotation of the whole data
 * grid by three Euler angles that maximises the summed similarity of every SOURCE vertex to the TARGET data around it.  The
 * reference's per-vertex Neighbourhood and sparse similarity matrix are not kept: a vertex's query list depends only on the
 * closest target triangle (one list per target triangle, built once) and its similarities only on the data (computed inline).
 * Host arrays are complete on return.
 * ---------------------------------------------------------------------------------------------- */
typedef struct msm_rigid msm_rigid;

/* Rigid_cost_function(target, source, FEAT) + set_simmeasure + initialise (:26-48): TARGET and SOURCE are both the level's data grid
 * (SOURCE's coordinates are copied; min_sigma = calculate_MeanVD of them, R/mesh.cpp:276-293); in_feat (D x Vsource) and ref_feat
 * (D x Vtarget) the level's featurespace.  simmeasure 1 (SSD) or 2 (correlation); anything else: MSM_ERR_INVALID (the reference computes
 * all-zero similarities there).  The target mesh must outlive the handle, and its coordinates and triangles must not change while the
 * handle exists: the query lists and min_sigma are built here, and the kernels read the target's coordinates on every evaluation. */
msm_rigid *msm_rigid_create(msm_ctx *ctx, msm_mesh *target, msm_mesh *source, const double *in_feat, const double *ref_feat, int32_t D,
                            int32_t simmeasure);
void msm_rigid_destroy(msm_rigid *r);
/* update_source (:50): SOURCE's coordinates (3 x V SoA) */
int msm_rigid_set_source(msm_rigid *r, const double *xyz);
int msm_rigid_get_source(msm_rigid *r, double *xyz);
/* rigid_cost_mesh (:123-139) for n Euler triples (euler: n x 3; n <= 4 per launch, more are split): sums[k] = the cost of triple k;
 * per_vertex (n x V, or NULL) = current_sim after each.  SOURCE is unchanged. */
int msm_rigid_cost(msm_rigid *r, const double *euler, int32_t n, double *sums, double *per_vertex);
/* rotate_in_mesh (:110-121): SOURCE rotated in place by euler_rotate (R/point.cpp:154-171) */
int msm_rigid_rotate(msm_rigid *r, const double euler[3]);
/* run (:164-228), quirks included: the optimiser's control flow on the host, one launch per gradient (three probes) and one per
 * accepted-or-not step.  trace (cap x 6, may be NULL with cap 0): one row per iteration {loop, iter, per, step, grad_zero, accepted}
 * where step is the step the iteration took and grad_zero the cost it evaluated; *n = the number of iterations (rows past cap are not
 * written).  summary = {RECinit, RECfinal, evaluations}.  SOURCE holds the result. */
int msm_rigid_run(msm_rigid *r, int32_t iters, double stepsize, double gradsampling, double *trace, int32_t cap, int32_t *n, double summary[3]);
/* GPU time of the cost launches of the last msm_rigid_run / msm_rigid_cost (HIP events): ms[0] total milliseconds, ms[1] launches */
int msm_rigid_kernel_ms(msm_rigid *r, double ms[2]);

/* ------------------------------------------------------------------------------------------------
 * strain maps of an aMSM run (save_transformed_data, M/mesh_registration.cpp:397-407).
 * ---------------------------------------------------------------------------------------------- */
/* calculate_strains(fit_radius, orig, final) (M/reg_tools.cpp:365-549): orig is the input anatomy with its own triangles (its normals are
 * estimate_normals', R/mesh.cpp:133-150), final_xyz (3 x V SoA) the same vertices after the registration (project_anatomical_mesh's result).
 * Per vertex i: the members j of |x_i - x_j| <= r with n_j . n_i >= 0, r = fit_radius grown by 0.5 until there are more than 8; a
 * least-squares quadratic fit of the neighbourhood in i's tangent frame; the principal stretches of the deformation gradient.
 * strains (4 x V): the maximum and minimum principal stretch and 0.5 (lambda^2 - 1) of each.  kept (V, optional): the member count;
 * radius (V, optional): the final r.  V must equal orig's vertex count and fit_radius be > 0.  A mesh where some vertex can never
 * have 9 members (the reference's radius would grow forever): MSM_ERR_INVALID.  Host arrays are complete on return. */
int msm_calculate_strains(msm_mesh *orig, const double *final_xyz, int32_t V, double fit_radius, double *strains, int32_t *kept, double *radius);

/* ------------------------------------------------------------------------------------------------
 * after a groupwise run: dedrifting and the group's statistics.  Replaces what the reference's tutorial pipeline does with wb_command and nibabel
 * once gMSM has written its spheres (gMSM_scripts/gMSM_tutorial/gw_MSM.sh:65-128, compare_stats.py; docs/guide.md, "After registration, we apply
 * dedrifting").  Per subject s: M_s its input sphere as the run used it (recentred, radius 100), R_s its registered sphere (sphere-<s>.reg: the
 * same triangles), F_s its data (D x V_s); T the template.  All searches and weights are Resampler::get_barycentric_weights (R/resampler.cpp:142-167).
 * Call order: accumulate every subject, finish, correct every subject, group statistics.  Everything between the uploads of a subject's arrays and
 * the downloads of its results stays on the device; the subjects' resampled maps stay resident in the handle (S x D x V(T) doubles).
 * Agreement with wb_command's own arithmetic (-surface-modify-sphere -recenter, -surface-distortion -local-affine-method) is unpinned: Workbench is
 * not available to this project; the definitions below are the contract.
 * ---------------------------------------------------------------------------------------------- */
typedef struct msm_dedrift msm_dedrift;
/* One handle per group of num_subjects subjects on the template's context.  The template must outlive the handle. */
msm_dedrift *msm_dedrift_create(msm_ctx *ctx, msm_mesh *template_mesh, int32_t num_subjects);
void msm_dedrift_destroy(msm_dedrift *d);
/* forget the running sum, the warp and the resident maps: the handle serves another group of the same size on the same template */
int msm_dedrift_reset(msm_dedrift *d);
/* gw_MSM.sh:76-80 (-surface-sphere-project-unproject, the inverse of one registration) and one term of :82-87 (-surface-average): for every vertex of
 * T the closest triangle of reg (= R_s) and its weights, applied to orig_xyz (= M_s, 3 x V SoA, V = reg's vertex count) without normalisation --
 * project_anatomical_mesh's sum (R/resampler.cpp:260-282) -- and added to the running sum.  The tutorial passes the template as the sphere to
 * unproject to, which is the same thing exactly when M_s is the template (its situation); M_s is the general form.  The additions happen in the
 * order of the calls.  Optional outputs (each may be NULL; with all three NULL the call only queues its work and msm_dedrift_finish reports a failed
 * search): tri_id (V(T)) and w (3 x V(T)) the search's decisions, inverse_xyz (3 x V(T)) the subject's inverse.  A later all-reduce of the running
 * sum over ranks fits between the last accumulate and finish; nothing else about several ranks is built. */
int msm_dedrift_accumulate(msm_dedrift *d, msm_mesh *reg, const double *orig_xyz, int32_t V, int32_t *tri_id, double *w, double *inverse_xyz);
/* gw_MSM.sh:82-92 (-surface-average, -surface-modify-sphere 100 -recenter): drift = running sum / S; the dedrift warp W = drift minus the midpoint of
 * its axis-aligned bounding box, every vertex scaled to length 100.  W stays on the device for msm_dedrift_correct; warp_xyz / drift_xyz (3 x V(T),
 * optional) receive copies.  Fails with MSM_ERR_STATE unless all S subjects have been accumulated. */
int msm_dedrift_finish(msm_dedrift *d, double *warp_xyz, double *drift_xyz);
/* gw_MSM.sh:94-128 for subject `subject`: corrected_s = sphere_project_warp(R_s, T, W) (-surface-sphere-project-unproject with the dedrift warp,
 * R/resampler.cpp:311-328) -- reg holds corrected_s afterwards, as msm_mesh_sphere_project_warp leaves a mesh; resampled_s = metric_resample of data
 * (D x V) from corrected_s onto T (-metric-resample ADAP_BARY_AREA; the arithmetic of msm_metric_resample), kept resident; distortion_s (2 x V):
 * per triangle of M_s (orig_xyz) against the same triangle of corrected_s, J and R as triangle_strain forms them (M/reg_tools.cpp:578-593, through the
 * tangent frames of calculate_triangular_strain :698-743), per vertex the plain mean over its incident triangles in trID order of log2 J (row 0,
 * areal) and log2 R (row 1, shape) (-surface-distortion -local-affine-method -log2).  Outputs may be NULL; tri_id (V) / w (3 x V): the decisions of
 * the search of R_s's vertices on T.  D must be the same for every subject of a group. */
int msm_dedrift_correct(msm_dedrift *d, int32_t subject, msm_mesh *reg, const double *orig_xyz, int32_t V, const double *data, int32_t D,
                        double *corrected_xyz, double *resampled, double *distortion, int32_t *tri_id, double *w);
/* a subject's maps on the template (D x V(T)) from the host instead of from msm_dedrift_correct: group statistics of maps that exist already (the
 * un-dedrifted transformed_and_reprojected-<i> files of the run, compare_stats.py's "before") */
int msm_dedrift_set_map(msm_dedrift *d, int32_t subject, const double *map, int32_t D);
/* gw_MSM.sh:108-119 (-metric-merge, -metric-reduce MEAN / STDEV) and compare_stats.py:12-69 over the resident maps: mean, stdev (D x V(T)): over the
 * subjects, two passes in subject order, population form; cc (D x S x S): Pearson correlation over the vertices (numpy.corrcoef's quantity); dice
 * (D x S x S): masks x > numpy.percentile(x, percentile) (linear interpolation between order statistics; compare_stats.py:20-23 uses 75),
 * 2 |A and B| / (|A| + |B|).  Any output may be NULL (its kernels are not run).  The group figures are the means over the pairs i < j. */
int msm_dedrift_group_stats(msm_dedrift *d, double percentile, double *mean, double *stdev, double *cc, double *dice);
/* gMSM_scripts/run_cgMSM_ver_gw_iter.sh:171-192 (every subject of a child group pushed through its group's dedrifted registration C_g when two groups are
 * merged): replaces the handle's warp W by warp_xyz (3 x V(T) SoA), a deformation of the template's vertices, taken as it is -- neither recentred nor
 * rescaled.  msm_dedrift_correct may follow without any accumulate / finish, and the call may be repeated between subjects (child g's subjects go through
 * C_g).  msm_dedrift_finish keeps its rule (MSM_ERR_STATE unless S subjects were accumulated) and replaces a set warp; msm_dedrift_reset forgets it.  NULL:
 * MSM_ERR_INVALID.  An upload and a state flag: no kernel. */
int msm_dedrift_set_warp(msm_dedrift *d, const double *warp_xyz);
/* run_cgMSM_ver_gw_iter.sh:194-218 and extract_info.py (the figures of a merged group and of each of its child groups; the medial wall kept out of them):
 * msm_dedrift_group_stats over the n listed resident subjects (distinct indices in [0, S), any order; matrices and sums follow the list's order) and the
 * template vertices the mask keeps (mask: V(T) values, v is kept iff mask[v] > 0, a NaN is not kept; NULL keeps all; K = the kept count).
 * mean, stdev (D x V(T)): over the listed subjects in list order, two passes, population form, for every vertex -- the mask does not enter.
 * cc (D x n x n): numpy.corrcoef(x[keep], y[keep])[0, 1], diagonal 1.  dice (D x n x n): masks x[keep] > numpy.percentile(x[keep], percentile) (linear
 * interpolation, virtual index and fraction from K), 2 |A and B| / (|A| + |B|), on the diagonal too.  cc_mean, dice_mean (D): the mean over the pairs
 * a < b of the list, summed on the device in one fixed tree per matrix; NaN when n = 1.  Any output may be NULL (its kernels are not run; the means may be
 * asked for without the matrices).  Integer atomics only: two calls give the same bits.  A pair tile of 8 x 8 listed subjects reads each of its map rows
 * once.  msm_dedrift_group_stats is this computation with every subject listed in order and no mask: the same bits.  MSM_ERR_INVALID: n < 1, an index
 * out of range or repeated, a mask that keeps nothing, a percentile outside [0, 100]; MSM_ERR_STATE: a listed subject without resident maps.  Nothing
 * is launched on either. */
int msm_dedrift_group_stats_select(msm_dedrift *d, const int32_t *subjects, int32_t n, const double *mask, double percentile, double *mean, double *stdev,
                                   double *cc, double *dice, double *cc_mean, double *dice_mean);

/* ------------------------------------------------------------------------------------------------
 * after a cohort has been registered to one template, subject by subject (gMSM_scripts/newMSM_HCP_to_template_v2.sh, run_HCP_to_template_v2.sh,
 * gMSM_tutorial/typical_MSM.sh; get_group_stats.py, compare_stats.py): the distortion maps and their summary without a dedrift handle, a mesh
 * handle, a search or a tree.
 * ---------------------------------------------------------------------------------------------- */
/* wb_command -surface-distortion -local-affine-method -log2 by the definition of msm_dedrift_correct's distortion, for S
 * deformed copies (final_xyz: S x 3 x V SoA each) of ONE original sphere (orig_xyz 3 x V SoA, tri 3 x T SoA): per triangle J and R as triangle_strain
 * forms them, each triangle evaluated once per copy; per vertex the plain mean over its incident triangles in trID order of log2 J (row 0, areal)
 * and log2 R (row 1, shape), 0 for a vertex without a triangle.  out: S x 2 x V.  One launch per step serves all S copies.  S <= 0, V <= 0 or a
 * triangle index outside [0, V): MSM_ERR_INVALID, nothing is launched. */
int msm_surface_distortion(msm_ctx *ctx, const double *orig_xyz, const int32_t *tri, int32_t V, int32_t T, const double *final_xyz, int32_t S, double *out);
/* the distortion summary of compare_stats.py over |x[i]|, i < n: *mean (one sum of fixed shape: two calls give the same bits), *max, and for every
 * percentiles[q] in [0, 100] values[q] = numpy.percentile(|x|, percentiles[q]) (linear interpolation between the two order statistics, which a radix
 * select over an integer key finds across workgroups; integer counters only).  A NaN anywhere makes every output NaN, as numpy does; infinities are
 * outside the contract.  mean / max may be NULL; np may be 0 (at most 16).  n <= 0, np < 0 or a percentile outside [0, 100]: MSM_ERR_INVALID. */
int msm_abs_summary(msm_ctx *ctx, const double *x, int64_t n, const double *percentiles, int32_t np, double *mean, double *max, double *values);

#ifdef __cplusplus
}
#endif
#endif /* MSMHIP_H */
