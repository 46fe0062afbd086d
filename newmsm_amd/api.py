"""Thin Python mirror of the reference's C++ interfaces on top of the libmsmhip C ABI.

Names follow newMSM: Mesh / Octree queries and the free functions of resampler.h
(/root/reference/libraries/msm-newresampler/src/resampler.h:38-53), and the evaluator interface of
DiscreteCostFunction (/root/reference/libraries/msm-newmeshreg/src/DiscreteCostFunction.h:41-59,
:161-209).  Points are (N,3) numpy arrays here; the ABI's 3 x N SoA layout is produced at the boundary.
This module is plumbing for tests and bench.py -- all computation happens in libmsmhip.so.
"""
import collections
import ctypes as C

import numpy as np

from ._lib import CostParams, LevelFeaturesParams, MsmError, c_dp, c_ip, c_lp, check, lib

WEIGHTS_PROJECTED = 0
WEIGHTS_RAW = 1
KINDS = dict(univariate=0, multivariate=1, patchwise=2, ho_univariate=3, ho_multivariate=4)


def _soa(points):
    """(N,3) -> contiguous 3 x N"""
    a = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3).T)
    return a, a.ctypes.data_as(c_dp)


def _aos(soa, n):
    return np.ascontiguousarray(np.asarray(soa).reshape(3, n).T)


def _tri_soa(tri):
    a = np.ascontiguousarray(np.asarray(tri, dtype=np.int32).reshape(-1, 3).T)
    return a, a.ctypes.data_as(c_ip)


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(c_dp)


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(c_ip)


# ------------------------------------------------------------------ host helpers
def device_count():
    return lib().msm_device_count()


def icosphere_counts(order):
    v, t = C.c_int32(), C.c_int32()
    check(lib().msm_icosphere_counts(order, C.byref(v), C.byref(t)))
    return v.value, t.value


def make_mesh_from_icosa(order, radius=100.0):
    """make_mesh_from_icosa(order) + true_rescale(radius). Returns (xyz[V,3], tri[T,3])."""
    V, T = icosphere_counts(order)
    xyz = np.zeros((3, V))
    tri = np.zeros((3, T), dtype=np.int32)
    check(lib().msm_icosphere(order, float(radius if radius else 0.0), xyz.ctypes.data_as(c_dp), tri.ctypes.data_as(c_ip)))
    return np.ascontiguousarray(xyz.T), np.ascontiguousarray(tri.T)


def mesh_adjacency(tri, V):
    t, pt = _tri_soa(tri)
    T = t.shape[1]
    nbr_ptr = np.zeros(V + 1, dtype=np.int32)
    tid_ptr = np.zeros(V + 1, dtype=np.int32)
    check(lib().msm_mesh_adjacency(pt, V, T, nbr_ptr.ctypes.data_as(c_ip), None, tid_ptr.ctypes.data_as(c_ip), None))
    nbr = np.zeros(nbr_ptr[-1], dtype=np.int32)
    tid = np.zeros(tid_ptr[-1], dtype=np.int32)
    check(lib().msm_mesh_adjacency(pt, V, T, nbr_ptr.ctypes.data_as(c_ip), nbr.ctypes.data_as(c_ip), tid_ptr.ctypes.data_as(c_ip),
                                   tid.ctypes.data_as(c_ip)))
    return nbr_ptr, nbr, tid_ptr, tid


def vertex_areas(xyz, tri):
    x, px = _soa(xyz)
    t, pt = _tri_soa(tri)
    out = np.zeros(x.shape[1])
    check(lib().msm_vertex_areas(px, pt, x.shape[1], t.shape[1], out.ctypes.data_as(c_dp)))
    return out


def cp_spacings(xyz, tri):
    x, px = _soa(xyz)
    t, pt = _tri_soa(tri)
    ms = np.zeros(x.shape[1])
    mvd = C.c_double()
    check(lib().msm_cp_spacings(px, pt, x.shape[1], t.shape[1], ms.ctypes.data_as(c_dp), C.byref(mvd)))
    return ms, mvd.value


def label_sampling_grid(sg_order, max_dist, abs_is_int=False, cap=4096):
    s = np.zeros((3, cap))
    b = np.zeros((3, cap))
    ns, nb = C.c_int32(), C.c_int32()
    check(lib().msm_label_sampling_grid(sg_order, float(max_dist), int(abs_is_int), cap, s.ctypes.data_as(c_dp), C.byref(ns),
                                        b.ctypes.data_as(c_dp), C.byref(nb)))
    return np.ascontiguousarray(s[:, : ns.value].T), np.ascontiguousarray(b[:, : nb.value].T)


def rescale_sampling_grid(samples, scale):
    s, ps = _soa(samples)
    n = s.shape[1]
    out = np.zeros((3, n))
    sc = C.c_double(scale)
    check(lib().msm_rescale_sampling_grid(ps, n, C.byref(sc), out.ctypes.data_as(c_dp)))
    return np.ascontiguousarray(out.T), sc.value


def estimate_rotation_matrix(ci, index):
    R = np.zeros(9)
    check(lib().msm_rotation_matrix(_d(ci)[1], _d(index)[1], R.ctypes.data_as(c_dp)))
    return R.reshape(3, 3)


def cp_rotations(centre, cp_xyz):
    x, px = _soa(cp_xyz)
    rot = np.zeros((x.shape[1], 9))
    check(lib().msm_cp_rotations(_d(centre)[1], px, x.shape[1], rot.ctypes.data_as(c_dp)))
    return rot


def octree_signature(xyz, tri):
    """[host] statistics and leaf signature of the search tree of a mesh (testing hook)."""
    x, px = _soa(xyz)
    t, pt = _tri_soa(tri)
    stats = (C.c_int64 * 5)()
    sig = C.c_uint64(0)
    check(lib().msm_octree_signature(px, pt, x.shape[1], t.shape[1], stats, C.byref(sig)))
    return dict(nodes=stats[0], leaves=stats[1], depth=stats[2], refs=stats[3], max_leaf=stats[4]), sig.value


def ray_table_check(xyz, tri, nsamples=20000, seed=1):
    """[host] the direction table's guarantee checked point by point against the reference's leaf search (testing hook, msm_ray_table_check)."""
    x, px = _soa(xyz)
    t, pt = _tri_soa(tri)
    rep = (C.c_int64 * 10)()
    check(lib().msm_ray_table_check(px, pt, x.shape[1], t.shape[1], nsamples, seed, rep))
    return dict(points=rep[0], by_float=rep[1], by_fp64=rep[2], open=rep[3], violations=rep[4], unusable=rep[5], with_exclusions=rep[6], simple=bool(rep[7]), boxes_checked=rep[8], refused_by_boxes=rep[9])


def ray_hint_check(xyz, tri, nsamples=20000, seed=1, return_cells=False):
    """[host] how often the direction table's first candidate is the answer, with and without the cells' sub-cell hints, and that the hints leave
    every cell's candidates alone (testing hook, msm_ray_hint_check).  return_cells: also the cell array as stored, (cells, 4) int32."""
    x, px = _soa(xyz)
    t, pt = _tri_soa(tri)
    rep = (C.c_int64 * 8)()
    cells = np.zeros((6 * 512 * 512, 4), dtype=np.int32) if return_cells else None  # (the largest table build_ray_table makes)
    check(lib().msm_ray_hint_check(px, pt, x.shape[1], t.shape[1], nsamples, seed, rep, cells.ctypes.data_as(c_ip) if return_cells else None, cells.size if return_cells else 0))
    out = dict(points=rep[0], hinted=rep[1], unhinted=rep[2], listed=rep[3], cells_changed=rep[4], cells=rep[5], cells_with_more=rep[6], subcells=rep[7])
    if return_cells:
        out["cell_array"] = cells[: rep[5]].copy()
    return out


def ray_depth_check(xyz, tri, nsamples=20000, seed=1):
    """[host] where in its cell's candidate list a point's triangle sits, in the order the kernels try the candidates (testing hook,
    msm_ray_depth_check; the points and the triangles of ray_hint_check).  at: points by position 0, 1, 2, 3, 4 and 5 or beyond."""
    x, px = _soa(xyz)
    t, pt = _tri_soa(tri)
    rep = (C.c_int64 * 8)()
    check(lib().msm_ray_depth_check(px, pt, x.shape[1], t.shape[1], nsamples, seed, rep))
    return dict(points=rep[0], at=[int(rep[k]) for k in range(1, 7)], unlisted=rep[7])


def ray_cert_check(xyz, tri, nsamples=20000, seed=1, return_cells=False):
    """[host] the certificates of the direction table's cells: every sampled point of a certified sub-cell must have the sub-cell's first candidate for its
    triangle, by the FP64 edge-plane test and by the reference's leaf search (testing hook, msm_ray_cert_check).  The points are `nsamples` random directions
    and some 10 000 placed ones (borders and corners of sub-cells, cells and cube faces; mesh vertices; edge midpoints).  return_cells: as ray_hint_check."""
    x, px = _soa(xyz)
    t, pt = _tri_soa(tri)
    rep = (C.c_int64 * 8)()
    cells = np.zeros((6 * 512 * 512, 4), dtype=np.int32) if return_cells else None  # (the largest table build_ray_table makes)
    check(lib().msm_ray_cert_check(px, pt, x.shape[1], t.shape[1], nsamples, seed, rep, cells.ctypes.data_as(c_ip) if return_cells else None, cells.size if return_cells else 0))
    out = dict(points=rep[0], certified_points=rep[1], fp64_failures=rep[2], reference_disagrees=rep[3], subcells=rep[4], certified_subcells=rep[5], cells=rep[6], placed=rep[7])
    if return_cells:
        out["cell_array"] = cells[: rep[6]].copy()
    return out


def ray_table_signature(xyz, tri):
    """[host] a signature of the whole direction table of a mesh: its sizes, its radius range (bit patterns) and a 64-bit hash of each of its four arrays
    (testing hook, msm_ray_table_signature).  A mesh without a table gives G = 0 and zero counts."""
    x, px = _soa(xyz)
    t, pt = _tri_soa(tri)
    out = (C.c_uint64 * 13)()
    check(lib().msm_ray_table_signature(px, pt, x.shape[1], t.shape[1], out))
    names = ("G", "simple", "certs", "cells", "edges", "more", "excl", "r2lo_bits", "r2hi_bits", "cell_hash", "edge_hash", "more_hash", "excl_hash")
    return dict(zip(names, (int(v) for v in out)))


def estimate_triplets(tri):
    t, pt = _tri_soa(tri)
    out = np.zeros((t.shape[1], 3), dtype=np.int32)
    check(lib().msm_estimate_triplets(pt, t.shape[1], out.ctypes.data_as(c_ip)))
    return out


def estimate_pairs(tri, V):
    t, pt = _tri_soa(tri)
    n = lib().msm_estimate_pairs(pt, V, t.shape[1], None)
    if n < 0:
        check(n)
    out = np.zeros((n, 2), dtype=np.int32)
    lib().msm_estimate_pairs(pt, V, t.shape[1], out.ctypes.data_as(c_ip))
    return out


# ------------------------------------------------------------------ context / mesh
class Context:
    """One per GPU (msm_ctx)."""

    def __init__(self, device=0, stream=None):
        L = lib()
        self.h = L.msm_ctx_create(device) if stream is None else L.msm_ctx_create_on_stream(device, C.c_void_p(stream))
        if not self.h:
            raise MsmError(-5, L.msm_last_error().decode())
        self.device = device

    def synchronize(self):
        check(lib().msm_ctx_synchronize(self.h))

    @property
    def stream(self):
        return lib().msm_ctx_stream(self.h)

    def wait_stream(self, hip_stream=None):
        """everything the library queues on this context from now on waits for what `hip_stream` (a hipStream_t value; None = the default stream)
        holds now (msm_ctx_wait_stream): the ordering a caller owes the ..._dev entry points for buffers its own stream is still filling"""
        check(lib().msm_ctx_wait_stream(self.h, C.c_void_p(hip_stream or 0)))

    def staging_stats(self):
        """pinned staging blocks of this context: dict(blocks, bytes, allocated, waits) (msm_ctx_staging_stats)"""
        out = (C.c_int64 * 4)()
        check(lib().msm_ctx_staging_stats(self.h, out))
        return dict(blocks=int(out[0]), bytes=int(out[1]), allocated=int(out[2]), waits=int(out[3]))

    def host_array(self, shape, dtype=np.float64):
        """A numpy array in pinned host memory mapped into the GPU's address space (msm_host_alloc): passed as an output array
        the kernels write it directly.  Lives as long as the context."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = lib().msm_host_alloc(self.h, max(n, 8))
        if not p:
            raise MsmError(-2, lib().msm_last_error().decode())
        buf = (C.c_char * max(n, 8)).from_address(p)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def scratch_host_array(self, name, shape, dtype=np.float64):
        """a view of a grow-only pinned buffer kept per `name` on this context.  When it has to grow a new block is taken and the old
        one is NOT freed: arrays handed out earlier may still be referenced by the caller (a freed block is unmapped -- reading such a
        view would fault).  Blocks grow by doubling, so what stays behind is less than the final block; all go with the context."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        bufs = self.__dict__.setdefault("_scratch_pinned", {})
        cur = bufs.get(name)
        if cur is None or cur[1] < n:
            cap = max(2 * n, 4096) if cur is not None else max(n + n // 8, 4096)
            p = lib().msm_host_alloc(self.h, cap)
            if not p:
                raise MsmError(-2, lib().msm_last_error().decode())
            cur = bufs[name] = (p, cap)
        buf = (C.c_char * cur[1]).from_address(cur[0])
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def release_host_array(self, arr):
        """gives a Context.host_array block back (msm_host_free); the caller guarantees that no view of it is used afterwards"""
        if getattr(self, "h", None):
            lib().msm_host_free(self.h, C.c_void_p(arr.ctypes.data))

    def set_mcmc_draw(self, mode):
        """msm_ctx_set_mcmc_draw: where the GPU entry points of the Monte Carlo optimiser get their proposals on this context -- 0 / "host" (the default)
        or 1 / "gpu": drawn by a kernel, the same proposals bit for bit"""
        check(lib().msm_ctx_set_mcmc_draw(self.h, {"host": 0, "gpu": 1}.get(mode, mode)))

    def get_mcmc_draw(self):
        mode = C.c_int32(-1)
        check(lib().msm_ctx_get_mcmc_draw(self.h, C.byref(mode)))
        return mode.value

    def time_queries(self, on=True):
        """HIP events around the search kernel of query_triangles / closest_vertex calls (msm_ctx_time_queries)"""
        check(lib().msm_ctx_time_queries(self.h, int(on)))

    def query_kernel_ms(self):
        ms = C.c_double(-1.0)
        check(lib().msm_ctx_query_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    @staticmethod
    def query_lanes(n_queries):
        """lanes per query (4 or 8) of the search kernels for a launch of n_queries (msm_query_lanes): the k_query<G> instantiation that runs"""
        return int(lib().msm_query_lanes(int(n_queries)))

    def forest_signatures(self, xyz_sets, tri):
        """leaf signatures (Mesh.octree_signature) of the trees of B coordinate sets over one triangle list, built together as a forest"""
        sets = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).T) for x in xyz_sets]
        big = np.ascontiguousarray(np.stack(sets))  # B x 3 x V
        t, pt = _tri_soa(tri)
        sig = (C.c_uint64 * len(sets))()
        check(lib().msm_octree_forest_signatures(self.h, big.ctypes.data_as(c_dp), big.shape[2], pt, t.shape[1], len(sets), sig))
        return [int(v) for v in sig]

    def register_host(self, address, nbytes):
        """Pin caller-owned host memory (e.g. a shared-memory mapping) and map it into the GPU's address space
        (msm_host_register): arrays inside it are then written by the GPU directly, like Context.host_array's."""
        check(lib().msm_host_register(self.h, C.c_void_p(address), nbytes))

    def unregister_host(self, address):
        lib().msm_host_free(self.h, C.c_void_p(address))

    def close(self):
        if getattr(self, "h", None):
            lib().msm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Mesh:
    """newresampler::Mesh as the hot path sees it + its Octree (built lazily on the device side)."""

    def __init__(self, ctx, xyz, tri):
        self.ctx = ctx
        x, px = _soa(xyz)
        t, pt = _tri_soa(tri)
        self.V, self.T = x.shape[1], t.shape[1]
        self.tri = np.ascontiguousarray(t.T)
        self.h = lib().msm_mesh_create(ctx.h, px, self.V, pt, self.T)
        if not self.h:
            raise MsmError(-1, lib().msm_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            lib().msm_mesh_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def set_coords(self, xyz):
        check(lib().msm_mesh_update_coords(self.h, _soa(xyz)[1]))

    def get_coords(self):
        out = np.zeros((3, self.V))
        check(lib().msm_mesh_get_coords(self.h, out.ctypes.data_as(c_dp)))
        return np.ascontiguousarray(out.T)

    def prepare_search(self, wait=True):
        """builds the target-side search structures (msm_mesh_prepare_search); returns True when nothing is pending"""
        ready = C.c_int32()
        check(lib().msm_mesh_prepare_search(self.h, int(bool(wait)), C.byref(ready)))
        return bool(ready.value)

    def unfold(self, radius=100.0):
        """unfold (M/reg_tools.cpp:131-178) on the current coordinates; returns (passes, folded vertices of the first pass)."""
        passes, first = C.c_int32(), C.c_int32()
        check(lib().msm_mesh_unfold(self.h, float(radius), C.byref(passes), C.byref(first)))
        return passes.value, first.value

    def set_pvalues(self, feat):
        f, pf = _d(np.atleast_2d(feat))
        assert f.shape[1] == self.V
        check(lib().msm_mesh_set_features(self.h, pf, f.shape[0]))

    def octree_stats(self):
        s = (C.c_int64 * 5)()
        check(lib().msm_mesh_octree_stats(self.h, s))
        return dict(nodes=s[0], leaves=s[1], depth=s[2], refs=s[3], max_leaf=s[4])

    def octree_signature(self):
        """(stats, leaf signature) of the tree as it sits in HBM -- comparable with octree_signature(xyz, tri) of the host build"""
        s = (C.c_int64 * 5)()
        sig = C.c_uint64()
        check(lib().msm_mesh_octree_signature(self.h, s, C.byref(sig)))
        return dict(nodes=s[0], leaves=s[1], depth=s[2], refs=s[3], max_leaf=s[4]), sig.value

    # Octree::get_closest_triangle + get_barycentric_weights
    def query_triangles_soa(self, q_soa, tri, vid, w, mode=WEIGHTS_PROJECTED):
        """msm_query_triangles on the ABI's own layout, no transposes and no allocation: q_soa 3 x N float64, tri N int32, vid 3 x N int32, w 3 x N
        float64 (C-contiguous).  Arrays from Context.host_array (pinned, mapped) are read and written by the copy engine directly -- the call is the
        upload, the kernel, three downloads and one synchronisation.  Returns the status."""
        N = q_soa.shape[1]
        assert q_soa.flags.c_contiguous and tri.flags.c_contiguous and vid.flags.c_contiguous and w.flags.c_contiguous and q_soa.dtype == np.float64
        assert tri.shape == (N,) and vid.shape == (3, N) and w.shape == (3, N) and tri.dtype == np.int32 and vid.dtype == np.int32 and w.dtype == np.float64
        return lib().msm_query_triangles(self.h, q_soa.ctypes.data_as(c_dp), N, tri.ctypes.data_as(c_ip), vid.ctypes.data_as(c_ip), w.ctypes.data_as(c_dp), mode)

    def query_triangles(self, q, mode=WEIGHTS_PROJECTED, check_status=True):
        x, px = _soa(q)
        N = x.shape[1]
        tri = np.zeros(N, dtype=np.int32)
        vid = np.zeros((3, N), dtype=np.int32)
        w = np.zeros((3, N))
        st = lib().msm_query_triangles(self.h, px, N, tri.ctypes.data_as(c_ip), vid.ctypes.data_as(c_ip), w.ctypes.data_as(c_dp), mode)
        if check_status:
            check(st)
        return st, tri, np.ascontiguousarray(vid.T), np.ascontiguousarray(w.T)

    def get_closest_vertex_ID(self, q):
        x, px = _soa(q)
        out = np.zeros(x.shape[1], dtype=np.int32)
        check(lib().msm_closest_vertex(self.h, px, x.shape[1], out.ctypes.data_as(c_ip)))
        return out


# ------------------------------------------------------------------ resampler free functions
def get_adaptive_barycentric_weights(in_mesh, new_mesh, excl=None):
    nnz = C.c_int64()
    pe = _d(excl)[1] if excl is not None else None
    check(lib().msm_adaptive_barycentric_weights(in_mesh.h, new_mesh.h, pe, None, None, None, 0, C.byref(nnz)))
    rp = np.zeros(new_mesh.V + 1, dtype=np.int32)
    col = np.zeros(nnz.value, dtype=np.int32)
    val = np.zeros(nnz.value)
    check(lib().msm_adaptive_barycentric_weights(in_mesh.h, new_mesh.h, pe, rp.ctypes.data_as(c_ip), col.ctypes.data_as(c_ip),
                                                 val.ctypes.data_as(c_dp), nnz.value, C.byref(nnz)))
    return rp, col, val


def metric_resample(in_mesh, data, new_mesh, excl=None, out=None):
    """metric_resample (R/resampler.cpp:304-309); with excl (the EXCL mesh's values on in_mesh) returns (data, resampled mask).  out (optional): the
    D x V(new) result array -- one from Context.host_array is written by the copy engine directly (no staging memcpy)."""
    d, pd = _d(np.atleast_2d(data))
    if out is None:
        out = np.zeros((d.shape[0], new_mesh.V))
    assert out.shape == (d.shape[0], new_mesh.V) and out.flags.c_contiguous and out.dtype == np.float64
    if excl is None:
        check(lib().msm_metric_resample(in_mesh.h, pd, d.shape[0], new_mesh.h, None, out.ctypes.data_as(c_dp), None))
        return out
    eo = np.zeros(new_mesh.V)
    check(lib().msm_metric_resample(in_mesh.h, pd, d.shape[0], new_mesh.h, _d(excl)[1], out.ctypes.data_as(c_dp), eo.ctypes.data_as(c_dp)))
    return out, eo


RESAMPLE_METHODS = dict(adap_bary=0, barycentric=1, nearest=2)
PLAN_DTYPES = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}  # MSM_F64, MSM_F32
PLAN_TILE = 64  # maps per tile of an apply (kPlanTile, csrc/resample_plan.hpp): a ragged tile takes the same kernels with lanes masked


class ResamplePlan:
    """msm_resample_plan: the rows of one (in_mesh -> new_mesh) resampling built once and applied to any number of maps.  A snapshot: later calls on the
    context, set_coords on either mesh or closing either mesh do not change what it does.  method: adap_bary (metric_resample's rows), barycentric
    (surface_resample's) or nearest; excl: the EXCL mesh's values on in_mesh (0 = excluded) or None.  ResamplePlan.smoothing(...) makes the fourth kind:
    smooth_data's Gaussian rows."""

    def __init__(self, in_mesh, new_mesh, method="adap_bary", excl=None):
        if method not in RESAMPLE_METHODS:
            raise ValueError("unknown resampling method %r (one of %s)" % (method, ", ".join(sorted(RESAMPLE_METHODS))))
        self.ctx = in_mesh.ctx
        self.method = method
        self.masked = excl is not None
        if self.masked:
            e, pe = _d(np.asarray(excl).reshape(-1))
            if e.shape[0] != in_mesh.V:
                raise ValueError("excl has %d values, the mesh %d vertices" % (e.shape[0], in_mesh.V))
        else:
            pe = None
        self.h = lib().msm_resample_plan_create(in_mesh.h, new_mesh.h, RESAMPLE_METHODS[method], pe)
        if not self.h:
            raise MsmError(-1, lib().msm_last_error().decode())
        self.V_in, self.V_out, self.nnz, self.longest_row = self.sizes()

    @classmethod
    def smoothing(cls, orig_mesh, sph_low, sigma, excl=None):
        """msm_resample_plan_create_smooth: smooth_data(orig_mesh, ., sph_low, sigma, excl) as a plan -- the neighbourhood sweep runs once, apply then
        smooths any number of float32 / float64 maps and returns (out, smoothed mask) when excl was given.  A float64 apply gives smooth_data's bits."""
        self = cls.__new__(cls)
        self.ctx = orig_mesh.ctx
        self.method = "smoothing"
        self.masked = excl is not None
        self.h = None
        if self.masked:
            e, pe = _d(np.asarray(excl).reshape(-1))
            if e.shape[0] != orig_mesh.V:
                raise ValueError("excl has %d values, the mesh %d vertices" % (e.shape[0], orig_mesh.V))
        else:
            pe = None
        self.h = lib().msm_resample_plan_create_smooth(orig_mesh.h, sph_low.h, float(sigma), pe)
        if not self.h:
            raise MsmError(-1, lib().msm_last_error().decode())
        self.V_in, self.V_out, self.nnz, self.longest_row = self.sizes()
        return self

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            lib().msm_resample_plan_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def sizes(self):
        """(V_in, V_out, nnz, longest row)"""
        vi, vo, lr, nnz = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        check(lib().msm_resample_plan_sizes(self.h, C.byref(vi), C.byref(vo), C.byref(nnz), C.byref(lr)))
        return vi.value, vo.value, nnz.value, lr.value

    def weights(self):
        """the rows as CSR (row_ptr, col, val), read back from the device"""
        rp = np.zeros(self.V_out + 1, dtype=np.int32)
        col = np.zeros(self.nnz, dtype=np.int32)
        val = np.zeros(self.nnz)
        check(lib().msm_resample_plan_weights(self.h, rp.ctypes.data_as(c_ip), col.ctypes.data_as(c_ip), val.ctypes.data_as(c_dp), self.nnz))
        return rp, col, val

    def divisors(self):
        """V_out values: what an apply divides each row's sum by; 0.0 = not divided (every row of the resampling methods)"""
        div = np.zeros(self.V_out)
        check(lib().msm_resample_plan_divisors(self.h, div.ctypes.data_as(c_dp)))
        return div

    def apply(self, data, out=None):
        """D x V_in float32 or float64 -> D x V_out of the same dtype; (out, resampled mask) when the plan has a mask"""
        d = np.asarray(data)
        if d.dtype not in PLAN_DTYPES:
            raise TypeError("ResamplePlan.apply takes float32 or float64 data, not %s" % d.dtype)
        d = np.ascontiguousarray(np.atleast_2d(d))
        if d.shape[1] != self.V_in:
            raise ValueError("data has %d columns, the plan's source %d vertices" % (d.shape[1], self.V_in))
        D = d.shape[0]
        if out is None:
            out = np.zeros((D, self.V_out), dtype=d.dtype)
        assert out.shape == (D, self.V_out) and out.flags.c_contiguous and out.dtype == d.dtype
        eo = np.zeros(self.V_out) if self.masked else None
        check(lib().msm_resample_plan_apply(self.h, d.ctypes.data, PLAN_DTYPES[d.dtype], D, out.ctypes.data, eo.ctypes.data_as(c_dp) if self.masked else None))
        return (out, eo) if self.masked else out

    def apply_dev(self, data, out=None, D=None, dtype=None):
        """The same on DEVICE memory.  data / out: torch tensors on the context's GPU (D x V_in / D x V_out, contiguous, float32 or float64; out is made when
        None), or integer device addresses with D and dtype given.  The caller orders its pending work with Context.wait_stream; complete on return."""
        if hasattr(data, "data_ptr"):
            import torch

            names = {torch.float64: np.float64, torch.float32: np.float32}
            if data.dtype not in names:
                raise TypeError("ResamplePlan.apply_dev takes float32 or float64 tensors, not %s" % data.dtype)
            t = data.reshape(-1, self.V_in)
            assert t.is_contiguous() and t.is_cuda
            D, dtype = t.shape[0], names[t.dtype]
            if out is None:
                out = torch.empty((D, self.V_out), dtype=t.dtype, device=t.device)
            assert out.is_contiguous() and out.dtype == t.dtype and tuple(out.shape) == (D, self.V_out)
            src, dst = t.data_ptr(), out.data_ptr()
        else:
            if D is None or dtype is None or out is None:
                raise ValueError("device addresses need out, D and dtype")
            src, dst = int(data), int(out.data_ptr() if hasattr(out, "data_ptr") else out)
        if np.dtype(dtype) not in PLAN_DTYPES:
            raise TypeError("ResamplePlan.apply_dev takes float32 or float64 data, not %s" % np.dtype(dtype))
        check(lib().msm_resample_plan_apply_dev(self.h, src or None, PLAN_DTYPES[np.dtype(dtype)], int(D), dst or None))
        return out

    def apply_labels(self, labels, unassigned=0):
        """D x V_in integer keys -> D x V_out int32 by the largest-summed-weight vote (msmhip.h); rows without kept entries get `unassigned`"""
        if self.method == "smoothing":
            raise ValueError("a smoothing plan takes no labels")
        l = np.asarray(labels)
        if not np.issubdtype(l.dtype, np.integer):
            raise TypeError("ResamplePlan.apply_labels takes integer keys, not %s" % l.dtype)
        l, pl = _i(np.atleast_2d(l))
        if l.shape[1] != self.V_in:
            raise ValueError("labels have %d columns, the plan's source %d vertices" % (l.shape[1], self.V_in))
        out = np.zeros((l.shape[0], self.V_out), dtype=np.int32)
        check(lib().msm_resample_plan_apply_labels(self.h, pl, l.shape[0], int(unassigned), out.ctypes.data_as(c_ip)))
        return out


def create_exclusion(data, thrl, thru):
    """create_exclusion (R/mesh.cpp:1257-1273) of a D x V matrix"""
    d, pd = _d(np.atleast_2d(data))
    out = np.zeros(d.shape[1])
    check(lib().msm_create_exclusion(pd, d.shape[0], d.shape[1], float(thrl), float(thru), out.ctypes.data_as(c_dp)))
    return out


def sphere_project_warp(sphere, from_mesh, to_xyz):
    s, ps = _soa(sphere)
    s = s.copy()
    check(lib().msm_sphere_project_warp(from_mesh.h, _soa(to_xyz)[1], s.ctypes.data_as(c_dp), s.shape[1]))
    return np.ascontiguousarray(s.T)


def sphere_project_warp_mesh(sphere_mesh, from_mesh, to_xyz):
    """msm_mesh_sphere_project_warp: the coordinates `sphere_mesh` holds moved through (from_mesh -> to_xyz), in place on the device"""
    check(lib().msm_mesh_sphere_project_warp(sphere_mesh.h, from_mesh.h, _soa(to_xyz)[1]))


def resample_anatomy_grid(cp_xyz, cp_tri, levels, rad=100.0):
    """Mesh_registration::resample_anatomy (M/mesh_registration.cpp:250-332) without its surface_resample call [host]: the control grid retessellated
    `levels` (= anatgrid - CPgrid) times and rescaled to `rad` -> dict(sphere_xyz, sphere_tri, w_ptr, w_cp, w_val (_ANATbaryweights as CSR),
    face_ptr, face_idx (NEARESTFACES as CSR, the reference's order)): the arguments of DiscreteCostFunction.set_anatomical besides the two anatomies."""
    x, px = _soa(cp_xyz)
    t, pt = _tri_soa(cp_tri)
    N, Tc = x.shape[1], t.shape[1]
    va, ta = C.c_int32(), C.c_int32()
    check(lib().msm_resample_anatomy_grid(px, N, pt, Tc, int(levels), float(rad), C.byref(va), C.byref(ta), None, None, None, None, None, None, None))
    Va, Ta = va.value, ta.value
    axyz, atri = np.zeros((3, Va)), np.zeros((3, Ta), dtype=np.int32)
    w_ptr, w_cp, w_val = np.zeros(Va + 1, dtype=np.int32), np.zeros(3 * Va, dtype=np.int32), np.zeros(3 * Va)
    face_ptr, face_idx = np.zeros(Tc + 1, dtype=np.int32), np.zeros(Ta, dtype=np.int32)
    check(lib().msm_resample_anatomy_grid(px, N, pt, Tc, int(levels), float(rad), C.byref(va), C.byref(ta), axyz.ctypes.data_as(c_dp), atri.ctypes.data_as(c_ip),
                                          w_ptr.ctypes.data_as(c_ip), w_cp.ctypes.data_as(c_ip), w_val.ctypes.data_as(c_dp), face_ptr.ctypes.data_as(c_ip),
                                          face_idx.ctypes.data_as(c_ip)))
    n = int(w_ptr[-1])
    return dict(sphere_xyz=np.ascontiguousarray(axyz.T), sphere_tri=np.ascontiguousarray(atri.T), w_ptr=w_ptr, w_cp=w_cp[:n].copy(), w_val=w_val[:n].copy(),
                face_ptr=face_ptr, face_idx=face_idx)


def barycentric_coords_resample(from_mesh, coords, q):
    x, px = _soa(q)
    out = np.zeros((3, x.shape[1]))
    check(lib().msm_barycentric_coords_resample(from_mesh.h, _soa(coords)[1], px, x.shape[1], out.ctypes.data_as(c_dp)))
    return np.ascontiguousarray(out.T)


def project_anatomical_mesh(sphere_mesh, target_mesh, anat_xyz):
    """project_anatomical_mesh (R/resampler.cpp:260-282): every vertex of sphere_mesh (the registered input sphere) placed on the anatomy by its
    barycentric weights on target_mesh (the reference sphere).  anat_xyz (the reference anatomy) gives the coordinates when it has target_mesh's
    vertex count, target_mesh's own coordinates do otherwise.  Returns (V(sphere), 3); the result's triangles are sphere_mesh's."""
    anat = np.asarray(anat_xyz, dtype=np.float64).reshape(-1, 3)
    coords = anat if len(anat) == target_mesh.V else target_mesh.get_coords()
    return barycentric_coords_resample(target_mesh, coords, sphere_mesh.get_coords())


def calculate_strains(orig_mesh, final_xyz, fit_radius=2.0, with_neighbourhoods=False):
    """calculate_strains(fit_radius, orig, final) (M/reg_tools.cpp:365-549) on the device: orig_mesh is the input anatomy with its own triangles,
    final_xyz (V, 3) its vertices after the registration.  Returns the 4 x V rows (maximum and minimum principal stretch, 0.5 (lambda^2 - 1) of
    each); with with_neighbourhoods also the member count and the final fit radius of every vertex."""
    x, px = _soa(final_xyz)
    V = x.shape[1]
    strains = np.zeros((4, V))
    kept = np.zeros(V, dtype=np.int32)
    radius = np.zeros(V)
    check(lib().msm_calculate_strains(orig_mesh.h, px, V, float(fit_radius), strains.ctypes.data_as(c_dp), kept.ctypes.data_as(c_ip),
                                      radius.ctypes.data_as(c_dp)))
    return (strains, kept, radius) if with_neighbourhoods else strains


def smooth_data(orig_mesh, data, sph_low, sigma, excl=None):
    """newresampler::smooth_data (R/resampler.cpp:168-230); returns the smoothed D x V rows (and the smoothed mask)."""
    d, pd = _d(np.atleast_2d(data))
    assert d.shape[1] == orig_mesh.V
    out = np.zeros((d.shape[0], sph_low.V))
    if excl is None:
        check(lib().msm_smooth_data(orig_mesh.h, pd, d.shape[0], sph_low.h, float(sigma), None, out.ctypes.data_as(c_dp), None))
        return out
    e, pe = _d(excl)
    eo = np.zeros(sph_low.V)
    check(lib().msm_smooth_data(orig_mesh.h, pd, d.shape[0], sph_low.h, float(sigma), pe, out.ctypes.data_as(c_dp), eo.ctypes.data_as(c_dp)))
    return out, eo


def variance_normalise(data, excl=None):
    """variance_normalise (M/reg_tools.cpp:804-843) of a D x V matrix; returns the normalised copy."""
    out = np.array(np.atleast_2d(data), dtype=np.float64, order="C")
    pe = _d(excl)[1] if excl is not None else None
    check(lib().msm_variance_normalise(out.ctypes.data_as(c_dp), out.shape[0], out.shape[1], pe))
    return out


def histogram_match(ctx, src, ref, src_excl=None, ref_excl=None):
    """multivariate_histogram_normalization (M/reg_tools.cpp:745-802; --IN / --INc) on the GPU: src (D x Vs, or n x D x Vs for n source matrices
    against the one target) matched row by row to ref (D x Vt) through 256-bin histograms, by the definition of DESIGN.md section 5.11.  src_excl
    (rows x Vs or Vs; n x rows x Vs for n sources) / ref_excl (rows x Vt or Vt): the EXCL masks, a value counts when it is finite and its mask
    is > 0; row d of a mask serves feature row d when the mask has that many rows, row 0 otherwise.  Returns the matched copy, shaped like src."""
    s, ps = _d(src)
    shape = s.shape
    s3 = s.reshape((1,) * (3 - s.ndim) + s.shape) if s.ndim < 3 else s
    assert s3.ndim == 3
    n, D, Vs = s3.shape
    r, pr = _d(np.atleast_2d(ref))
    assert r.ndim == 2 and r.shape[0] == D, "the target has %s rows, the sources %d" % (r.shape[:1], D)
    pse, se_rows, pre, re_rows = None, 0, None, 0
    if src_excl is not None:
        se, pse = _d(src_excl)
        se = se.reshape(n, -1, Vs)
        se_rows = se.shape[1]
    if ref_excl is not None:
        re_, pre = _d(np.atleast_2d(ref_excl))
        assert re_.shape[1] == r.shape[1]
        re_rows = re_.shape[0]
    out = np.empty(s3.shape)
    check(lib().msm_histogram_match(ctx.h, n, D, Vs, ps, pse, se_rows, r.shape[1], pr, pre, re_rows, out.ctypes.data_as(c_dp)))
    return out.reshape(shape)


def level_features(grid, meshes, datas, sigmas, exclude=False, intensity=False, varnorm=False, cutthr=(0.0, 0.0001)):
    """msm_level_features: featurespace::initialise (M/featurespace.cpp:39-86) for n data sets on the level grid `grid` in ONE call -- per data set
    create_exclusion (with exclude), metric_resample from its native mesh and smooth_data on the grid (sigmas[i] > 0), then histogram_match of
    data sets 1.. against data set 0 (intensity) and variance_normalise (varnorm): the bytes of those calls one after another.  meshes: n Mesh
    handles of grid's context; datas: n matrices D x V(meshes[i]).  Returns (n x D x V(grid) features, n x V(grid) masks or None without exclude)."""
    n = len(meshes)
    mats = [_d(np.atleast_2d(d))[0] for d in datas]
    assert len(mats) == n and len(sigmas) == n
    D = mats[0].shape[0] if n else 0
    for m, a in zip(meshes, mats):
        assert a.shape == (D, m.V), "a data set has shape %s, its mesh %d vertices and the first data set %d rows" % (a.shape, m.V, D)
    handles = (C.c_void_p * max(n, 1))(*[m.h for m in meshes])
    rows = (c_dp * max(n, 1))(*[a.ctypes.data_as(c_dp) for a in mats])
    sg, psg = _d(np.asarray(sigmas, dtype=np.float64).reshape(-1))
    p = LevelFeaturesParams(int(bool(exclude)), int(bool(intensity)), int(bool(varnorm)), 0, float(cutthr[0]), float(cutthr[1]))
    feat = np.zeros((n, D, grid.V))
    mask = np.zeros((n, grid.V)) if exclude else None
    check(lib().msm_level_features(grid.h, n, handles, rows, D, psg, C.byref(p), feat.ctypes.data_as(c_dp), None if mask is None else mask.ctypes.data_as(c_dp)))
    return feat, mask


def surface_distortion(ctx, orig_xyz, tri, final_xyz):
    """msm_surface_distortion: wb_command -surface-distortion -local-affine-method -log2 by the definition of DESIGN.md section 5.10 for S deformed
    copies of one sphere in one call.  orig_xyz (V, 3), tri (T, 3), final_xyz (V, 3) or (S, V, 3).  Returns (2, V) or (S, 2, V): row 0 the areal
    distortion (mean over a vertex's triangles of log2 J), row 1 the shape distortion (log2 R); 0 for a vertex without a triangle."""
    x, px = _soa(orig_xyz)
    t, pt = _tri_soa(tri)
    f = np.asarray(final_xyz, dtype=np.float64)
    single = f.ndim == 2
    f = f.reshape(-1, x.shape[1], 3) if f.size else f.reshape(0, x.shape[1], 3)
    fs = np.ascontiguousarray(f.transpose(0, 2, 1))  # S x 3 x V
    out = np.zeros((max(len(fs), 1), 2, x.shape[1]))
    check(lib().msm_surface_distortion(ctx.h, px, pt, x.shape[1], t.shape[1], fs.ctypes.data_as(c_dp), len(fs), out.ctypes.data_as(c_dp)))
    return out[0] if single else out


def abs_summary(ctx, x, percentiles=()):
    """msm_abs_summary over |x| of all values of x: (mean, max, values) with values[q] = numpy.percentile(|x|, percentiles[q]) (linear interpolation)."""
    a, pa = _d(np.asarray(x, dtype=np.float64).ravel())
    p, pp = _d(np.asarray(percentiles, dtype=np.float64).ravel())
    mean, mx = C.c_double(0.0), C.c_double(0.0)
    values = np.zeros(max(len(p), 1))
    check(lib().msm_abs_summary(ctx.h, pa, a.size, pp, len(p), C.byref(mean), C.byref(mx), values.ctypes.data_as(c_dp)))
    return mean.value, mx.value, values[:len(p)]


def mcmc_optimise(unary, tcosts, triplets, labeling, mcparam=0.8, iters=100, seed=0):
    """MCMC::optimise (M/mcmc_opt.h:31-134) over the unary (L x N) and triplet (T x L x L x L) tables; returns the new labeling."""
    U, pu = _d(unary)
    L, N = U.shape
    tc, ptc = _d(tcosts)
    tr = np.ascontiguousarray(triplets, dtype=np.int32)
    T = tr.shape[0]
    assert tc.size == T * L ** 3
    lab = np.array(labeling, dtype=np.int32)
    check(lib().msm_mcmc_optimise(pu, ptc, tr.ctypes.data_as(c_ip), N, L, T, float(mcparam), int(iters), int(seed), lab.ctypes.data_as(c_ip)))
    return lab


def mcmc_optimise_gpu(ctx, unary, tcosts, triplets, labeling, mcparam=0.8, iters=100, seed=0):
    """msm_mcmc_optimise_gpu: mcmc_optimise with the sweeps on the GPU (one workgroup walks the triplets level by level, the proposals come from the
    host's own stream); the labeling mcmc_optimise returns for the same arguments, bit for bit."""
    U, pu = _d(unary)
    L, N = U.shape
    tc, ptc = _d(tcosts)
    tr = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    T = tr.shape[0]
    assert tc.size == T * L ** 3
    lab = np.array(labeling, dtype=np.int32)
    check(lib().msm_mcmc_optimise_gpu(ctx.h, pu, ptc, tr.ctypes.data_as(c_ip), N, L, T, float(mcparam), int(iters), int(seed), lab.ctypes.data_as(c_ip)))
    return lab


MplpResult = collections.namedtuple("MplpResult", "labeling sweeps_run energy bound energies bounds messages")


def _mplp_outputs(N, L, T, sweeps, labeling, bound, bounds, messages):
    """the arrays of one MPLP call and the tail of its argument list (labeling .. messages); what is not asked for travels as NULL and comes back None"""
    out = dict(lab=np.array(labeling, dtype=np.int32), run=C.c_int32(-1), energy=C.c_double(np.nan), bound=C.c_double(np.nan) if bound or bounds else None,
               energies=np.full(int(sweeps), np.nan), bounds=np.full(int(sweeps), np.nan) if bounds else None,
               messages=np.zeros((T, 3, L)) if messages else None)
    assert out["lab"].size == N
    null = C.cast(None, c_dp)
    args = [out["lab"].ctypes.data_as(c_ip), C.byref(out["run"]), C.byref(out["energy"]), C.byref(out["bound"]) if out["bound"] is not None else null,
            out["energies"].ctypes.data_as(c_dp), out["bounds"].ctypes.data_as(c_dp) if bounds else null,
            out["messages"].ctypes.data_as(c_dp) if messages else null]
    return out, args


def _mplp_result(out):
    return MplpResult(out["lab"], out["run"].value, out["energy"].value, None if out["bound"] is None else out["bound"].value, out["energies"],
                      out["bounds"], out["messages"])


def _mplp_tables(unary, tcosts, triplets):
    U, pu = _d(unary)
    L, N = U.shape
    tc, ptc = _d(tcosts)
    tr = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    T = tr.shape[0]
    assert tc.size == T * L ** 3
    return (U, tc, tr), (pu, ptc, tr.ctypes.data_as(c_ip), N, L, T)


def _mplp_counts(counts):
    """the pointer of the optional counts argument of the forbid entry points: an int64 array of 4 that the call fills, or NULL"""
    if counts is None:
        return C.cast(None, c_lp)
    assert counts.dtype == np.int64 and counts.size == 4 and counts.flags.c_contiguous and counts.flags.writeable
    return counts.ctypes.data_as(c_lp)


def mplp_classify(unary, tcosts):
    """msm_mplp_classify [host]: int64 array of (non-finite unary entries, NaN, +inf, -inf triplet entries) -- what the forbid route of the MPLP entry
    points decides by (DESIGN.md 5.19 "Forbidden entries")"""
    U, pu = _d(unary)
    tc, ptc = _d(tcosts)
    L, N = U.shape
    T = tc.size // L ** 3
    assert tc.size == T * L ** 3
    counts = np.zeros(4, dtype=np.int64)
    check(lib().msm_mplp_classify(pu, ptc, N, L, T, counts.ctypes.data_as(c_lp)))
    return counts


def mplp_optimise(unary, tcosts, triplets, labeling, sweeps=30, bound=True, bounds=False, messages=False, forbid=False, counts=None):
    """msm_mplp_optimise [host]: max-product linear programming over the unary (L x N) and triplet (T x L x L x L) tables -- an extension, not newMSM's
    (DESIGN.md 5.19).  Returns MplpResult(labeling, sweeps_run, energy, bound, energies, bounds, messages): the labelling is the lowest-energy one among
    the start and the decode after every sweep (never worse than the start), bound is a lower bound on every labelling's energy.  bounds=True costs a
    second pass over the triplet table per sweep, bound=True alone one pass.  forbid (msm_mplp_optimise_forbid): NaN and +inf triplet entries are
    forbidden label combinations instead of a refusal (DESIGN.md 5.19 "Forbidden entries"): energies are then finite or +inf, the bound holds for the
    labellings that use no forbidden entry, and counts (an int64 array of 4, optional) receives mplp_classify's values."""
    keep, head = _mplp_tables(unary, tcosts, triplets)
    out, tail = _mplp_outputs(head[3], head[4], head[5], sweeps, labeling, bound, bounds, messages)
    if forbid:
        check(lib().msm_mplp_optimise_forbid(*head, int(sweeps), *tail, _mplp_counts(counts)))
    else:
        check(lib().msm_mplp_optimise(*head, int(sweeps), *tail))
    return _mplp_result(out)


def mplp_optimise_gpu(ctx, unary, tcosts, triplets, labeling, sweeps=30, bound=True, bounds=False, messages=False, forbid=False, counts=None):
    """msm_mplp_optimise_gpu: mplp_optimise with the sweeps on the GPU (a launch per level of mcmc_schedule, a workgroup per factor); the same
    MplpResult, bit for bit; forbid: msm_mplp_optimise_forbid_gpu, counts filled by the device's classification pass"""
    keep, head = _mplp_tables(unary, tcosts, triplets)
    out, tail = _mplp_outputs(head[3], head[4], head[5], sweeps, labeling, bound, bounds, messages)
    if forbid:
        check(lib().msm_mplp_optimise_forbid_gpu(ctx.h, *head, int(sweeps), *tail, _mplp_counts(counts)))
    else:
        check(lib().msm_mplp_optimise_gpu(ctx.h, *head, int(sweeps), *tail))
    return _mplp_result(out)


def mplp_gpu_stats(ctx):
    """msm_mplp_gpu_stats of the context's last GPU MPLP run: dict(kernel_ms, levels_per_sweep, sweeps_run, widest_level)"""
    s = np.zeros(4)
    check(lib().msm_mplp_gpu_stats(ctx.h, s.ctypes.data_as(c_dp)))
    return dict(kernel_ms=float(s[0]), levels_per_sweep=int(s[1]), sweeps_run=int(s[2]), widest_level=int(s[3]))


MplpRound = collections.namedtuple("MplpRound", "labeling passes_run energy energies")


def _mplp_round_outputs(N, mode, polish, labeling):
    out = dict(lab=np.array(labeling, dtype=np.int32), run=C.c_int32(-1), energy=C.c_double(np.nan),
               energies=np.full((2 if int(mode) == 0 else 1) + max(int(polish), 0), np.nan))
    assert out["lab"].size == N
    return out, [out["lab"].ctypes.data_as(c_ip), C.byref(out["run"]), C.byref(out["energy"]), out["energies"].ctypes.data_as(c_dp)]


def _mplp_messages(messages, T, L):
    """(the array kept alive, its pointer or NULL)"""
    if messages is None:
        return None, C.cast(None, c_dp)
    m, pm = _d(messages)
    assert m.size == T * 3 * L
    return m, pm


def mplp_colouring(triplets, N):
    """msm_mplp_colouring [host]: (colour per node, number of colours) -- nodes ascending, each the smallest colour no lower-index node sharing a
    triplet with it holds (DESIGN.md 5.19 "Rounding")"""
    tr = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    colour, classes = np.zeros(int(N), dtype=np.int32), C.c_int32(0)
    check(lib().msm_mplp_colouring(tr.ctypes.data_as(c_ip), int(N), tr.shape[0], colour.ctypes.data_as(c_ip), C.byref(classes)))
    return colour, classes.value


def mplp_round(unary, tcosts, triplets, labeling, messages=None, mode=0, polish=8, forbid=False, counts=None):
    """msm_mplp_round [host]: rounds MPLP's messages (T x 3 x L; None: all zero) to a labelling -- the conditioned decode over the colour classes and
    `polish` passes of iterated conditional modes (mode 0), or the polish passes of `labeling` alone (mode 1); DESIGN.md 5.19 "Rounding".  Returns
    MplpRound(labeling, passes_run, energy, energies): the lowest-energy candidate, never worse than the labelling handed in.  forbid
    (msm_mplp_round_forbid): NaN / +inf triplet entries are forbidden combinations and the messages may hold +inf; counts as in mplp_optimise."""
    keep, head = _mplp_tables(unary, tcosts, triplets)
    m, pm = _mplp_messages(messages, head[5], head[4])
    out, tail = _mplp_round_outputs(head[3], mode, polish, labeling)
    if forbid:
        check(lib().msm_mplp_round_forbid(*head, pm, int(mode), int(polish), *tail, _mplp_counts(counts)))
    else:
        check(lib().msm_mplp_round(*head, pm, int(mode), int(polish), *tail))
    return MplpRound(out["lab"], out["run"].value, out["energy"].value, out["energies"])


def mplp_round_gpu(ctx, unary, tcosts, triplets, labeling, messages=None, mode=0, polish=8, forbid=False, counts=None):
    """msm_mplp_round_gpu: mplp_round on the GPU (a launch per colour class and pass); the same MplpRound, bit for bit; forbid:
    msm_mplp_round_forbid_gpu"""
    keep, head = _mplp_tables(unary, tcosts, triplets)
    m, pm = _mplp_messages(messages, head[5], head[4])
    out, tail = _mplp_round_outputs(head[3], mode, polish, labeling)
    if forbid:
        check(lib().msm_mplp_round_forbid_gpu(ctx.h, *head, pm, int(mode), int(polish), *tail, _mplp_counts(counts)))
    else:
        check(lib().msm_mplp_round_gpu(ctx.h, *head, pm, int(mode), int(polish), *tail))
    return MplpRound(out["lab"], out["run"].value, out["energy"].value, out["energies"])


def mplp_round_gpu_stats(ctx):
    """msm_mplp_round_gpu_stats of the context's last GPU rounding: dict(decode_ms, polish_ms, classes, passes_run)"""
    s = np.zeros(4)
    check(lib().msm_mplp_round_gpu_stats(ctx.h, s.ctypes.data_as(c_dp)))
    return dict(decode_ms=float(s[0]), polish_ms=float(s[1]), classes=int(s[2]), passes_run=int(s[3]))


def _mplp_pair_tables(unary, paircosts, pairs):
    U, pu = _d(unary)
    L, N = U.shape
    pc, ppc = _d(paircosts)
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    P = pr.shape[0]
    assert pc.size == P * L * L
    return (U, pc, pr), (pu, ppc, pr.ctypes.data_as(c_ip), N, L, P)


def _mplp_pair_outputs(N, L, P, sweeps, labeling, bound, bounds, messages):
    """_mplp_outputs with messages of P x 2 x L"""
    out, args = _mplp_outputs(N, L, 0, sweeps, labeling, bound, bounds, False)
    if messages:
        out["messages"] = np.zeros((P, 2, L))
        args[-1] = out["messages"].ctypes.data_as(c_dp)
    return out, args


def mplp_pairs_colouring(pairs, N):
    """msm_mplp_pairs_colouring [host]: (colour per pair, pair colours, colour per node, node colours) of DESIGN.md 5.20 -- a sweep walks the pair
    colours, a polish pass the node colours"""
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    pcol, ncol, pk, nk = np.zeros(pr.shape[0], dtype=np.int32), np.zeros(int(N), dtype=np.int32), C.c_int32(0), C.c_int32(0)
    check(lib().msm_mplp_pairs_colouring(pr.ctypes.data_as(c_ip), int(N), pr.shape[0], pcol.ctypes.data_as(c_ip), C.byref(pk), ncol.ctypes.data_as(c_ip),
                                         C.byref(nk)))
    return pcol, pk.value, ncol, nk.value


def mplp_pairs_energy(unary, paircosts, pairs, labeling):
    """msm_mplp_pairs_energy [host]: the energy of a labelling over the unary (L x N) and pair (P x L x L, [p, b, a]) tables"""
    keep, head = _mplp_pair_tables(unary, paircosts, pairs)
    lab = np.ascontiguousarray(labeling, dtype=np.int32)
    assert lab.size == head[3]
    e = C.c_double(np.nan)
    check(lib().msm_mplp_pairs_energy(*head, lab.ctypes.data_as(c_ip), C.byref(e)))
    return e.value


def mplp_pairs_optimise(unary, paircosts, pairs, labeling, sweeps=30, bound=True, bounds=False, messages=False):
    """msm_mplp_pairs_optimise [host]: MPLP over the unary table (L x N) and the pair table of a --regoption=1 level (P x L x L as
    computePairwiseCosts returns it: [p, b, a]) -- an extension, DESIGN.md 5.20.  Returns MplpResult as mplp_optimise does, messages P x 2 x L."""
    keep, head = _mplp_pair_tables(unary, paircosts, pairs)
    out, tail = _mplp_pair_outputs(head[3], head[4], head[5], sweeps, labeling, bound, bounds, messages)
    check(lib().msm_mplp_pairs_optimise(*head, int(sweeps), *tail))
    return _mplp_result(out)


def mplp_pairs_optimise_gpu(ctx, unary, paircosts, pairs, labeling, sweeps=30, bound=True, bounds=False, messages=False):
    """msm_mplp_pairs_optimise_gpu: mplp_pairs_optimise with the sweeps on the GPU (a launch per pair colour); the same MplpResult, bit for bit"""
    keep, head = _mplp_pair_tables(unary, paircosts, pairs)
    out, tail = _mplp_pair_outputs(head[3], head[4], head[5], sweeps, labeling, bound, bounds, messages)
    check(lib().msm_mplp_pairs_optimise_gpu(ctx.h, *head, int(sweeps), *tail))
    return _mplp_result(out)


def mplp_pairs_polish(unary, paircosts, pairs, labeling, polish=8):
    """msm_mplp_pairs_polish [host]: `polish` passes of iterated conditional modes over the node colours; MplpRound(labeling,
    passes_run, energy, energies) with 1 + polish energies, never worse than the labelling handed in"""
    keep, head = _mplp_pair_tables(unary, paircosts, pairs)
    out, tail = _mplp_round_outputs(head[3], 1, polish, labeling)
    check(lib().msm_mplp_pairs_polish(*head, int(polish), *tail))
    return MplpRound(out["lab"], out["run"].value, out["energy"].value, out["energies"])


def mplp_pairs_polish_gpu(ctx, unary, paircosts, pairs, labeling, polish=8):
    """msm_mplp_pairs_polish_gpu: mplp_pairs_polish on the GPU (a launch per node colour and pass); the same MplpRound, bit for bit"""
    keep, head = _mplp_pair_tables(unary, paircosts, pairs)
    out, tail = _mplp_round_outputs(head[3], 1, polish, labeling)
    check(lib().msm_mplp_pairs_polish_gpu(ctx.h, *head, int(polish), *tail))
    return MplpRound(out["lab"], out["run"].value, out["energy"].value, out["energies"])


def mplp_pairs_gpu_stats(ctx):
    """msm_mplp_pairs_gpu_stats of the context's last GPU run over pair tables: dict(kernel_ms, classes, sweeps_run, widest_class, polish_ms,
    passes_run)"""
    s = np.zeros(6)
    check(lib().msm_mplp_pairs_gpu_stats(ctx.h, s.ctypes.data_as(c_dp)))
    return dict(kernel_ms=float(s[0]), classes=int(s[1]), sweeps_run=int(s[2]), widest_class=int(s[3]), polish_ms=float(s[4]), passes_run=int(s[5]))


def _chain_args(seeds, N):
    """(seeds array or None, its pointer or NULL, K, labelings K x N, energies K) of a chains call; seeds=None passes a NULL pointer with K = 1"""
    c_u64p = C.POINTER(C.c_uint64)
    if seeds is None:
        sd, ps, K = None, C.cast(None, c_u64p), 1
    else:
        sd = np.ascontiguousarray(np.atleast_1d(seeds), dtype=np.uint64)
        ps, K = sd.ctypes.data_as(c_u64p), len(sd)
    return sd, ps, K, np.zeros((K, N), dtype=np.int32), np.zeros(K)


def mcmc_optimise_chains(unary, tcosts, triplets, labeling, seeds, mcparam=0.8, iters=100):
    """msm_mcmc_optimise_chains: len(seeds) runs of mcmc_optimise from the one start; returns (the best chain's labeling, labelings K x N, energies K, best)"""
    U, pu = _d(unary)
    L, N = U.shape
    tc, ptc = _d(tcosts)
    tr = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    T = tr.shape[0]
    assert tc.size == T * L ** 3
    lab = np.array(labeling, dtype=np.int32)
    sd, ps, K, labs, E = _chain_args(seeds, N)
    best = C.c_int32(-1)
    check(lib().msm_mcmc_optimise_chains(pu, ptc, tr.ctypes.data_as(c_ip), N, L, T, float(mcparam), int(iters), ps, K, lab.ctypes.data_as(c_ip),
                                         labs.ctypes.data_as(c_ip), E.ctypes.data_as(c_dp), C.byref(best)))
    return lab, labs, E, best.value


def mcmc_optimise_chains_gpu(ctx, unary, tcosts, triplets, labeling, seeds, mcparam=0.8, iters=100):
    """msm_mcmc_optimise_chains_gpu: mcmc_optimise_chains with every chain's sweeps on the GPU, a workgroup per chain in one launch per chunk; the
    same labelings, energies and best, bit for bit"""
    U, pu = _d(unary)
    L, N = U.shape
    tc, ptc = _d(tcosts)
    tr = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    T = tr.shape[0]
    assert tc.size == T * L ** 3
    lab = np.array(labeling, dtype=np.int32)
    sd, ps, K, labs, E = _chain_args(seeds, N)
    best = C.c_int32(-1)
    check(lib().msm_mcmc_optimise_chains_gpu(ctx.h, pu, ptc, tr.ctypes.data_as(c_ip), N, L, T, float(mcparam), int(iters), ps, K, lab.ctypes.data_as(c_ip),
                                             labs.ctypes.data_as(c_ip), E.ctypes.data_as(c_dp), C.byref(best)))
    return lab, labs, E, best.value


def mcmc_energy(unary, tcosts, triplets, labeling):
    """msm_mcmc_energy: the table form of evaluateTotalCostSum -- the unary terms, 0.0 and the triplet terms, each sum serial and ascending from 0.0"""
    U, pu = _d(unary)
    L, N = U.shape
    tc, ptc = _d(tcosts)
    tr = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    T = tr.shape[0]
    assert tc.size == T * L ** 3
    lab = np.ascontiguousarray(labeling, dtype=np.int32)
    assert lab.shape == (N,)
    e = C.c_double()
    check(lib().msm_mcmc_energy(pu, ptc, tr.ctypes.data_as(c_ip), N, L, T, lab.ctypes.data_as(c_ip), C.byref(e)))
    return e.value


def mcmc_best(energies):
    """msm_mcmc_best: std::min_element's index over the chains' energies (ties to the lower index; a NaN never wins but stays in slot 0)"""
    E, pe = _d(np.atleast_1d(energies))
    best = C.c_int32(-1)
    check(lib().msm_mcmc_best(pe, E.size, C.byref(best)))
    return best.value


def mcmc_chains_info(ctx):
    """msm_mcmc_chains_info: (chains, host draw threads) of the context's last GPU sweeps"""
    K, threads = C.c_int32(), C.c_int32()
    check(lib().msm_mcmc_chains_info(ctx.h, C.byref(K), C.byref(threads)))
    return K.value, threads.value


def chain_seeds(seed, it, chains):
    """the level loops' seeds of iteration `it`: chain k takes seed + it + 1000003 k (chain 0 is the single-chain run's seed; distinct in their low 32 bits,
    which is what the engine keeps, for k < 256)"""
    return [(int(seed) + int(it) + 1000003 * k) & 0xFFFFFFFFFFFFFFFF for k in range(int(chains))]


def mcmc_gpu_stats(ctx):
    """msm_mcmc_gpu_stats of the context's last GPU sweeps: dict(kernel_ms, levels, draw_ms, chunks, levels_per_sweep, widest_level)"""
    s = np.zeros(6)
    check(lib().msm_mcmc_gpu_stats(ctx.h, s.ctypes.data_as(c_dp)))
    return dict(kernel_ms=s[0], levels=int(s[1]), draw_ms=s[2], chunks=int(s[3]), levels_per_sweep=int(s[4]), widest_level=int(s[5]))


def mcmc_proposals(L, mcparam, seed, T, sweeps, chunk_sweeps=0):
    """msm_mcmc_proposals: the labels MCMC::optimise proposes, (sweeps, T) uint16 in visit order, drawn in chunks of chunk_sweeps sweeps"""
    out = np.zeros((int(sweeps), int(T)), dtype=np.uint16)
    check(lib().msm_mcmc_proposals(int(L), float(mcparam), int(seed), int(T), int(sweeps), int(chunk_sweeps), out.ctypes.data_as(C.POINTER(C.c_uint16))))
    return out


def mcmc_draw_thresholds(L, mcparam):
    """msm_mcmc_draw_thresholds: thr[k - 1], k = 1 .. L (uint64 bit patterns): the smallest double x in [2^-53, 1] with floor(log(x) / log(1 - mcparam)) <= k - 1"""
    thr = np.zeros(int(L), dtype=np.uint64)
    check(lib().msm_mcmc_draw_thresholds(int(L), float(mcparam), thr.ctypes.data_as(C.POINTER(C.c_uint64))))
    return thr


def mcmc_draw_block_bound(need, L, mcparam):
    """msm_mcmc_draw_block_bound: the 312-candidate blocks the draw kernel may generate for `need` accepted proposals of one chain"""
    n = C.c_int64()
    check(lib().msm_mcmc_draw_block_bound(int(need), int(L), float(mcparam), C.byref(n)))
    return n.value


def mcmc_proposals_mirror(L, mcparam, seed, T, sweeps, counted=False):
    """msm_mcmc_proposals_mirror: mcmc_proposals' stream from the hand-written pieces of the draw kernel, (sweeps, T) uint16 in visit order; counted: also
    the candidates the stream consumed (msm_mcmc_proposals_mirror_counted)"""
    out = np.zeros((int(sweeps), int(T)), dtype=np.uint16)
    po = out.ctypes.data_as(C.POINTER(C.c_uint16))
    if not counted:
        check(lib().msm_mcmc_proposals_mirror(int(L), float(mcparam), int(seed), int(T), int(sweeps), po))
        return out
    n = C.c_uint64()
    check(lib().msm_mcmc_proposals_mirror_counted(int(L), float(mcparam), int(seed), int(T), int(sweeps), po, C.byref(n)))
    return out, n.value


def mcmc_draw_gpu(ctx, L, mcparam, seeds, T, sweeps, chunk_sweeps=0, pos=None):
    """msm_mcmc_draw_gpu: the proposal streams of len(seeds) chains drawn by the draw kernel alone, (K, sweeps, T) uint16; the label of triplet t of a sweep
    stands at pos[t] (None: t), as the sweeps kernels read it"""
    sd = np.ascontiguousarray(np.atleast_1d(seeds), dtype=np.uint64)
    K = len(sd)
    out = np.zeros((K, int(sweeps), int(T)), dtype=np.uint16)
    if pos is None:
        pp = C.cast(None, c_ip)
    else:
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        assert pos.shape == (int(T),)
        pp = pos.ctypes.data_as(c_ip)
    check(lib().msm_mcmc_draw_gpu(ctx.h, int(L), float(mcparam), sd.ctypes.data_as(C.POINTER(C.c_uint64)), K, int(T), int(sweeps), int(chunk_sweeps), pp,
                                  out.ctypes.data_as(C.POINTER(C.c_uint16))))
    return out


def mcmc_draw_stats(ctx):
    """msm_mcmc_draw_stats of the context's last device draw: dict(draw_ms, candidates, accepted, block_bound)"""
    s = np.zeros(4)
    check(lib().msm_mcmc_draw_stats(ctx.h, s.ctypes.data_as(c_dp)))
    return dict(draw_ms=s[0], candidates=int(s[1]), accepted=int(s[2]), block_bound=int(s[3]))


def group_mcmc_incidence(pairs, nodes):
    """msm_group_mcmc_incidence: the incidence of a pair list (P x 2) over `nodes` nodes as CSR (ptr nodes + 1, idx): for node n the pair indices p with
    pairs[p][0] == n or pairs[p][1] == n, ascending"""
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    P = pr.shape[0]
    ptr = np.zeros(int(nodes) + 1, dtype=np.int32)
    idx = np.zeros(max(2 * P, 1), dtype=np.int32)
    check(lib().msm_group_mcmc_incidence(pr.ctypes.data_as(c_ip), P, int(nodes), ptr.ctypes.data_as(c_ip), idx.ctypes.data_as(c_ip)))
    return ptr, idx[: ptr[-1]].copy()


def group_mcmc_seeds(seed, it, K, S, subject, pass_=0):
    """msm_group_mcmc_seeds: chain k of `subject` in pass pass_ of iteration it: seed + it + 1000003 k + 15485863 (pass_ S + subject), uint64 (K,)"""
    out = np.zeros(int(K), dtype=np.uint64)
    check(lib().msm_group_mcmc_seeds(int(seed) & 0xFFFFFFFFFFFFFFFF, int(it), int(pass_), int(S), int(subject), int(K), out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out


def group_mcmc_accept(start, best):
    """msm_group_mcmc_accept: whether a block's best chain replaces the subject's labels -- its energy strictly below the start's, never with a NaN"""
    a = C.c_int32(-1)
    check(lib().msm_group_mcmc_accept(float(start), float(best), C.byref(a)))
    return bool(a.value)


def mcmc_schedule(triplets, N):
    """msm_mcmc_schedule: (level per triplet, the triplets by level, level offsets) of the GPU sweeps' level schedule"""
    tr = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    T = tr.shape[0]
    level, order, off = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32), np.zeros(T + 1, dtype=np.int32)
    n = C.c_int32()
    check(lib().msm_mcmc_schedule(tr.ctypes.data_as(c_ip), int(N), T, level.ctypes.data_as(c_ip), order.ctypes.data_as(c_ip), off.ctypes.data_as(c_ip), C.byref(n)))
    return level, order, off[: n.value + 1]


def fusion_icm_step(unary2, octets, triplets, passes=5, quads=None, pairs=None):
    """msm_fusion_icm_step: the stand-in binary solve of one label step (iterated conditional modes; NOT ELC + FastPD).  unary2 N x 2
    (current, proposed) or an int N (no unary costs), octets T x 8 / quads P x 4 as tripletOctets / fusionMove return them; returns x (N):
    1 where the proposed label is taken."""
    if np.ndim(unary2) == 0:
        N, u, pu = int(unary2), None, None
    else:
        u = np.ascontiguousarray(unary2, dtype=np.float64)
        N, pu = u.shape[0], u.ctypes.data_as(c_dp)
        assert u.shape == (N, 2)
    tr = np.ascontiguousarray(triplets if triplets is not None else np.zeros((0, 3)), dtype=np.int32)
    e = np.ascontiguousarray(octets if octets is not None else np.zeros((0, 8)), dtype=np.float64)
    pr = np.ascontiguousarray(pairs if pairs is not None else np.zeros((0, 2)), dtype=np.int32)
    q = np.ascontiguousarray(quads if quads is not None else np.zeros((0, 4)), dtype=np.float64)
    T, P = tr.shape[0], pr.shape[0]
    assert e.size == 8 * T and q.size == 4 * P
    x = np.zeros(N, dtype=np.int32)
    check(lib().msm_fusion_icm_step(pu, q.ctypes.data_as(c_dp), pr.ctypes.data_as(c_ip), P, e.ctypes.data_as(c_dp), tr.ctypes.data_as(c_ip), T, N, int(passes),
                                    x.ctypes.data_as(c_ip)))
    return x


FusionMplp = collections.namedtuple("FusionMplp", "x sweeps_run passes_run energy bound energies bounds")


def _fusion_mplp_outputs(N, sweeps, polish):
    """the output arrays of the msm_fusion_mplp_step family and their pointers; energies: 1 + sweeps values, then 1 + polish where polish > 0"""
    S, P = max(int(sweeps), 0), max(int(polish), 0)
    out = dict(x=np.zeros(int(N), dtype=np.int32), run=C.c_int32(-1), passes=C.c_int32(-1), energy=C.c_double(np.nan), bound=C.c_double(np.nan),
               energies=np.full(1 + S + (1 + P if P > 0 else 0), np.nan), bounds=np.full(S, np.nan))
    return out, [out["x"].ctypes.data_as(c_ip), C.byref(out["run"]), C.byref(out["passes"]), C.byref(out["energy"]), C.byref(out["bound"]),
                 out["energies"].ctypes.data_as(c_dp), out["bounds"].ctypes.data_as(c_dp)]


def _fusion_mplp_result(out):
    return FusionMplp(out["x"], out["run"].value, out["passes"].value, out["energy"].value, out["bound"].value, out["energies"], out["bounds"])


def _fusion_mplp_tables(unary2, octets, triplets):
    if unary2 is None or np.ndim(unary2) == 0:
        assert unary2 is None or int(unary2) > 0
        u, pu, N = None, C.cast(None, c_dp), (None if unary2 is None else int(unary2))
    else:
        u = np.ascontiguousarray(unary2, dtype=np.float64)
        N, pu = u.shape[0], u.ctypes.data_as(c_dp)
        assert u.shape == (N, 2)
    tr = np.ascontiguousarray(triplets if triplets is not None else np.zeros((0, 3)), dtype=np.int32).reshape(-1, 3)
    e = np.ascontiguousarray(octets if octets is not None else np.zeros((0, 8)), dtype=np.float64)
    T = tr.shape[0]
    assert e.size == 8 * T
    return (u, e, tr), (pu, e.ctypes.data_as(c_dp), tr.ctypes.data_as(c_ip), T), N


def fusion_mplp_step(unary2, octets, triplets, sweeps=10, polish=8, N=None):
    """msm_fusion_mplp_step [host]: MPLP over the binary problem of one label step (an extension) -- api.mplp_optimise from x = 0 and,
    polish > 0, api.mplp_round(mode 0) at L = 2 over the transposed unary2 (N x 2: current, proposed; None with N given: no unary costs) and the octets
    (T x 8).  Returns FusionMplp(x, sweeps_run, passes_run, energy, bound, energies, bounds): x is 1 where the proposed label is taken and never worse
    than x = 0 (energies[0]); bound is a lower bound on the step's optimum."""
    keep, head, n = _fusion_mplp_tables(unary2, octets, triplets)
    N = n if n is not None else int(N)
    out, tail = _fusion_mplp_outputs(N, sweeps, polish)
    check(lib().msm_fusion_mplp_step(*head, N, int(sweeps), int(polish), *tail))
    return _fusion_mplp_result(out)


def fusion_mplp_step_gpu(ctx, unary2, octets, triplets, sweeps=10, polish=8, N=None):
    """msm_fusion_mplp_step_gpu: fusion_mplp_step in one launch of one workgroup on the GPU; the same FusionMplp, bit for bit"""
    keep, head, n = _fusion_mplp_tables(unary2, octets, triplets)
    N = n if n is not None else int(N)
    out, tail = _fusion_mplp_outputs(N, sweeps, polish)
    check(lib().msm_fusion_mplp_step_gpu(ctx.h, *head, N, int(sweeps), int(polish), *tail))
    return _fusion_mplp_result(out)


def fusion_mplp_gpu_stats(ctx):
    """msm_fusion_mplp_gpu_stats of the context's last GPU label-step solve: dict(kernel_ms, levels_per_sweep, sweeps_run, launches)"""
    s = np.zeros(4)
    check(lib().msm_fusion_mplp_gpu_stats(ctx.h, s.ctypes.data_as(c_dp)))
    return dict(kernel_ms=float(s[0]), levels_per_sweep=int(s[1]), sweeps_run=int(s[2]), launches=int(s[3]))


def pairwise_icm(unary, paircosts, pairs, labeling=None, passes=100):
    """msm_pairwise_icm: the stand-in solve of the multi-label pairwise MRF of --regoption=1 (iterated conditional modes; NOT FastPD).
    unary L x N, paircosts P x L x L flat as computePairwiseCosts returns it, pairs P x 2; returns the labeling (N)."""
    u = np.ascontiguousarray(unary, dtype=np.float64)
    L, N = u.shape
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    pc = np.ascontiguousarray(paircosts, dtype=np.float64)
    assert pc.size == pr.shape[0] * L * L
    lab = np.zeros(N, dtype=np.int32) if labeling is None else np.array(labeling, dtype=np.int32)
    check(lib().msm_pairwise_icm(u.ctypes.data_as(c_dp), pc.ctypes.data_as(c_dp), pr.ctypes.data_as(c_ip), N, L, pr.shape[0], int(passes), lab.ctypes.data_as(c_ip)))
    return lab


def nearest_neighbour_interpolation(orig_mesh, data, q, excl=None):
    d, pd = _d(np.atleast_2d(data))
    x, px = _soa(q)
    out = np.zeros((d.shape[0], x.shape[1]))
    if excl is None:
        check(lib().msm_nearest_neighbour(orig_mesh.h, pd, d.shape[0], px, x.shape[1], None, out.ctypes.data_as(c_dp), None))
        return out
    eo = np.zeros(x.shape[1])
    check(lib().msm_nearest_neighbour(orig_mesh.h, pd, d.shape[0], px, x.shape[1], _d(excl)[1], out.ctypes.data_as(c_dp), eo.ctypes.data_as(c_dp)))
    return out, eo


# ------------------------------------------------------------------ cost function
class DiscreteCostFunction:
    """NonLinearSRegDiscreteCostFunction family behind the DiscreteCostFunction evaluator interface."""

    def __init__(self, ctx, kind="univariate", simmeasure=2, rmode=3, lambda_=0.1, mu=0.1, kappa=10.0, k_exp=2.0, rexp=2.0, range_=1.0,
                 percentile=0.75):
        self.ctx = ctx
        self.params = CostParams(KINDS[kind], simmeasure, rmode, 0, lambda_, mu, kappa, k_exp, rexp, range_, percentile)
        self.h = lib().msm_cost_create(ctx.h, C.byref(self.params))
        if not self.h:
            raise MsmError(-1, lib().msm_last_error().decode())
        self._keep = {}

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            lib().msm_cost_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def set_meshes(self, target, source, cpgrid):
        self._keep.update(target=target, source=source, cpgrid=cpgrid)
        self.N = cpgrid.V
        check(lib().msm_cost_set_meshes(self.h, target.h, source.h, cpgrid.h))

    def set_anatomical(self, sphere, atarget_xyz, asource_xyz, asource_tri, w_ptr, w_cp, w_val, face_ptr, face_idx):
        """set_anatomical + set_anatomical_neighbourhood (M/DiscreteCostFunction.h:160-170): sphere = _TARGEThi (a Mesh),
        atarget_xyz = _aTARGET coordinates on the sphere's vertices, asource_* = _aSOURCE, w_* = _ANATbaryweights (CSR over
        _aSOURCE vertices, control point ids ascending), face_* = NEARESTFACES (CSR over triplets)."""
        at, pat = _soa(atarget_xyz)
        asx, pas = _soa(asource_xyz)
        tri, ptri = _tri_soa(asource_tri)
        wp, pwp = _i(w_ptr)
        wc, pwc = _i(w_cp)
        wv, pwv = _d(w_val)
        fp, pfp = _i(face_ptr)
        fi, pfi = _i(face_idx)
        assert at.shape[1] == sphere.V
        self._keep.update(asphere=sphere)
        check(lib().msm_cost_set_anatomical(self.h, sphere.h, pat, pas, asx.shape[1], ptri, tri.shape[1], pwp, pwc, pwv, pfp, pfi))

    def reset_source(self, source):
        self._keep["source"] = source
        check(lib().msm_cost_reset_source(self.h, source.h))

    def reset_CPgrid(self, cpgrid):
        self._keep["cpgrid"] = cpgrid
        check(lib().msm_cost_reset_cpgrid(self.h, cpgrid.h))

    def set_featurespace(self, src_feat, ref_feat=None):
        f, pf = _d(np.atleast_2d(src_feat))
        if ref_feat is not None:
            self._keep["target"].set_pvalues(ref_feat)
        check(lib().msm_cost_set_source_features(self.h, pf, f.shape[0]))

    def set_dataaffintyweighting(self, w):
        if w is None:
            check(lib().msm_cost_set_cfweight(self.h, None, 0))
        else:
            w, pw = _d(np.atleast_2d(w))
            check(lib().msm_cost_set_cfweight(self.h, pw, w.shape[0]))

    def set_spacings(self, maxsep, mvdmax):
        check(lib().msm_cost_set_spacings(self.h, _d(maxsep)[1], float(mvdmax)))

    def set_labels(self, labels, rot):
        l, pl = _soa(labels)
        self.L = l.shape[1]
        check(lib().msm_cost_set_labels(self.h, pl, self.L, _d(rot)[1]))

    def setTriplets(self, triplets):
        t, pt = _i(triplets)
        self.T = len(t)
        check(lib().msm_cost_set_triplets(self.h, pt, self.T))

    def setPairs(self, pairs):
        p, pp = _i(pairs)
        self.P = len(p)
        check(lib().msm_cost_set_pairs(self.h, pp, self.P))

    def get_source_data(self):
        check(lib().msm_cost_get_source_data(self.h))

    def patches(self):
        ng = C.c_int32()
        check(lib().msm_cost_patches(self.h, C.byref(ng), None, None, 0))
        ptr = np.zeros(ng.value + 1, dtype=np.int32)
        check(lib().msm_cost_patches(self.h, C.byref(ng), ptr.ctypes.data_as(c_ip), None, 0))
        idx = np.zeros(max(int(ptr[-1]), 1), dtype=np.int32)
        check(lib().msm_cost_patches(self.h, C.byref(ng), ptr.ctypes.data_as(c_ip), idx.ctypes.data_as(c_ip), len(idx)))
        return ptr, idx[: int(ptr[-1])]

    def absolute_weights(self):
        out = np.zeros(self.N)
        check(lib().msm_cost_absolute_weights(self.h, out.ctypes.data_as(c_dp)))
        return out

    # computeUnaryCosts() + getUnaryCosts(): table[label, node]
    def computeUnaryCosts(self, out=None):
        """computeUnaryCosts() + getUnaryCosts().  `out` (optional, L x N): the array to fill, e.g. Context.host_array((L, N)):
        pinned memory the copy engine writes directly."""
        U = np.zeros((self.L, self.N)) if out is None else out
        assert U.shape == (self.L, self.N) and U.dtype == np.float64 and U.flags.c_contiguous
        check(lib().msm_cost_unary_table(self.h, U.ctypes.data_as(c_dp)))
        return U

    def computeUnaryCosts_async(self):
        check(lib().msm_cost_unary_table_async(self.h))

    def getUnaryCosts(self):
        U = np.zeros((self.L, self.N))
        check(lib().msm_cost_unary_table_fetch(self.h, U.ctypes.data_as(c_dp)))
        return U

    def computeUnaryCost(self, nodes, labels):
        n, pn = _i(np.atleast_1d(nodes))
        l, pl = _i(np.atleast_1d(labels))
        out = np.zeros(len(n))
        check(lib().msm_cost_unary_batch(self.h, pn, pl, len(n), out.ctypes.data_as(c_dp)))
        return out

    def computeTripletCost(self, triplet, la, lb, lc):
        t, pt = _i(np.atleast_1d(triplet))
        a, pa = _i(np.atleast_1d(la))
        b, pb = _i(np.atleast_1d(lb))
        c_, pc = _i(np.atleast_1d(lc))
        out = np.zeros(len(t))
        check(lib().msm_cost_triplet_batch(self.h, pt, pa, pb, pc, len(t), out.ctypes.data_as(c_dp)))
        return out

    def tripletOctets(self, labeling, label, out=None):
        """One label step of Fusion (Fusion.h:181-196).  `out` (optional, T x 8): the array to fill, e.g. Context.host_array((T, 8))
        -- mapped pinned memory the kernels write directly, as the optimiser's per-step buffer would be."""
        lab = labeling if (type(labeling) is np.ndarray and labeling.dtype == np.int32 and labeling.flags.c_contiguous) else np.ascontiguousarray(labeling, dtype=np.int32)
        assert lab.shape == (self.N,)
        if out is None:
            out = np.zeros((self.T, 8))
        assert out.shape == (self.T, 8) and out.dtype == np.float64 and out.flags.c_contiguous
        st = lib().msm_cost_triplet_octets(self.h, lab.ctypes.data, int(label), out.ctypes.data)
        if st:
            check(st)
        return out

    def prefetchTripletOctets(self, labeling, label, out):
        """msm_cost_triplet_octets_prefetch: queue the label step (labeling, label) into `out` (a Context.host_array, T x 8) without waiting -- a hint;
        the next tripletOctets with the same labeling, label and out only waits for it, any other call on this cost function drops it"""
        lab = labeling if (type(labeling) is np.ndarray and labeling.dtype == np.int32 and labeling.flags.c_contiguous) else np.ascontiguousarray(labeling, dtype=np.int32)
        st = lib().msm_cost_triplet_octets_prefetch(self.h, lab.ctypes.data, int(label), out.ctypes.data)
        if st:
            check(st)

    def prefetch_stats(self):
        """(label steps taken from a prefetch, prefetches dropped) since creation"""
        a, b = C.c_int64(), C.c_int64()
        check(lib().msm_cost_prefetch_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def computeTripletCosts(self, t0=0, t1=None, pinned=False):
        """tcosts[t][a][b][c] (M/DiscreteCostFunction.cpp:245-253) for the triplets t0 <= t < t1.  Like the reference's
        tcosts member the table lives in the object: the returned array is reused by the next call of the same shape (a fresh
        281 MB array per call costs more in page faults than the table takes to compute and copy).  pinned=True: the table is delivered into
        a pinned buffer of the CONTEXT instead -- valid until the next pinned table of any cost function on this context."""
        t1 = self.T if t1 is None else t1
        shape = (t1 - t0, self.L, self.L, self.L)
        if pinned:  # one grow-only pinned buffer per context: the 281 MB of an ico4 table arrive at PCIe speed (5 ms; 25 ms into pageable memory)
            out = self.ctx.scratch_host_array("tcosts", shape)
        else:
            out = self._keep.get("tcosts")
            if out is None or out.shape != shape:
                out = self._keep["tcosts"] = np.empty(shape)
        check(lib().msm_cost_triplet_table(self.h, int(t0), int(t1), out.ctypes.data_as(c_dp)))
        return out

    def mcmc_optimise(self, labeling, mcparam=0.8, iters=100, seed=0):
        """msm_cost_mcmc_optimise: computeUnaryCosts + computeTripletCosts + MCMC::optimise with both tables staying on the device; the labeling
        computeUnaryCosts() + computeTripletCosts() + api.mcmc_optimise give, bit for bit"""
        lab = np.array(labeling, dtype=np.int32)
        assert lab.shape == (self.N,)
        check(lib().msm_cost_mcmc_optimise(self.h, float(mcparam), int(iters), int(seed), lab.ctypes.data_as(c_ip)))
        return lab

    def mcmc_optimise_chains(self, labeling, seeds, mcparam=0.8, iters=100):
        """msm_cost_mcmc_optimise_chains: mcmc_optimise for len(seeds) chains side by side over the same device tables; returns (the best chain's
        labeling, labelings K x N, energies K, best) -- what the fetched tables and api.mcmc_optimise_chains give, bit for bit"""
        lab = np.array(labeling, dtype=np.int32)
        assert lab.shape == (self.N,)
        sd, ps, K, labs, E = _chain_args(seeds, self.N)
        best = C.c_int32(-1)
        check(lib().msm_cost_mcmc_optimise_chains(self.h, float(mcparam), int(iters), ps, K, lab.ctypes.data_as(c_ip), labs.ctypes.data_as(c_ip),
                                                  E.ctypes.data_as(c_dp), C.byref(best)))
        return lab, labs, E, best.value

    def set_mplp_forbid(self, on=True):
        """msm_cost_set_mplp_forbid: mplp_optimise / mplp_round / mplp_polish read the device triplet table's NaN and +inf entries as forbidden label
        combinations (DESIGN.md 5.19 "Forbidden entries") instead of refusing the table"""
        check(lib().msm_cost_set_mplp_forbid(self.h, int(bool(on))))

    def mplp_forbidden(self):
        """msm_cost_mplp_forbidden: what the last such call counted -- int64 (non-finite unary, NaN, +inf, -inf triplet entries)"""
        counts = np.zeros(4, dtype=np.int64)
        check(lib().msm_cost_mplp_forbidden(self.h, counts.ctypes.data_as(c_lp)))
        return counts

    def mplp_optimise(self, labeling, sweeps=30, bound=True, bounds=False, messages=False):
        """msm_cost_mplp_optimise: computeUnaryCosts + computeTripletCosts + MPLP with both tables staying on the device; the MplpResult that
        computeUnaryCosts() + computeTripletCosts() + api.mplp_optimise give, bit for bit"""
        out, tail = _mplp_outputs(self.N, self.L, self.T, sweeps, labeling, bound, bounds, messages)
        check(lib().msm_cost_mplp_optimise(self.h, int(sweeps), *tail))
        return _mplp_result(out)

    def mplp_round(self, labeling, sweeps=30, polish=8, then_polish=False):
        """msm_cost_mplp_round: MPLP's sweeps and the rounding of mode 0 with tables and messages staying on the device; what mplp_optimise(messages=True)
        followed by api.mplp_round on those messages with that winner give, bit for bit.  then_polish: one mode-1 call on the result follows.  Returns
        (MplpRound, sweeps_run, bound)."""
        out, tail = _mplp_round_outputs(self.N, 0, polish, labeling)
        run, bound = C.c_int32(-1), C.c_double(np.nan)
        check(lib().msm_cost_mplp_round(self.h, int(sweeps), int(polish), int(bool(then_polish)), tail[0], C.byref(run), tail[1], tail[2], C.byref(bound),
                                        tail[3]))
        return MplpRound(out["lab"], out["run"].value, out["energy"].value, out["energies"]), run.value, bound.value

    def fusion_mplp_step(self, labeling, label, sweeps=10, polish=8):
        """msm_cost_fusion_mplp_step: the label step (labeling, label) solved by MPLP with octets and unary costs staying on the device; the FusionMplp
        that unary_table() + triplet_octets(labeling, label) + api.fusion_mplp_step give, bit for bit"""
        lab = np.ascontiguousarray(labeling, dtype=np.int32)
        assert lab.shape == (self.N,)
        out, tail = _fusion_mplp_outputs(self.N, sweeps, polish)
        check(lib().msm_cost_fusion_mplp_step(self.h, lab.ctypes.data_as(c_ip), int(label), int(sweeps), int(polish), *tail))
        return _fusion_mplp_result(out)

    def mplp_polish(self, labeling, polish=8):
        """msm_cost_mplp_polish: api.mplp_round(mode=1) over the cost function's own device tables"""
        out, tail = _mplp_round_outputs(self.N, 1, polish, labeling)
        check(lib().msm_cost_mplp_polish(self.h, int(polish), *tail))
        return MplpRound(out["lab"], out["run"].value, out["energy"].value, out["energies"])

    def mplp_pairs_optimise(self, labeling, sweeps=30, polish=0, bound=True, bounds=False):
        """msm_cost_mplp_pairs_optimise: computeUnaryCosts + computePairwiseCosts + MPLP over the pair tables with both tables
        staying on the device, then `polish` passes of the sweeps' winner; what computeUnaryCosts() + computePairwiseCosts() + api.mplp_pairs_optimise
        (+ api.mplp_pairs_polish) give, bit for bit.  Returns (MplpResult of the sweeps with the final labelling and energy, MplpRound of the polish or
        None).  The forbidden-entry switch (set_mplp_forbid) is ignored: a pair cost is finite or the folding value."""
        out, tail = _mplp_pair_outputs(self.N, self.L, getattr(self, "P", 0), sweeps, labeling, bound, bounds, False)  # (no pairs: the library says so)
        passes, pe = C.c_int32(-1), np.full(1 + max(int(polish), 0), np.nan)
        check(lib().msm_cost_mplp_pairs_optimise(self.h, int(sweeps), int(polish), tail[0], tail[1], C.byref(passes), tail[2], tail[3], tail[4], tail[5],
                                                 pe.ctypes.data_as(c_dp)))
        res = _mplp_result(out)
        return res, (MplpRound(res.labeling, passes.value, res.energy, pe) if int(polish) > 0 else None)

    def computePairwiseCost(self, pair, la, lb):
        p, pp = _i(np.atleast_1d(pair))
        a, pa = _i(np.atleast_1d(la))
        b, pb = _i(np.atleast_1d(lb))
        out = np.zeros(len(p))
        check(lib().msm_cost_pairwise_batch(self.h, pp, pa, pb, len(p), out.ctypes.data_as(c_dp)))
        return out

    def computePairwiseCosts(self):
        out = np.zeros(self.P * self.L * self.L)
        check(lib().msm_cost_pairwise_table(self.h, out.ctypes.data_as(c_dp)))
        return out

    def evaluateTotalCostSum(self, labeling):
        lab, pl = _i(labeling)
        tot = C.c_double()
        parts = np.zeros(3)
        check(lib().msm_cost_total(self.h, pl, C.byref(tot), parts.ctypes.data_as(c_dp)))
        return tot.value, parts

    def enable_timing(self, on=True):
        check(lib().msm_cost_enable_timing(self.h, int(on)))

    def kernel_times(self):
        ms = np.zeros(64)
        n = C.c_int32()
        check(lib().msm_cost_kernel_times(self.h, ms.ctypes.data_as(c_dp), 64, C.byref(n)))
        return ms[: n.value].copy()

    def counters(self):
        c = (C.c_int64 * 4)()
        check(lib().msm_cost_counters(self.h, c))
        return dict(samples=c[0], unary=c[1], triplet=c[2], pairwise=c[3])

    UNARY_ROUTES = ("none", "univariate", "flat", "features", "mv8", "pw8<4>", "pw8<8>")  # MSM_UNARY_* of include/msmhip.h
    UNARY_FORMS = ("staged", "rows")  # MSM_UNARY_FORM_*
    MOVE_ROUTES = ("none", "fused0", "fused1", "fused2", "fused3", "octets_sample", "octets_sample_mv8", "octets_ho", "strain")  # MSM_MOVE_*

    def routes(self):
        """msm_cost_routes: which kernels this cost function ran, as the launchers recorded them.  unary: the reduction kernel of the last unary
        table (UNARY_ROUTES); move: the route of the last triclique label step (MOVE_ROUTES: fusedM = k_ho_move<., M>, octets_* = the three-kernel
        path with that sampling kernel, octets_ho = k_triplet_octets_ho); move_nblk / move_cap / move_maxtri: workgroups of the fused move, bin slots
        and control triangles one of them holds at most; move_tails: moves that needed the tail kernel, since creation; move_deferred: evaluations the last fused
        move handed to the tail kernel (0 when it launched none); unary_form: "rows" where k_unary_reduce_rows stood in for the "flat" reduction of the
        last table (no patch above 96 points), else "staged"."""
        r = (C.c_int32 * 8)()
        check(lib().msm_cost_routes(self.h, r))
        return dict(unary=self.UNARY_ROUTES[r[0]], move=self.MOVE_ROUTES[r[1]], move_nblk=r[2], move_cap=r[3], move_maxtri=r[4], move_tails=r[5], move_deferred=r[6],
                    unary_form=self.UNARY_FORMS[r[7]])

    SAMPLERS = ("none", "samples", "rays")  # MSM_SAMPLER_* of include/msmhip.h
    REFUSALS = ("", "sampler", "reduction")  # MSM_PLAN_REFUSED_*

    @classmethod
    def _plan(cls, p):
        return dict(nsplit=p[0], sampler=cls.SAMPLERS[p[1]], sampler_lds=p[2], reduce=cls.UNARY_ROUTES[p[3]], reduce_lds=p[4], reduce_threads=p[5],
                    refused=cls.REFUSALS[p[6]], pmax=p[7])

    def unary_launch(self):
        """msm_cost_unary_launch: the launch plan of the last unary table as its launchers acted on it (a refused one included): nsplit (workgroups
        per control point), sampler ("rays" / "samples") and sampler_lds (bytes of dynamic LDS), reduce (UNARY_ROUTES) with reduce_lds and
        reduce_threads, refused ("" / "sampler" / "reduction": that kernel's LDS does not fit a workgroup), pmax (the largest patch)."""
        p = (C.c_int32 * 8)()
        check(lib().msm_cost_unary_launch(self.h, p))
        return self._plan(p)

    def unary_fix_counters(self):
        """msm_cost_unary_fix_counters: the redo counter and the 64 fix-up segment counters, read back after the queued work; all zero between tables"""
        n = (C.c_uint32 * 65)()
        check(lib().msm_cost_unary_fix_counters(self.h, n))
        return np.array(n[:], dtype=np.int64)


def unary_launch_plan(kind, simmeasure, D, L, pmax, ray_table):
    """msm_unary_launch_plan: what a unary table of these sizes would do (DiscreteCostFunction.unary_launch's fields); host arithmetic, no GPU."""
    p = (C.c_int32 * 8)()
    check(lib().msm_unary_launch_plan(KINDS[kind] if isinstance(kind, str) else int(kind), simmeasure, D, L, pmax, int(bool(ray_table)), p))
    return DiscreteCostFunction._plan(p)


def unary_launch_order(cp_xyz):
    """msm_unary_launch_order: the order in which the unary kernels take the control points cp_xyz (N x 3)"""
    cp = np.ascontiguousarray(np.asarray(cp_xyz, dtype=np.float64).T)
    order = np.zeros(cp.shape[1], dtype=np.int32)
    check(lib().msm_unary_launch_order(cp.ctypes.data_as(c_dp), cp.shape[1], order.ctypes.data_as(c_ip)))
    return order


def unary_fix_offsets(L, pmax, pptr, order):
    """msm_unary_fix_offsets: the 65 segment offsets of the unary kernels' fix-up list for the patches pptr (N + 1) taken in `order`"""
    pptr = np.ascontiguousarray(pptr, dtype=np.int32)
    order = np.ascontiguousarray(order, dtype=np.int32)
    off = np.zeros(65, dtype=np.uint32)
    check(lib().msm_unary_fix_offsets(len(order), L, pmax, pptr.ctypes.data_as(c_ip), order.ctypes.data_as(c_ip), off.ctypes.data_as(C.POINTER(C.c_uint32))))
    return off


# ------------------------------------------------------------------ groupwise (gMSM)
class DiscreteGroupCostFunction:
    """DiscreteGroupModel::setupCostFunction + DiscreteGroupCostFunction's evaluators
    (/root/reference/libraries/msm-newmeshreg/src/DiscreteGroupModel.cpp:163-196, DiscreteGroupCostFunction.cpp:26-98)."""

    def __init__(self, ctx, num_subjects, simmeasure=2, fixnan=False, lambda_=0.1, mu=0.1, kappa=10.0, k_exp=2.0, rexp=2.0, range_=1.0,
                 percentile=0.75):
        from ._lib import GroupParams

        self.ctx = ctx
        self.S = num_subjects
        self.params = GroupParams(simmeasure, int(fixnan), lambda_, mu, kappa, k_exp, rexp, range_, percentile)
        self.h = lib().msm_group_create(ctx.h, C.byref(self.params), num_subjects)
        if not self.h:
            raise MsmError(-1, lib().msm_last_error().decode())
        self._keep = {}

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            lib().msm_group_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def set_template(self, mesh, mask=None):
        self._keep["template"] = mesh
        check(lib().msm_group_set_template(self.h, mesh.h, _d(mask)[1] if mask is not None else None))

    def Initialize(self, cp_xyz, cp_tri):
        x, px = _soa(cp_xyz)
        t, pt = _tri_soa(cp_tri)
        self.N, self.Tc = x.shape[1], t.shape[1]
        check(lib().msm_group_set_controlgrid(self.h, px, pt, self.N, self.Tc))

    def reset_meshspace(self, subject, data_mesh, feat):
        f, pf = _d(np.atleast_2d(feat))
        self._keep[("data", subject)] = data_mesh
        self.D = f.shape[0]
        check(lib().msm_group_set_subject(self.h, subject, data_mesh.h, pf, f.shape[0]))

    def reset_CPgrid(self, subject, cp_xyz):
        check(lib().msm_group_reset_cpgrid(self.h, subject, _soa(cp_xyz)[1]))

    def set_labels(self, labels):
        l, pl = _soa(labels)
        self.L = l.shape[1]
        check(lib().msm_group_set_labels(self.h, pl, self.L))

    REFERENCE_ORDER, CP_MAJOR = 0, 1
    DEVICE_ROTATIONS, HOST_ROTATIONS = 0, 1

    def set_rotation_mode(self, mode):
        """who computes the rotation matrices of the data meshes' vertices in get_patch_data: HOST_ROTATIONS (default) -- the host's libm, as the reference
        calls it: the rotated meshes are then the reference's to the bit, which decides the resampled values where a label carries data vertices exactly onto
        template vertices (regular icospheres on both sides) -- or DEVICE_ROTATIONS (msm_group_set_rotation_mode).  Takes effect at the next set-up."""
        check(lib().msm_group_set_rotation_mode(self.h, int(mode)))

    def set_pair_layout(self, layout):
        """the order of the pair list (getPairs and every pair index / range): REFERENCE_ORDER = estimate_pairs' own (subject A, control point, subject
        B), CP_MAJOR = control point by control point along a space-filling curve -- a contiguous slice is then a region of the sphere (the layout
        dist.sharded_group_setup chooses for more than one rank).  Takes effect at the next set-up (msm_group_set_pair_layout)."""
        check(lib().msm_group_set_pair_layout(self.h, int(layout)))

    def setupCostFunction(self):
        check(lib().msm_group_setup(self.h))
        n, p, t = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().msm_group_sizes(self.h, C.byref(n), C.byref(p), C.byref(t)))
        self.num_nodes, self.P, self.T = n.value, p.value, t.value

    # ---- sharded set-up (one process per GPU; see newmsm_amd.dist.sharded_group_setup) ----
    def setup_subjects(self, subjects):
        s, ps = _i(np.asarray(list(subjects), dtype=np.int32))
        check(lib().msm_group_setup_subjects(self.h, ps, len(s)))

    def setup_more_subjects(self, subjects):
        """further subjects of this rank after setup_subjects (msm_group_setup_more_subjects): the set-up in chunks"""
        s, ps = _i(np.asarray(list(subjects), dtype=np.int32))
        check(lib().msm_group_setup_more_subjects(self.h, ps, len(s)))

    def export_subject(self, subject):
        n = C.c_int64()
        check(lib().msm_group_export_subject(self.h, int(subject), None, None, None, 0, C.byref(n)))
        Vt = self._keep["template"].V
        F = np.zeros((self.L, self.D, Vt))
        pptr = np.zeros(self.N * self.L + 1, dtype=np.int32)
        pidx = np.zeros(max(n.value, 1), dtype=np.int32)
        check(lib().msm_group_export_subject(self.h, int(subject), F.ctypes.data_as(c_dp), pptr.ctypes.data_as(c_ip), pidx.ctypes.data_as(c_ip),
                                             len(pidx), C.byref(n)))
        return F, pptr, pidx[: n.value]

    def import_subject(self, subject, F, pptr, pidx):
        F, pF = _d(F)
        pp, ppp = _i(pptr)
        pi, ppi = _i(pidx)
        check(lib().msm_group_import_subject(self.h, int(subject), pF, ppp, ppi if len(pi) else None, len(pi)))

    # device-resident variants: the buffers are torch tensors on this context's GPU (data_ptr()), see newmsm_amd.dist
    def subject_index_count(self, subject):
        n = C.c_int64()
        check(lib().msm_group_export_subject_dev(self.h, int(subject), None, None, None, 0, C.byref(n)))
        return n.value

    def export_subject_dev(self, subject, F_ptr, pptr_ptr, pidx_ptr, cap):
        n = C.c_int64()
        check(lib().msm_group_export_subject_dev(self.h, int(subject), C.c_void_p(F_ptr), C.c_void_p(pptr_ptr), C.c_void_p(pidx_ptr), int(cap), C.byref(n)))
        return n.value

    def import_subject_dev(self, subject, F_ptr, pptr_ptr, pidx_ptr, npidx):
        check(lib().msm_group_import_subject_dev(self.h, int(subject), C.c_void_p(F_ptr), C.c_void_p(pptr_ptr), C.c_void_p(pidx_ptr), int(npidx)))

    def export_subjects_dev(self, subjects, F_ptr, F_stride, pptr_ptr, pptr_stride, pidx_ptr, pidx_stride):
        """subjects[k] into F_ptr + k * F_stride doubles, pptr_ptr + k * pptr_stride, pidx_ptr + k * pidx_stride int32 (device addresses): the send
        buffers of one all-gather, one synchronisation (msm_group_export_subjects_dev); returns the index counts"""
        s, ps = _i(np.asarray(list(subjects), dtype=np.int32))
        n = np.zeros(max(len(s), 1), dtype=np.int64)
        check(lib().msm_group_export_subjects_dev(self.h, ps, len(s), C.c_void_p(F_ptr), int(F_stride), C.c_void_p(pptr_ptr), int(pptr_stride),
                                                  C.c_void_p(pidx_ptr), int(pidx_stride), n.ctypes.data_as(C.POINTER(C.c_int64))))
        return n[: len(s)]

    def import_subjects_dev(self, subjects, F_ptr, F_stride, pptr_ptr, pptr_stride, pidx_ptr, pidx_stride, npidx):
        """the counterpart: subjects[k] out of the receive buffers of one all-gather, range-checked on the device (msm_group_import_subjects_dev)"""
        s, ps = _i(np.asarray(list(subjects), dtype=np.int32))
        n = np.ascontiguousarray(np.asarray(npidx, dtype=np.int64))
        assert len(n) == len(s)
        check(lib().msm_group_import_subjects_dev(self.h, ps, len(s), C.c_void_p(F_ptr), int(F_stride), C.c_void_p(pptr_ptr), int(pptr_stride),
                                                  C.c_void_p(pidx_ptr), int(pidx_stride), n.ctypes.data_as(C.POINTER(C.c_int64))))

    def fusionMove_dev(self, labeling, label, pair_range, triplet_range, quads_ptr, octets_ptr):
        """a slice of a label step, results left in device memory (quads_ptr / octets_ptr: device addresses)"""
        lab, pl = _i(labeling)
        check(lib().msm_group_fusion_move_dev(self.h, pl, int(label), int(pair_range[0]), int(pair_range[1]), int(triplet_range[0]), int(triplet_range[1]),
                                              C.c_void_p(quads_ptr), C.c_void_p(octets_ptr)))

    def time_moves(self, on=True):
        """HIP events around the kernels of every label step (msm_group_time_moves)"""
        check(lib().msm_group_time_moves(self.h, int(on)))

    def move_kernels_ms(self):
        ms = C.c_double(-1.0)
        check(lib().msm_group_move_kernels_ms(self.h, C.byref(ms)))
        return ms.value

    def finalize(self):
        check(lib().msm_group_finalize(self.h))
        n, p, t = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().msm_group_sizes(self.h, C.byref(n), C.byref(p), C.byref(t)))
        self.num_nodes, self.P, self.T = n.value, p.value, t.value

    def getPairs(self):
        out = np.zeros((self.P, 2), dtype=np.int32)
        check(lib().msm_group_get_pairs(self.h, out.ctypes.data_as(c_ip)))
        return out

    def fusionMove(self, labeling, label, out=None):
        """one label step of Fusion::optimize (Fusion.h:157-196): (pair_data buffers P x 4, triplet_data buffers T x 8).
        `out` (optional): the pair (quads, octets) of arrays to fill, e.g. Context.host_array((P, 4)) and ((T, 8)) -- pinned
        memory a copy kernel writes directly."""
        lab, pl = _i(labeling)
        quads, octets = (np.zeros((self.P, 4)), np.zeros((self.T, 8))) if out is None else out
        assert quads.shape == (self.P, 4) and octets.shape == (self.T, 8) and quads.dtype == octets.dtype == np.float64
        assert quads.flags.c_contiguous and octets.flags.c_contiguous
        check(lib().msm_group_fusion_move(self.h, pl, int(label), quads.ctypes.data_as(c_dp), octets.ctypes.data_as(c_dp)))
        return quads, octets

    def getTriplets(self):
        out = np.zeros((self.T, 3), dtype=np.int32)
        check(lib().msm_group_get_triplets(self.h, out.ctypes.data_as(c_ip)))
        return out

    def patch(self, subject, cp, label):
        subject, cp, label = int(subject), int(cp), int(label)
        n = C.c_int32()
        check(lib().msm_group_patch(self.h, subject, cp, label, None, None, 0, C.byref(n)))
        ids = np.zeros(n.value, dtype=np.int32)
        data = np.zeros((n.value, self.D))
        check(lib().msm_group_patch(self.h, subject, cp, label, ids.ctypes.data_as(c_ip), data.ctypes.data_as(c_dp), n.value, C.byref(n)))
        return ids, data

    def computePairwiseCost(self, pair, la, lb):
        p, pp = _i(np.atleast_1d(pair))
        a, pa = _i(np.atleast_1d(la))
        b, pb = _i(np.atleast_1d(lb))
        out = np.zeros(len(p))
        check(lib().msm_group_pairwise_batch(self.h, pp, pa, pb, len(p), out.ctypes.data_as(c_dp)))
        return out

    PAIR_ROUTES = ("fast64", "fast128", "fast256", "staged", "staged_beyond", "unstaged", "unstaged_beyond")
    DICE_FIT = ("default", "attribute", "refused")

    @staticmethod
    def pair_route(cntA, cntB, D, simmeasure, lanes):
        """msm_group_pair_route: the path k_group_pairwise takes for a query over patches of cntA and cntB entries (the function the kernel calls; host
        arithmetic, no GPU): dict(fast, padded, staged, beyond, name), name one of PAIR_ROUTES"""
        r = (C.c_int32 * 4)()
        check(lib().msm_group_pair_route(int(cntA), int(cntB), int(D), int(simmeasure), int(lanes), r))
        fast, padded, staged, beyond = bool(r[0]), int(r[1]), bool(r[2]), bool(r[3])
        name = "fast%d" % padded if fast else ("staged" if staged else "unstaged") + ("_beyond" if beyond else "")
        return dict(fast=fast, padded=padded, staged=staged, beyond=beyond, name=name)

    def pair_launch(self):
        """msm_group_pair_launch: what finalize() decided for this group's pair costs and what an evaluation would be handed now (host bookkeeping)"""
        o = (C.c_int64 * 8)()
        check(lib().msm_group_pair_launch(self.h, o))
        return dict(lanes=int(o[0]), patch_max=int(o[1]), npatch=int(o[2]), nsmall=int(o[3]), dice_lds=int(o[4]), dice_fit=self.DICE_FIT[o[5]], pval=bool(o[6]),
                    dir=bool(o[7]))

    def computeTripletCost(self, t, la, lb, lc):
        t_, pt = _i(np.atleast_1d(t))
        a, pa = _i(np.atleast_1d(la))
        b, pb = _i(np.atleast_1d(lb))
        c_, pc = _i(np.atleast_1d(lc))
        out = np.zeros(len(t_))
        check(lib().msm_group_triplet_batch(self.h, pt, pa, pb, pc, len(t_), out.ctypes.data_as(c_dp)))
        return out

    # ---- the Monte Carlo optimiser, subject by subject (an extension: the reference refuses MCMC in groupwise mode) ----
    def conditional_unary(self, subject, labeling, fetch=True):
        """msm_group_conditional_unary: U_s (L x N) of `subject` under `labeling` (S * N): per node and label the sum, in ascending pair index, of its
        incident pairs' costs against the partners' current labels; fetch=False leaves it on the device and returns None"""
        lab, pl = _i(labeling)
        assert lab.size == self.S * self.N
        U = np.zeros((self.L, self.N)) if fetch else None
        check(lib().msm_group_conditional_unary(self.h, int(subject), pl, U.ctypes.data_as(c_dp) if fetch else None))
        return U

    def subject_triplet_table(self, subject, fetch=True):
        """msm_group_subject_triplet_table: tc_s (Tc x L x L x L) of the subject's triplets in list order"""
        tc = np.zeros((self.Tc, self.L, self.L, self.L)) if fetch else None
        check(lib().msm_group_subject_triplet_table(self.h, int(subject), tc.ctypes.data_as(c_dp) if fetch else None))
        return tc

    def subject_triplets(self, subject):
        """the subject's triplets with local node ids (Tc x 3)"""
        s = int(subject)
        return (self.getTriplets()[s * self.Tc:(s + 1) * self.Tc] - s * self.N).astype(np.int32)

    def mcmc_subject(self, subject, labeling, seeds, mcparam=0.8, iters=100):
        """msm_group_mcmc_subject: one block -- the chains of `seeds` on (U_s, tc_s) from the subject's labels, the best one kept when its energy is
        strictly below the start's; returns (labeling S * N, (start energy, kept energy), accepted)"""
        lab = np.array(labeling, dtype=np.int32).reshape(-1)
        assert lab.size == self.S * self.N
        sd = np.ascontiguousarray(np.atleast_1d(seeds), dtype=np.uint64)
        e = np.zeros(2)
        acc = C.c_int32(-1)
        check(lib().msm_group_mcmc_subject(self.h, int(subject), lab.ctypes.data_as(c_ip), float(mcparam), int(iters), sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           len(sd), e.ctypes.data_as(c_dp), C.byref(acc)))
        return lab, (float(e[0]), float(e[1])), bool(acc.value)

    BLOCK_RECORD = ("start", "kept", "accepted", "best", "pair_ms", "sum_ms", "triplet_ms", "sweep_ms")

    def mcmc_pass(self, labeling, mcparam=0.8, iters=100, seed=0, it=0, chains=1, passes=1):
        """msm_group_mcmc_pass: `passes` passes of blocks over the subjects in ascending order, chain k of subject s in pass p seeded
        seed + it + 1000003 k + 15485863 (p S + s); returns (labeling S * N, per-block records (passes, S, 8): BLOCK_RECORD)"""
        lab = np.array(labeling, dtype=np.int32).reshape(-1)
        assert lab.size == self.S * self.N
        rec = np.zeros((max(int(passes), 1), self.S, 8))
        check(lib().msm_group_mcmc_pass(self.h, lab.ctypes.data_as(c_ip), float(mcparam), int(iters), int(seed) & 0xFFFFFFFFFFFFFFFF, int(it), int(chains),
                                        int(passes), rec.ctypes.data_as(c_dp)))
        return lab, rec


# ------------------------------------------------------------------ rigid level
def rigid_loops(gradsampling):
    """the number of outer loops of Rigid_cost_function::run (M/rigid_costfunction.cpp:173-225): the sampling spacing halves while it is > 0.05"""
    n, spacing = 0, float(gradsampling)
    while spacing > 0.05:
        n, spacing = n + 1, spacing * 0.5
    return n


class RigidCostFunction:
    """Rigid_cost_function (M/rigid_costfunction.cpp) over msm_rigid_*: the rotation of the level's data grid (SOURCE) that maximises its
    summed similarity to the reference data (TARGET).  target / source: Meshes of the level's data grid (SPH_orig, both); in_feat / ref_feat:
    the level's featurespace (D x V).  simmeasure 1 (SSD) or 2 (correlation)."""

    def __init__(self, ctx, target, source, in_feat, ref_feat, simmeasure=1):
        self.ctx, self.target, self.source = ctx, target, source
        self.in_feat = np.ascontiguousarray(np.atleast_2d(in_feat), dtype=np.float64)
        self.ref_feat = np.ascontiguousarray(np.atleast_2d(ref_feat), dtype=np.float64)
        if self.in_feat.shape != (self.ref_feat.shape[0], source.V) or self.ref_feat.shape[1] != target.V:
            raise ValueError("RigidCostFunction: features must be D x V of the source and of the target")
        self.simmeasure = int(simmeasure)
        self.V = source.V
        self.h = None

    def initialise(self):
        """initialise (:32-48): min_sigma from SOURCE, the per-target-triangle query lists, the data on the device"""
        self.close()
        self.h = lib().msm_rigid_create(self.ctx.h, self.target.h, self.source.h, self.in_feat.ctypes.data_as(c_dp),
                                        self.ref_feat.ctypes.data_as(c_dp), self.in_feat.shape[0], self.simmeasure)
        if not self.h:
            raise MsmError(-1, lib().msm_last_error().decode())
        return self

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            lib().msm_rigid_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def update_source(self, xyz):
        """update_source (:50): SOURCE's coordinates (V x 3)"""
        check(lib().msm_rigid_set_source(self.h, _soa(xyz)[1]))

    def get_source(self):
        out = np.zeros((3, self.V))
        check(lib().msm_rigid_get_source(self.h, out.ctypes.data_as(c_dp)))
        return np.ascontiguousarray(out.T)

    def cost(self, euler, per_vertex=False):
        """rigid_cost_mesh (:123-139) for each Euler triple (n x 3): the sums, and with per_vertex=True also the n x V values; SOURCE unchanged"""
        e, pe = _d(np.atleast_2d(euler))
        n = e.shape[0]
        sums = np.zeros(n)
        pv = np.zeros((n, self.V)) if per_vertex else None
        check(lib().msm_rigid_cost(self.h, pe, n, sums.ctypes.data_as(c_dp), pv.ctypes.data_as(c_dp) if pv is not None else None))
        return (sums, pv) if per_vertex else sums

    def rotate(self, euler):
        """rotate_in_mesh (:110-121) of SOURCE in place"""
        check(lib().msm_rigid_rotate(self.h, _d(np.asarray(euler, dtype=np.float64).reshape(3))[1]))

    def run(self, iters=20, stepsize=0.01, gradsampling=0.5):
        """run (:164-228).  Returns (SOURCE after the run (V x 3), trace, summary): trace rows {loop, iter, per, step, grad_zero, accepted},
        summary dict(RECinit, RECfinal, evaluations)"""
        cap = max(1, rigid_loops(gradsampling) * int(iters))
        trace = np.zeros((cap, 6))
        n = C.c_int32()
        summary = np.zeros(3)
        check(lib().msm_rigid_run(self.h, int(iters), float(stepsize), float(gradsampling), trace.ctypes.data_as(c_dp), cap, C.byref(n),
                                  summary.ctypes.data_as(c_dp)))
        return self.get_source(), trace[: n.value].copy(), dict(RECinit=summary[0], RECfinal=summary[1], evaluations=int(summary[2]))

    def kernel_ms(self):
        """GPU milliseconds and launches of the cost kernels of the last run / cost call"""
        ms = np.zeros(2)
        check(lib().msm_rigid_kernel_ms(self.h, ms.ctypes.data_as(c_dp)))
        return float(ms[0]), int(ms[1])
