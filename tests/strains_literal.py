"""calculate_strains (M/reg_tools.cpp:365-549) and what it stands on, restated statement by statement in numpy (test infrastructure: only tests
import this).

    estimate_normals        R/mesh.cpp:133-150  (Mesh::local_normal: Triangle::normal R/triangle.cpp:42-47 summed in trID order, normalised)
    calculate_tangs         M/reg_tools.cpp:205-262  (the local normal flipped when a . x_i < 0; rigid_literal.tangent_pairs)
    calculate_strains       :498-549  (the neighbourhood: |x_i - x_j| <= r and n_j . n_i >= 0, r = fit_radius grown by 0.5 until 9 members)
    calculate_strains       :365-496  (the local fit, get_coordinate_transformation :179-203, F, C, the stretches)
    project_anatomical_mesh R/resampler.cpp:260-282  (the oracle's barycentric weights, summed in std::map order)

The fit solves the 5-column problem: the reference's alpha has an identically zero first column, to which the minimum-norm solution of its
pseudo-inverse gives coefficient 0, and coefficients 2-6 are the least-squares solution over the other five (a 6-column SVD can leave a
singular value near 1e-17 for that column and invert it).  The pseudo-inverse here comes from numpy's SVD of the 5-column block, inverting only
non-zero singular values as the reference does; its condition number is reported for the comparisons.

literal=True rescans every vertex against every vertex for every radius step, as the reference does (O(V^2) per step: small meshes only).
The fast mode finds the same neighbourhoods from an x-sorted candidate slab with the same exact tests, and the radius from the 9th smallest
member distance (count(r) > 8 exactly when d9 <= r); tests/test_strains_cpu.py checks it against the literal mode.  The fit is the same code in
both modes, batched over vertices with the same member count.  Sums are written out in the reference's order (x, y, z; trID order)."""
import time

import numpy as np

from oracle import oracle as O
from rigid_literal import _cross, _dot, _normalize, tangent_pairs

STEP = 0.5  # fit_temp += 0.5 (:541)


class NeverNine(Exception):
    """some vertex can never have more than 8 members: the reference's radius loop would not end"""


def trid_lists(tri, V):
    """Mpoint::trID of every vertex as CSR: the triangles that name it, in the order they were added (ascending id)"""
    tri = np.asarray(tri, dtype=np.int64)
    owner = tri.ravel()
    tids = np.repeat(np.arange(len(tri)), 3)
    key = np.argsort(owner, kind="stable")
    tid_ptr = np.zeros(V + 1, dtype=np.int64)
    np.add.at(tid_ptr, owner + 1, 1)
    return np.cumsum(tid_ptr), tids[key]


def estimate_normals(xyz, tri):
    """estimate_normals: Mesh::local_normal of every vertex"""
    xyz = np.asarray(xyz, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int64)
    tid_ptr, tid = trid_lists(tri, len(xyz))
    v0, v1, v2 = xyz[tri[:, 0]], xyz[tri[:, 1]], xyz[tri[:, 2]]
    tn = _normalize(_cross(v2 - v0, v1 - v0))
    deg = np.diff(tid_ptr)
    acc = np.zeros_like(xyz)
    for k in range(int(deg.max()) if len(deg) else 0):
        has = deg > k
        acc[has] = acc[has] + tn[tid[tid_ptr[:-1][has] + k]]
    return _normalize(acc)


def _norm_rows(d):  # Point::norm
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def _dot_rows(a, b):  # operator|
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def final_radius(d9, fit_radius):
    """the radius the reference's loop stops at: fit_radius + 0.5 + 0.5 + ... (its own additions), the first with count > 8, i.e. >= d9"""
    r = fit_radius
    while not d9 <= r:
        r += STEP
    return r


def neighbourhoods_literal(xyz, nrm, fit_radius):
    """the loop of :519-547 for every vertex: a full rescan per radius step"""
    V = len(xyz)
    span = float(np.max(_norm_rows(xyz - xyz[0]))) * 2 + 1.0
    kept, radius = [], np.zeros(V)
    for index in range(V):
        fit_temp = fit_radius
        k = np.zeros(0, dtype=np.int64)
        while len(k) <= 8:
            dist = _norm_rows(xyz[index] - xyz)
            dir_chk1 = _dot_rows(nrm, nrm[index])
            k = np.nonzero((dist <= fit_temp) & (dir_chk1 >= 0))[0]
            if len(k) <= 8:
                if fit_temp > span:
                    raise NeverNine("vertex %d: %d members" % (index, len(k)))
                fit_temp += STEP
        kept.append(k)
        radius[index] = fit_temp
    return kept, radius


def neighbourhoods_fast(xyz, nrm, fit_radius):
    """the same sets from an x-sorted slab of candidates: the exact distance and normal tests on the vertices within the radius in x"""
    V = len(xyz)
    order = np.argsort(xyz[:, 0], kind="stable")
    xs = xyz[order, 0]
    kept, radius = [], np.zeros(V)

    def slab(i, R):
        w = R + 1e-9 * (abs(xyz[i, 0]) + R)
        lo, hi = np.searchsorted(xs, xyz[i, 0] - w, "left"), np.searchsorted(xs, xyz[i, 0] + w, "right")
        cand = order[lo:hi]
        return cand, _norm_rows(xyz[i] - xyz[cand]), _dot_rows(nrm[cand], nrm[i]) >= 0, lo == 0 and hi == V

    for i in range(V):
        R = fit_radius
        while True:
            cand, d, ok, full = slab(i, R)
            sel = ok & (full | (d <= R))
            if np.count_nonzero(sel) >= 9:
                d9 = np.partition(d[sel], 8)[8]
                break
            if full:
                raise NeverNine("vertex %d: %d members" % (i, np.count_nonzero(sel)))
            R *= 2.0
        r = final_radius(d9, fit_radius)
        if r > R and not full:
            cand, d, ok, full = slab(i, r)
        kept.append(np.sort(cand[ok & (d <= r)]))
        radius[i] = r
    return kept, radius


def _fit(orig, final, nrm, e1, e2, idx, members):
    """the local fits of :365-496 for a batch of vertices idx (B) with the same member count (members: B x m, ascending)"""
    oi, fi = orig[idx][:, None, :], final[idx][:, None, :]
    n_o, t1v, t2v = nrm[idx][:, None, :], e1[idx][:, None, :], e2[idx][:, None, :]
    tmp = orig[members] - oi
    T1, T2 = _dot_rows(tmp, t1v), _dot_rows(tmp, t2v)  # project_point(tmp, T, T1, T2)
    N = _dot_rows(tmp, n_o)
    alpha = np.stack([T1, T2, 0.5 * T1 * T1, 0.5 * T2 * T2, T1 * T2], axis=-1)  # columns 2-6 of alpha
    tf = final[members] - fi
    rhs = np.stack([N, _dot_rows(tf, t1v), _dot_rows(tf, t2v), _dot_rows(tf, n_o)], axis=-1)
    U, S, Vt = np.linalg.svd(alpha, full_matrices=False)
    Sinv = np.zeros_like(S)
    nz = S != 0
    Sinv[nz] = 1.0 / S[nz]
    coef = np.swapaxes(Vt, 1, 2) @ (Sinv[:, :, None] * (np.swapaxes(U, 1, 2) @ rhs))  # pinv(alpha) {N, t1, t2, n}: B x 5 x 4
    with np.errstate(divide="ignore"):
        cond = np.where(S[:, -1] > 0, S[:, 0] / np.where(S[:, -1] > 0, S[:, -1], 1.0), np.inf)
    dNdT1, dNdT2 = coef[:, 0, 0], coef[:, 1, 0]
    dt1dT1, dt1dT2 = coef[:, 0, 1], coef[:, 1, 1]
    dt2dT1, dt2dT2 = coef[:, 0, 2], coef[:, 1, 2]
    dndT1, dndT2 = coef[:, 0, 3], coef[:, 1, 3]
    B = len(idx)
    one, zero = np.ones(B), np.zeros(B)
    G1, G2 = np.stack([one, zero, dNdT1], 1), np.stack([zero, one, dNdT2], 1)
    G3 = _cross(G1, G2)
    G3 = G3 / np.sqrt(_dot(G3, G3))[:, None]
    G = np.stack([G1, G2, G3], axis=2)  # columns
    G_cont = np.swapaxes(np.linalg.inv(G), 1, 2)
    g1, g2 = np.stack([dt1dT1, dt2dT1, dndT1], 1), np.stack([dt1dT2, dt2dT2, dndT2], 1)
    g3 = _cross(g1, g2)
    g3 = g3 / np.sqrt(_dot(g3, g3))[:, None]
    g = np.stack([g1, g2, g3], axis=2)
    F = g @ np.swapaxes(G_cont, 1, 2)
    Cm = np.swapaxes(F, 1, 2) @ F
    Uc, Omega, _ = np.linalg.svd(Cm)  # SVD(C, Omega, U): decreasing singular values
    mm = np.abs(np.einsum("bk,bkl->bl", G3, Uc))
    sq = np.sqrt(Omega)
    c0 = (mm[:, 0] >= mm[:, 1]) & (mm[:, 0] >= mm[:, 2])
    c1 = ~c0 & (mm[:, 1] >= mm[:, 0]) & (mm[:, 1] >= mm[:, 2])
    maxind = np.where(c0, np.where(sq[:, 1] > sq[:, 2], 1, 2), np.where(c1, np.where(sq[:, 0] > sq[:, 2], 0, 2), np.where(sq[:, 0] > sq[:, 1], 0, 1)))
    minind = np.where(c0, np.where(sq[:, 1] > sq[:, 2], 2, 1), np.where(c1, np.where(sq[:, 0] > sq[:, 2], 2, 0), np.where(sq[:, 0] > sq[:, 1], 1, 0)))
    s1 = np.sqrt(Omega[np.arange(B), maxind])
    s2 = np.sqrt(Omega[np.arange(B), minind])
    return np.stack([s1, s2, 0.5 * (s1 * s1 - 1), 0.5 * (s2 * s2 - 1)]), cond


def calculate_strains(orig_xyz, orig_tri, final_xyz, fit_radius=2.0, literal=False):
    """calculate_strains(fit_radius, orig, final) with orig's own triangles.  Returns dict(strains 4 x V, kept (V,), radius (V,), cond (V,):
    the condition number of each vertex's 5-column block, members: the member lists)"""
    orig = np.ascontiguousarray(orig_xyz, dtype=np.float64)
    final = np.ascontiguousarray(final_xyz, dtype=np.float64)
    nrm = estimate_normals(orig, orig_tri)
    e1, e2 = tangent_pairs(orig, nrm)  # calculate_tangs: the local normal, flipped when a . x_i < 0
    members, radius = (neighbourhoods_literal if literal else neighbourhoods_fast)(orig, nrm, fit_radius)
    V = len(orig)
    strains, cond = np.zeros((4, V)), np.zeros(V)
    counts = np.array([len(k) for k in members])
    if literal:
        for i in range(V):
            s, c = _fit(orig, final, nrm, e1, e2, np.array([i]), members[i][None, :])
            strains[:, i], cond[i] = s[:, 0], c[0]
    else:
        for m in np.unique(counts):
            idx = np.nonzero(counts == m)[0]
            s, c = _fit(orig, final, nrm, e1, e2, idx, np.stack([members[i] for i in idx]))
            strains[:, idx], cond[idx] = s, c
    return dict(strains=strains, kept=counts, radius=radius, cond=cond, members=members)


def project_anatomical_mesh(sphere_xyz, target_xyz, target_tri, anat_xyz):
    """project_anatomical_mesh(orig = the registered input sphere, target = the reference sphere, anat = the reference anatomy): every sphere vertex
    placed by its barycentric weights on target (get_barycentric_weights through target's octree), new_coord += coord(id) * w in std::map order;
    the coordinates are anat's when it has target's vertex count, target's own otherwise"""
    anat = np.asarray(anat_xyz, dtype=np.float64)
    coords = anat if len(anat) == len(target_xyz) else np.asarray(target_xyz, dtype=np.float64)
    mesh = O.Mesh(np.asarray(target_xyz, dtype=np.float64), np.asarray(target_tri, dtype=np.int32))
    return O.surface_resample(coords, O.Octree(mesh), np.asarray(sphere_xyz, dtype=np.float64))


def flattened_ellipsoid(order, axes=(30.0, 30.0, 1.0), seed=0, jitter=0.05):
    """an icosphere scaled to the semi-axes (mm) with a little jitter: two close sheets whose normals face apart"""
    xyz, tri = O.icosphere(order, radius=1.0)
    rng = np.random.default_rng(seed)
    xyz = xyz * np.asarray(axes)[None, :]
    return xyz + rng.normal(scale=jitter, size=xyz.shape) * np.array([1.0, 1.0, 0.02]), tri


def jittered_plane(n=12, spacing=1.0, seed=0, jitter=0.2):
    """a triangulated n x n patch of the plane z = 0 with jittered vertices"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij"), -1).reshape(-1, 2) * spacing
    g = g + rng.uniform(-jitter, jitter, size=g.shape) * spacing
    xyz = np.concatenate([g, np.zeros((len(g), 1))], 1)
    tri = []
    for a in range(n - 1):
        for b in range(n - 1):
            v = a * n + b
            tri += [[v, v + n, v + 1], [v + 1, v + n, v + n + 1]]
    return xyz, np.asarray(tri, dtype=np.int32)


def cpu_seconds(xyz, tri, final, fit_radius=2.0):
    """a single-core timing of the fast mode (tools/time_strains.py cannot import tests/)"""
    t0 = time.process_time()
    calculate_strains(xyz, tri, final, fit_radius)
    return time.process_time() - t0

