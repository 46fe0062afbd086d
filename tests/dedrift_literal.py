"""A literal restatement of the dedrift stage (newmsm_amd/dedrift.py, include/msmhip.h: msm_dedrift_*) in numpy over the oracle: the yardstick of
tests/test_dedrift_cpu.py (which establishes it) and tests/test_gpu_dedrift.py (which holds the product against it).

Searches and barycentric weights: the oracle's Octree.barycentric_weights; sphere_project_warp and metric_resample: the oracle's; the J / R
arithmetic of triangle_strain (M/reg_tools.cpp:578-593, through the tangent frames of calculate_triangular_strain :698-743 and calculate_tri
:267-313) is written out below.  Wherever the order of a sum is part of the definition (the drift, the moments, the per-vertex means) the loop is
explicit and runs in that order.  LiteralOps answers the calls of dedrift.dedrift_group, so the same caller function drives both sides.

TEST INFRASTRUCTURE: nothing here is imported by the product."""
import numpy as np

from oracle import oracle as O


# ------------------------------------------------------------------------------------------------ geometry, as the reference writes it
def _cross(a, b):
    """operator* of R/point.cpp:178-183 (the Y term is written b.x a.z - b.z a.x)"""
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], b[:, 0] * a[:, 2] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1)


def _norm(a):
    return np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])


def _normalize(a):
    """Point::normalize, R/point.cpp:26-34: divided by its length when that exceeds EPSILON"""
    n = _norm(a)
    ok = n > 1e-8
    out = a.copy()
    out[ok] = a[ok] / n[ok][:, None]
    return out


def _tri_normal(v0, v1, v2):
    """Triangle::normal, R/triangle.cpp:45-50"""
    return _normalize(_cross(v2 - v0, v1 - v0))


def _calculate_tri(a):
    """calculate_tri(const Point&), M/reg_tools.cpp:267-313: a tangent pair for the normals a (n, 3)"""
    b = np.zeros_like(a)
    b[:, 0] = 1.0
    c = _cross(a, b)
    len2 = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]
    par = len2 == 0.0
    if np.any(par):
        b[par] = [0.0, 1.0, 0.0]
        c[par] = _cross(a[par], b[par])
        len2 = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]
    ln = np.sqrt(len2)
    ln[ln == 0.0] = 1.0
    e1 = c / ln[:, None]
    b2 = _cross(a, c)
    l2 = np.sqrt(b2[:, 0] * b2[:, 0] + b2[:, 1] * b2[:, 1] + b2[:, 2] * b2[:, 2])
    l2[l2 == 0.0] = 1.0
    return e1, b2 / l2[:, None]


def _det3_columns(c1, c2, c3):
    """determinant of the matrices whose COLUMNS are c1, c2, c3 (form_matrix_from_points)"""
    M = np.stack([c1, c2, c3], axis=2)  # (n, row, column)
    return (M[:, 0, 0] * (M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1]) - M[:, 0, 1] * (M[:, 1, 0] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 0])
            + M[:, 0, 2] * (M[:, 1, 0] * M[:, 2, 1] - M[:, 1, 1] * M[:, 2, 0]))


def triangle_JR(orig, final):
    """J and R of triangle_strain for n triangles: orig, final (n, 3 vertices, 3 coordinates).  calculate_triangular_strain (:698-743) brings both
    triangles into 2-D frames; triangle_strain (:551-593) forms F = edges * Edges^-1, C = F^T F (3 x 3, last diagonal entry 1), I1 = trace, I3 = det,
    J = sqrt(I3), I1* = (I1 - 1) / J, R = 1 when I1* <= 2 else (I1* + sqrt(I1*^2 - 4)) / 2."""
    orig = np.asarray(orig, dtype=np.float64)
    final = np.asarray(final, dtype=np.float64)
    nO = _tri_normal(orig[:, 0], orig[:, 1], orig[:, 2])
    nF = _tri_normal(final[:, 0], final[:, 1], final[:, 2])
    e1, e2 = _calculate_tri(nO)
    t1, t2 = _calculate_tri(nF)
    neg = _det3_columns(e1, e2, nO) < 0  # TRANS.Determinant() < 0: its first two columns are swapped (:713-719)
    c1 = np.where(neg[:, None], e2, e1)
    c2 = np.where(neg[:, None], e1, e2)
    neg2 = _det3_columns(c1, c2, nO) < 0  # the reference tests TRANS again here, not TRANS2 (:721): kept as it is
    d1 = np.where(neg2[:, None], t2, t1)
    d2 = np.where(neg2[:, None], t1, t2)

    def to2d(P, a, b):  # ORIG2D = ORIG3D * TRANS: rows are vertices, the first two columns their coordinates along a and b
        x = P[:, :, 0] * a[:, None, 0] + P[:, :, 1] * a[:, None, 1] + P[:, :, 2] * a[:, None, 2]
        y = P[:, :, 0] * b[:, None, 0] + P[:, :, 1] * b[:, None, 1] + P[:, :, 2] * b[:, None, 2]
        return x, y

    Ax, Ay = to2d(orig, c1, c2)
    Bx, By = to2d(final, d1, d2)
    c0, c1_, c4, c5 = Ax[:, 1] - Ax[:, 0], Ay[:, 1] - Ay[:, 0], Ax[:, 2] - Ax[:, 0], Ay[:, 2] - Ay[:, 0]
    c0c, c1c, c4c, c5c = Bx[:, 1] - Bx[:, 0], By[:, 1] - By[:, 0], Bx[:, 2] - Bx[:, 0], By[:, 2] - By[:, 0]
    det = c0 * c5 - c4 * c1_  # Edges = [[c0, c4], [c1, c5]]
    i00, i01, i10, i11 = c5 / det, -c4 / det, -c1_ / det, c0 / det
    F00, F01 = c0c * i00 + c4c * i10, c0c * i01 + c4c * i11  # edges = [[c0c, c4c], [c1c, c5c]]
    F10, F11 = c1c * i00 + c5c * i10, c1c * i01 + c5c * i11
    G00, G01 = F00 * F00 + F10 * F10, F00 * F01 + F10 * F11
    G10, G11 = F01 * F00 + F11 * F10, F01 * F01 + F11 * F11
    I1 = G00 + G11 + 1.0
    I3 = G00 * (G11 * 1.0 - 0.0 * 0.0) - G01 * (G10 * 1.0 - 0.0 * 0.0) + 0.0
    J = np.sqrt(I3)
    I1st = (I1 - 1.0) / J
    with np.errstate(invalid="ignore"):
        R = np.where(I1st <= 2, 1.0, 0.5 * (I1st + np.sqrt(np.where(I1st <= 2, 4.0, I1st * I1st) - 4)))
    return J, R


def vertex_distortion(orig_xyz, corrected_xyz, tri, adjacency=None):
    """(2, V): per vertex the plain mean over its incident triangles, in trID order, of log2 J (row 0) and log2 R (row 1)"""
    orig_xyz = np.asarray(orig_xyz, dtype=np.float64)
    corrected_xyz = np.asarray(corrected_xyz, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int32)
    J, R = triangle_JR(orig_xyz[tri], corrected_xyz[tri])
    lj, lr = np.log2(J), np.log2(R)
    if adjacency is None:
        adjacency = O.Mesh(orig_xyz, tri).adjacency()
    _, _, tid_ptr, tid = adjacency
    V = len(orig_xyz)
    out = np.zeros((2, V))
    for v in range(V):
        sj = sr = 0.0
        n = tid_ptr[v + 1] - tid_ptr[v]
        for e in range(tid_ptr[v], tid_ptr[v + 1]):
            sj += lj[tid[e]]
            sr += lr[tid[e]]
        if n:
            out[0, v], out[1, v] = sj / n, sr / n
    return out


def min_J_and_folds(orig_xyz, corrected_xyz, tri):
    """(smallest J, number of corrected triangles whose normal points inwards): the conditions a comparison of distortion maps rests on"""
    tri = np.asarray(tri)
    J, _ = triangle_JR(np.asarray(orig_xyz)[tri], np.asarray(corrected_xyz)[tri])
    c = np.asarray(corrected_xyz)[tri]
    o = np.asarray(orig_xyz)[tri]
    side = np.sign(np.einsum("ij,ij->i", _cross(c[:, 2] - c[:, 0], c[:, 1] - c[:, 0]), c.mean(axis=1)))
    side0 = np.sign(np.einsum("ij,ij->i", _cross(o[:, 2] - o[:, 0], o[:, 1] - o[:, 0]), o.mean(axis=1)))
    return float(J.min()), int(np.sum(side != side0))


# ------------------------------------------------------------------------------------------------ the stages
def interpolate_sorted(vid, w, coords):
    """project_anatomical_mesh's sum (R/resampler.cpp:260-282): newPt += coords(id) * weight over the query's std::map, i.e. ascending vertex id, from 0"""
    key = np.argsort(vid, axis=1, kind="stable")
    vid, w = np.take_along_axis(vid, key, axis=1), np.take_along_axis(w, key, axis=1)
    out = np.zeros((len(vid), 3))
    for k in range(3):
        out = out + coords[vid[:, k]] * w[:, k][:, None]
    return out


def finish_warp(total, S):
    """drift = sum / S; W = drift minus the midpoint of its bounding box, every vertex scaled to length 100"""
    drift = total / float(S)
    mid = (drift.min(axis=0) + drift.max(axis=0)) / 2
    p = drift - mid
    n = _norm(p)
    return (p / n[:, None]) * 100.0, drift


def moments(maps):
    """mean and population standard deviation over the subjects, two passes in subject order"""
    S = len(maps)
    acc = np.zeros_like(maps[0])
    for s in range(S):
        acc = acc + maps[s]
    mean = acc / S
    q = np.zeros_like(maps[0])
    for s in range(S):
        d = maps[s] - mean
        q = q + d * d
    return mean, np.sqrt(q / S)


def dice_overlap(a, b, perc=75):
    """compare_stats.py:20-23"""
    ma = np.where(a > np.percentile(a, perc), 1, 0)
    mb = np.where(b > np.percentile(b, perc), 1, 0)
    return (2 * np.sum(ma * mb)) / (np.sum(ma) + np.sum(mb))


def pair_matrices(maps, perc=75):
    """cc, dice (D, S, S) by numpy.corrcoef and dice_overlap, pair by pair as compare_stats.py:44-69 does it"""
    S, D = len(maps), maps[0].shape[0]
    cc, dice = np.zeros((D, S, S)), np.zeros((D, S, S))
    for d in range(D):
        for i in range(S):
            cc[d, i, i] = 1.0
            dice[d, i, i] = dice_overlap(maps[i][d], maps[i][d], perc)
            for j in range(i + 1, S):
                cc[d, i, j] = cc[d, j, i] = np.corrcoef(maps[i][d], maps[j][d])[0, 1]
                dice[d, i, j] = dice[d, j, i] = dice_overlap(maps[i][d], maps[j][d], perc)
    return cc, dice


def threshold_gaps(maps, perc=75):
    """the smallest distance of any value of any map to that map's percentile threshold, relative to the map's range (0: a tie -- masks then depend
    on the last bit of the threshold and may not be compared)"""
    worst = np.inf
    for m in maps:
        for row in np.atleast_2d(m):
            worst = min(worst, float(np.min(np.abs(row - np.percentile(row, perc))) / (row.max() - row.min())))
    return worst


class LiteralOps:
    """dedrift.dedrift_group's calls answered by the restatement"""

    def begin(self, template_xyz, template_tri, num_subjects):
        T = O.Mesh(template_xyz, template_tri)
        return dict(T=T, Ttree=O.Octree(T), txyz=np.array(template_xyz, dtype=np.float64), S=num_subjects, total=np.zeros((len(template_xyz), 3)),
                    n=0, maps={})

    def accumulate(self, st, s, reg_xyz, tri, orig_xyz, details):
        R = O.Mesh(reg_xyz, tri)
        status, t, vid, w = O.Octree(R).barycentric_weights(st["txyz"])
        assert np.all(status == 0), "the oracle's search failed"
        inv = interpolate_sorted(vid, w, np.asarray(orig_xyz, dtype=np.float64))
        st["total"] = st["total"] + inv  # subject order = call order
        st["n"] += 1
        return dict(tri=t, w=w, inverse=inv) if details else None

    def finish(self, st):
        assert st["n"] == st["S"]
        st["W"], drift = finish_warp(st["total"], st["S"])
        return st["W"], drift

    def correct(self, st, s, reg_xyz, tri, orig_xyz, data, details):
        found = None
        if details:
            status, t, _, w = st["Ttree"].barycentric_weights(np.asarray(reg_xyz, dtype=np.float64))
            assert np.all(status == 0)
            found = dict(tri=t, w=w)
        corrected = O.sphere_project_warp(reg_xyz, st["T"], st["W"])
        cm = O.Mesh(corrected, tri)
        resampled = O.metric_resample(cm, np.atleast_2d(data), st["T"])
        distortion = vertex_distortion(orig_xyz, corrected, tri, cm.adjacency())
        st["maps"][s] = resampled
        return (corrected, resampled, distortion, found) if details else (corrected, resampled, distortion)

    def set_map(self, st, s, data):
        st["maps"][s] = np.array(np.atleast_2d(data), dtype=np.float64)

    def group_stats(self, st, percentile):
        maps = [st["maps"][s] for s in range(st["S"])]
        mean, sd = moments(maps)
        cc, dice = pair_matrices(maps, percentile)
        return mean, sd, cc, dice

    def end(self, st):
        pass


# ------------------------------------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
def rotation(axis, degrees):
    """Rodrigues' matrix"""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(degrees)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


Q_COMMON = rotation((1.0, 2.0, 3.0), 2.0)


def smooth_warp(xyz, s, amp=1.5):
    """subject s's smooth synthetic warp of a radius-100 sphere: with u = x / 100, C (3 x 3) and a (3) standard normals from default_rng(s) drawn in
    that order, x + amp (C u) sin(2 a.u), rescaled to radius 100"""
    rng = np.random.default_rng(s)
    Cm = rng.standard_normal((3, 3))
    a = rng.standard_normal(3)
    u = np.asarray(xyz, dtype=np.float64) / 100.0
    y = xyz + amp * (u @ Cm.T) * np.sin(2.0 * (u @ a))[:, None]
    return y / np.linalg.norm(y, axis=1, keepdims=True) * 100.0


def smooth_data(xyz, D, seed, noise=0.05):
    """continuous random-plus-smooth data rows on a sphere: low-order trigonometric bumps of random orientation plus white noise, so that no value
    ties with a percentile threshold"""
    rng = np.random.default_rng(1000 + seed)
    u = np.asarray(xyz, dtype=np.float64) / 100.0
    rows = []
    for _ in range(D):
        A = rng.standard_normal((4, 3))
        f = np.sin(3.0 * (u @ A[0])) + 0.7 * np.cos(2.0 * (u @ A[1])) + 0.5 * np.sin(5.0 * (u @ A[2]) + 1.0) * np.cos(u @ A[3])
        rows.append(f + noise * rng.standard_normal(len(u)))
    return np.array(rows)


def group_data(reg_xyz, D, s, noise=0.05):
    """subject s's data for a group whose registered spheres are reg_xyz: one smooth field shared by the group, read where the registration puts the
    subject's vertices, plus the subject's own white noise (continuous values: no ties with a percentile threshold)"""
    A = np.random.default_rng(999).standard_normal((D, 4, 3))
    u = np.asarray(reg_xyz, dtype=np.float64) / 100.0
    rng = np.random.default_rng(2000 + s)
    rows = []
    for d in range(D):
        f = np.sin(3.0 * (u @ A[d, 0])) + 0.7 * np.cos(2.0 * (u @ A[d, 1])) + 0.5 * np.sin(5.0 * (u @ A[d, 2]) + 1.0) * np.cos(u @ A[d, 3])
        rows.append(f + noise * rng.standard_normal(len(u)))
    return np.array(rows)


def mean_angle_deg(a, b):
    """(mean, max) angle in degrees between corresponding vertices of two spheres"""
    ua = a / np.linalg.norm(a, axis=1, keepdims=True)
    ub = b / np.linalg.norm(b, axis=1, keepdims=True)
    ang = np.rad2deg(2.0 * np.arcsin(np.minimum(1.0, 0.5 * np.linalg.norm(ua - ub, axis=1))))
    return float(ang.mean()), float(ang.max())
