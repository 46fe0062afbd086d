"""Rigid_cost_function (M/rigid_costfunction.cpp) restated statement by statement over the ORACLE's mesh and octree (test infrastructure: only
tests import this).  It keeps the reference's own state: the per-vertex Neighbourhood built O(V^2) at initialise (Neighbourhood::update,
M/reg_tools.cpp:31-57), rewritten by every Evaluate_SIMGradient; the sparse similarity map (sparsesimkernel's mp, M/similarities.cpp:37-52) that
only grows; current_sim; and every quirk of run() (:164-228): the gradient against a grad_zero that keeps a rejected value, the evaluation at the
doubly rotated mesh, rotations applied in place one after the other.

    initialise              :32-48  (+ calculate_MeanVD R/mesh.cpp:276-293)
    rotate_in_mesh          :110-121 (euler_rotate R/point.cpp:154-171: R^T v, row sums left to right)
    rigid_cost_mesh         :123-139
    Evaluate_SIMGradient    :87-108  (get_all_neighbours :141-162, calculate_sim_column_nbh / corr / SSD / meanvector M/similarities.cpp:37-120)
    WLS_simgradient         :60-85   (calculate_tangs M/reg_tools.cpp:205-262, Mesh::local_normal R/mesh.cpp:133-141)
    run                     :164-228

fast=True replaces only what the product replaces -- one query list per closest target triangle, similarities computed where they are read, the
per-vertex loop vectorised over numpy -- and is itself checked against the literal mode (tests/test_rigid_cpu.py).  The geometry (rotation,
local normals, tangent pairs, plane coordinates) is the same code in both modes: elementwise numpy operations in the reference's order."""
import math

import numpy as np

from oracle import oracle as O

RAD = 100.0
EPSILON = 1e-8


def euler_matrix(w1, w2, w3):
    """euler_rotate's matrix (R/point.cpp:157-165), row-major, libm sin / cos"""
    c, s = math.cos, math.sin
    return [c(w2) * c(w3), -c(w1) * s(w3) + s(w1) * s(w2) * c(w3), s(w1) * s(w3) + c(w1) * s(w2) * c(w3),
            c(w2) * s(w3), c(w1) * c(w3) + s(w1) * s(w2) * s(w3), -s(w1) * c(w3) + c(w1) * s(w2) * s(w3),
            -s(w2), s(w1) * c(w2), c(w1) * c(w2)]


def euler_rotate(xyz, w1, w2, w3):
    """every vertex v -> R^T v (rotation.t() * vector: component k = R(1,k) x + R(2,k) y + R(3,k) z)"""
    R = euler_matrix(w1, w2, w3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([R[0] * x + R[3] * y + R[6] * z, R[1] * x + R[4] * y + R[7] * z, R[2] * x + R[5] * y + R[8] * z], axis=1)


def _cross(a, b):  # operator* R/point.cpp:178-183
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], b[:, 0] * a[:, 2] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _normalize(a):  # Point::normalize R/point.cpp:26-34
    n = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
    ok = n > EPSILON
    out = a.copy()
    out[ok] = a[ok] / n[ok][:, None]
    return out


def mean_vd(xyz, tri):
    """calculate_MeanVD (R/mesh.cpp:276-293) through the oracle's mesh (its neighbour order)"""
    m = O.Mesh(xyz, tri)
    O.lib().orc_mesh_mean_vd.restype = O.C.c_double
    return float(O.lib().orc_mesh_mean_vd(m.h))


def local_normals(xyz, tri, tid_ptr, tid):
    """Mesh::local_normal of every vertex: the incident triangles' normals (Triangle::normal R/triangle.cpp:42-47) summed in trID order"""
    v0, v1, v2 = xyz[tri[:, 0]], xyz[tri[:, 1]], xyz[tri[:, 2]]
    tn = _normalize(_cross(v2 - v0, v1 - v0))
    deg = np.diff(tid_ptr)
    acc = np.zeros_like(xyz)
    for k in range(int(deg.max())):
        has = deg > k
        acc[has] = acc[has] + tn[tid[tid_ptr[:-1][has] + k]]
    return _normalize(acc)


def tangent_pairs(xyz, a):
    """calculate_tangs (M/reg_tools.cpp:205-262) for every vertex given its local normal a"""
    a = np.where((_dot(a, xyz) < 0)[:, None], a * -1, a)
    ax, ay, az = np.abs(a[:, 0]), np.abs(a[:, 1]), np.abs(a[:, 2])
    bx = (ax >= ay) & (ax >= az)
    by = ~bx & (ay >= ax) & (ay >= az)
    bz = ~bx & ~by
    e1 = np.zeros_like(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.sqrt(a[:, 2] * a[:, 2] + a[:, 1] * a[:, 1])
        m = bx & (mag == 0)
        e1[m] = [0, 0, 1]
        m = bx & (mag != 0)
        e1[m, 1], e1[m, 2] = -a[m, 2] / mag[m], a[m, 1] / mag[m]
        mag = np.sqrt(a[:, 2] * a[:, 2] + a[:, 0] * a[:, 0])
        m = by & (mag == 0)
        e1[m] = [0, 0, 1]
        m = by & (mag != 0)
        e1[m, 0], e1[m, 2] = -a[m, 2] / mag[m], a[m, 0] / mag[m]
        mag = np.sqrt(a[:, 1] * a[:, 1] + a[:, 0] * a[:, 0])
        m = bz & (mag == 0)
        e1[m] = [1, 0, 0]
        m = bz & (mag != 0)
        e1[m, 0], e1[m, 1] = -a[m, 1] / mag[m], a[m, 0] / mag[m]
    e2 = _normalize(_cross(a, e1))
    return e1, e2


def meanvector(F):
    """meanvector (M/similarities.cpp:100-120): one global mean for a single row, per column otherwise"""
    D, n = F.shape
    if D == 1:
        s = 0.0
        for v in F[0]:
            s += v
        return np.full(n, s / n)
    out = np.zeros(n)
    for i in range(n):
        s = 0.0
        for d in range(D):
            s += F[d, i]
        out[i] = s / D
    return out


class RigidLiteral:
    def __init__(self, target_xyz, tri, in_feat, ref_feat, simmeasure, fast=False):
        """Rigid_cost_function(SPH_orig, SPH_orig, FEAT) + set_parameters' simmeasure; TARGET and SOURCE are the same grid"""
        self.TARGET = np.array(target_xyz, dtype=np.float64)
        self.SOURCE = self.TARGET.copy()
        self.tri = np.asarray(tri, dtype=np.int32)
        self.A = np.ascontiguousarray(np.atleast_2d(in_feat), dtype=np.float64)   # input: m_A
        self.B = np.ascontiguousarray(np.atleast_2d(ref_feat), dtype=np.float64)  # reference: m_B
        self.simmeasure, self.fast = simmeasure, fast
        self.evaluations = 0

    # ---------------------------------------------------------------- initialise
    def initialise(self):
        V = len(self.SOURCE)
        self.current_sim = np.zeros(V)
        self.min_sigma = self.MVD = mean_vd(self.SOURCE, self.tri)
        self.mp = {}  # the sparse similarity matrix: (target vertex, source vertex) -> sim
        self.rmeanA, self.rmeanB = meanvector(self.A), meanvector(self.B)
        mesh = O.Mesh(self.TARGET, self.tri)
        _, _, self.tid_ptr, self.tid = mesh.adjacency()
        self.tree = O.Octree(mesh)
        self._keep = mesh
        if self.fast:
            self._build_query_lists()
            return self
        self.nbh = self._neighbourhood(2 * math.asin(4 * self.MVD / (2 * RAD)))
        for i in range(V):
            self.calculate_sim_column_nbh(i)
        return self

    def _neighbourhood(self, angsep):
        """Neighbourhood::update: per source vertex the target vertices within angsep, nearest first"""
        src = _normalize(self.SOURCE)
        tgt = _normalize(self.TARGET)
        ca = math.cos(angsep)
        out = []
        for i in range(len(src)):
            d = _dot(tgt, np.broadcast_to(src[i], tgt.shape))
            cand = np.nonzero(d >= ca)[0]
            dist = np.sqrt(((tgt[cand] - src[i]) ** 2).sum(axis=1))
            out.append([int(n) for n in cand[np.argsort(dist, kind="stable")]])
        return out

    def update_source(self, xyz):
        self.SOURCE = np.array(xyz, dtype=np.float64)

    # ---------------------------------------------------------------- similarity
    def SSD(self, i, j):
        prod = 0.0
        for d in range(self.A.shape[0]):
            prod += (self.A[d, i] - self.B[d, j]) * (self.A[d, i] - self.B[d, j])
        return math.sqrt(prod) / self.A.shape[0]

    def corr(self, i, j):
        prod = varA = varB = 0.0
        ma, mb = self.rmeanA[i], self.rmeanB[j]
        for d in range(self.A.shape[0]):
            prod += (self.A[d, i] - ma) * (self.B[d, j] - mb)
            varA += (self.A[d, i] - ma) * (self.A[d, i] - ma)
            varB += (self.B[d, j] - mb) * (self.B[d, j] - mb)
        if varA == 0.0 or varB == 0.0:
            return 0.0
        return prod / (math.sqrt(varA) * math.sqrt(varB))

    def calculate_sim_column_nbh(self, ind):
        for q in self.nbh[ind]:
            if q != 0:
                if self.simmeasure == 1:
                    self.mp[(q, ind)] = -self.SSD(ind, q)
                elif self.simmeasure == 2:
                    self.mp[(q, ind)] = self.corr(ind, q)

    # ---------------------------------------------------------------- one evaluation
    def rotate_in_mesh(self, a1, a2, a3):
        self.SOURCE = euler_rotate(self.SOURCE, a1, a2, a3)

    def _geometry(self):
        """per vertex of the (rotated) SOURCE: tangent pair, plane origin, the vertex's plane coordinates, its closest target triangle"""
        e1, e2 = tangent_pairs(self.SOURCE, local_normals(self.SOURCE, self.tri, self.tid_ptr, self.tid))
        origin = _normalize(_cross(e1, e2)) * RAD
        po = self.SOURCE - origin
        closest = self.tree.closest_triangle(self.SOURCE)
        if np.any(closest < 0):
            raise RuntimeError("octree search failed")
        return e1, e2, origin, _dot(po, e1), _dot(po, e2), closest

    def get_all_neighbours(self, index, N, n, found):
        update = False
        for j in self.tid[self.tid_ptr[n]:self.tid_ptr[n + 1]]:
            n0, n1, n2 = (int(v) for v in self.tri[j])
            first = self.nbh[index][0]
            if first != n0 or first != n1 or first != n2:
                update = True
            for nk in (n0, n1, n2):
                if nk not in found:
                    N.append(nk)
                    found.add(nk)
        return update

    def WLS_simgradient(self, e1, e2, origin, y11, y21, index, querypoints):
        SUM = JPsim = 0.0
        two = 2 * self.min_sigma * self.min_sigma
        for q in querypoints:
            c = self.TARGET[q] - origin
            x11 = c[0] * e1[0] + c[1] * e1[1] + c[2] * e1[2]
            x21 = c[0] * e2[0] + c[1] * e2[1] + c[2] * e2[2]
            d1, d2 = x11 - y11, x21 - y21
            if d1 * d1 + d2 * d2 > 0:
                w = float(np.exp(-(d1 * d1 + d2 * d2) / two))
                SUM += w
                JPsim += self.mp.get((q, index), 0.0) * w
        if SUM > 0:
            JPsim /= SUM
        self.current_sim[index] = JPsim

    def rigid_cost_mesh(self, dw1, dw2, dw3):
        self.evaluations += 1
        tmp = self.SOURCE
        self.rotate_in_mesh(dw1, dw2, dw3)
        if self.fast:
            self._evaluate_fast()
        else:
            e1, e2, origin, y1, y2, closest = self._geometry()
            for i in range(len(self.SOURCE)):
                if len(self.nbh[i]) > 0:
                    querypoints, found, update = [], set(), False
                    ct = self.tri[closest[i]]
                    if self.get_all_neighbours(i, querypoints, int(ct[0]), found):
                        update = True
                    if self.get_all_neighbours(i, querypoints, int(ct[1]), found) or update:
                        update = True
                    if self.get_all_neighbours(i, querypoints, int(ct[2]), found) or update:
                        update = True
                    if update:
                        self.nbh[i] = querypoints
                        self.calculate_sim_column_nbh(i)
                    self.WLS_simgradient(e1[i], e2[i], origin[i], y1[i], y2[i], i, querypoints)
        SUM = 0.0
        for v in self.current_sim:
            SUM += v
        self.SOURCE = tmp
        return SUM

    # ---------------------------------------------------------------- fast mode
    def _build_query_lists(self):
        """get_all_neighbours of every target triangle (it depends on the closest triangle only), padded with -1"""
        lists = []
        for t in range(len(self.tri)):
            seen, out = set(), []
            for n in self.tri[t]:
                for j in self.tid[self.tid_ptr[n]:self.tid_ptr[n + 1]]:
                    for v in self.tri[j]:
                        if int(v) not in seen:
                            seen.add(int(v))
                            out.append(int(v))
            lists.append(out)
        W = max(len(x) for x in lists)
        self.qlist = np.full((len(lists), W), -1, dtype=np.int64)
        for t, x in enumerate(lists):
            self.qlist[t, :len(x)] = x

    def _sims(self, Q):
        """sim(q, i) for the V x W candidates Q (-1: padding), 0 where q == 0"""
        V = len(self.SOURCE)
        qi = np.where(Q >= 0, Q, 0)
        iv = np.broadcast_to(np.arange(V)[:, None], Q.shape)
        D = self.A.shape[0]
        if self.simmeasure == 1:
            prod = np.zeros(Q.shape)
            for d in range(D):
                diff = self.A[d][iv] - self.B[d][qi]
                prod = prod + diff * diff
            s = -(np.sqrt(prod) / D)
        else:
            ma, mb = self.rmeanA[iv], self.rmeanB[qi]
            prod, varA, varB = np.zeros(Q.shape), np.zeros(Q.shape), np.zeros(Q.shape)
            for d in range(D):
                a, b = self.A[d][iv] - ma, self.B[d][qi] - mb
                prod, varA, varB = prod + a * b, varA + a * a, varB + b * b
            with np.errstate(divide="ignore", invalid="ignore"):
                s = np.where((varA == 0.0) | (varB == 0.0), 0.0, prod / (np.sqrt(varA) * np.sqrt(varB)))
        return np.where(qi != 0, s, 0.0)

    def _evaluate_fast(self):
        e1, e2, origin, y1, y2, closest = self._geometry()
        Q = self.qlist[closest]
        S = self._sims(Q)
        two = 2 * self.min_sigma * self.min_sigma
        SUM, JP = np.zeros(len(Q)), np.zeros(len(Q))
        for k in range(Q.shape[1]):
            q = Q[:, k]
            c = self.TARGET[np.where(q >= 0, q, 0)] - origin
            d1 = _dot(c, e1) - y1
            d2 = _dot(c, e2) - y2
            dd = d1 * d1 + d2 * d2
            take = (q >= 0) & (dd > 0)
            w = np.exp(-dd / two)
            SUM = np.where(take, SUM + w, SUM)
            JP = np.where(take, JP + S[:, k] * w, JP)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.current_sim = np.where(SUM > 0, JP / SUM, JP)

    # ---------------------------------------------------------------- run
    def run(self, iters, stepsize, gradsampling):
        """run (:164-228); returns (SOURCE, trace rows {loop, iter, per, step, grad_zero, accepted}, dict(RECinit, RECfinal, evaluations))"""
        self.evaluations = 0
        Euler1 = Euler2 = Euler3 = 0.0
        RECfinal, min_iter, loop = 0.0, 0, 0
        spacing = gradsampling
        grad_zero = self.rigid_cost_mesh(Euler1, Euler2, Euler3)
        mingrad_zero = RECinit = grad_zero
        trace = []
        while spacing > 0.05:
            step, per = stepsize, spacing
            for it in range(1, iters + 1):
                Euler1 = Euler2 = Euler3 = 0.0
                g = np.array([[(self.rigid_cost_mesh(Euler1 + per, Euler2, Euler3) - grad_zero) / per,
                               (self.rigid_cost_mesh(Euler1, Euler2 + per, Euler3) - grad_zero) / per,
                               (self.rigid_cost_mesh(Euler1, Euler2, Euler3 + per) - grad_zero) / per]])
                g = _normalize(g)[0]
                Euler1 += step * g[0]
                Euler2 += step * g[1]
                Euler3 += step * g[2]
                taken = step
                tmp = self.SOURCE
                self.rotate_in_mesh(Euler1, Euler2, Euler3)
                grad_zero = self.rigid_cost_mesh(Euler1, Euler2, Euler3)
                if grad_zero > mingrad_zero:
                    mingrad_zero = grad_zero
                    min_iter = loop * iters + it
                    RECfinal = mingrad_zero
                rejected = loop * iters + it - min_iter > 0
                if rejected:
                    step *= 0.5
                    self.SOURCE = tmp
                trace.append([loop, it, per, taken, grad_zero, 0.0 if rejected else 1.0])
                if step < 1e-3:
                    break
            loop += 1
            spacing *= 0.5
        return self.SOURCE.copy(), np.array(trace).reshape(-1, 6), dict(RECinit=RECinit, RECfinal=RECfinal, evaluations=self.evaluations)


def rigid_level(target_xyz, tri, ref_feat, src_feat, sph_in, iters, simmeasure, stepsize, gradsampling, fast=True):
    """Mesh_registration's RIGID level over the literal: construct, initialise, update_source, run; returns (SOURCE, trace)"""
    r = RigidLiteral(target_xyz, tri, src_feat, ref_feat, simmeasure, fast=fast).initialise()
    r.update_source(sph_in)
    xyz, trace, _ = r.run(iters, stepsize, gradsampling)
    return xyz, trace


def rigid_inputs(order, D, seed):
    """an icosphere with D smooth input and reference feature rows (plus a little noise): the data of the rigid tests"""
    xyz, tri = O.icosphere(order)
    rng = np.random.default_rng(seed)
    u = xyz / 100.0
    A = np.stack([np.sin(3 * u[:, 0] + d) * np.cos(2 * u[:, 1]) + 0.5 * u[:, 2] * (d + 1) for d in range(D)]) + 0.05 * rng.normal(size=(D, len(xyz)))
    B = np.stack([np.sin(3 * u[:, 1] + d) + np.cos(4 * u[:, 2] - d) * u[:, 0] for d in range(D)]) + 0.05 * rng.normal(size=(D, len(xyz)))
    return xyz, tri, A, B
