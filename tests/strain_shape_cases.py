"""Inputs on which the strain map's neighbourhoods are decided at their edges, and the comparison of the device with the restatement
(tests/test_strain_shapes_cpu.py pins the restatement's side and shows that each case discriminates, tests/test_gpu_strain_shapes.py compares
msm_calculate_strains; tests/test_gpu_strains.py uses compare() too).

The smooth anatomies of tests/test_gpu_strains.py at fit radius 2.0 never put a vertex exactly at the radius, never make two normals exactly
perpendicular, always coarsen the grid and always give it many cells per axis.  Here:

    lattice(n, spacing)   the unjittered plane: distances are exact multiples of the spacing, so members lie exactly at the radius (`<=` against
                          `<`), the 9th smallest distance equals the radius (`d9 <= r`), every vertex lies on a cell boundary and nz == 1
    box(n, spacing)       a cube's surface: face-interior normals are exactly +-e_k, so normals of adjacent faces have the product 0.0 (`>= 0`
                          against `> 0`)
    anatomy_case          the smooth anatomy at fit radii from 0.05 (radius doublings, dozens of 0.5 steps) to 500 (one cell, the `full` box on
                          the first round, over a thousand QR rows), on meshes of 42 and 162 vertices (over a hundred 0.5 steps; the `full` box by doubling and, at fit radius 62.5, with the 9th member beyond R), divided by 6
                          (the uncoarsened grid with full 3 x 3 x 3 boxes) and far from the origin (the margin of box_of)

Everything but compare() is numpy and the restatement; the product's objects are built by compare() from a context."""
import collections
import functools

import numpy as np

import newmsm_amd as M
import strains_literal as SL
from newmsm_amd import synthetic
from oracle import oracle as O

ILL = 1e6  # a 5-column block above this condition number is compared at a tolerance scaled by it
A = np.array([[1.3, 0.2, 0.0], [-0.1, 0.8, 0.0], [0.25, -0.15, 1.0]])  # the map of test_planar_patch_under_a_linear_map


def anatomy_case(order, seed=0):
    """a synthetic anatomy on icosphere(order) and the same anatomy after a known warp of the sphere"""
    xyz, tri = O.icosphere(order)
    orig = synthetic.anatomy(xyz, seed=seed)
    final = synthetic.anatomy(synthetic.known_warp(xyz, seed=seed + 5, rot_deg=2.0, amp=1.5), seed=seed)
    return orig, tri, final


def lattice(n, spacing):
    """the n x n patch of the plane z = 0, triangulated as strains_literal.jittered_plane triangulates it, without the jitter"""
    xyz, tri = SL.jittered_plane(n, spacing=spacing, jitter=0.0)
    return xyz + 0.0, tri  # (-0.0 from the zero jitter becomes +0.0)


def box(n, spacing):
    """the closed surface of a cube of n cells per edge, centred on the origin: the vertices of the six faces merged on their integer keys, every
    triangle wound the same way round the outward direction"""
    ids, tri = {}, []

    def vid(key):
        return ids.setdefault(key, len(ids))

    for k in range(3):
        u, v = (k + 1) % 3, (k + 2) % 3
        for side in (0, n):
            for a in range(n):
                for b in range(n):
                    def at(da, db):
                        key = [0, 0, 0]
                        key[k], key[u], key[v] = side, a + da, b + db
                        return vid(tuple(key))

                    quad = [[at(0, 0), at(1, 0), at(0, 1)], [at(1, 0), at(1, 1), at(0, 1)]]  # (v1 - v0) x (v2 - v0) = +e_k
                    tri += quad if side else [t[::-1] for t in quad]
    keys = np.array(sorted(ids, key=ids.get), dtype=np.float64)
    return (keys - 0.5 * n) * spacing, np.asarray(tri, dtype=np.int32)


def grid_of(xyz, fit_radius):
    """grid_of of vertex_strains.cpp: (nx, ny, nz, h, C, the number of times h was coarsened)"""
    xyz = np.asarray(xyz, dtype=np.float64)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    cap = 4.0 * len(xyz) + 1024.0
    h, times = float(fit_radius), 0
    while True:
        n = np.floor((hi - lo) / h) + 1
        if n[0] * n[1] * n[2] <= cap:
            break
        h *= 1.5
        times += 1
    nx, ny, nz = (int(v) for v in n)
    return nx, ny, nz, h, nx * ny * nz, times


# kind: "lattice" and "box" are small enough for the literal mode and the O(V^2) counts.  grid: (nx, ny, nz, times coarsened).  kept, radius:
# (smallest, largest) of the restatement.  ties: (members exactly at the final radius, vertices with d9 == radius, (vertex, member) pairs with
# n . n == 0.0), lattice and box only.  twice: two calls are compared byte for byte on the device.
Case = collections.namedtuple("Case", "name kind build fit_radius grid kept radius ties twice")


def _linear(builder, *args):
    xyz, tri = builder(*args)
    return xyz, tri, xyz @ A.T


def _anatomy(order, divide=1.0, shift=(0.0, 0.0, 0.0)):
    orig, tri, final = anatomy_case(order, seed=order)
    shift = np.asarray(shift, dtype=np.float64)
    return orig / divide + shift, tri, final / divide + shift


def _case(name, kind, builder, args, fit_radius, grid, kept, radius, ties=None, twice=False):
    return Case(name, kind, functools.partial(builder, *args), fit_radius, grid, kept, radius, ties, twice)


CASES = [
    _case("lattice24_r0.5", "lattice", _linear, (lattice, 24, 0.5), 0.5, (24, 24, 1, 0), (9, 14), (1.0, 1.5), (2112, 80, 0)),
    _case("lattice24_r2", "lattice", _linear, (lattice, 24, 0.5), 2.0, (6, 6, 1, 0), (17, 49), (2.0, 2.0), (1920, 0, 0)),
    _case("lattice24_r2.5", "lattice", _linear, (lattice, 24, 0.5), 2.5, (5, 5, 1, 0), (26, 81), (2.5, 2.5), (5184, 0, 0)),
    _case("lattice40_r1", "lattice", _linear, (lattice, 40, 0.125), 1.0, (5, 5, 1, 0), (58, 197), (1.0, 1.0), (5120, 0, 0), twice=True),
    _case("box12_r2", "box", _linear, (box, 12, 0.5), 2.0, (4, 4, 4, 0), (37, 64), (2.0, 2.0), (2592, 0, 10512)),
    _case("box12_r1", "box", _linear, (box, 12, 0.5), 1.0, (7, 7, 7, 0), (10, 16), (1.0, 1.0), (3168, 8, 792)),
    _case("ico4_r0.05", "anatomy", _anatomy, (4,), 0.05, (22, 19, 20, 12), (9, 15), (5.55, 10.55)),
    _case("ico4_r0.75", "anatomy", _anatomy, (4,), 0.75, (17, 14, 15, 6), (9, 14), (5.75, 10.25)),
    _case("ico4_r7.3", "anatomy", _anatomy, (4,), 7.3, (19, 17, 18, 0), (9, 18), (7.3, 10.3)),
    _case("ico4_r40", "anatomy", _anatomy, (4,), 40.0, (4, 3, 4, 0), (196, 366), (40.0, 40.0)),
    _case("ico4_r500", "anatomy", _anatomy, (4,), 500.0, (1, 1, 1, 0), (1100, 1455), (500.0, 500.0), twice=True),
    _case("ico1_r2", "anatomy", _anatomy, (1,), 2.0, (9, 8, 9, 5), (9, 11), (52.0, 66.0)),
    _case("ico1_r62.5", "anatomy", _anatomy, (1,), 62.5, (2, 2, 2, 0), (9, 15), (62.5, 66.0)),
    _case("ico2_r2", "anatomy", _anatomy, (2,), 2.0, (9, 9, 9, 5), (9, 12), (25.0, 36.0)),
    _case("ico5_div6_r2", "anatomy", _anatomy, (5, 6.0), 2.0, (11, 11, 11, 0), (54, 161), (2.0, 2.0), twice=True),
    _case("ico4_shifted_r2", "anatomy", _anatomy, (4, 1.0, (5000.0, -3000.0, 800.0)), 2.0, (21, 18, 19, 3), (9, 15), (5.5, 10.5)),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(orig, tri, final) of a case: left unchanged by everyone who asks"""
    got = BY_NAME[name].build()
    for x in got:
        x.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's fast mode on a case, computed once: left unchanged by everyone who asks"""
    orig, tri, final = inputs(name)
    want = SL.calculate_strains(orig, tri, final, BY_NAME[name].fit_radius)
    for k in ("strains", "kept", "radius", "cond"):
        want[k].setflags(write=False)
    return want


def pair_tables(orig, tri):
    """(D, P): the distance and the normal product of every pair of vertices, by the restatement's own arithmetic (row i is what its literal loop
    computes for vertex i)"""
    nrm = SL.estimate_normals(orig, tri)
    return SL._norm_rows(orig[:, None, :] - orig[None, :, :]), SL._dot_rows(nrm[None, :, :], nrm[:, None, :])


def radius_rounds(orig, tri, fit_radius):
    """the rounds of k_strain_radius for every vertex, from box_of and axis_cell restated: (times R was doubled, whether the last box was the whole
    grid, members of that round that lie beyond its R).  A box that is not the whole grid still holds every vertex within R, so a round's count is
    that of the exact tests at R."""
    nx, ny, nz, h, _, _ = grid_of(orig, fit_radius)
    n, x0, inv_h = np.array([nx, ny, nz]), orig.min(axis=0), 1.0 / h
    D, P = pair_tables(orig, tri)

    def cells(x):
        f = np.floor((x - x0) * inv_h)
        return np.where(f > 0.0, np.minimum(f, n - 1), 0.0)

    doubled, full, beyond = np.zeros(len(orig), dtype=int), np.zeros(len(orig), dtype=bool), np.zeros(len(orig), dtype=int)
    for i, p in enumerate(orig):
        R = fit_radius
        while True:
            w = R + 1e-9 * (np.abs(p) + R)
            full[i] = np.all(cells(p - w) == 0) and np.all(cells(p + w) == n - 1)
            sel = (P[i] >= 0) & (full[i] | (D[i] <= R))
            if sel.sum() >= 9 or full[i]:
                break
            R *= 2.0
            doubled[i] += 1
        beyond[i] = np.count_nonzero(sel & (D[i] > R))
    return doubled, full, beyond


def stretches_of_the_map():
    """the four rows every vertex of a plane mapped by A has: the singular values of A on the plane and 0.5 (s^2 - 1) of each"""
    sv = np.linalg.svd(A[:, :2], compute_uv=False)
    return np.array([sv[0], sv[1], 0.5 * (sv[0] ** 2 - 1), 0.5 * (sv[1] ** 2 - 1)])


def assert_same(a, b, rtol=1e-12, atol=1e-14):
    """two results of the restatement (its literal and its fast mode): the same neighbourhoods, member by member, and the same strains"""
    assert np.array_equal(a["kept"], b["kept"])
    assert np.array_equal(a["radius"], b["radius"])
    for x, y in zip(a["members"], b["members"]):
        assert np.array_equal(x, y)
    np.testing.assert_allclose(a["strains"], b["strains"], rtol=rtol, atol=atol)


def compare(ctx, orig, tri, final, max_ill=0.02, fit_radius=2.0, want=None):
    """the device against the restatement: neighbourhoods equal, strains to rtol 1e-9 / atol 1e-12 (scaled by the condition number above ILL)"""
    got, kept, radius = M.calculate_strains(M.Mesh(ctx, orig, tri), final, fit_radius, with_neighbourhoods=True)
    if want is None:
        want = SL.calculate_strains(orig, tri, final, fit_radius)
    assert np.array_equal(kept, want["kept"])
    assert np.array_equal(radius, want["radius"])
    cond = want["cond"]
    ill = cond > ILL
    assert np.count_nonzero(ill) <= max_ill * len(orig)
    scale = np.where(ill, cond / ILL, 1.0)
    err = np.abs(got - want["strains"])
    assert np.all(err <= 1e-12 * scale + 1e-9 * scale * np.abs(want["strains"])), (err.max(), cond.max())
    return got, kept, radius, want
