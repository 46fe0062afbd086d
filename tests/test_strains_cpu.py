"""The strain map of an aMSM run without a GPU: the literal restatement of calculate_strains (tests/strains_literal.py) -- its fast mode against
its literal mode, analytic cases, the radius growth, the normal test and the flip of calculate_tangs -- and the C ABI's new entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import newmsm_amd as M
import strains_literal as SL
from newmsm_amd import _lib
from oracle import oracle as O
from tests.strain_shape_cases import anatomy_case, assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", [2, 3])
def test_fast_mode_matches_literal(order):
    orig, tri, final = anatomy_case(order, seed=order)
    assert_same(SL.calculate_strains(orig, tri, final, literal=True), SL.calculate_strains(orig, tri, final))


def test_fast_mode_matches_literal_ellipsoid_and_flips():
    xyz, tri = SL.flattened_ellipsoid(3)
    final = xyz * np.array([1.1, 0.95, 1.0])
    assert_same(SL.calculate_strains(xyz, tri, final, literal=True), SL.calculate_strains(xyz, tri, final))
    orig, tri, final = anatomy_case(2, seed=4)
    shift = np.array([150.0, -20.0, 10.0])
    assert_same(SL.calculate_strains(orig + shift, tri, final + shift, literal=True), SL.calculate_strains(orig + shift, tri, final + shift))
    rev = tri[:, ::-1].copy()
    assert_same(SL.calculate_strains(orig, rev, final, literal=True), SL.calculate_strains(orig, rev, final))


def test_identity_gives_unit_stretch():
    orig, tri, _ = anatomy_case(4, seed=1)
    s = SL.calculate_strains(orig, tri, orig)["strains"]
    np.testing.assert_allclose(s[:2], 1.0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(s[2:], 0.0, rtol=0, atol=1e-9)


@pytest.mark.parametrize("scale", [0.8, 1.25])
def test_uniform_scaling(scale):
    orig, tri, _ = anatomy_case(4, seed=2)
    s = SL.calculate_strains(orig, tri, orig * scale)["strains"]
    np.testing.assert_allclose(s[:2], scale, rtol=1e-9, atol=0)
    np.testing.assert_allclose(s[2:], 0.5 * (scale * scale - 1), rtol=1e-9, atol=1e-12)


def test_planar_patch_under_a_linear_map():
    """a jittered plane mapped by A: every vertex's stretches are the singular values of A on the plane"""
    xyz, tri = SL.jittered_plane(14, spacing=0.7, seed=3)
    A = np.array([[1.3, 0.2, 0.0], [-0.1, 0.8, 0.0], [0.25, -0.15, 1.0]])
    r = SL.calculate_strains(xyz, tri, xyz @ A.T)
    sv = np.linalg.svd(A[:, :2], compute_uv=False)
    np.testing.assert_allclose(r["strains"][0], sv[0], rtol=1e-9)
    np.testing.assert_allclose(r["strains"][1], sv[1], rtol=1e-9)
    np.testing.assert_allclose(r["strains"][2], 0.5 * (sv[0] ** 2 - 1), rtol=1e-9)
    np.testing.assert_allclose(r["strains"][3], 0.5 * (sv[1] ** 2 - 1), rtol=1e-9)


def test_radius_grows_on_a_coarse_mesh():
    orig, tri, final = anatomy_case(3)
    r = SL.calculate_strains(orig, tri, final)
    assert np.all(r["radius"] > 2.0) and np.all(r["kept"] > 8)
    steps = (r["radius"] - 2.0) / 0.5
    assert np.allclose(steps, np.round(steps), atol=1e-9)
    # one step less would have left 8 or fewer members
    nrm = SL.estimate_normals(orig, tri)
    for i in range(0, len(orig), 37):
        d = np.sqrt(((orig[i] - orig) ** 2).sum(1))
        ok = (nrm @ nrm[i]) >= 0
        assert np.count_nonzero(ok & (d <= r["radius"][i] - 0.5)) <= 8


def test_normal_test_drops_the_opposite_sheet():
    """a flattened ellipsoid (semi-axes 30, 30, 1 mm): within 2 mm of a vertex near the middle lie vertices of the other sheet, none is kept"""
    xyz, tri = SL.flattened_ellipsoid(4)
    r = SL.calculate_strains(xyz, tri, xyz * np.array([1.05, 1.0, 1.0]))
    nrm = SL.estimate_normals(xyz, tri)
    dropped = 0
    for i in np.nonzero(np.hypot(xyz[:, 0], xyz[:, 1]) < 15)[0]:
        d = np.sqrt(((xyz[i] - xyz) ** 2).sum(1))
        near = np.nonzero(d <= r["radius"][i])[0]
        other = near[np.sign(xyz[near, 2]) != np.sign(xyz[i, 2])]
        dropped += len(other)
        assert not set(other) & set(r["members"][i].tolist())
        assert np.all(nrm[r["members"][i]] @ nrm[i] >= 0)
    assert dropped > 0


def test_flip_of_calculate_tangs():
    """anatomy translated off the origin (a . x_i < 0 at some vertices only) and reversed winding (every normal turned over): calculate_tangs flips
    the local normal where it points away from the vertex, and the stretches stay those of the centred mesh"""
    orig, tri, final = anatomy_case(4, seed=6)
    base = SL.calculate_strains(orig, tri, final)
    shift = np.array([0.0, 90.0, 0.0])
    nrm = SL.estimate_normals(orig + shift, tri)
    assert 0 < np.count_nonzero(np.einsum("ij,ij->i", nrm, orig + shift) < 0) < len(orig)
    moved = SL.calculate_strains(orig + shift, tri, final + shift)
    assert np.array_equal(moved["kept"], base["kept"])
    np.testing.assert_allclose(moved["strains"], base["strains"], rtol=1e-8, atol=1e-10)
    rev = tri[:, ::-1].copy()
    side = np.einsum("ij,ij->i", SL.estimate_normals(orig, tri), orig)
    assert np.all(np.sign(np.einsum("ij,ij->i", SL.estimate_normals(orig, rev), orig)) == -np.sign(side)) and np.all(side != 0)
    flipped = SL.calculate_strains(orig, rev, final)
    assert np.array_equal(flipped["kept"], base["kept"])
    np.testing.assert_allclose(flipped["strains"], base["strains"], rtol=1e-8, atol=1e-10)


def test_never_nine_is_refused():
    xyz, tri = O.icosphere(0)
    with pytest.raises(SL.NeverNine):
        SL.calculate_strains(xyz, tri, xyz, literal=True)
    with pytest.raises(SL.NeverNine):
        SL.calculate_strains(xyz, tri, xyz)


def test_calculate_strains_is_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msmhip.h")).read(), flags=re.S)
    assert re.search(r"\bint msm_calculate_strains\s*\(", text)
    assert hasattr(M.lib(), "msm_calculate_strains")
    assert "msm_calculate_strains" in _lib.SIGNATURES
    assert callable(M.calculate_strains) and callable(M.project_anatomical_mesh)
    hpp = open(os.path.join(ROOT, "include", "msmhip.hpp")).read()
    assert "inline Matrix calculate_strains(" in hpp and "inline Points project_anatomical_mesh(" in hpp
    # argument checks come before any device work
    out = np.zeros(4)
    assert M.lib().msm_calculate_strains(None, out.ctypes.data_as(_lib.c_dp), 1, C.c_double(2.0), out.ctypes.data_as(_lib.c_dp), None, None) == -1
