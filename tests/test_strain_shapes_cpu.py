"""The cases of tests/strain_shape_cases.py without a GPU: the restatement (tests/strains_literal.py) answers every one of them with a
well-conditioned fit, the grid the device will build has the shape each case is there for, and -- on the lattice and the box, by plain numpy over
all pairs -- members do lie exactly at the radius, the 9th smallest distance does equal it, normals are exactly perpendicular, and a `<` for the
`<=` or a `> 0` for the `>= 0` counts another neighbourhood.  tests/test_gpu_strain_shapes.py asks the device for the restatement's `kept` and
`radius` exactly, so a kernel with one of those comparisons wrong cannot pass it."""
import numpy as np
import pytest

import strains_literal as SL
from tests import strain_shape_cases as SC

SMALL = [c.name for c in SC.CASES if c.kind != "anatomy"]
LATTICES = [c.name for c in SC.CASES if c.kind == "lattice"]
kScanThreads = 1024  # vertex_strain_kernels.hip


@pytest.mark.parametrize("name", SC.NAMES)
def test_restatement_answers_the_case(name):
    case = SC.BY_NAME[name]
    orig, _, _ = SC.inputs(name)
    want = SC.reference(name)  # raises NeverNine where a vertex can never have 9 members
    assert want["kept"].min() >= 9
    assert np.all(np.isfinite(want["strains"]))
    assert want["cond"].max() < SC.ILL
    assert (want["kept"].min(), want["kept"].max()) == case.kept
    np.testing.assert_allclose([want["radius"].min(), want["radius"].max()], case.radius, rtol=1e-12)
    nx, ny, nz, h, C, times = SC.grid_of(orig, case.fit_radius)
    assert (nx, ny, nz, times) == case.grid
    assert C == nx * ny * nz and (h == case.fit_radius) == (times == 0)


def test_grid_shapes_the_cases_are_there_for():
    shape = {c.name: SC.grid_of(SC.inputs(c.name)[0], c.fit_radius) for c in SC.CASES}
    assert all(shape[n][2] == 1 for n in LATTICES)  # a one-cell axis
    assert shape["ico4_r500"][4] == 1  # one cell
    assert 1 < shape["lattice40_r1"][4] < kScanThreads and 1 < shape["ico4_r40"][4] < kScanThreads and shape["ico5_div6_r2"][4] > kScanThreads
    assert shape["ico4_r0.05"][4] > kScanThreads  # k_grid_scan with per > 1 and with per == 1
    # one vertex per cell, each on its cell's boundary; 64 and about 8 vertices per cell on uncoarsened grids
    orig = SC.inputs("lattice24_r0.5")[0]
    assert len(orig) == shape["lattice24_r0.5"][4] and np.array_equal(orig[:, :2] / 0.5, np.round(orig[:, :2] / 0.5))
    assert len(SC.inputs("lattice40_r1")[0]) == 64 * shape["lattice40_r1"][4]
    assert len(SC.inputs("ico5_div6_r2")[0]) > 7 * shape["ico5_div6_r2"][4]
    # the radius is no multiple of 0.5 and lies dozens of steps above the fit radius
    r = SC.reference("ico4_r0.05")["radius"]
    assert np.all(np.round(r / 0.5) * 0.5 != r) and r.min() > 0.05 + 10 * 0.5
    assert (SC.reference("ico1_r2")["radius"].min() - 2.0) / 0.5 >= 100


def test_whole_grid_boxes_are_reached():
    """where k_strain_radius meets a box that is the whole grid: on the first round at every vertex (one cell; 2 x 2 x 2 cells), after six doublings
    at one vertex of the 42; and where it then needs the members it accepts beyond that round's R -- four of the 42 vertices at fit radius 62.5
    have fewer than 9 members within it, so their d9 and their radius come from farther away (without `full ||` they would be refused)"""
    def rounds(name):
        orig, tri, _ = SC.inputs(name)
        return SC.radius_rounds(orig, tri, SC.BY_NAME[name].fit_radius)

    doubled, full, _ = rounds("ico4_r500")
    assert np.all(full) and np.all(doubled == 0)
    doubled, full, beyond = rounds("ico1_r62.5")
    assert np.all(full) and np.all(doubled == 0) and np.all(beyond > 0)
    assert np.count_nonzero(SC.reference("ico1_r62.5")["radius"] > 62.5) == 4
    doubled, full, _ = rounds("ico1_r2")
    assert np.count_nonzero(full) == 1 and doubled[full] == 6 and np.all(doubled >= 5)
    doubled, full, _ = rounds("ico2_r2")  # (no box of the 162 is the whole grid: at most 5 doublings, R = 64)
    assert not np.any(full) and np.all(doubled >= 4)


@pytest.mark.parametrize("name", SMALL)
def test_literal_mode_gives_the_same(name):
    orig, tri, final = SC.inputs(name)
    SC.assert_same(SL.calculate_strains(orig, tri, final, SC.BY_NAME[name].fit_radius, literal=True), SC.reference(name))


@pytest.mark.parametrize("name", SMALL)
def test_case_discriminates(name):
    case = SC.BY_NAME[name]
    orig, tri, _ = SC.inputs(name)
    want = SC.reference(name)
    D, P = SC.pair_tables(orig, tri)
    r = want["radius"][:, None]
    faces = P >= 0
    assert np.array_equal(((D <= r) & faces).sum(axis=1), want["kept"])
    at_radius = int(((D == r) & faces).sum())
    d9 = np.sort(np.where(faces, D, np.inf), axis=1)[:, 8]
    d9_at_radius = int((d9 == want["radius"]).sum())
    perpendicular = int(((D <= r) & (P == 0.0)).sum())
    print("%s: %d members at the radius, %d vertices with d9 == radius, %d perpendicular members" % (name, at_radius, d9_at_radius, perpendicular))
    assert (at_radius, d9_at_radius, perpendicular) == case.ties
    assert at_radius > 0
    assert np.any(((D < r) & faces).sum(axis=1) != want["kept"])  # `<` for `<=` in the distance test
    if case.kind == "box":
        assert perpendicular > 0
        assert np.any(((D <= r) & (P > 0)).sum(axis=1) != want["kept"])  # `> 0` for `>= 0` in the normal test
    if d9_at_radius:
        # `d9 < r` for `d9 <= r` in the radius loop: one more step
        assert np.any(np.array([SL.final_radius(np.nextafter(d, np.inf), case.fit_radius) for d in d9]) != want["radius"])


@pytest.mark.parametrize("name", LATTICES)
def test_lattice_stretches_are_the_maps(name):
    """every vertex of the plane mapped by A has the singular values of A on the plane"""
    got = SC.reference(name)["strains"]
    np.testing.assert_allclose(got, np.broadcast_to(SC.stretches_of_the_map()[:, None], got.shape), rtol=1e-9)
