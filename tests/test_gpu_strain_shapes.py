"""msm_calculate_strains (vertex_strain_kernels.hip, vertex_strains.cpp) on the cases of tests/strain_shape_cases.py: members exactly at the
radius, exactly perpendicular normals, one-cell axes, one cell, uncoarsened grids with many vertices per cell, the `full` box and fit radii from
0.05 to 500.  The member count and the final radius of every vertex are the restatement's exactly; the strains are within the tolerance of
tests/test_gpu_strains.py without its condition-number allowance (tests/test_strain_shapes_cpu.py: the largest condition number is 262); on
the lattice they are also the singular values of the map itself, which asks nothing of the restatement."""
import time

import numpy as np
import pytest

import newmsm_amd as M
from tests import strain_shape_cases as SC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", SC.NAMES)
def test_matches_restatement(ctx, name):
    case = SC.BY_NAME[name]
    orig, tri, final = SC.inputs(name)
    want = SC.reference(name)
    t0 = time.perf_counter()
    got, kept, radius, _ = SC.compare(ctx, orig, tri, final, max_ill=0, fit_radius=case.fit_radius, want=want)
    print("%s: V %d, %.3f s on the device, largest difference %.3e" % (name, len(orig), time.perf_counter() - t0, np.abs(got - want["strains"]).max()))
    assert np.all(kept > 8) and np.all(np.isfinite(got))
    if case.kind == "lattice":
        np.testing.assert_allclose(got, np.broadcast_to(SC.stretches_of_the_map()[:, None], got.shape), rtol=1e-9)


@pytest.mark.parametrize("name", [c.name for c in SC.CASES if c.twice])
def test_two_calls_same_bits(ctx, name):
    """64 vertices per cell, the whole mesh in one cell, full 3 x 3 x 3 boxes: k_grid_sort undoes whatever order the atomics of k_grid_scatter left"""
    orig, tri, final = SC.inputs(name)
    mesh = M.Mesh(ctx, orig, tri)
    a = M.calculate_strains(mesh, final, SC.BY_NAME[name].fit_radius, with_neighbourhoods=True)
    b = M.calculate_strains(mesh, final, SC.BY_NAME[name].fit_radius, with_neighbourhoods=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
