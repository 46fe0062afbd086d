"""Where in a direction cell's candidate list the answer sits, in the order the kernels try the candidates, through the testing hook msm_ray_depth_check
(no GPU needed).  k_unary_rays settles a first-candidate miss in two rounds (csrc/unary_kernels.hip: k_unary_rays): round A takes position 1, the team
round positions 2 to 6.  The bounds below are the condition under which tests/test_gpu_unary_retries.py reaches every branch of both rounds on these
meshes; measured with 200 000 directions, seed 7: at least 13 165 / 2 216 / 2 089 / 1 187 / 733 points at positions 1, 2, 3, 4 and 5 or beyond."""
import pytest

import newmsm_amd as M
from newmsm_amd import api
from ray_retry_cases import TARGETS, mesh


@pytest.fixture(scope="module")
def reports(built):
    return {name: api.ray_depth_check(*mesh(name), nsamples=200000, seed=7) for name in TARGETS}


@pytest.mark.parametrize("name", TARGETS)
def test_every_position_of_the_list_is_reached(reports, name):
    rep = reports[name]
    print(name, rep)
    assert rep["points"] == 200000
    assert sum(rep["at"]) == rep["points"]  # every point has a triangle, and its cell lists it
    assert rep["unlisted"] == 0
    assert rep["at"][0] > 0.85 * rep["points"]  # the hinted first candidate (tests/test_ray_hints_cpu.py holds it to its own bar)
    for position in range(1, 6):
        assert rep["at"][position] >= 500, (position, rep["at"])


def test_ico6_has_the_recorded_distribution(built):
    """the mesh of the benchmark: the shares DESIGN.md section 5.2 sizes the two rounds with"""
    rep = api.ray_depth_check(*M.make_mesh_from_icosa(6), nsamples=200000, seed=7)
    print(rep)
    assert rep["points"] == 200000 and rep["unlisted"] == 0
    assert rep["at"] == [180557, 13296, 2229, 2014, 1188, 716]
