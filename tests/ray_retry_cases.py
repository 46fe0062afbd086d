"""Cases of the tests of what k_unary_rays does behind a first-candidate miss (csrc/unary_kernels.hip: round A, round T and the reload): warped targets, whose cells hold
the answer at every position of their candidate lists (tests/test_ray_depth_cpu.py has the counts), under control grids that give patches of a few
points, of about 65 and of several hundred."""
import numpy as np

import newmsm_amd as M
from newmsm_amd import problem, synthetic

TARGETS = ["ico4", "ico4_warped", "ico3_strongly_warped"]
# (target, control grid order): ico4 / ico2 -- patches of about 65 points, partial last wavefront rounds; ico3 / ico3 -- about 7 points, most lanes of a
# wavefront without a sample in the team round; ico4 / ico1 -- several hundred points
GRIDS = [("ico4_warped", 2), ("ico3_strongly_warped", 3), ("ico4_warped", 1)]


def mesh(name):
    """the meshes of tests/test_ray_table_signature_cpu.py, built as it builds them"""
    xyz, tri = M.make_mesh_from_icosa(int(name[3]))
    if name.endswith("strongly_warped"):
        xyz = synthetic.known_warp(xyz, seed=5, rot_deg=5.0, amp=6.0)
    elif name.endswith("warped"):
        xyz = synthetic.known_warp(xyz, seed=3, rot_deg=5.0, amp=2.0)
    return xyz, tri


def inputs(target, cp_order, D=1):
    """problem.pairwise_inputs on the target's data grid, with the named mesh for target and the features on its vertices"""
    inp = problem.pairwise_inputs(int(target[3]), cp_order, D=D)
    xyz, tri = mesh(target)
    assert np.array_equal(tri, inp["target_tri"])
    return dict(inp, target_xyz=xyz, ref_feat=synthetic.features(xyz, D, 1234))
