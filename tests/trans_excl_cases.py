"""Shared by tests/test_trans_excl_cpu.py (the level loops over the oracle alone) and tests/test_gpu_trans_excl.py (the MI355X path against the
oracle): the oracle-backed ops with exclusion masks, the synthetic cases of --trans and --excl, and the run shapes both files check."""
import numpy as np

import newmsm_amd as M
from newmsm_amd import registration, synthetic

import rigid_literal as RL
from helpers import OracleOps
from oracle import oracle as O

CUTTHR = (0.0, 0.0001)  # --cutthr's default: the zero-valued medial wall
CAP_Z = 80.0            # vertices above z = 80 on the sphere of radius 100: a cap of (1 - 0.8) / 2 = 10 % of the surface


class MaskOracleOps(OracleOps):
    """OracleOps plus what the new options call: the mask arguments of featurespace::initialise's steps, create_exclusion, and the rigid level (from the
    literal restatement, as tests/test_gpu_rigid.py does)"""

    def metric_resample(self, in_mesh, data, new_mesh, slot=None, excl=None):
        if excl is None:
            return O.metric_resample(in_mesh, data, new_mesh)
        return O.metric_resample_excl(in_mesh, data, new_mesh, excl)

    def smooth_data(self, mesh, data, sigma, excl=None):
        return O.smooth_data(mesh, data, mesh, sigma, excl=excl)

    def variance_normalise(self, data, excl=None):
        return O.variance_normalise(data, excl=excl)

    def create_exclusion(self, data, thrl, thru):
        return O.create_exclusion(data, thrl, thru)

    def rigid_level(self, target_xyz, target_tri, ref_feat, source_xyz, source_tri, src_feat, sph_in, iters, simmeasure, stepsize, gradsampling):
        return RL.rigid_level(target_xyz, target_tri, ref_feat, src_feat, sph_in, iters, simmeasure, stepsize, gradsampling)


def oracle_ops():
    return MaskOracleOps(M.mcmc_optimise)


F32_001 = float(np.float32(0.01))  # --stepsize's default as the reference's float option holds it
DISCRETE_PAIR = [dict(data_order=3, cp_order=1, sigma_in=4.0, sigma_ref=4.0, iters=2, mciters=40),
                 dict(data_order=4, cp_order=2, sigma_in=2.0, sigma_ref=0.0, iters=2, mciters=40)]
RIGID_THEN_DISCRETE = [dict(method="RIGID", data_order=4, sigma_in=2.0, sigma_ref=2.0, iters=5, simmeasure=1, stepsize=F32_001, gradsampling=0.5),
                       dict(data_order=4, cp_order=2, sigma_in=2.0, sigma_ref=2.0, iters=2, mciters=40)]
RUN_KW = dict(varnorm=True, mcparam=0.3, seed=9, cost_params=dict(lambda_=0.05))


def pairwise_case(order=5, D=2, seed=31, cap=False):
    """input = reference sphere (ico<order>), the input data a displaced copy of the reference's pattern; cap: every feature of both data sets exactly
    0 above CAP_Z (the medial-wall case), on an irregular sphere (a smoothly warped icosphere) as a subject's native mesh is.  (A native mesh whose
    vertices coincide with a level grid's makes barycentric weights of exactly 0, and get_adaptive_barycentric_weights, R/resampler.cpp:72-140, then
    divides 0 by a scatter sum of 0 at the rim of the cut: NaN features in the reference, in the oracle and here -- test_gpu_trans_excl.py pins that
    separately.)  Returns (xyz, tri, src, ref, cap vertices)."""
    xyz, tri = M.make_mesh_from_icosa(order)
    if cap:
        xyz = synthetic.known_warp(xyz, seed=3, rot_deg=0.0, amp=0.7)
    ref = synthetic.features(xyz, D, seed)
    src = synthetic.features(synthetic.known_warp(xyz, seed=seed + 2, rot_deg=4.0, amp=2.5), D, seed)
    inside = xyz[:, 2] > CAP_Z
    if cap:
        ref[:, inside] = 0.0
        src[:, inside] = 0.0
    return xyz, tri, src, ref, inside


def run(ops, case, levels, labelings=None, **kw):
    xyz, tri, src, ref, _ = case
    kind = "multivariate" if src.shape[0] > 1 else "univariate"
    return registration.run_multiresolution(ops, xyz, tri, src, xyz, tri, ref, levels, labelings_out=labelings, kind=kind, **dict(RUN_KW, **kw))


def composition(ops, case, levels):
    """Check 1: A = one run over [L1, L2]; B1 = [L1] alone; B2 = [L2] alone started from B1's sphere.reg.  In A level 2 starts from the input sphere
    carried through level 1's warp, which is what B1 returns; B2's first level performs the same projections and unfolds.  Returns (A's result, A's
    labelings of level 2, B1's sphere.reg, B2's result, B2's labelings)."""
    lab_a, lab_1, lab_b = [], [], []
    a = run(ops, case, levels, lab_a)
    b1 = run(ops, case, levels[:1], lab_1)
    b2 = run(ops, case, levels[1:], lab_b, trans_xyz=b1[0])
    return a, lab_a[len(lab_1):], b1[0], b2, lab_b


def assert_composition(a, lab_a2, b2, lab_b):
    assert len(lab_b) == len(lab_a2) > 0 and all(np.array_equal(x, y) for x, y in zip(lab_a2, lab_b))
    assert np.array_equal(b2[0], a[0])               # sphere.reg: the same calls on the same inputs, no tolerance
    assert np.array_equal(b2[1][0], a[1][-1])        # the level's registered data grid
    assert np.array_equal(np.asarray(b2[2][0]), np.asarray(a[2][-1]))


def level_features(ops, case, levels, excl):
    """what run_multiresolution prepares per level and data set: [(features, mask), ...] in the loop's order (input, reference; level after level)"""
    xyz, tri, src, ref, _ = case

    def timed(name, fn, *a):
        return fn(*a)

    out = []
    meshes = [ops.mesh(xyz, tri), ops.mesh(xyz, tri)]
    for lv in levels:
        ico = ops.mesh(*ops.icosphere(lv["data_order"]))
        for mesh, data, sigma in ((meshes[0], src, lv["sigma_in"]), (meshes[1], ref, lv["sigma_ref"])):
            out.append(registration.level_features(ops, timed, mesh, data, ico, sigma, True, None, excl, CUTTHR))
    return out


def group_case(cap=True):
    """three subjects on irregular ico4 spheres of their own, an irregular template (the shape of tests/test_gpu_group.py's multiresolution test);
    cap: every subject's data exactly 0 above CAP_Z of its own sphere"""
    S, D = 3, 2
    xyz, tri = M.make_mesh_from_icosa(4)
    txyz = synthetic.known_warp(xyz, seed=33, rot_deg=7.0, amp=1.5)
    meshes = [(synthetic.known_warp(xyz, seed=40 + s, rot_deg=0.0, amp=1.0), tri) for s in range(S)]
    datas = [synthetic.features(synthetic.known_warp(meshes[s][0], seed=90 + s, rot_deg=3.0, amp=2.0), D, seed=5) for s in range(S)]
    caps = [meshes[s][0][:, 2] > CAP_Z for s in range(S)]
    if cap:
        for s in range(S):
            datas[s][:, caps[s]] = 0.0
    levels = [dict(data_order=3, cp_order=1, sg_order=3, iters=2, simmeasure=2, cost_params=dict(lambda_=1e-3), sigma_in=2.0),
              dict(data_order=4, cp_order=2, sg_order=4, iters=2, simmeasure=2, cost_params=dict(lambda_=1e-3), sigma_in=0.0)]
    mask = (np.random.default_rng(1).random(len(xyz)) > 0.2).astype(np.float64)
    return meshes, datas, txyz, tri, levels, mask, caps
