"""The rigid level on the MI355X (msm_rigid_*, rigid_kernels.hip) against the literal restatement of Rigid_cost_function (tests/rigid_literal.py):
single evaluations, whole runs, the level inside run_multiresolution and both executables with MSMHIP_RIGID=on."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
import rigid_literal as RL
from helpers import OracleOps, angles
from newmsm_amd import registration, synthetic
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_001 = float(np.float32(0.01))
EULERS = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.5], [0.01, -0.02, 0.03], [-0.2, 0.1, 0.05]])


def _inputs(order, D, seed):
    xyz, tri = O.icosphere(order)
    ref = synthetic.features(xyz, D, seed)
    src = synthetic.features(synthetic.known_warp(xyz, seed=seed + 1, rot_deg=4.0, amp=1.0), D, seed)
    return xyz, tri, src, ref


def _product(ctx, xyz, tri, src, ref, sim):
    mesh = M.Mesh(ctx, xyz, tri)
    return M.RigidCostFunction(ctx, mesh, mesh, src, ref, simmeasure=sim).initialise(), mesh


@pytest.mark.parametrize("order", [4, 5])
@pytest.mark.parametrize("D,sim", [(1, 1), (1, 2), (3, 1), (3, 2)])
def test_cost_matches_literal(ctx, order, D, sim):
    """rigid_cost_mesh for several Euler triples (0, the gradsampling probes, small and large rotations) of a rotated SOURCE: sums to rtol 1e-12, every
    vertex's value to 1e-12 -- the vertices around target vertex 0 included, whose similarity is never set (0) while its weight counts"""
    xyz, tri, src, ref = _inputs(order, D, 3 + D)
    start = RL.euler_rotate(xyz, 0.03, -0.02, 0.04)
    lit = RL.RigidLiteral(xyz, tri, src, ref, sim, fast=order > 4).initialise()  # the literal mode at ico4; its fast mode (tested equal) at ico5
    lit.update_source(start)
    rcf, _ = _product(ctx, xyz, tri, src, ref, sim)
    rcf.update_source(start)
    sums, pv = rcf.cost(EULERS, per_vertex=True)
    for k, e in enumerate(EULERS):
        want = lit.rigid_cost_mesh(*e)
        assert sums[k] == pytest.approx(want, rel=1e-12, abs=1e-12)
        assert np.abs(pv[k] - lit.current_sim).max() <= 1e-12
    assert np.allclose(rcf.get_source(), start, rtol=0, atol=0)  # SOURCE unchanged
    # target vertex 0 is in the query lists of the vertices next to it (its similarity is 0, its weight counts): they are among those compared above
    near0 = np.nonzero(angles(start, np.broadcast_to(xyz[0], xyz.shape)) < 0.05)[0]
    assert len(near0) > 0 and np.all(pv[0][near0] != 0.0)


def test_simmeasure_outside_1_2_is_refused(ctx):
    xyz, tri, src, ref = _inputs(3, 1, 1)
    mesh = M.Mesh(ctx, xyz, tri)
    with pytest.raises(M.MsmError) as e:
        M.RigidCostFunction(ctx, mesh, mesh, src, ref, simmeasure=3).initialise()
    assert e.value.code == -1


def test_two_runs_are_bit_identical(ctx):
    xyz, tri, src, ref = _inputs(4, 1, 2)
    rcf, _ = _product(ctx, xyz, tri, src, ref, 2)
    a = rcf.cost(EULERS, per_vertex=True)
    b = rcf.cost(EULERS, per_vertex=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ra = rcf.run(3, F32_001, 0.5)
    rcf.update_source(xyz)
    rb = rcf.run(3, F32_001, 0.5)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]


@pytest.mark.parametrize("D,sim", [(1, 1), (3, 2)])
def test_run_matches_literal(ctx, D, sim):
    """run at ico4, 5 iterations per loop: the same accept / reject decisions, grad_zero to rtol 1e-10, SOURCE to 1e-8 (radius 100)"""
    xyz, tri, src, ref = _inputs(4, D, 7)
    lit = RL.RigidLiteral(xyz, tri, src, ref, sim, fast=True).initialise()
    want_xyz, want_trace, want_sum = lit.run(5, F32_001, 0.5)
    rcf, _ = _product(ctx, xyz, tri, src, ref, sim)
    got_xyz, got_trace, got_sum = rcf.run(5, F32_001, 0.5)
    assert got_trace.shape == want_trace.shape
    assert np.array_equal(got_trace[:, [0, 1, 2, 3, 5]], want_trace[:, [0, 1, 2, 3, 5]])
    assert np.allclose(got_trace[:, 4], want_trace[:, 4], rtol=1e-10, atol=0)
    assert np.abs(got_xyz - want_xyz).max() <= 1e-8
    assert got_sum["evaluations"] == want_sum["evaluations"]
    assert got_sum["RECinit"] == pytest.approx(want_sum["RECinit"], rel=1e-12) and got_sum["RECfinal"] == pytest.approx(want_sum["RECfinal"], rel=1e-10)


def test_product_recovers_a_rotation(ctx):
    """simmeasure 1, D = 3, ico4: the input is the reference seen through a ~0.1 rad rotation (tests/test_rigid_cpu.py's case, there through the
    literal); the run raises the cost and shrinks the residual rotation"""
    xyz, tri, _, B = RL.rigid_inputs(4, 3, 11)
    w = (0.06, -0.05, 0.06)
    R = np.array(RL.euler_matrix(*w)).reshape(3, 3)
    A = B[:, O.Octree(O.Mesh(xyz, tri)).closest_vertex(RL.euler_rotate(xyz, *w))]
    rcf, _ = _product(ctx, xyz, tri, A, B, 1)
    out, trace, summary = rcf.run(10, F32_001, 0.5)
    assert summary["RECfinal"] >= summary["RECinit"] and summary["evaluations"] == 1 + 4 * len(trace)
    U, _, Vt = np.linalg.svd(np.linalg.lstsq(xyz, out, rcond=None)[0])
    P = U @ Vt
    ang = lambda Q: float(np.arccos(np.clip((np.trace(Q) - 1) / 2, -1, 1)))  # noqa: E731
    assert ang(R @ P.T) < ang(R) - 0.005, (ang(R), ang(R @ P.T), summary)


def test_ico6_single_feature_samples(ctx):
    """ico6, D = 1 (the MSMSulc level's size): sampled evaluations against the literal's fast mode"""
    xyz, tri, src, ref = _inputs(6, 1, 5)
    lit = RL.RigidLiteral(xyz, tri, src, ref, 2, fast=True).initialise()
    rcf, _ = _product(ctx, xyz, tri, src, ref, 2)
    sums, pv = rcf.cost(EULERS[[0, 1, 4]], per_vertex=True)
    for k, e in enumerate(EULERS[[0, 1, 4]]):
        assert sums[k] == pytest.approx(lit.rigid_cost_mesh(*e), rel=1e-12)
        assert np.abs(pv[k] - lit.current_sim).max() <= 1e-12


class RigidOracleOps(OracleOps):
    """OracleOps plus the rigid level from the literal restatement"""

    def rigid_level(self, target_xyz, target_tri, ref_feat, source_xyz, source_tri, src_feat, sph_in, iters, simmeasure, stepsize, gradsampling):
        return RL.rigid_level(target_xyz, target_tri, ref_feat, src_feat, sph_in, iters, simmeasure, stepsize, gradsampling)


def test_multiresolution_with_a_rigid_level(ctx):
    """RIGID(ico4) + DISCRETE(ico4, control grid ico2, 2 iterations) through run_multiresolution over the product and over the oracle + literal"""
    in_xyz, in_tri = M.make_mesh_from_icosa(5)
    ref = synthetic.features(in_xyz, 1, 21)
    src = synthetic.features(synthetic.known_warp(in_xyz, seed=22, rot_deg=5.0, amp=1.0), 1, 21)
    levels = [dict(method="RIGID", data_order=4, sigma_in=2.0, sigma_ref=2.0, iters=5, simmeasure=1, stepsize=F32_001, gradsampling=0.5),
              dict(data_order=4, cp_order=2, sigma_in=2.0, sigma_ref=2.0, iters=2)]
    lab_got, lab_want = [], []
    got, regs, energies = registration.run_multiresolution(registration.ProductOps(ctx), in_xyz, in_tri, src, in_xyz, in_tri, ref, levels, labelings_out=lab_got)
    want, wregs, wenergies = registration.run_multiresolution(RigidOracleOps(M.mcmc_optimise), in_xyz, in_tri, src, in_xyz, in_tri, ref, levels,
                                                              labelings_out=lab_want)
    assert len(lab_got) == len(lab_want) == 2 and all(np.array_equal(a, b) for a, b in zip(lab_got, lab_want))
    assert np.array_equal(energies[0][:, [0, 1, 2, 3, 5]], wenergies[0][:, [0, 1, 2, 3, 5]])
    assert np.allclose(energies[0][:, 4], wenergies[0][:, 4], rtol=1e-10, atol=0)  # grad_zero of every iteration
    assert angles(regs[0], wregs[0]).max() <= 1e-6 and angles(regs[0], O.icosphere(4)[0]).max() > 1e-4  # the rigid level rotated the grid
    assert angles(got, want).max() <= 1e-6


# the built-in sulc schedule of a run without --conf (M/mesh_registration.cpp:629-642), written out with one iteration per DISCRETE level
DEFAULT_SCHEDULE_SHORT = """--opt=RIGID,DISCRETE,DISCRETE,DISCRETE
--lambda=0,0.1,0.2,0.3
--simval=1,2,2,2
--sigma_in=2,2,3,2
--sigma_ref=2,2,1.5,1
--it=50,1,1,1
--CPgrid=0,2,3,4
--anatgrid=0,4,5,6
--datagrid=4,4,5,6
--SGgrid=0,4,5,6
"""


def test_executables_run_the_rigid_level(ctx, tmp_path):
    """MSMHIP_RIGID=on: tools/register_files.py and tools/cpp/newmsm run the RIGID level (no "skipped" note), write the same bytes, and a result
    different from the run without it"""
    import __graft_entry__ as g
    from newmsm_amd import config, meshio

    assert config.levels_from_config(config.parse_config(DEFAULT_SCHEDULE_SHORT), 1, rigid=True)[0][0] == dict(
        config.levels_from_config(config.parse_config(None), 1, rigid=True)[0][0])
    exe = g.build_cpp_newmsm()
    xyz, tri = M.make_mesh_from_icosa(5)
    ref = synthetic.features(xyz, 1, 5)
    src = synthetic.features(synthetic.known_warp(xyz, seed=8, rot_deg=4.0, amp=1.0), 1, 5)
    d = str(tmp_path) + "/"
    with open(d + "conf", "w") as f:
        f.write(DEFAULT_SCHEDULE_SHORT)
    meshio.save_ascii(d + "in.asc", xyz, tri)
    meshio.save_ascii(d + "in_data.asc", xyz, tri, src[0])
    meshio.save_ascii(d + "ref_data.asc", xyz, tri, ref[0])
    common = ["--inmesh=" + d + "in.asc", "--refmesh=" + d + "in.asc", "--indata=" + d + "in_data.asc", "--refdata=" + d + "ref_data.asc", "--conf=" + d + "conf",
              "-f", "ASCII"]
    env = dict(os.environ, MSMHIP_RIGID="on")
    py = subprocess.run([sys.executable, "tools/register_files.py"] + common + ["--out=" + d + "py."], cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert py.returncode == 0, py.stderr
    cpp = subprocess.run([exe] + common + ["--out=" + d + "cpp."], cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert cpp.returncode == 0, cpp.stderr
    assert "skipped" not in py.stderr and "skipped" not in cpp.stderr
    names = ["sphere.reg.asc", "sphere.LR.reg.asc", "transformed_and_reprojected.dpv"]
    for n in names:
        with open(d + "py." + n, "rb") as a, open(d + "cpp." + n, "rb") as b:
            assert a.read() == b.read(), n
    env.pop("MSMHIP_RIGID")
    off = subprocess.run([sys.executable, "tools/register_files.py"] + common + ["--out=" + d + "off."], cwd=ROOT, capture_output=True, text=True, timeout=600,
                         env=env)
    assert off.returncode == 0, off.stderr
    assert "level 1 (--opt=RIGID)" in off.stderr and "skipped" in off.stderr
    with open(d + "py.sphere.reg.asc", "rb") as a, open(d + "off.sphere.reg.asc", "rb") as b:
        assert a.read() != b.read()
