"""The strain map of an aMSM run on the MI355X (msm_calculate_strains, vertex_strain_kernels.hip) against the literal restatement of
calculate_strains (tests/strains_literal.py), and the two files both executables now write after an aMSM run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
import strains_literal as SL
from newmsm_amd import config, meshio, registration, synthetic
from oracle import oracle as O
from tests.strain_shape_cases import anatomy_case, compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order", [4, 5, 6])
def test_matches_restatement(ctx, order):
    orig, tri, final = anatomy_case(order, seed=order)
    got, kept, radius, _ = compare(ctx, orig, tri, final)
    if order == 4:
        assert np.all(radius > 2.0)  # the coarse anatomy reaches the radius growth everywhere
    assert np.all(kept > 8) and np.all(np.isfinite(got))


def test_ellipsoid_and_flips(ctx):
    xyz, tri = SL.flattened_ellipsoid(5)
    compare(ctx, xyz, tri, xyz * np.array([1.1, 0.95, 1.0]), max_ill=0.1)
    orig, tri, final = anatomy_case(5, seed=9)
    shift = np.array([0.0, 90.0, 0.0])
    compare(ctx, orig + shift, tri, final + shift)
    compare(ctx, orig, tri[:, ::-1].copy(), final)


def test_analytic_cases(ctx):
    orig, tri, _ = anatomy_case(5, seed=2)
    mesh = M.Mesh(ctx, orig, tri)
    s = M.calculate_strains(mesh, orig)
    np.testing.assert_allclose(s[:2], 1.0, rtol=0, atol=1e-9)
    s = M.calculate_strains(mesh, orig * 1.25)
    np.testing.assert_allclose(s[:2], 1.25, rtol=1e-9)
    np.testing.assert_allclose(s[2:], 0.5 * (1.25 ** 2 - 1), rtol=1e-9)


def test_two_calls_same_bits(ctx):
    orig, tri, final = anatomy_case(5, seed=3)
    mesh = M.Mesh(ctx, orig, tri)
    a = M.calculate_strains(mesh, final, with_neighbourhoods=True)
    b = M.calculate_strains(mesh, final, with_neighbourhoods=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_bad_arguments_refused(ctx):
    orig, tri, final = anatomy_case(3)
    mesh = M.Mesh(ctx, orig, tri)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(M.MsmError):
            M.calculate_strains(mesh, final, r)
    with pytest.raises(M.MsmError):
        M.calculate_strains(mesh, final[:-1])
    bad = final.copy()
    bad[7, 1] = np.nan
    with pytest.raises(M.MsmError):
        M.calculate_strains(mesh, bad)
    xyz, t0 = O.icosphere(0)  # 12 vertices: at most 7 face the same way as any one, the reference's radius would grow forever
    with pytest.raises(M.MsmError, match="never the 9"):
        M.calculate_strains(M.Mesh(ctx, xyz, t0), xyz)
    M.calculate_strains(mesh, final)  # the context is still usable


def test_project_anatomical_mesh(ctx):
    xyz, tri = O.icosphere(5)
    moved = synthetic.known_warp(xyz, seed=4, rot_deg=3.0, amp=2.0)
    anat = synthetic.anatomy(xyz, seed=12)
    sphere, target = M.Mesh(ctx, moved, tri), M.Mesh(ctx, xyz, tri)
    got = M.project_anatomical_mesh(sphere, target, anat)
    np.testing.assert_allclose(got, SL.project_anatomical_mesh(moved, xyz, tri, anat), rtol=0, atol=1e-12)
    # an anatomy of another vertex count: the reference sphere's own coordinates
    other = M.project_anatomical_mesh(sphere, target, anat[:100])
    np.testing.assert_allclose(other, SL.project_anatomical_mesh(moved, xyz, tri, anat[:100]), rtol=0, atol=1e-12)
    assert np.abs(np.linalg.norm(other, axis=1) - 100.0).max() < 1.0


def _f32_equal(file_values, want):
    np.testing.assert_allclose(np.asarray(file_values, dtype=np.float64), want, rtol=1.2e-7, atol=1e-30)


def test_amsm_runs_write_strains(ctx, tmp_path):
    """tools/register_files.py and tools/cpp/newmsm with --inanat / --refanat: anat.reg.surf.gii and STRAINS.func.gii hold project_anatomical_mesh and
    calculate_strains of the registered sphere run_multiresolution returns for the same inputs, byte for byte the same from both; without anatomy
    neither is written"""
    import __graft_entry__ as g

    exe = g.build_cpp_newmsm()
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 1, 5)
    src = synthetic.features(synthetic.known_warp(xyz, seed=8, rot_deg=3.0, amp=2.0), 1, 5)
    ian, ran = synthetic.anatomy(xyz, seed=61, base=60.0), synthetic.anatomy(xyz, seed=71, base=62.0)
    d = str(tmp_path) + "/"
    text = ("--simval=2,2\n--sigma_in=2,0\n--sigma_ref=2,0\n--lambda=0.025,0.025\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=1,2\n--SGgrid=3,4\n--datagrid=3,4\n"
            "--anatgrid=3,4\n--regoption=5\n--dopt=HOCR\n--triclique\n--rescaleL\n--shearmod=0.4\n--bulkmod=1.6\n--k_exponent=2\n")
    with open(d + "conf", "w") as f:
        f.write(text)
    with open(d + "conf_plain", "w") as f:
        f.write(text.replace("--regoption=5\n", "--regoption=3\n").replace("--anatgrid=3,4\n", ""))
    meshio.save_surface(d + "sphere.surf.gii", xyz, tri)
    meshio.save_surface(d + "in.anat.surf.gii", ian, tri)
    meshio.save_surface(d + "ref.anat.surf.gii", ran, tri)
    meshio.save_metric(d + "in.func.gii", src)
    meshio.save_metric(d + "ref.func.gii", ref)
    args = ["--inmesh=" + d + "sphere.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "ref.func.gii"]
    anat = ["--inanat=" + d + "in.anat.surf.gii", "--refanat=" + d + "ref.anat.surf.gii"]
    py = subprocess.run([sys.executable, "tools/register_files.py"] + args + anat + ["--conf=" + d + "conf", "--out=" + d + "py."], cwd=ROOT,
                        capture_output=True, text=True, timeout=600)
    assert py.returncode == 0, py.stderr
    cpp = subprocess.run([exe] + args + anat + ["--conf=" + d + "conf", "--out=" + d + "cpp.", "-f", "ASCII"], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert cpp.returncode == 0, cpp.stderr
    for n in ("anat.reg.surf.gii", "STRAINS.func.gii"):  # GIFTI whatever -f says
        with open(d + "py." + n, "rb") as fa, open(d + "cpp." + n, "rb") as fb:
            assert fa.read() == fb.read(), "%s differs between the two programs" % n

    in_xyz, _ = meshio.load_surface(d + "sphere.surf.gii")
    in_xyz = in_xyz - in_xyz.mean(axis=0)
    in_xyz = in_xyz * (100.0 / np.linalg.norm(in_xyz, axis=1, keepdims=True))
    in_anat, in_anat_tri = meshio.load_surface(d + "in.anat.surf.gii")
    ref_anat = meshio.load_surface(d + "ref.anat.surf.gii")[0]
    levels, run_kw, _ = config.levels_from_config(config.parse_config(text), 1, anat=True)
    want, _, _ = registration.run_multiresolution(registration.ProductOps(ctx), in_xyz, tri, meshio.load_data(d + "in.func.gii", len(xyz)), in_xyz, tri,
                                                  meshio.load_data(d + "ref.func.gii", len(xyz)), levels, in_anat=in_anat, ref_anat=ref_anat, **run_kw)
    anat_reg = M.project_anatomical_mesh(M.Mesh(ctx, want, tri), M.Mesh(ctx, in_xyz, tri), ref_anat)
    got_xyz, got_tri = meshio.load_surface(d + "py.anat.reg.surf.gii")
    assert np.array_equal(got_tri, tri)
    _f32_equal(got_xyz, anat_reg)
    strains = M.calculate_strains(M.Mesh(ctx, in_anat, in_anat_tri), anat_reg)
    got_strains = meshio.load_metric(d + "py.STRAINS.func.gii")
    assert got_strains.shape == (4, len(xyz))
    _f32_equal(got_strains, strains)
    # and the device's strains are the restatement's
    np.testing.assert_allclose(strains, SL.calculate_strains(in_anat, in_anat_tri, anat_reg)["strains"], rtol=1e-9, atol=1e-12)

    for prog, out in (([sys.executable, "tools/register_files.py"], "pyn."), ([exe], "cppn.")):
        run = subprocess.run(prog + args + ["--conf=" + d + "conf_plain", "--out=" + d + out], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr
        assert os.path.exists(d + out + "sphere.reg.surf.gii")
        assert not os.path.exists(d + out + "anat.reg.surf.gii") and not os.path.exists(d + out + "STRAINS.func.gii")
