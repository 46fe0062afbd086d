"""--trans (a transformed input sphere as the starting point) and --excl (exclusion masks from the cut thresholds) on the MI355X path: the level
loops over the product against the same loops over the oracle (tests/trans_excl_cases.py), by the criteria of tests/test_gpu_registration.py for
pairwise runs (every labeling identical, energies rtol 1e-10, coordinates within 1e-9) and of tests/test_gpu_group.py for groupwise ones (labelings
identical, energies rtol 1e-9, coordinates within 1e-8 and 1e-4 rad); then both executables from files to files."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
import trans_excl_cases as C
from helpers import angles, ulp_close
from newmsm_amd import config, group_registration, meshio, registration, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXCL_LEVELS = [dict(data_order=3, cp_order=1, sigma_in=4.0, sigma_ref=4.0, iters=2, mciters=40),
               dict(data_order=4, cp_order=2, sigma_in=0.0, sigma_ref=0.0, iters=2, mciters=40)]


def assert_pairwise_parity(got, lab_got, want, lab_want):
    assert len(lab_got) == len(lab_want) > 0 and all(np.array_equal(a, b) for a, b in zip(lab_got, lab_want))
    assert np.allclose(np.concatenate(got[2]), np.concatenate(want[2]), rtol=1e-10, atol=0)
    assert np.abs(got[0] - want[0]).max() < 1e-9
    for a, b in zip(got[1], want[1]):
        assert np.abs(a - b).max() < 1e-9


# ---------------------------------------------------------------- --trans
@pytest.mark.parametrize("levels", [C.DISCRETE_PAIR, C.RIGID_THEN_DISCRETE], ids=["discrete_discrete", "rigid_discrete"])
def test_trans_continues_a_run_exactly(ctx, levels):
    """check 1: [L2] started from the sphere.reg of [L1] is [L1, L2] bit for bit: level 2 of the whole run starts from the input sphere carried through
    level 1's warp, which is what the first stage returns, and the second stage's first level performs the very same projections and unfolds"""
    case = C.pairwise_case(order=5, D=2)
    a, lab_a2, reg1, b2, lab_b = C.composition(registration.ProductOps(ctx), case, levels)
    C.assert_composition(a, lab_a2, b2, lab_b)
    assert angles(reg1, case[0]).max() > 1e-4 and angles(b2[0], reg1).max() > 1e-4  # both stages moved the sphere


def test_trans_equal_to_the_input_sphere_warns_and_is_ignored(ctx, capfd):
    """check 2"""
    case = C.pairwise_case(order=4, D=1)
    plain = C.run(registration.ProductOps(ctx), case, C.DISCRETE_PAIR[:1])
    capfd.readouterr()
    same = C.run(registration.ProductOps(ctx), case, C.DISCRETE_PAIR[:1], trans_xyz=np.array(case[0]))
    assert "WARNING: transformed mesh has the same coordinates as the input mesh" in capfd.readouterr().err
    assert np.array_equal(same[0], plain[0]) and np.array_equal(same[1][0], plain[1][0]) and same[2] == plain[2]
    with pytest.raises(ValueError, match="642 vertices, the input mesh has 2562"):
        C.run(registration.ProductOps(ctx), case, C.DISCRETE_PAIR[:1], trans_xyz=M.make_mesh_from_icosa(3)[0])


def test_trans_from_a_known_warp_matches_oracle(ctx):
    """check 3: an input mesh that is not the level's grid (ico5 input, ico4 data grid), started from a known smooth warp of the input sphere"""
    case = C.pairwise_case(order=5, D=2)
    levels = C.DISCRETE_PAIR[1:]
    trans = synthetic.known_warp(case[0], seed=77, rot_deg=3.0, amp=2.0)
    lg, lw = [], []
    got = C.run(registration.ProductOps(ctx), case, levels, lg, trans_xyz=trans)
    want = C.run(C.oracle_ops(), case, levels, lw, trans_xyz=trans)
    assert_pairwise_parity(got, lg, want, lw)
    plain = C.run(registration.ProductOps(ctx), case, levels)
    assert angles(got[0], plain[0]).max() > 1e-3  # the option is not a no-op


# ---------------------------------------------------------------- --excl
def test_excl_pairwise_matches_oracle(ctx):
    """check 4: both data sets exactly 0 on a cap of 10 % of the vertices; --excl --VN, sigma > 0 at the first level and 0 at the second"""
    case = C.pairwise_case(order=5, D=2, cap=True)
    assert case[4].sum() == 1024 and 0.05 * len(case[0]) <= case[4].sum() <= 0.15 * len(case[0])
    ops = registration.ProductOps(ctx)
    # the prepared features of every level and data set, directly
    got_f, want_f = C.level_features(ops, case, EXCL_LEVELS, True), C.level_features(C.oracle_ops(), case, EXCL_LEVELS, True)
    plain_f = C.level_features(ops, case, EXCL_LEVELS, False)
    assert len(got_f) == len(want_f) == 4
    for k, ((f, m), (wf, wm), (pf, pm)) in enumerate(zip(got_f, want_f, plain_f)):
        worst = float(np.nanmax(np.abs(f - wf))), float(np.abs(m - wm).max())
        print("level features %d: max |feature diff| %.3e, max |mask diff| %.3e, kept %d of %d" % (k, worst[0], worst[1], int((m > 0).sum()), m.size))
        assert m.shape == wm.shape and np.array_equal(m > 0, wm > 0)  # the same set of kept vertices, every vertex compared
        assert 0 < (m > 0).sum() < m.size and not np.isnan(f).any()
        assert ulp_close(m, wm) and ulp_close(f, wf)
        assert pm is None and not np.allclose(pf, f, atol=1e-3)        # the mask matters
    lg, lw = [], []
    got = C.run(ops, case, EXCL_LEVELS, lg, excl=True, cutthr=C.CUTTHR)
    want = C.run(C.oracle_ops(), case, EXCL_LEVELS, lw, excl=True, cutthr=C.CUTTHR)
    assert_pairwise_parity(got, lg, want, lw)
    plain = C.run(ops, case, EXCL_LEVELS, excl=False)
    assert not np.allclose(np.concatenate(got[2]), np.concatenate(plain[2]), rtol=1e-6)


def test_excl_on_a_native_mesh_that_coincides_with_the_grid(ctx):
    """The reference's behaviour at the rim of the cut when the native mesh's vertices ARE the level grid's (a regular ico4 onto the ico4 grid):
    barycentric weights of exactly 0 meet a scatter sum of 0 in get_adaptive_barycentric_weights (R/resampler.cpp:72-140) and the rim's features are
    NaN.  Real native meshes are irregular; the path follows the reference here too: the same vertices are NaN, everything else agrees."""
    xyz, tri = M.make_mesh_from_icosa(4)
    data = synthetic.features(xyz, 2, 31)
    data[:, xyz[:, 2] > C.CAP_Z] = 0.0
    out = []
    for ops in (registration.ProductOps(ctx), C.oracle_ops()):
        mesh = ops.mesh(xyz, tri)
        out.append(registration.level_features(ops, lambda name, fn, *a: fn(*a), mesh, data, ops.mesh(xyz, tri), 0.0, False, None, True, C.CUTTHR))
    (f, m), (wf, wm) = out
    assert np.isnan(wf).any() and np.array_equal(np.isnan(f), np.isnan(wf)) and np.array_equal(np.isnan(m), np.isnan(wm))
    assert ulp_close(f, wf) and ulp_close(m, wm)


@pytest.mark.parametrize("with_mask", [False, True], ids=["no_template_mask", "template_mask"])
def test_excl_groupwise_matches_oracle(ctx, with_mask):
    """check 4 for three subjects over two levels, with and without --mask beside it"""
    meshes, datas, txyz, tri, levels, mask, caps = C.group_case()
    assert all(0.05 * len(c) <= c.sum() <= 0.15 * len(c) for c in caps) and [int(c.sum()) for c in caps] == [257, 256, 254]
    kw = dict(mask=mask if with_mask else None, varnorm=True, fixnan=True)
    lg, lw, lp = [], [], []
    got = group_registration.run_group_multiresolution(group_registration.ProductGroupOps(ctx), meshes, datas, txyz, tri, levels, labelings_out=lg, excl=True,
                                                       cutthr=C.CUTTHR, **kw)
    want = group_registration.run_group_multiresolution(C.oracle_ops(), meshes, datas, txyz, tri, levels, labelings_out=lw, excl=True, cutthr=C.CUTTHR, **kw)
    assert len(lg) == len(lw) == 4 and all(np.array_equal(a, b) for a, b in zip(lg, lw))
    for a, b in zip(got[2], want[2]):
        assert np.allclose(a, b, rtol=1e-9)
    for s in range(len(meshes)):
        assert angles(got[0][s], want[0][s]).max() <= 1e-4 and np.abs(got[0][s] - want[0][s]).max() < 1e-8
    for a, b in zip(got[1], want[1]):
        assert np.abs(a - b).max() < 1e-8
    plain = group_registration.run_group_multiresolution(group_registration.ProductGroupOps(ctx), meshes, datas, txyz, tri, levels, labelings_out=lp, **kw)
    assert not np.allclose(got[2][0], plain[2][0], rtol=1e-6)  # the masks changed what the model compares


# ---------------------------------------------------------------- files in, files out
def _on_sphere(xyz):
    xyz = xyz - xyz.mean(axis=0)
    return xyz * (100.0 / np.linalg.norm(xyz, axis=1, keepdims=True))


def _same_files(a_prefix, b_prefix, names):
    for n in names:
        with open(a_prefix + n, "rb") as fa, open(b_prefix + n, "rb") as fb:
            assert fa.read() == fb.read(), "%s differs between the two programs" % n


STAGE1 = "--simval=2\n--sigma_in=4\n--sigma_ref=4\n--lambda=0.05\n--it=2\n--opt=DISCRETE\n--CPgrid=1\n--SGgrid=3\n--datagrid=3\n--regoption=3\n--dopt=HOCR\n--VN\n"
STAGE2 = ("--simval=2,2\n--sigma_in=2,0\n--sigma_ref=2,0\n--lambda=0.05,0.05\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=2,2\n--SGgrid=4,4\n--datagrid=4,4\n--regoption=3\n"
          "--dopt=HOCR\n--VN\n--excl\n--cutthr=0,0.0001\n")


def test_executables_start_from_a_previous_registration_with_masks(ctx, tmp_path):
    """check 5: tools/register_files.py and tools/cpp/newmsm with --trans=<the sphere.reg.surf.gii a first run wrote> and --excl in the configuration:
    every output byte for byte the same from both, and sphere.reg what the library gives for the coordinates read back from that file, to the float32
    the files hold.  (Files hold float32: the exact equality with a single run over all levels that test_trans_continues_a_run_exactly demands of
    the library is not expected through files.)"""
    import __graft_entry__ as g

    exe = g.build_cpp_newmsm()
    xyz, tri, src, ref, inside = C.pairwise_case(order=5, D=2, cap=True)
    d = str(tmp_path) + "/"
    meshio.save_surface(d + "in.surf.gii", xyz + 0.25, tri)  # off-centre: recentre / rescale matter for the input, and must not touch --trans
    meshio.save_surface(d + "ref.surf.gii", xyz, tri)
    meshio.save_metric(d + "in.func.gii", src)
    meshio.save_metric(d + "ref.func.gii", ref)
    for name, text in (("conf1", STAGE1), ("conf2", STAGE2)):
        with open(d + name, "w") as f:
            f.write(text)
    common = ["--inmesh=" + d + "in.surf.gii", "--refmesh=" + d + "ref.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "ref.func.gii"]
    first = subprocess.run([sys.executable, "tools/register_files.py"] + common + ["--conf=" + d + "conf1", "--out=" + d + "s1."], cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
    assert first.returncode == 0, first.stderr
    stage2 = common + ["--conf=" + d + "conf2", "--trans=" + d + "s1.sphere.reg.surf.gii"]
    py = subprocess.run([sys.executable, "tools/register_files.py"] + stage2 + ["--out=" + d + "py."], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert py.returncode == 0, py.stderr
    cpp = subprocess.run([exe] + stage2[:-1] + ["-t", d + "s1.sphere.reg.surf.gii", "-o", d + "cpp."], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert cpp.returncode == 0, cpp.stderr
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    _same_files(d + "py.", d + "cpp.", names)
    # the library on what the files hold
    in_xyz, ref_xyz = _on_sphere(meshio.load_surface(d + "in.surf.gii")[0]), _on_sphere(meshio.load_surface(d + "ref.surf.gii")[0])
    trans = meshio.load_surface(d + "s1.sphere.reg.surf.gii")[0]
    src_f, ref_f = meshio.load_data(d + "in.func.gii", len(xyz)), meshio.load_data(d + "ref.func.gii", len(xyz))
    cfg = config.parse_config(STAGE2)
    levels, run_kw, _ = config.levels_from_config(cfg, 2)
    assert config.run_options(cfg) == dict(excl=True, cutthr=(0.0, float(np.float32(0.0001))))
    want, regs, _ = registration.run_multiresolution(registration.ProductOps(ctx), in_xyz, tri, src_f, ref_xyz, tri, ref_f, levels, trans_xyz=trans, **run_kw,
                                                     **config.run_options(cfg))
    reg = meshio.load_surface(d + "py.sphere.reg.surf.gii")[0]
    assert np.array_equal(reg.astype(np.float32), want.astype(np.float32))
    assert np.array_equal(meshio.load_surface(d + "py.sphere.LR.reg.surf.gii")[0].astype(np.float32), regs[-1].astype(np.float32))
    assert angles(reg, trans).max() > 1e-4  # the second stage moved on from the first
    notrans = registration.run_multiresolution(registration.ProductOps(ctx), in_xyz, tri, src_f, ref_xyz, tri, ref_f, levels, **run_kw, **config.run_options(cfg))[0]
    assert angles(want, notrans).max() > 1e-4  # and --trans was used
    # transformed_and_reprojected: zero inside the cap.  A reference vertex is surely fed by cut vertices alone when it lies deeper in the cap than the
    # registration moved any vertex plus two edge lengths of the mesh (the triangle around it and the adaptive weights' one-ring)
    moved = meshio.load_data(d + "py.transformed_and_reprojected.func.gii", len(xyz))
    edge = np.linalg.norm(xyz[tri[:, 0]] - xyz[tri[:, 1]], axis=1).max() / 100.0
    depth = np.arccos(C.CAP_Z / 100.0) - np.arccos(np.clip(ref_xyz[:, 2] / 100.0, -1.0, 1.0))  # rad inside the cap's rim
    deep = depth > angles(want, in_xyz).max() + 2.0 * edge
    assert deep.sum() > 100 and np.all(moved[:, deep] == 0.0) and np.abs(moved[:, ~inside]).max() > 0.1
    # --excl together with both weightings: refused by both, with the reason
    meshio.save_metric(d + "w.func.gii", np.ones((1, len(xyz))))
    for cmd in ([sys.executable, "tools/register_files.py"], [exe]):
        bad = subprocess.run(cmd + stage2 + ["--inweight=" + d + "w.func.gii", "--refweight=" + d + "w.func.gii", "--out=" + d + "bad."], cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert bad.returncode == 1 and "downsample_cfweighting" in bad.stderr


def test_groupwise_executables_take_excl_and_ignore_trans(ctx, tmp_path):
    """-g with --excl in the configuration: the same bytes from both executables, and the masks reach the model (the energies newmsm -v prints differ
    from the run without --excl; on this coarse grid the labelings, and with them the spheres, need not); --trans is not handed to a groupwise run
    (CLI/newmsm.cpp:13-27): a note on stderr"""
    import __graft_entry__ as g

    exe = g.build_cpp_newmsm()
    meshes, datas, txyz, tri, _, _, _ = C.group_case()
    d = str(tmp_path) + "/"
    text = "--simval=2\n--sigma_in=2\n--lambda=0.001\n--it=2\n--opt=DISCRETE\n--CPgrid=1\n--SGgrid=3\n--datagrid=3\n--dopt=HOCR\n--VN\n--fixnan\n"
    for name, t in (("conf", text), ("conf_excl", text + "--excl\n")):
        with open(d + name, "w") as f:
            f.write(t)
    meshio.save_surface(d + "template.surf.gii", txyz, tri)
    for s in range(len(meshes)):
        meshio.save_surface(d + "sphere%d.surf.gii" % s, meshes[s][0], tri)
        meshio.save_metric(d + "data%d.func.gii" % s, datas[s])
    with open(d + "meshes.txt", "w") as f:
        f.write("".join(d + "sphere%d.surf.gii\n" % s for s in range(len(meshes))))
    with open(d + "data.txt", "w") as f:
        f.write("".join(d + "data%d.func.gii\n" % s for s in range(len(meshes))))
    common = ["--groupwise", "--meshes=" + d + "meshes.txt", "--data=" + d + "data.txt", "--template=" + d + "template.surf.gii"]
    runs = {}
    for tag, cmd, conf in (("py", [sys.executable, "tools/register_files.py"], "conf_excl"), ("cpp", [exe], "conf_excl"), ("plain", [exe], "conf")):
        runs[tag] = subprocess.run(cmd + common + ["--conf=" + d + conf, "--trans=" + d + "sphere0.surf.gii", "--out=" + d + tag + ".", "-v"], cwd=ROOT,
                                   capture_output=True, text=True, timeout=600)
        assert runs[tag].returncode == 0, runs[tag].stderr
        assert "--trans is not used in groupwise mode" in runs[tag].stderr
    names = [n % s for s in range(len(meshes)) for n in ("sphere-%d.reg.surf.gii", "sphere-%d.LR.reg.surf.gii", "transformed_and_reprojected-%d.func.gii")]
    _same_files(d + "py.", d + "cpp.", names)
    energies = {tag: [ln for ln in runs[tag].stdout.splitlines() if ln.startswith("level 1: energies per iteration")] for tag in ("cpp", "plain")}
    assert len(energies["cpp"]) == len(energies["plain"]) == 1 and energies["cpp"] != energies["plain"], energies
