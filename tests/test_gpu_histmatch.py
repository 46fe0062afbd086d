"""--IN / --INc on the MI355X path: msm_histogram_match against the literal restatement (tests/histmatch_literal.py) bit for bit -- integer counts,
and the definition's divisions and products repeated one rounding each (the library is built with -ffp-contract=off) --, then the level loops and
both executables with MSMHIP_HISTMATCH=on.  Agreement with FSL's MISCMATHS::Histogram itself is unpinned (it is not in the reference tree)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import histmatch_literal as HL
import newmsm_amd as M
from newmsm_amd import config, group_registration, meshio, registration, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 3, 642, 642), (1, 1, 2562, 642), (5, 2, 2562, 2562)]  # n_src, D, Vs, Vt
VARIANTS = ["random", "ties", "lo_hi", "half_zero", "constant", "nan_inf", "all_masked", "target_constant", "target_all_masked", "target_nan"]


def make_inputs(shape, variant, seed):
    """n_src x D x Vs sources, a D x Vt target and their masks; `variant` shapes row 0 of source 0 (or of the target), the other rows stay random.
    Masks alternate with the seed between none, one row and D rows."""
    n, D, Vs, Vt = shape
    rng = np.random.default_rng(seed)
    src = rng.normal(size=(n, D, Vs)) * rng.uniform(0.5, 3.0, size=(n, D, 1))
    ref = rng.gamma(2.0, 2.0, size=(D, Vt)) - 1.5
    rows = (None, 1, D)[seed % 3]
    src_excl = None if rows is None else (rng.random((n, rows, Vs)) > 0.25).astype(np.float64)
    ref_excl = None if rows is None else (rng.random((rows, Vt)) > 0.25).astype(np.float64)
    x = src[0, 0]
    if variant == "ties":
        src[0, 0] = np.round(x, 1)                       # about 80 distinct values
        ref[0] = np.round(ref[0], 1)
    elif variant == "lo_hi":
        x[:40], x[40:80] = x.min(), x.max()              # many values exactly on the range's ends
        ref[0, :30], ref[0, 30:60] = ref[0].min(), ref[0].max()
    elif variant == "half_zero":
        x[rng.permutation(Vs)[:Vs // 2]] = 0.0           # one dominant bin, scattered
        ref[0, :Vt // 2] = 0.0                           # and contiguous: whole wavefronts in one counter
    elif variant == "constant":
        x[:] = 1.25
    elif variant == "nan_inf":
        x[3], x[Vs // 2], x[Vs - 1] = np.nan, np.inf, -np.inf
    elif variant == "all_masked":  # (D mask rows, so that only feature row 0 loses its values)
        src_excl = (rng.random((n, D, Vs)) > 0.25).astype(np.float64)
        src_excl[0, 0] = 0.0
    elif variant == "target_constant":
        ref[0] = -2.0
    elif variant == "target_all_masked":
        ref_excl = (rng.random((D, Vt)) > 0.25).astype(np.float64)
        ref_excl[0] = 0.0
    elif variant == "target_nan":
        ref[0, 7], ref[0, 8] = np.nan, np.inf
    return src, ref, src_excl, ref_excl


def literal(src, ref, src_excl, ref_excl):
    return np.stack([HL.histogram_match(src[s], ref, None if src_excl is None else src_excl[s], ref_excl) for s in range(src.shape[0])])


@pytest.mark.parametrize("shape", SHAPES, ids=["ico3_D3", "ico4_to_ico3_D1", "five_sources_D2_ico4"])
def test_histogram_match_equals_the_literal_bit_for_bit(ctx, shape):
    for k, variant in enumerate(VARIANTS):
        src, ref, se, re_ = make_inputs(shape, variant, 100 + k)
        want = literal(src, ref, se, re_)
        got = M.histogram_match(ctx, src, ref, se, re_)
        assert got.shape == src.shape
        same = (got == want) | (np.isnan(got) & np.isnan(want))  # == on the doubles; a NaN that was left in place is a NaN
        assert same.all(), "%s: %d of %d values differ, first at %s" % (variant, (~same).sum(), same.size, np.argwhere(~same)[0])
        changed = ~((got == src) | (np.isnan(got) & np.isnan(src)))
        row0_unchanged = variant in ("constant", "all_masked", "target_constant", "target_all_masked")
        assert changed[0, 0].any() != row0_unchanged and (shape[0] * shape[1] == 1 or changed.reshape(-1, shape[2])[1:].any())
        again = M.histogram_match(ctx, src, ref, se, re_)
        assert again.tobytes() == got.tobytes()  # two calls on the same input give the same bits


def test_single_matrix_and_mask_shapes(ctx):
    """a D x Vs matrix and a V-vector mask go in as they are; mask rows beyond the first follow the feature row only when there are enough of them"""
    rng = np.random.default_rng(5)
    src, ref = rng.normal(size=(3, 700)), rng.normal(size=(3, 900)) * 2.0 + 1.0
    m3, m1 = (rng.random((3, 700)) > 0.4).astype(np.float64), (rng.random(700) > 0.4).astype(np.float64)
    for se in (m3, m1, m3[:2]):
        got = M.histogram_match(ctx, src, ref, se, None)
        assert got.shape == (3, 700) and np.array_equal(got, HL.histogram_match(src, ref, se, None))
    with pytest.raises(M.MsmError):
        M.histogram_match(ctx, np.zeros((1, 0)), ref[:1])


# ---------------------------------------------------------------- the loops and the executables
def _on_sphere(xyz):
    xyz = xyz - xyz.mean(axis=0)
    return xyz * (100.0 / np.linalg.norm(xyz, axis=1, keepdims=True))


def _same_files(a_prefix, b_prefix, names):
    for n in names:
        with open(a_prefix + n, "rb") as fa, open(b_prefix + n, "rb") as fb:
            assert fa.read() == fb.read(), "%s differs between the two programs" % n


def _run(cmd, histmatch=True):
    env = dict(os.environ)
    env.pop("MSMHIP_HISTMATCH", None)
    if histmatch:
        env["MSMHIP_HISTMATCH"] = "on"
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)


PAIR_CONF = ("--simval=2,2\n--sigma_in=4,2\n--sigma_ref=4,2\n--lambda=0.05,0.05\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=1,2\n--SGgrid=3,4\n--datagrid=3,4\n"
             "--regoption=3\n--dopt=HOCR\n--VN\n")


def pairwise_inputs():
    """the synthetic subject of tools/make_registration_inputs.py (seeds 7 / 9) at ico4, the reference's data on another scale"""
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 2, 7) * 3.0 + 1.0
    src = synthetic.features(synthetic.known_warp(xyz, seed=9, rot_deg=3.0, amp=2.0), 2, 7)
    return xyz, tri, src, ref


@pytest.mark.parametrize("flags", ["--IN\n", "--INc\n--cutthr=0,0.0001\n"], ids=["IN", "INc"])
def test_pairwise_executables_with_histogram_matching(ctx, tmp_path, flags):
    import __graft_entry__ as g

    exe = g.build_cpp_newmsm()
    xyz, tri, src, ref = pairwise_inputs()
    d = str(tmp_path) + "/"
    meshio.save_surface(d + "in.surf.gii", xyz, tri)
    meshio.save_metric(d + "in.func.gii", src)
    meshio.save_metric(d + "ref.func.gii", ref)
    with open(d + "conf", "w") as f:
        f.write(PAIR_CONF + flags)
    common = ["--inmesh=" + d + "in.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "ref.func.gii", "--conf=" + d + "conf"]
    for tag, cmd in (("py", [sys.executable, "tools/register_files.py"]), ("cpp", [exe])):
        out = _run(cmd + common + ["--out=" + d + tag + "."])
        assert out.returncode == 0, out.stderr
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    _same_files(d + "py.", d + "cpp.", names)
    # the Python loop on what the files hold
    in_xyz = _on_sphere(meshio.load_surface(d + "in.surf.gii")[0])
    src_f, ref_f = meshio.load_data(d + "in.func.gii", len(xyz)), meshio.load_data(d + "ref.func.gii", len(xyz))
    cfg = config.parse_config(PAIR_CONF + flags)
    levels, run_kw, _ = config.levels_from_config(cfg, 2, histmatch=True)
    assert run_kw == dict(varnorm=True, intensity=True, cut="INc" in flags)
    ops = registration.ProductOps(ctx)
    reg, regs, _ = registration.run_multiresolution(ops, in_xyz, tri, src_f, in_xyz, tri, ref_f, levels, **run_kw, **config.run_options(cfg))
    assert np.array_equal(meshio.load_surface(d + "py.sphere.reg.surf.gii")[0].astype(np.float32), reg.astype(np.float32))
    want = registration.transformed_data(ops, M.Mesh(ctx, reg, tri), src_f, M.Mesh(ctx, in_xyz, tri), ref_f, intensity=True, **config.run_options(cfg))
    moved = meshio.load_data(d + "py.transformed_and_reprojected.func.gii", len(xyz))
    assert np.array_equal(moved, want.astype(np.float32).astype(np.float64))
    plain = registration.transformed_data(ops, M.Mesh(ctx, reg, tri), src_f, M.Mesh(ctx, in_xyz, tri), ref_f, **config.run_options(cfg))
    assert np.abs(want - plain).max() > 0.5 and np.all(plain.std(axis=1) < 0.5 * ref_f.std(axis=1))
    assert np.all(np.abs(want.std(axis=1) / ref_f.std(axis=1) - 1.0) < 0.15)  # the input data took the reference's scale
    # the level features: the literal applied to the same resampled and smoothed matrices
    in_mesh = M.Mesh(ctx, in_xyz, tri)
    timed = lambda name, fn, *a: fn(*a)  # noqa: E731
    for lv in levels:
        ico = M.Mesh(ctx, *M.make_mesh_from_icosa(lv["data_order"]))
        prep = [registration.level_features(ops, timed, in_mesh, data, ico, sigma, False, None, run_kw["cut"], config.run_options(cfg)["cutthr"])
                for data, sigma in ((src_f, lv["sigma_in"]), (ref_f, lv["sigma_ref"]))]
        got = registration.finish_features(ops, timed, [p[0] for p in prep], [p[1] for p in prep], True, False)
        assert (prep[0][1] is not None) == run_kw["cut"]
        assert np.array_equal(got[0], prep[0][0]) and np.array_equal(got[1], HL.histogram_match(prep[1][0], prep[0][0], prep[1][1], prep[0][1]))
        assert np.abs(got[1] - prep[1][0]).max() > 0.5


def test_groupwise_executables_with_histogram_matching(ctx, tmp_path):
    """a 4-subject level: every later subject's data matched to subject 0's, the same bytes from both programs, the Python loop's spheres"""
    import __graft_entry__ as g

    exe = g.build_cpp_newmsm()
    S, D = 4, 2
    xyz, tri = M.make_mesh_from_icosa(4)
    txyz = synthetic.known_warp(xyz, seed=33, rot_deg=7.0, amp=1.5)
    meshes = [(synthetic.known_warp(xyz, seed=40 + s, rot_deg=0.0, amp=1.0), tri) for s in range(S)]
    datas = [synthetic.features(synthetic.known_warp(meshes[s][0], seed=90 + s, rot_deg=3.0, amp=2.0), D, seed=5) * (1.0 + s) + s for s in range(S)]
    d = str(tmp_path) + "/"
    text = "--simval=2\n--sigma_in=2\n--lambda=0.001\n--it=2\n--opt=DISCRETE\n--CPgrid=1\n--SGgrid=3\n--datagrid=3\n--dopt=HOCR\n--VN\n--fixnan\n--IN\n"
    with open(d + "conf", "w") as f:
        f.write(text)
    meshio.save_surface(d + "template.surf.gii", txyz, tri)
    for s in range(S):
        meshio.save_surface(d + "sphere%d.surf.gii" % s, meshes[s][0], tri)
        meshio.save_metric(d + "data%d.func.gii" % s, datas[s])
    for name, pattern in (("meshes.txt", "sphere%d.surf.gii\n"), ("data.txt", "data%d.func.gii\n")):
        with open(d + name, "w") as f:
            f.write("".join(d + pattern % s for s in range(S)))
    common = ["--groupwise", "--meshes=" + d + "meshes.txt", "--data=" + d + "data.txt", "--template=" + d + "template.surf.gii", "--conf=" + d + "conf"]
    for tag, cmd in (("py", [sys.executable, "tools/register_files.py"]), ("cpp", [exe])):
        out = _run(cmd + common + ["--out=" + d + tag + "."])
        assert out.returncode == 0, out.stderr
    _same_files(d + "py.", d + "cpp.", [n % s for s in range(S) for n in ("sphere-%d.reg.surf.gii", "sphere-%d.LR.reg.surf.gii", "transformed_and_reprojected-%d.func.gii")])
    cfg = config.parse_config(text)
    levels, run_kw, _ = config.levels_from_config(cfg, D, groupwise=True, histmatch=True)
    f_meshes = [(_on_sphere(meshio.load_surface(d + "sphere%d.surf.gii" % s)[0]), tri) for s in range(S)]
    f_datas = [meshio.load_data(d + "data%d.func.gii" % s, len(xyz)) for s in range(S)]
    f_txyz = _on_sphere(meshio.load_surface(d + "template.surf.gii")[0])
    ops = group_registration.ProductGroupOps(ctx)
    regs, _, _ = group_registration.run_group_multiresolution(ops, f_meshes, f_datas, f_txyz, tri, levels, fixnan=True, **run_kw, **config.run_options(cfg))
    for s in range(S):
        assert np.array_equal(meshio.load_surface(d + "py.sphere-%d.reg.surf.gii" % s)[0].astype(np.float32), regs[s].astype(np.float32))
    # the level's features: subjects 1 .. 3 matched to subject 0, subject 0 as it was
    timed = lambda name, fn, *a: fn(*a)  # noqa: E731
    ico = M.Mesh(ctx, *M.make_mesh_from_icosa(3))
    prep = [registration.level_features(ops, timed, M.Mesh(ctx, *f_meshes[s]), f_datas[s], ico, 2.0, False, None, False, (0.0, 0.0001))[0] for s in range(S)]
    got = registration.finish_features(ops, timed, prep, [None] * S, True, False)
    assert np.array_equal(got[0], prep[0])
    for s in range(1, S):
        assert np.array_equal(got[s], HL.histogram_match(prep[s], prep[0])) and np.abs(got[s] - prep[s]).max() > 0.5


def test_without_the_variable_both_programs_refuse(tmp_path):
    import __graft_entry__ as g

    exe = g.build_cpp_newmsm()
    xyz, tri, src, ref = pairwise_inputs()
    d = str(tmp_path) + "/"
    meshio.save_surface(d + "in.surf.gii", xyz, tri)
    meshio.save_metric(d + "in.func.gii", src)
    with open(d + "conf", "w") as f:
        f.write(PAIR_CONF + "--IN\n")
    args = ["--inmesh=" + d + "in.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "in.func.gii", "--conf=" + d + "conf", "--out=" + d + "x."]
    for cmd in ([sys.executable, "tools/register_files.py"], [exe]):
        out = _run(cmd + args, histmatch=False)
        assert out.returncode == 1 and "--IN / --INc" in out.stderr and "is not available" in out.stderr
        assert not os.path.exists(d + "x.sphere.reg.surf.gii")
