"""A cohort registered to one template on the GPU: msm_surface_distortion against the literal restatement (tests/dedrift_literal.py) and against
msm_dedrift_correct's own kernel, msm_abs_summary against numpy, run_cohort against plain run_multiresolution calls, tools/cohort_files.py against
tools/register_files.py.

Bars: distortion rows rtol 1e-9 / atol 1e-12 (device log2 against glibc; the bar of tests/test_gpu_dedrift.py) on inputs whose restated min J exceeds
0.2 with no folded triangle; bit equality wherever two routes of the product are compared; the summary's maximum and percentiles equal numpy's exactly
(integer selection, numpy's own interpolation arithmetic), its mean within 2 n 2^-53 relative (any order of adding n non-negative doubles, both sides)."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import cohort, config, dedrift, meshio, registration, synthetic
from newmsm_amd._lib import c_dp, check
from oracle import oracle as O
from tests import dedrift_literal as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def trid_lists(tri, V):
    """Mpoint::trID as CSR: per vertex its triangles in ascending id"""
    ptr, ids = [0], []
    for v in range(V):
        ids += [t for t in range(len(tri)) if v in tri[t]]
        ptr.append(len(ids))
    return None, None, np.array(ptr), np.array(ids)


# ---------------------------------------------------------------- distortion
@pytest.fixture(scope="module")
def ico3_copies():
    xyz, tri = O.icosphere(3)
    assert len(xyz) == 642 and np.sum(np.bincount(tri.ravel()) == 5) == 12
    finals = [xyz.copy(), xyz @ L.rotation((3.0, -1.0, 2.0), 25.0).T, L.smooth_warp(xyz, 4)]
    for f in finals:
        minJ, folds = L.min_J_and_folds(xyz, f, tri)
        assert minJ > 0.2 and folds == 0
    want = [L.vertex_distortion(xyz, f, tri) for f in finals]
    return xyz, tri, finals, want


def test_distortion_of_three_copies_in_one_call(ctx, ico3_copies):
    xyz, tri, finals, want = ico3_copies
    got = M.surface_distortion(ctx, xyz, tri, np.stack(finals))
    assert got.shape == (3, 2, 642)
    for s in range(3):
        err = np.abs(got[s] - want[s])
        print("copy %d: distortion max abs err %.3g (areal) %.3g (shape)" % (s, err[0].max(), err[1].max()))
        assert np.allclose(got[s], want[s], rtol=1e-9, atol=1e-12), s
    assert np.abs(want[2]).max() > 1e-3 and np.abs(want[0]).max() < 1e-6 and np.abs(want[1]).max() < 1e-6  # the warp distorts, identity and rotation do not
    # the batched call is three single calls, bit for bit; and two calls give the same bits
    for s in range(3):
        assert same_bits(got[s], M.surface_distortion(ctx, xyz, tri, finals[s]))
    assert same_bits(got, M.surface_distortion(ctx, xyz, tri, np.stack(finals)))


def test_distortion_equals_the_dedrift_stage_bit_for_bit(ctx):
    """for the subjects of a small dedrift group (ico3 template): msm_surface_distortion(M_s, corrected_s) is the distortion msm_dedrift_correct returned"""
    txyz, ttri = O.icosphere(3)
    subjects, data = [], []
    for s, order in enumerate([3, 2, 3]):
        xyz, tri = O.icosphere(order)
        reg = L.smooth_warp(xyz, s)
        subjects.append((xyz, reg, tri))
        data.append(L.group_data(reg, 2, s))
    got = dedrift.dedrift_group(ctx, (txyz, ttri), subjects, data)
    for s, (orig, _, tri) in enumerate(subjects):
        mine = M.surface_distortion(ctx, orig, tri, got["corrected"][s])
        assert np.abs(got["distortion"][s]).max() > 1e-4
        assert same_bits(mine, got["distortion"][s]), "subject %d" % s  # (NaNs included, were there any)


def test_distortion_on_an_irregular_mesh_with_a_bare_vertex(ctx):
    """a warped ico2 with one vertex's triangles removed: that vertex has no triangle and gets 0; its neighbours have fewer triangles than before"""
    xyz, tri = O.icosphere(2)
    xyz = L.smooth_warp(xyz, 11, amp=3.0)
    bare = 17
    kept = tri[~np.any(tri == bare, axis=1)]
    assert len(kept) < len(tri) and bare not in kept
    finals = [L.smooth_warp(xyz, 12), L.smooth_warp(xyz, 13)]
    for f in finals:
        minJ, folds = L.min_J_and_folds(xyz, f, kept)
        assert minJ > 0.2 and folds == 0
    adj = trid_lists(kept, len(xyz))
    got = M.surface_distortion(ctx, xyz, kept, np.stack(finals))
    for s, f in enumerate(finals):
        want = L.vertex_distortion(xyz, f, kept, adj)
        assert np.allclose(got[s], want, rtol=1e-9, atol=1e-12)
        assert np.all(got[s][:, bare] == 0.0) and np.count_nonzero(got[s][0]) == len(xyz) - 1


def test_distortion_refuses_bad_arguments(ctx):
    xyz, tri = O.icosphere(1)
    V = len(xyz)
    for bad_tri in (np.where(tri == 3, V, tri), np.where(tri == 3, -1, tri)):
        with pytest.raises(M.MsmError) as e:
            M.surface_distortion(ctx, xyz, bad_tri, xyz)
        assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        M.surface_distortion(ctx, xyz, tri, np.zeros((0, V, 3)))  # S = 0
    assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        M.surface_distortion(ctx, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32), np.zeros((1, 0, 3)))  # V = 0
    assert e.value.code == -1
    assert np.all(np.isfinite(M.surface_distortion(ctx, xyz, tri, xyz)))  # the context is as usable as before


# ---------------------------------------------------------------- summary
PERCENTILES = (0.0, 50.0, 95.0, 98.0, 100.0)


def summary_values(n, seed):
    """n values with many exact ties (one decimal), both signs and signed zeros"""
    rng = np.random.default_rng(seed)
    x = np.round(rng.standard_normal(n) * 2.0, 1)
    x[rng.random(n) < 0.05] = 0.0
    x[rng.random(n) < 0.05] = -0.0
    if n >= 255:
        assert len(np.unique(np.abs(x))) < n // 2 and np.any(x < 0) and np.any(x > 0) and np.any(np.signbit(x) & (x == 0)) and np.any(~np.signbit(x) & (x == 0))
    return x


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 70001])
def test_abs_summary_against_numpy(ctx, n):
    x = summary_values(n, 100 + n)
    a = np.abs(x)
    mean, mx, values = M.abs_summary(ctx, x, PERCENTILES)
    want = np.array([np.percentile(a, p) for p in PERCENTILES])
    print("n = %d: mean rel err %.3g (bound %.3g)" % (n, abs(mean - a.mean()) / a.mean() if a.mean() else 0.0, 2 * n * 2.0 ** -53))
    assert mx == a.max()
    assert values[0] == a.min() and values[-1] == a.max()  # order statistics 0 and n - 1
    srt = np.sort(a)
    k = int(np.floor((n - 1) * 0.5))
    assert srt[k] <= values[1] <= srt[min(k + 1, n - 1)]
    assert np.array_equal(values, want), (values, want)
    assert abs(mean - a.mean()) <= 2 * n * 2.0 ** -53 * a.mean()
    again = M.abs_summary(ctx, x, PERCENTILES)
    assert same_bits([mean, mx], again[:2]) and same_bits(values, again[2])
    mean0, mx0, none = M.abs_summary(ctx, x)  # no percentile asked for
    assert same_bits([mean0, mx0], [mean, mx]) and len(none) == 0


def test_abs_summary_order_statistics_without_interpolation(ctx):
    """percentiles whose virtual index is whole: the order statistics themselves"""
    n = 70001
    x = summary_values(n, 7)
    srt = np.sort(np.abs(x))
    ps = (10.0, 25.0, 50.0, 70.0, 90.0)
    values = M.abs_summary(ctx, x, ps)[2]
    assert all(((n - 1) * (p / 100.0)) % 1 == 0 for p in ps)
    assert np.array_equal(values, srt[[(n - 1) * int(p) // 100 for p in ps]])


def test_one_nan_makes_every_output_nan(ctx):
    x = summary_values(257, 3)
    x[200] = np.nan
    mean, mx, values = M.abs_summary(ctx, x, PERCENTILES)
    assert np.isnan(mean) and np.isnan(mx) and np.all(np.isnan(values))
    assert np.isnan(np.percentile(np.abs(x), 50)) and np.isnan(np.abs(x).max())  # as numpy does


def test_abs_summary_refuses_bad_arguments(ctx):
    for x, ps in ((np.zeros(0), (50.0,)), (np.ones(4), (-1.0,)), (np.ones(4), (100.5,)), (np.ones(4), (np.nan,))):
        with pytest.raises(M.MsmError) as e:
            M.abs_summary(ctx, x, ps)
        assert e.value.code == -1
    x = np.ones(4)
    with pytest.raises(M.MsmError) as e:  # np < 0
        check(M.lib().msm_abs_summary(ctx.h, x.ctypes.data_as(c_dp), 4, None, -1, None, None, None))
    assert e.value.code == -1
    assert M.abs_summary(ctx, np.ones(4), (50.0,))[2][0] == 1.0


# ---------------------------------------------------------------- cohort
CONF = ("--simval=2,2\n--sigma_in=2,1\n--sigma_ref=2,0\n--lambda=0.05,0.05\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=2,3\n--SGgrid=4,5\n--datagrid=4,5\n"
        "--regoption=3\n--dopt=HOCR\n--VN\n")
VARIANTS = dict(plain=(CONF, {}), IN=(CONF + "--IN\n", dict(histmatch=True)), excl=(CONF + "--excl\n--cutthr=0,0.0001\n", {}),
                rigid=(CONF.replace("--opt=DISCRETE,DISCRETE", "--opt=RIGID,DISCRETE").replace("--simval=2,2", "--simval=1,2"), dict(rigid=True)))
CAP_Z = 80.0


def cohort_inputs(cap=False):
    """S = 3 subjects on warped ico4 spheres of their own (irregular native meshes), D = 2, one irregular reference sphere; cap: every data set exactly 0
    above CAP_Z of its own sphere (the medial wall of --excl)"""
    xyz, tri = M.make_mesh_from_icosa(4)
    rxyz = synthetic.known_warp(xyz, seed=3, rot_deg=0.0, amp=0.7)
    rdata = synthetic.features(rxyz, 2, 31) * 2.0 + 0.5
    subjects = []
    for s in range(3):
        sxyz = synthetic.known_warp(xyz, seed=40 + s, rot_deg=0.0, amp=1.0)
        data = synthetic.features(synthetic.known_warp(sxyz, seed=90 + s, rot_deg=3.0, amp=2.0), 2, 31)
        if cap:
            data[:, sxyz[:, 2] > CAP_Z] = 0.0
        subjects.append(dict(xyz=sxyz, tri=tri, data=data))
    if cap:
        rdata[:, rxyz[:, 2] > CAP_Z] = 0.0
    return subjects, rxyz, tri, rdata


def levels_of(variant):
    text, opt = VARIANTS[variant]
    cfg = config.parse_config(text)
    levels, run_kw, skipped = config.levels_from_config(cfg, 2, **opt)
    assert len(levels) == 2 and not skipped
    return levels, dict(run_kw, **config.run_options(cfg))


def one_by_one(ctx, subjects, rxyz, rtri, rdata, levels, run_kw):
    """the parent's way: a plain run_multiresolution per subject on one context, then transformed_data"""
    out = []
    ops = registration.ProductOps(ctx)
    for sub in subjects:
        labelings = []
        reg, regs, _ = registration.run_multiresolution(ops, sub["xyz"], sub["tri"], sub["data"], rxyz, rtri, rdata, levels, labelings_out=labelings, **run_kw)
        moved = registration.transformed_data(ops, M.Mesh(ctx, reg, sub["tri"]), sub["data"], M.Mesh(ctx, rxyz, rtri), rdata, excl=run_kw["excl"],
                                              cutthr=run_kw["cutthr"], intensity=run_kw.get("intensity", False))
        out.append(dict(sphere_reg=reg, level_regs=regs, labelings=labelings, transformed=np.array(moved)))
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cohort_equals_plain_runs(ctx, variant):
    levels, run_kw = levels_of(variant)
    assert (levels[0].get("method") == "RIGID") == (variant == "rigid") and bool(run_kw.get("intensity")) == (variant == "IN") and run_kw["excl"] == (variant == "excl")
    subjects, rxyz, rtri, rdata = cohort_inputs(cap=variant == "excl")
    want = one_by_one(ctx, subjects, rxyz, rtri, rdata, levels, run_kw)
    assert all(np.abs(w["sphere_reg"] - s["xyz"]).max() > 1e-3 for w, s in zip(want, subjects))  # the runs moved the spheres
    assert not np.array_equal(want[0]["transformed"], want[1]["transformed"])
    for workers in (1, 2):
        cache = registration.ReferenceCache()
        got = cohort.run_cohort(cohort.product_ops(0), subjects, rxyz, rtri, rdata, levels, workers=workers, ref_cache=cache, **run_kw)
        assert cache.fills == 2 and cache.hits == 4  # the reference side: prepared once per level, read by the other two subjects
        assert len(got) == 3
        for s, (g, w) in enumerate(zip(got, want)):
            label = "%s, %d workers, subject %d" % (variant, workers, s)
            assert np.array_equal(g["sphere_reg"], w["sphere_reg"]), label
            assert len(g["level_regs"]) == 2 and all(np.array_equal(a, b) for a, b in zip(g["level_regs"], w["level_regs"])), label
            assert len(g["labelings"]) == len(w["labelings"]) > 0 and all(np.array_equal(a, b) for a, b in zip(g["labelings"], w["labelings"])), label
            assert np.array_equal(g["transformed"], w["transformed"]) and np.all(np.isfinite(g["transformed"])), label


@pytest.mark.parametrize("workers", [1, 2])
def test_an_error_in_a_worker_names_the_subject(ctx, workers):
    """subject 1's triangles name a vertex its sphere does not have: the library refuses the mesh (MSM_ERR_INVALID) in the worker, the cohort stops and
    says which subject it was; a data matrix of another width than the sphere is refused before the library sees it"""
    levels, run_kw = levels_of("plain")
    subjects, rxyz, rtri, rdata = cohort_inputs()
    bad = np.array(subjects[1]["tri"])
    bad[5, 1] = len(subjects[1]["xyz"])
    broken = [subjects[0], dict(subjects[1], tri=bad), subjects[2]]
    with pytest.raises(cohort.CohortError, match="subject 1 failed: MsmError: MSM_ERR_INVALID") as e:
        cohort.run_cohort(cohort.product_ops(0), broken, rxyz, rtri, rdata, levels, workers=workers, **run_kw)
    assert isinstance(e.value.cause, M.MsmError) and e.value.cause.code == -1 and e.value.results[1] is None
    if workers == 1:
        assert e.value.results[0] is not None and e.value.results[2] is None  # subject 0 had finished, subject 2 never started
    narrow = [dict(subjects[0], data=subjects[0]["data"][:, :-1])] + subjects[1:]
    with pytest.raises(cohort.CohortError, match=r"subject 0 failed: ValueError: the subject's data is \(2, 2561\) for a sphere of 2562 vertices") as e:
        cohort.run_cohort(cohort.product_ops(0), narrow, rxyz, rtri, rdata, levels, workers=workers, **run_kw)
    assert e.value.results == [None] * 3 if workers == 1 else e.value.results[0] is None


# ---------------------------------------------------------------- the tool
def load_tool():
    spec = importlib.util.spec_from_file_location("cohort_files", os.path.join(ROOT, "tools", "cohort_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_subjects_that_share_a_mesh_file_go_in_one_call(ctx, ico3_copies):
    xyz, tri, finals, _ = ico3_copies
    tool = load_tool()
    shared = tool.distortion_maps(ctx, [("a", "d0", None), ("b", "d1", None), ("a", "d2", None)], [(xyz, tri)] * 3, finals)
    apart = tool.distortion_maps(ctx, [("a", "d0", None), ("b", "d1", None), ("c", "d2", None)], [(xyz, tri)] * 3, finals)
    assert all(same_bits(a, b) for a, b in zip(shared, apart)) and not same_bits(shared[0], shared[2])


def _sphere(path):
    p, _ = meshio.load_surface(path)
    p = p - p.mean(axis=0)
    return p * (100.0 / np.linalg.norm(p, axis=1, keepdims=True))


@pytest.mark.parametrize("fmt", ["ASCII", "GIFTI"])
def test_cohort_files_against_register_files(ctx, tmp_path, fmt):
    """tools/cohort_files.py writes, per subject, the bytes tools/register_files.py writes for that subject alone; its distortion files are
    msm_surface_distortion of the spheres it wrote; group_stats.txt holds the product's figures of the maps it wrote, which equal numpy's (cc to 1e-9
    absolute, dice exactly; mean within its bound, maximum and percentiles exactly).  The child processes run one after another."""
    subjects, rxyz, rtri, rdata = cohort_inputs()
    S = len(subjects)
    d = str(tmp_path) + os.sep
    meshio.save_surface(d + "ref.surf.gii", rxyz, rtri)
    meshio.save_metric(d + "ref.func.gii", rdata)
    for s, sub in enumerate(subjects):
        meshio.save_surface(d + "in%d.surf.gii" % s, sub["xyz"], sub["tri"])
        meshio.save_metric(d + "in%d.func.gii" % s, sub["data"])
    for name, pattern in (("meshes.txt", "in%d.surf.gii"), ("data.txt", "in%d.func.gii")):
        with open(d + name, "w") as f:
            f.write("\n".join(d + pattern % s for s in range(S)) + "\n")
    with open(d + "conf", "w") as f:
        f.write(CONF)
    surf_ext, data_ext = {"GIFTI": (".surf.gii", ".func.gii"), "ASCII": (".asc", ".dpv")}[fmt]
    env = {k: v for k, v in os.environ.items() if k not in ("MSMHIP_RIGID", "MSMHIP_HISTMATCH", "MSMHIP_HOST_THREADS")}
    ref_args = ["--refmesh=" + d + "ref.surf.gii", "--refdata=" + d + "ref.func.gii", "--conf=" + d + "conf", "-f", fmt]
    run = subprocess.run([sys.executable, "tools/cohort_files.py", "--meshes=" + d + "meshes.txt", "--data=" + d + "data.txt", "--out=" + d + "c.", "--workers=2"]
                         + ref_args, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stderr
    for s in range(S):
        one = subprocess.run([sys.executable, "tools/register_files.py", "--inmesh=" + d + "in%d.surf.gii" % s, "--indata=" + d + "in%d.func.gii" % s,
                              "--out=" + d + "p%d." % s] + ref_args, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
        assert one.returncode == 0, one.stderr
        for mine, theirs in (("sphere-%d.reg" % s + surf_ext, "sphere.reg" + surf_ext), ("sphere-%d.LR.reg" % s + surf_ext, "sphere.LR.reg" + surf_ext),
                             ("transformed_and_reprojected-%d" % s + data_ext, "transformed_and_reprojected" + data_ext)):
            with open(d + "c." + mine, "rb") as a, open(d + "p%d." % s + theirs, "rb") as b:
                assert a.read() == b.read(), mine

    def as_float(a, b):
        return np.array_equal(np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32))

    def rows(a):
        return np.atleast_2d(a)[:1] if data_ext == ".dpv" else np.atleast_2d(a)

    frxyz = _sphere(d + "ref.surf.gii")
    distortions, maps = [], []
    for s in range(S):
        orig = _sphere(d + "in%d.surf.gii" % s)
        written, wtri = meshio.load_surface(d + "c.sphere-%d.reg" % s + surf_ext)
        assert np.array_equal(wtri, subjects[s]["tri"]) and np.abs(written - orig).max() > 1e-3
        distortions.append(M.surface_distortion(ctx, orig, wtri, written))
        assert np.abs(distortions[s]).max() > 1e-4
        assert as_float(meshio.load_data(d + "c.sphere-%d.distortion" % s + data_ext, len(orig)), rows(distortions[s]))
        maps.append(meshio.load_data(d + "c.transformed_and_reprojected-%d" % s + data_ext, len(frxyz)))
    stats = dedrift.pairwise_stats(ctx, (frxyz, rtri), maps)
    assert as_float(meshio.load_data(d + "c.mean" + data_ext, len(frxyz)), rows(stats["mean"]))
    assert as_float(meshio.load_data(d + "c.stdev" + data_ext, len(frxyz)), rows(stats["stdev"]))
    # the product's figures against numpy's on the written maps
    assert L.threshold_gaps(maps) > 0
    cc, dice = L.pair_matrices(maps)
    print("cc max abs err %.3g" % np.abs(stats["cc"] - cc).max())
    assert np.abs(stats["cc"] - cc).max() <= 1e-9 and np.array_equal(stats["dice"], dice)
    want = dedrift.distortion_summary(distortions)
    areal = np.concatenate([x[0] for x in distortions])
    shape = np.concatenate([x[1] for x in distortions])
    a_mean, a_max, a_p = M.abs_summary(ctx, areal, (95.0, 98.0))
    s_mean, s_max, _ = M.abs_summary(ctx, shape)
    assert (a_max, a_p[0], a_p[1], s_max) == (want["areal_max"], want["areal_95"], want["areal_98"], want["shape_max"])
    assert abs(a_mean - want["areal_mean"]) <= 2 * areal.size * 2.0 ** -53 * want["areal_mean"]
    assert abs(s_mean - want["shape_mean"]) <= 2 * shape.size * 2.0 ** -53 * want["shape_mean"]
    # and the text holds exactly those figures, in compare_stats.py's wording
    text = open(d + "c.group_stats.txt").read()
    assert text == run.stdout and text.startswith("\tStats for group typical MSM\n")
    figures = [float(x) for x in re.findall(r": ([-+0-9.eE]+|nan)", text)]
    expect = []
    for dd in range(maps[0].shape[0]):
        expect += [stats["cc_mean"][dd], stats["dice_mean"][dd]]
    expect += [a_mean, a_max, a_p[0], a_p[1], s_mean, s_max]
    assert figures == [float("{:.4}".format(float(v))) for v in expect]
