"""The hierarchy stage on the GPU (msm_dedrift_set_warp, msm_dedrift_group_stats_select, newmsm_amd/hierarchy.py, tools/hierarchy_files.py) against the
literal restatement (tests/hierarchy_literal.py over tests/dedrift_literal.py), driven by the same caller function (hierarchy.merge_groups).

Bars, those of tests/test_gpu_dedrift.py: mean and stdev 1e-12 relative; cc 1e-9 absolute (wavefront-parallel sums); dice exactly (the masks are
identical; no value ties with its threshold, asserted on the restatement first); cc_mean 1e-9 absolute; dice_mean 1e-12 relative (the dice entries are
exact, at most 36 values in [0, 1] are added in another order).  Searches equal; W, C_g, composed_s to 1e-12 of the radius; resampled maps to 1e-12;
distortion rtol 1e-9 / atol 1e-12 on spheres whose restated min J exceeds 0.2 with no fold.  Where a mask is empty (percentile 100: nothing exceeds
the maximum) the formula's 0 / 0 is NaN on both sides, and NaN equals NaN here."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

from oracle import oracle as O
from tests import dedrift_literal as L
from tests import hierarchy_literal as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -6
KEYS = ("mean", "stdev", "cc", "dice", "cc_mean", "dice_mean")


def close_rel(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max()) <= tol * float(np.abs(b).max())


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def compare_stats(got, want, label):
    """the statistics bars; got / want: dicts of KEYS"""
    assert close_rel(got["mean"], want["mean"], 1e-12) and close_rel(got["stdev"], want["stdev"], 1e-12), label
    print("%s: cc max abs err %.3g" % (label, np.abs(got["cc"] - want["cc"]).max()))
    assert np.abs(got["cc"] - want["cc"]).max() <= 1e-9, label
    assert same(got["dice"], want["dice"]), label
    assert np.allclose(got["cc_mean"], want["cc_mean"], rtol=0, atol=1e-9, equal_nan=True), label
    assert np.allclose(got["dice_mean"], want["dice_mean"], rtol=1e-12, atol=0, equal_nan=True), label


def literal_select(maps, subjects, mask, perc):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # 0 / 0 of two empty masks
        return dict(zip(KEYS, H.select_stats([maps[s] for s in subjects], mask, perc)))


@pytest.fixture(scope="module")
def nine_maps(ctx):
    """ico3 template (642 vertices: the last ballot word is partial), S = 9 resident maps, D = 2"""
    import newmsm_amd as M
    from newmsm_amd import dedrift

    txyz, ttri = O.icosphere(3)
    maps = [L.smooth_data(txyz, 2, s) for s in range(9)]
    tmpl = M.Mesh(ctx, txyz, ttri)
    d = dedrift.Dedrift(ctx, tmpl, 9)
    for s, m in enumerate(maps):
        d.set_map(s, m)
    yield d, maps
    d.close()
    tmpl.close()


def vertex_mask(V, kept, seed):
    """a mask that keeps `kept` of V vertices: positive values of any size there; zeros, negative values and a NaN elsewhere"""
    rng = np.random.default_rng(seed)
    mask = np.zeros(V)
    mask[rng.choice(V, kept, replace=False)] = rng.uniform(0.1, 3.0, kept)
    out = np.flatnonzero(mask == 0)
    mask[out[0]] = np.nan
    mask[out[1]] = -1.0
    assert int(np.sum(mask > 0)) == kept
    return mask


@pytest.mark.parametrize("kept", [601, 37])
def test_selection_and_mask_against_numpy(nine_maps, kept):
    """the list [7, 2, 5, 0, 8] (unsorted; five subjects do not fill a tile) under a mask that keeps 601 vertices, and one that keeps 37 (fewer than one
    wavefront), at the percentiles 75, 0 and 100"""
    d, maps = nine_maps
    subjects = [7, 2, 5, 0, 8]
    mask = vertex_mask(642, kept, kept)
    for perc in (75, 0, 100):
        assert H.threshold_gaps([maps[s] for s in subjects], mask, perc) > 0, "a value ties with its percentile threshold"
        want = literal_select(maps, subjects, mask, perc)
        got = dict(zip(KEYS, d.group_stats_select(subjects, mask, perc)))
        compare_stats(got, want, "%d kept, percentile %g" % (kept, perc))
        assert np.array_equal(got["cc"][:, range(5), range(5)], np.ones((2, 5)))


def test_the_whole_set_without_a_mask_is_group_stats(nine_maps):
    d, maps = nine_maps
    mean, stdev, cc, dice = d.group_stats(75)
    got = d.group_stats_select(list(range(9)), None, 75)
    assert np.array_equal(got[0], mean) and np.array_equal(got[1], stdev)  # the same arithmetic
    assert np.array_equal(got[2], cc)
    assert np.array_equal(got[3], dice)
    assert H.threshold_gaps(maps, None, 75) > 0
    compare_stats(dict(zip(KEYS, got)), literal_select(maps, list(range(9)), None, 75), "whole set")
    again = d.group_stats_select(list(range(9)), None, 75)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)  # two calls, the same bits
    assert all(np.array_equal(a, b) for a, b in zip(d.group_stats(75), (mean, stdev, cc, dice)))


def test_one_subject(nine_maps):
    d, maps = nine_maps
    mean, stdev, cc, dice, cc_mean, dice_mean = d.group_stats_select([4], vertex_mask(642, 601, 601), 75)
    assert np.isnan(cc_mean).all() and np.isnan(dice_mean).all()
    assert np.array_equal(cc, np.ones((2, 1, 1))) and np.array_equal(dice, np.ones((2, 1, 1)))
    assert np.array_equal(mean, maps[4]) and np.array_equal(stdev, np.zeros_like(maps[4]))


def test_refusals(ctx, nine_maps):
    import ctypes as C

    import newmsm_amd as M
    from newmsm_amd import dedrift
    from newmsm_amd._lib import c_dp, c_ip, lib

    d, maps = nine_maps

    def code(call, *args):
        with pytest.raises(M.MsmError) as e:
            call(*args)
        return e.value.code

    assert code(d.group_stats_select, [1, 3, 1]) == INVALID  # repeated
    assert code(d.group_stats_select, [1, 9]) == INVALID and code(d.group_stats_select, [-1]) == INVALID  # out of range
    assert code(d.group_stats_select, [0, 1], np.zeros(642)) == INVALID  # an all-zero mask
    assert code(d.group_stats_select, [0, 1], None, 101.0) == INVALID
    none = np.zeros(0, dtype=np.int32)
    assert lib().msm_dedrift_group_stats_select(d.h, none.ctypes.data_as(c_ip), 0, None, C.c_double(75.0), None, None, None, None, None, None) == INVALID
    assert lib().msm_dedrift_set_warp(d.h, C.cast(None, c_dp)) == INVALID
    txyz, ttri = O.icosphere(3)
    tmpl = M.Mesh(ctx, txyz, ttri)
    e = dedrift.Dedrift(ctx, tmpl, 3)
    e.set_map(0, maps[0])
    e.set_map(2, maps[2])
    assert code(e.group_stats_select, [0, 1]) == STATE  # subject 1 has no maps
    assert same(e.group_stats_select([2, 0])[2], d.group_stats_select([2, 0])[2])  # the subjects that have maps serve
    e.set_warp(txyz)
    assert code(e.finish) == STATE  # nothing accumulated: set_warp does not stand for it
    e.reset()  # forgets the set warp: correct is refused again
    xyz, tri = O.icosphere(2)
    m = M.Mesh(ctx, xyz, tri)
    assert code(e.correct, 0, m, xyz, np.zeros((1, len(xyz)))) == STATE
    m.close()
    e.close()
    tmpl.close()


def test_set_warp_and_correct_equal_the_older_entry_points(ctx):
    """set_warp + correct against msm_mesh_sphere_project_warp + msm_metric_resample on the same inputs: the same bits; the warp replaced between subjects"""
    import newmsm_amd as M
    from newmsm_amd import api, dedrift

    txyz, ttri = O.icosphere(4)
    tmpl = M.Mesh(ctx, txyz, ttri)
    d = dedrift.Dedrift(ctx, tmpl, 2)
    for s, order in enumerate((3, 5)):
        xyz, tri = O.icosphere(order)
        reg = L.smooth_warp(xyz, s)
        data = L.group_data(reg, 2, s)
        W = L.smooth_warp(txyz, 40 + s, amp=1.0) * (1.0 + 0.01 * s)  # the second one is no radius-100 sphere: taken as it is
        d.set_warp(W)
        m = M.Mesh(ctx, reg, tri)
        corrected, resampled, _ = d.correct(s, m, xyz, data)
        older = M.Mesh(ctx, reg, tri)
        api.sphere_project_warp_mesh(older, tmpl, W)
        assert np.array_equal(corrected, older.get_coords()) and np.array_equal(m.get_coords(), corrected)
        assert np.array_equal(resampled, M.metric_resample(older, data, tmpl))
        assert not np.array_equal(corrected, reg)
        m.close()
        older.close()
    d.close()
    tmpl.close()


def merge_case():
    """ico4 template; two children of 2 and 3 subjects on ico3 / ico4 / ico5 meshes; child registrations: smooth warps of the template"""
    txyz, ttri = O.icosphere(4)
    children, seed = [], 0
    for g, orders in enumerate(([3, 5], [4, 3, 5])):
        subjects, data = [], []
        for order in orders:
            xyz, tri = O.icosphere(order)
            corrected = L.smooth_warp(xyz, seed, amp=1.0)
            subjects.append((xyz, corrected, tri))
            data.append(L.group_data(corrected, 2, seed))
            seed += 1
        children.append(dict(reg=L.smooth_warp(txyz, 30 + g, amp=1.0), mean=L.smooth_data(txyz, 2, 50 + g), subjects=subjects, data=data))
    return (txyz, ttri), children


def test_merge_groups_against_the_restatement(ctx):
    from newmsm_amd import hierarchy

    template, children = merge_case()
    mask = vertex_mask(len(template[0]), 2400, 7)
    want = hierarchy.merge_groups(H.LiteralOps(), template, children, mask=mask, details=True)
    got = hierarchy.merge_groups(ctx, template, children, mask=mask, details=True)
    assert got["order"] == want["order"] == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
    for g in range(2):
        for phase in ("accumulate", "correct"):
            a, b = got["searches"]["children"][g][phase], want["searches"]["children"][g][phase]
            assert np.array_equal(a["tri"], b["tri"]) and np.array_equal(a["w"], b["w"]), (g, phase)
        assert close_rel(got["child_corrected"][g], want["child_corrected"][g], 1e-12), g
        assert np.allclose(got["child_mean"][g], want["child_mean"][g], rtol=1e-12, atol=1e-12), g
        assert np.allclose(got["child_distortion"][g], want["child_distortion"][g], rtol=1e-9, atol=1e-12), g
    assert close_rel(got["W"], want["W"], 1e-12)
    for slot, (g, s) in enumerate(want["order"]):
        orig, _, tri = children[g]["subjects"][s]
        a, b = got["searches"]["subjects"][slot]["correct"], want["searches"]["subjects"][slot]["correct"]
        assert np.array_equal(a["tri"], b["tri"]) and np.array_equal(a["w"], b["w"]), slot
        assert close_rel(got["composed"][slot], want["composed"][slot], 1e-12), slot
        assert np.allclose(got["resampled"][slot], want["resampled"][slot], rtol=1e-12, atol=1e-12), slot
        minJ, folds = L.min_J_and_folds(orig, want["composed"][slot], tri)
        assert minJ > 0.2 and folds == 0, "slot %d is too distorted for a comparison of distortion maps (min J %.3g, %d folds)" % (slot, minJ, folds)
        err = np.abs(got["distortion"][slot] - want["distortion"][slot])
        print("slot %d: distortion max abs err %.3g (areal) %.3g (shape), min J %.3f" % (slot, err[0].max(), err[1].max(), minJ))
        assert np.allclose(got["distortion"][slot], want["distortion"][slot], rtol=1e-9, atol=1e-12), slot
    assert H.threshold_gaps(want["resampled"], mask, 75) > 0
    compare_stats(got, want, "parent")
    for g, slots in enumerate(([0, 1], [2, 3, 4])):
        assert H.threshold_gaps([want["resampled"][s] for s in slots], mask, 75) > 0
        compare_stats(got["children_stats"][g], want["children_stats"][g], "child %d" % g)
        assert same(got["children_stats"][g]["dice"], got["dice"][:, slots[0]:slots[-1] + 1, slots[0]:slots[-1] + 1])  # a select over its slots
    for k, v in want["summary"].items():
        assert got["summary"][k] == pytest.approx(v, rel=1e-9, abs=1e-12), k


GROUP_CONF = "--simval=2\n--sigma_in=2\n--lambda=0.001\n--it=2\n--opt=DISCRETE\n--CPgrid=1\n--SGgrid=3\n--datagrid=3\n--dopt=HOCR\n--VN\n--fixnan\n"


def test_hierarchy_files(ctx, tmp_path):
    """tools/hierarchy_files.py from files to files (ASCII_MAT): fabricated leaf outputs for groups of two subjects, a first path row, and a second one
    that names the new root as a child and runs from the files just written.  What the first row wrote equals merge_groups over the registered spheres it
    wrote (data files hold floats; .asc surfaces hold doubles)."""
    from newmsm_amd import hierarchy, meshio

    d = str(tmp_path) + os.sep
    xyz, tri = O.icosphere(3)
    meshio.save_surface(d + "template.asc", xyz, tri)
    meshio.save_surface(d + "sphere.asc", xyz, tri)
    names, groups = [], {"GA": ["a0", "a1"], "GB": ["b0", "b1"], "GC": ["c0", "c1"]}
    for g, (group, members) in enumerate(groups.items()):
        for i, name in enumerate(members):
            s = len(names)
            corrected = L.smooth_warp(xyz, s, amp=1.0)
            meshio.save_surface(d + "%s.sphere-%d.reg.corrected.asc" % (group, i), corrected, tri)
            meshio.save_matrix(d + "data-%s.txt" % name, L.group_data(corrected, 2, s), digits=9)
            names.append(name)
        meshio.save_matrix(d + "%s.mean.txt" % group, L.group_data(L.smooth_warp(xyz, 20 + g, amp=1.0), 2, 60 + g, noise=0.01), digits=9)
    with open(d + "clusters.csv", "w") as f:
        f.write("".join("%d,%s,%s\n" % (i, name, group) for group, members in groups.items() for i, name in enumerate(members)))
    with open(d + "path.csv", "w") as f:
        f.write("GA,GB,R1\nR1,GC,R2\n")
    for fname, text in (("names.txt", "\n".join(names)), ("meshes.txt", d + "sphere.asc"), ("data.txt", "\n".join(d + "data-%s.txt" % n for n in names)),
                        ("conf", GROUP_CONF)):
        with open(d + fname, "w") as f:
            f.write(text + ("\n" if fname != "conf" else ""))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hierarchy_files.py"), "--clusters=" + d + "clusters.csv", "--path=" + d + "path.csv",
                          "--subjects=" + d + "names.txt", "--meshes=" + d + "meshes.txt", "--data=" + d + "data.txt", "--template=" + d + "template.asc",
                          "--conf=" + d + "conf", "--dir=" + d, "-f", "ASCII_MAT"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr

    def sphere(path):
        p, _ = meshio.load_surface(path)
        p = p - p.mean(axis=0)
        return p * (100.0 / np.linalg.norm(p, axis=1, keepdims=True))

    def as_float(a, b):
        return np.array_equal(np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32))

    txyz, M_in = sphere(d + "template.asc"), sphere(d + "sphere.asc")
    children = []
    for g, group in enumerate(("GA", "GB")):
        reg = meshio.load_surface(d + "R1.child-%d.reg.asc" % g)[0]
        print("child %d: the registration of the mean maps moved it by %.3f degrees at most" % (g, L.mean_angle_deg(reg, txyz)[1]))
        subjects = [(M_in, meshio.load_surface(d + "%s.sphere-%d.reg.corrected.asc" % (group, i))[0], tri) for i in range(2)]
        data = [meshio.load_data(d + "data-%s.txt" % n, len(xyz)) for n in groups[group]]
        children.append(dict(reg=reg, mean=meshio.load_data(d + "%s.mean.txt" % group, len(xyz)), subjects=subjects, data=data))
    want = hierarchy.merge_groups(ctx, (txyz, tri), children)
    W, wtri = meshio.load_surface(d + "R1.dedriftwarp.asc")
    assert as_float(W, want["W"]) and np.array_equal(wtri, tri)
    for i in range(4):
        c, ctri = meshio.load_surface(d + "R1.sphere-%d.reg.corrected.asc" % i)
        assert as_float(c, want["composed"][i]) and np.array_equal(ctri, tri)
        assert as_float(meshio.load_data(d + "R1.transformed_and_reprojected.dedrift-%d.txt" % i, len(xyz)), want["resampled"][i])
        assert as_float(meshio.load_data(d + "R1.sphere-%d.distortion.txt" % i, len(xyz)), want["distortion"][i])
    assert as_float(meshio.load_data(d + "R1.mean.txt", len(xyz)), want["mean"]) and as_float(meshio.load_data(d + "R1.stdev.txt", len(xyz)), want["stdev"])
    assert open(d + "R1.clusters.csv").read() == "0,a0,R1\n1,a1,R1\n2,b0,R1\n3,b1,R1\n"
    text = open(d + "R1.group_stats.txt").read()
    assert run.stdout.startswith(text) and "Stats for group R1" in text and "GA within R1" in text and "GB within R1" in text
    figures = [float(x) for x in re.findall(r": ([-+0-9.eE]+|nan)", text)]
    expect = []
    for dd in range(2):
        expect += [want["cc_mean"][dd], want["dice_mean"][dd]]
    sm = want["summary"]
    expect += [sm["areal_mean"], sm["areal_max"], sm["areal_95"], sm["areal_98"], sm["shape_mean"], sm["shape_max"]]
    for g in range(2):
        for dd in range(2):
            expect += [want["children_stats"][g]["cc_mean"][dd], want["children_stats"][g]["dice_mean"][dd]]
    assert figures == [float("{:.4}".format(float(v))) for v in expect]
    # the second row read R1 like a leaf
    assert open(d + "R2.clusters.csv").read() == "0,a0,R2\n1,a1,R2\n2,b0,R2\n3,b1,R2\n4,c0,R2\n5,c1,R2\n"
    for i in range(6):
        assert len(meshio.load_surface(d + "R2.sphere-%d.reg.corrected.asc" % i)[0]) == len(xyz)
    assert meshio.load_data(d + "R2.mean.txt", len(xyz)).shape == (2, len(xyz)) and "R1 within R2" in open(d + "R2.group_stats.txt").read()
