"""The dedrift stage on the GPU (msm_dedrift_*, newmsm_amd/dedrift.py) against the literal restatement (tests/dedrift_literal.py), driven by the same
caller function (dedrift.dedrift_group).

Bars: triangle ids and weights of both searches equal; inverse_s, drift, W, corrected_s to 1e-12 of the sphere's radius (fixed-order sums of +, x, /,
sqrt with contraction off; whether they are in fact bit-equal is printed); resampled_s to 1e-12 (msm_metric_resample's bar); distortion rows rtol 1e-9 /
atol 1e-12 (device log2 against glibc) on inputs whose restated min J exceeds 0.2 with no folded triangle; mean / stdev to 1e-12; cc to 1e-9 absolute
(wavefront-parallel sums); dice exactly (the masks are identical; no value ties with its threshold, asserted on the restatement)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import dedrift_literal as L
from tests import hierarchy_literal as H

pytestmark = pytest.mark.gpu


def close_rel(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max()) <= tol * float(np.abs(b).max())


def compare(got, want, subjects, label):
    S = len(subjects)
    bit = dict(inverse=True, corrected=True, resampled=True)
    for s in range(S):
        for phase in ("accumulate", "correct"):
            g, w = got["searches"][s][phase], want["searches"][s][phase]
            assert np.array_equal(g["tri"], w["tri"]), "%s: subject %d, %s: triangle ids differ" % (label, s, phase)
            assert np.array_equal(g["w"], w["w"]), "%s: subject %d, %s: weights differ" % (label, s, phase)
        gi, wi = got["searches"][s]["accumulate"]["inverse"], want["searches"][s]["accumulate"]["inverse"]
        assert close_rel(gi, wi, 1e-12), "%s: inverse of subject %d" % (label, s)
        bit["inverse"] &= np.array_equal(gi, wi)
        assert close_rel(got["corrected"][s], want["corrected"][s], 1e-12), "%s: corrected sphere of subject %d" % (label, s)
        bit["corrected"] &= np.array_equal(got["corrected"][s], want["corrected"][s])
        assert np.allclose(got["resampled"][s], want["resampled"][s], rtol=1e-12, atol=1e-12), "%s: resampled data of subject %d" % (label, s)
        bit["resampled"] &= np.array_equal(got["resampled"][s], want["resampled"][s])
        minJ, folds = L.min_J_and_folds(subjects[s][0], want["corrected"][s], subjects[s][2])
        assert minJ > 0.2 and folds == 0, "%s: subject %d is too distorted for a comparison of distortion maps (min J %.3g, %d folds)" % (label, s, minJ, folds)
        err = np.abs(got["distortion"][s] - want["distortion"][s])
        print("%s: subject %d distortion max abs err %.3g (areal) %.3g (shape), min J %.3f" % (label, s, err[0].max(), err[1].max(), minJ))
        assert np.allclose(got["distortion"][s], want["distortion"][s], rtol=1e-9, atol=1e-12), "%s: distortion of subject %d" % (label, s)
    assert close_rel(got["drift"], want["drift"], 1e-12) and close_rel(got["W"], want["W"], 1e-12), label
    bit["drift"], bit["W"] = np.array_equal(got["drift"], want["drift"]), np.array_equal(got["W"], want["W"])
    print("%s: bit-equal to the restatement: %s" % (label, ", ".join("%s %s" % (k, "yes" if v else "no") for k, v in sorted(bit.items()))))
    assert L.threshold_gaps(want["resampled"]) > 0, "%s: a value ties with its percentile threshold" % label
    assert close_rel(got["mean"], want["mean"], 1e-12) and close_rel(got["stdev"], want["stdev"], 1e-12), label
    print("%s: cc max abs err %.3g" % (label, np.abs(got["cc"] - want["cc"]).max()))
    assert np.abs(got["cc"] - want["cc"]).max() <= 1e-9, label
    assert np.array_equal(got["dice"], want["dice"]), label
    assert np.allclose(got["cc_mean"], want["cc_mean"], rtol=0, atol=1e-9) and np.array_equal(got["dice_mean"], want["dice_mean"])
    for k, v in want["summary"].items():
        assert got["summary"][k] == pytest.approx(v, rel=1e-9, abs=1e-12), k


def both(ctx, template, subjects, data, label):
    from newmsm_amd import dedrift

    got = dedrift.dedrift_group(ctx, template, subjects, data, details=True)
    want = dedrift.dedrift_group(L.LiteralOps(), template, subjects, data, details=True)
    compare(got, want, subjects, label)
    return got, want


def same_bits(a, b):
    for k in ("W", "drift", "mean", "stdev", "cc", "dice"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("corrected", "resampled", "distortion"):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k


def case_a():
    txyz, ttri = O.icosphere(4)
    subjects, data = [], []
    for s, order in enumerate([3, 4, 5, 4, 3]):  # three sizes, two of them not the template's topology
        xyz, tri = O.icosphere(order)
        reg = L.smooth_warp(xyz, s)
        subjects.append((xyz, reg, tri))
        data.append(L.group_data(reg, 2, s))
    return (txyz, ttri), subjects, data


def test_mixed_meshes_against_the_restatement_and_twice(ctx):
    """(a) ico4 template, S = 5, subject meshes of three sizes, D = 2; and two runs of the whole pipeline give the same bits"""
    from newmsm_amd import dedrift

    template, subjects, data = case_a()
    got, _ = both(ctx, template, subjects, data, "case a")
    again = dedrift.dedrift_group(ctx, template, subjects, data)
    same_bits(got, again)
    # with the direction tables of the registered spheres: the same decisions, the same bits
    rays = dedrift.dedrift_group(dedrift.ProductOps(ctx, prepare_search=True), template, subjects, data)
    same_bits(got, rays)


def test_handle_reset_and_call_order(ctx):
    import newmsm_amd as M
    from newmsm_amd import dedrift

    template, subjects, data = case_a()
    tmpl = M.Mesh(ctx, *template)
    d = dedrift.Dedrift(ctx, tmpl, len(subjects))
    runs = []
    for _ in range(2):
        meshes = [M.Mesh(ctx, reg, tri) for _, reg, tri in subjects]
        with pytest.raises(M.MsmError):
            d.finish()  # nothing accumulated yet
        for m, (orig, _, _) in zip(meshes, subjects):
            d.accumulate(m, orig)
        with pytest.raises(M.MsmError):
            d.group_stats()  # no maps yet
        W, _ = d.finish()
        out = [d.correct(s, meshes[s], subjects[s][0], data[s]) for s in range(len(subjects))]
        runs.append((W, out, d.group_stats(75)))
        for s, m in enumerate(meshes):
            assert np.array_equal(m.get_coords(), out[s][0])  # the handle holds corrected_s
        d.reset()
    assert np.array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][2], runs[1][2]))
    d.close()


@pytest.mark.parametrize("S", [1, 8, 9, 17, 65])
def test_group_stats_across_the_pair_tiles(ctx, S):
    """group_stats(75) against the restatement with every subject listed and no mask, on the ico3 template (642 vertices: the last ballot word is
    partial), D = 2: a single subject, exactly one tile of 8 x 8 subjects, one past a tile, three tiles with a ragged edge -- sets this small go
    through the per-pair kernels -- and 65 subjects, one past the size up to which they do: nine tiles a side with a ragged edge, read without a list.
    The select over the whole set, which takes the tile kernels at any size, gives the same bits"""
    import newmsm_amd as M
    from newmsm_amd import dedrift

    txyz, ttri = O.icosphere(3)
    maps = [L.smooth_data(txyz, 2, s) for s in range(S)]
    assert H.threshold_gaps(maps, None, 75) > 0, "a value ties with its percentile threshold"
    want_mean, want_stdev, want_cc, want_dice = H.select_stats(maps, None, 75)[:4]
    tmpl = M.Mesh(ctx, txyz, ttri)
    d = dedrift.Dedrift(ctx, tmpl, S)
    for s, m in enumerate(maps):
        d.set_map(s, m)
    mean, stdev, cc, dice = d.group_stats(75)
    tiled = d.group_stats_select(list(range(S)), None, 75)
    d.close()
    tmpl.close()
    assert close_rel(mean, want_mean, 1e-12) and close_rel(stdev, want_stdev, 1e-12)
    assert np.abs(cc - want_cc).max() <= 1e-9
    assert np.array_equal(cc[:, range(S), range(S)], np.ones((2, S)))
    assert np.array_equal(dice, want_dice)
    assert all(np.array_equal(a, b) for a, b in zip(tiled[:4], (mean, stdev, cc, dice)))


def test_group_run_warps_at_ico6(ctx):
    """(b) ico6, S = 8, D = 2, all on the template's topology, the warps of a real short groupwise run (one level, two iterations)"""
    import newmsm_amd as M
    from newmsm_amd import group_registration as GR
    from newmsm_amd import synthetic

    S, D = 8, 2
    xyz, tri = M.make_mesh_from_icosa(6)
    datas = [synthetic.features(synthetic.known_warp(xyz, seed=11 + s, rot_deg=2.0, amp=1.5), D, seed=5) for s in range(S)]
    levels = [dict(data_order=4, cp_order=2, sg_order=4, iters=2, simmeasure=2, sigma_in=2.0, cost_params=dict(lambda_=0.1, mu=0.4, kappa=1.6))]
    regs, _, _ = GR.run_group_multiresolution(GR.ProductGroupOps(ctx), [(xyz, tri)] * S, datas, xyz, tri, levels, fixnan=True)
    moved = max(L.mean_angle_deg(r, xyz)[1] for r in regs)
    assert moved > 0.01, "the groupwise run moved nothing"
    noisy = [datas[s] + 0.05 * np.random.default_rng(300 + s).standard_normal(datas[s].shape) for s in range(S)]
    subjects = [(xyz, np.asarray(regs[s]), tri) for s in range(S)]
    got, _ = both(ctx, (xyz, tri), subjects, noisy, "case b")
    print("case b: largest move of the run %.3f deg; mean pairwise cc %s, dice %s" % (moved, got["cc_mean"], got["dice_mean"]))


def test_invariance_to_a_common_drift_at_ico6(ctx):
    """(c) the CPU test's smooth synthetic warps at ico6, S = 8, as they are and with Q (2 degrees) composed onto every registered sphere: the product equals
    the restatement on both runs, and its own two runs agree to a mean angle below 0.004 degrees (measured for the restatement: 0.00042)"""
    S, D = 8, 2
    xyz, tri = O.icosphere(6)
    regs = [L.smooth_warp(xyz, s) for s in range(S)]
    data = [L.group_data(r, D, s) for s, r in enumerate(regs)]
    a, _ = both(ctx, (xyz, tri), [(xyz, r, tri) for r in regs], data, "case c")
    b, _ = both(ctx, (xyz, tri), [(xyz, r @ L.Q_COMMON.T, tri) for r in regs], data, "case c + Q")
    angles = [L.mean_angle_deg(ca, cb) for ca, cb in zip(a["corrected"], b["corrected"])]
    mean_deg, max_deg = float(np.mean([m for m, _ in angles])), max(m for _, m in angles)
    print("case c: group drift %.3f deg (+Q: %.3f); mean angle between the two runs %.5f deg, max %.5f" %
          (L.mean_angle_deg(a["drift"], xyz)[0], L.mean_angle_deg(b["drift"], xyz)[0], mean_deg, max_deg))
    print("case c: mean pairwise cc %s | %s; dice %s | %s" % (a["cc_mean"], b["cc_mean"], a["dice_mean"], b["dice_mean"]))
    assert mean_deg < 0.004


@pytest.mark.parametrize("fmt", ["GIFTI", "ASCII", "ASCII_MAT"])
def test_dedrift_files(ctx, tmp_path, fmt):
    """tools/dedrift_files.py from files to files: what it writes equals the Python call on what the input files hold, to the rounding of a float (GIFTI
    stores floats; the text formats are written with the nine digits that give a float back; FreeSurfer .asc surfaces hold doubles), and group_stats.txt
    parses to the call's figures.  A .dpv file holds the first data row only (Mesh::save_dpv)."""
    import os
    import re
    import subprocess
    import sys

    import newmsm_amd as M
    from newmsm_amd import dedrift, meshio

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = str(tmp_path) + os.sep
    (txyz, ttri), subjects, data = case_a()
    S = len(subjects)
    meshio.save_surface(d + "template.surf.gii", txyz, ttri)
    tmesh = M.Mesh(ctx, txyz, ttri)
    for s, (orig, reg, tri) in enumerate(subjects):
        meshio.save_surface(d + "sphere%d.surf.gii" % s, orig, tri)
        meshio.save_metric(d + "data%d.func.gii" % s, data[s])
        meshio.save_surface(d + "gw.sphere-%d.reg.surf.gii" % s, reg, tri)  # what the groupwise run wrote
        meshio.save_metric(d + "gw.transformed_and_reprojected-%d.func.gii" % s, M.metric_resample(M.Mesh(ctx, reg, tri), data[s], tmesh))
    with open(d + "meshes.txt", "w") as f:
        f.write("\n".join(d + "sphere%d.surf.gii" % s for s in range(S)) + "\n")
    with open(d + "data.txt", "w") as f:
        f.write("\n".join(d + "data%d.func.gii" % s for s in range(S)) + "\n")
    run = subprocess.run([sys.executable, os.path.join(root, "tools", "dedrift_files.py"), "--meshes=" + d + "meshes.txt", "--data=" + d + "data.txt",
                          "--template=" + d + "template.surf.gii", "--regs=" + d + "gw.", "--out=" + d + "dd.", "-f", fmt, "--before"],
                         cwd=root, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr

    def sphere(path):
        p, _ = meshio.load_surface(path)
        p = p - p.mean(axis=0)
        return p * (100.0 / np.linalg.norm(p, axis=1, keepdims=True))

    held = [(sphere(d + "sphere%d.surf.gii" % s), meshio.load_surface(d + "gw.sphere-%d.reg.surf.gii" % s)[0], subjects[s][2]) for s in range(S)]
    fdata = [meshio.load_data(d + "data%d.func.gii" % s, len(held[s][0])) for s in range(S)]
    ftxyz = sphere(d + "template.surf.gii")
    want = dedrift.dedrift_group(ctx, (ftxyz, ttri), held, fdata)
    before = dedrift.pairwise_stats(ctx, (ftxyz, ttri), [meshio.load_data(d + "gw.transformed_and_reprojected-%d.func.gii" % s, len(ftxyz)) for s in range(S)])
    surf_ext, data_ext = {"GIFTI": (".surf.gii", ".func.gii"), "ASCII": (".asc", ".dpv"), "ASCII_MAT": (".asc", ".txt")}[fmt]

    def as_float(a, b):  # a and b are the same floats (nine digits of text give a float back exactly; .asc surfaces hold doubles)
        return np.array_equal(np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32))

    def rows(a):
        return np.atleast_2d(a)[:1] if data_ext == ".dpv" else np.atleast_2d(a)

    W, wtri = meshio.load_surface(d + "dd.dedriftwarp" + surf_ext)
    assert as_float(W, want["W"]) and np.array_equal(wtri, ttri)
    for s in range(S):
        c, ctri = meshio.load_surface(d + "dd.sphere-%d.reg.corrected" % s + surf_ext)
        assert as_float(c, want["corrected"][s]) and np.array_equal(ctri, held[s][2])
        assert as_float(meshio.load_data(d + "dd.transformed_and_reprojected.dedrift-%d" % s + data_ext, len(ftxyz)), rows(want["resampled"][s]))
        assert as_float(meshio.load_data(d + "dd.sphere-%d.distortion" % s + data_ext, len(c)), rows(want["distortion"][s]))
    assert as_float(meshio.load_data(d + "dd.mean" + data_ext, len(ftxyz)), rows(want["mean"]))
    assert as_float(meshio.load_data(d + "dd.stdev" + data_ext, len(ftxyz)), rows(want["stdev"]))
    text = open(d + "dd.group_stats.txt").read()
    assert text == run.stdout
    figures = [float(x) for x in re.findall(r": ([-+0-9.eE]+|nan)", text)]
    expect = []
    for blk in (before, want):
        for dd in range(2):
            expect += [blk["cc_mean"][dd], blk["dice_mean"][dd]]
    sm = want["summary"]
    expect += [sm["areal_mean"], sm["areal_max"], sm["areal_95"], sm["areal_98"], sm["shape_mean"], sm["shape_max"]]
    assert figures == [float("{:.4}".format(float(v))) for v in expect]
