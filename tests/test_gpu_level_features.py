"""msm_level_features: a level's featurespace::initialise for all data sets in one call, with create_exclusion, the masked
list surgery and the masked sums on the device.  Every case compares BYTES with the composition of the existing entry points on the same context
(registration.composed_level_features over ProductOps: msm_create_exclusion, msm_metric_resample, msm_smooth_data, msm_histogram_match,
msm_variance_normalise) and helpers.ulp_close with the same composition over the oracle (tests/histmatch_literal.py for the matching).  The shapes are
the smallest at which each kernel path can go wrong: 1, 8 and 64 lanes per row, forward and reverse lists, empty rows, the long-list sort."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import histmatch_literal as HL
import newmsm_amd as M
import trans_excl_cases as T
from helpers import angles, ulp_close
from newmsm_amd import _lib, api, group_registration, meshio, registration, synthetic
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_SHORT_LIST = 16  # resample_kernels.hip: kShortList


class LiteralOps(HL.LiteralMatchMixin, T.MaskOracleOps):
    pass


def timed(name, fn, *a):
    return fn(*a)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def native(order, seed, D, cap=True, regular=False):
    """an irregular sphere (a smoothly warped icosphere, as a subject's native mesh is) with D feature rows, exactly 0 above CAP_Z when cap"""
    xyz, tri = M.make_mesh_from_icosa(order)
    if not regular:
        xyz = synthetic.known_warp(xyz, seed=seed, rot_deg=0.0, amp=0.7)
    data = synthetic.features(synthetic.known_warp(xyz, seed=seed + 50, rot_deg=3.0, amp=2.0), D, seed)
    if cap:
        data[:, xyz[:, 2] > T.CAP_Z] = 0.0
    for a in (xyz, tri, data):
        a.setflags(write=False)
    return xyz, tri, data


def both(ctx, grid_order, natives, sigmas, exclude, intensity, varnorm):
    """(one call, composition on the same context, composition over the oracle), each (features n x D x V, masks n x V or None)"""
    gxyz, gtri = M.make_mesh_from_icosa(grid_order)
    ops = registration.ProductOps(ctx)
    grid = ops.mesh(gxyz, gtri)
    meshes = [ops.mesh(x, t) for x, t, _ in natives]
    datas = [d for _, _, d in natives]
    got = api.level_features(grid, meshes, datas, sigmas, exclude=exclude, intensity=intensity, varnorm=varnorm, cutthr=T.CUTTHR)
    lit = LiteralOps(None)
    out = [got]
    for o, g, ms in ((ops, grid, meshes), (lit, O.Mesh(gxyz, gtri), [O.Mesh(x, t) for x, t, _ in natives])):
        f, m = registration.composed_level_features(o, timed, g, ms, datas, sigmas, exclude, intensity, varnorm, T.CUTTHR)
        out.append((np.stack([np.atleast_2d(x) for x in f]), np.stack(m) if exclude else None))
    return out


def check(ctx, grid_order, natives, sigmas, exclude=True, intensity=False, varnorm=False, nan_ok=False):
    (f, m), (cf, cm), (of, om) = both(ctx, grid_order, natives, sigmas, exclude, intensity, varnorm)
    print("level features: max |f - composition| %.3e, max |f - oracle| %.3e" % (float(np.nanmax(np.abs(f - cf))), float(np.nanmax(np.abs(f - of)))))
    assert same_bytes(f, cf), "features differ from the composition of the entry points"
    assert nan_ok or not np.isnan(f).any()
    assert np.array_equal(np.isnan(f), np.isnan(of)) and ulp_close(f, of)
    if exclude:
        assert same_bytes(m, cm), "masks differ from the composition of the entry points"
        assert np.array_equal(np.isnan(m), np.isnan(om)) and ulp_close(m, om)
        kept = (m > 0).sum(axis=1)
        assert np.all(kept >= 0.05 * m.shape[1]) and np.all(kept <= 0.95 * m.shape[1]), kept  # the cap condition
    else:
        assert m is None and cm is None
    return f, m


# ---------------------------------------------------------------- one data set: every row route of the surgery and the apply
def test_coarser_grid_medium_rows(ctx):
    """irregular ico4 native onto the ico3 grid: the transposed reverse lists win, rows of about 12 entries (8 lanes per row); D = 2, sigma 2, --VN"""
    nat = native(4, 11, 2)
    rp, _, _ = api.get_adaptive_barycentric_weights(M.Mesh(ctx, nat[0], nat[1]), M.Mesh(ctx, *M.make_mesh_from_icosa(3)))
    assert 6 < np.diff(rp).mean() <= 96
    check(ctx, 3, [nat], [2.0], varnorm=True)


def test_finer_grid_forward_lists_and_empty_rows(ctx):
    """irregular ico3 native onto the ico4 grid: the forward lists win (a lane per row); a grid vertex whose closest native vertex is cut has an empty
    row -- feature 0 and mask 0"""
    nat = native(3, 12, 2)
    gxyz, gtri = M.make_mesh_from_icosa(4)
    f, m = check(ctx, 4, [nat], [0.0])
    closest = O.Octree(O.Mesh(nat[0], nat[1])).closest_vertex(gxyz)
    cut = (nat[0][:, 2] > T.CAP_Z)[np.asarray(closest)]
    assert 50 < cut.sum() < len(gxyz) and np.all(m[0][cut] == 0.0) and np.all(f[0][:, cut] == 0.0) and (m[0][~cut] > 0).any()


def test_long_lists(ctx):
    """irregular ico5 native onto ico2: rows of about 190 entries -- beyond kShortList, so k_sort_long_lists sorts the transposed reverse lists and the
    64-lanes-per-row kernels walk them; sigma 4, --VN"""
    nat = native(5, 13, 2)
    rp, col, _ = api.get_adaptive_barycentric_weights(M.Mesh(ctx, nat[0], nat[1]), M.Mesh(ctx, *M.make_mesh_from_icosa(2)))
    rows = np.diff(rp)
    assert rows.min() > K_SHORT_LIST and 3.0 * len(nat[0]) / len(rows) > 96 and len(col) == rp[-1] > 96 * len(rows)  # the long-list route, 64 lanes per row
    check(ctx, 2, [nat], [4.0], varnorm=True)


def test_coincident_meshes_keep_the_reference_rim_nans(ctx):
    """a regular ico3 onto the ico3 grid with the cap: weights of exactly 0 meet a scatter sum of 0 at the rim of the cut (R/resampler.cpp:72-140); the
    NaNs sit where the oracle has them (tests/test_gpu_trans_excl.py: test_excl_on_a_native_mesh_that_coincides_with_the_grid)"""
    nat = native(3, 14, 2, True, True)
    f, m = check(ctx, 3, [nat], [0.0], nan_ok=True)
    assert np.isnan(f).any()


# ---------------------------------------------------------------- the switches
def test_all_three_switches_three_data_sets(ctx):
    """exclude, intensity and varnorm: three data sets on native meshes of their own (two resolutions), so two sources are matched to data set 0"""
    nats = [native(4, 21, 2), native(3, 22, 2), native(4, 23, 2)]
    f, m = check(ctx, 3, nats, [2.0, 2.0, 2.0], exclude=True, intensity=True, varnorm=True)
    plain, _ = check(ctx, 3, nats, [2.0, 2.0, 2.0], exclude=True, intensity=False, varnorm=True)
    assert same_bytes(f[0], plain[0]) and not np.allclose(f[1:], plain[1:], atol=1e-3)  # the matching changed the sources and only them


def test_no_switch_is_the_unmasked_device_route(ctx):
    """nothing on: mask is NULL and the bytes are msm_metric_resample's and msm_smooth_data's without masks (sigma > 0 and sigma 0 side by side)"""
    nats = [native(4, 21, 2, False), native(3, 22, 2, False)]
    f, m = check(ctx, 3, nats, [2.0, 0.0], exclude=False)
    grid = M.Mesh(ctx, *M.make_mesh_from_icosa(3))
    assert same_bytes(f[1], api.metric_resample(M.Mesh(ctx, nats[1][0], nats[1][1]), nats[1][2], grid))
    check(ctx, 3, nats, [2.0, 0.0], exclude=False, intensity=True, varnorm=True)  # --IN --VN without masks


def test_one_data_set_and_one_row(ctx):
    """n = 1 with intensity set (nothing to match), and D = 1 for three data sets: every data set's one mask row serves its one feature row"""
    check(ctx, 3, [native(4, 24, 2)], [2.0], exclude=True, intensity=True, varnorm=True)
    check(ctx, 3, [native(4, 25, 1), native(3, 26, 1), native(4, 27, 1)], [2.0, 0.0, 2.0], exclude=True, intensity=True, varnorm=True)


@pytest.mark.parametrize("n,D", [(1, 1), (3, 1), (2, 2), (17, 1)], ids=["1_row", "3_rows", "4_rows", "17_rows"])
def test_row_counts_around_the_batched_normalisation(ctx, n, D):
    """n x D = 1, 3 (one thread), 4 and 17 rows (the workers' chunks) through the one parallel section of the variance normalisation"""
    check(ctx, 2, [native(3, 30 + i, D) for i in range(n)], [0.0] * n, exclude=True, varnorm=True)


# ---------------------------------------------------------------- degenerate data sets
def degenerate(which):
    """(natives, note): beside a normal data set, one whose mask keeps nothing / one grid vertex / with a constant feature row.  Each was first
    run through O.variance_normalise on the CPU: it returns without error for all three (n = 0: var = 0 / 2^64; n = 1: var = 0 / 0 = NaN, sd = NaN,
    `var > 0` is false; constant: var = 0), so all three stay."""
    xyz, tri, data = native(4, 41, 2)
    data = np.array(data)
    if which == "nothing_kept":
        data[:] = 0.0
    elif which == "one_kept":
        keep = int(np.argmin(np.linalg.norm(xyz - M.make_mesh_from_icosa(3)[0][100], axis=1)))  # the native vertex closest to grid vertex 100
        kept = data[:, keep].copy()
        data[:] = 0.0
        data[:, keep] = np.where(np.abs(kept) > 0.01, kept, 1.0)
    else:
        data[1, :] = 0.0  # the second feature row is 0 everywhere (the first still decides the mask): its resampled values are one constant
    return [native(4, 42, 2), (xyz, tri, data)]


@pytest.mark.parametrize("which", ["nothing_kept", "one_kept", "constant"])
def test_degenerate_data_sets(ctx, which):
    nats = degenerate(which)
    (f, m), (cf, cm), (of, om) = both(ctx, 3, nats, [0.0, 0.0], True, False, True)
    raw, _ = api.level_features(M.Mesh(ctx, *M.make_mesh_from_icosa(3)), [M.Mesh(ctx, x, t) for x, t, _ in nats], [d for _, _, d in nats], [0.0, 0.0], exclude=True,
                                varnorm=False, cutthr=T.CUTTHR)
    assert same_bytes(f, cf) and same_bytes(m, cm)
    assert np.array_equal(np.isnan(f), np.isnan(of)) and ulp_close(f, of) and ulp_close(m, om)
    kept = int((m[1] > 0).sum())
    if which == "nothing_kept":
        assert kept == 0 and same_bytes(f[1], raw[1])  # features unchanged by --VN
    elif which == "one_kept":
        assert kept == 1 and np.all(f[1][:, m[1] > 0] == 0.0)  # the n - 1 == 0 division: the one value minus its mean, not divided
    else:
        assert kept > 100 and np.all(f[1][1] == 0.0) and f[1][0].std() > 0.5  # var == 0: the mean is taken off, nothing is divided
    assert 0.05 * m.shape[1] <= (m[0] > 0).sum() <= 0.95 * m.shape[1]


# ---------------------------------------------------------------- the level loops
def test_pairwise_loop_with_the_opt_in(ctx):
    """trans_excl_cases.DISCRETE_PAIR with --excl: sphere.reg, the registered grids and the labelings of the run without the option; with --IN --VN and a
    ReferenceCache (n = 1 calls, the cache filled and hit) likewise"""
    case = T.pairwise_case(order=5, D=2, cap=True)
    assert case[4].sum() == 1024
    for kw in (dict(excl=True, cutthr=T.CUTTHR), dict(excl=True, cutthr=T.CUTTHR, intensity=True), dict(cut=True, intensity=True, ref_cache=True)):
        runs = []
        for gpu in (True, False):
            lab, clock = [], {}
            k = dict(kw)
            if k.pop("ref_cache", False):
                k["ref_cache"] = registration.ReferenceCache()
            r = T.run(registration.ProductOps(ctx, features_gpu=gpu), case, T.DISCRETE_PAIR, lab, timings=clock, **k)
            assert ("level_features" in clock) == gpu and ("metric_resample" in clock) == (not gpu)
            runs.append((r, lab))
        (got, lg), (want, lw) = runs
        assert len(lg) == len(lw) == 4 and all(np.array_equal(a, b) for a, b in zip(lg, lw))
        assert same_bytes(got[0], want[0]) and all(same_bytes(a, b) for a, b in zip(got[1], want[1])) and got[2] == want[2]
    assert angles(got[0], case[0]).max() > 1e-4


@pytest.mark.parametrize("with_mask", [False, True], ids=["no_template_mask", "template_mask"])
def test_group_loop_with_the_opt_in(ctx, with_mask):
    meshes, datas, txyz, tri, levels, mask, caps = T.group_case()
    assert [int(c.sum()) for c in caps] == [257, 256, 254]
    kw = dict(mask=mask if with_mask else None, varnorm=True, fixnan=True, excl=True, cutthr=T.CUTTHR)
    runs = []
    for gpu in (True, False):
        lab = []
        r = group_registration.run_group_multiresolution(group_registration.ProductGroupOps(ctx, features_gpu=gpu), meshes, datas, txyz, tri, levels, labelings_out=lab, **kw)
        runs.append((r, lab))
    (got, lg), (want, lw) = runs
    assert len(lg) == len(lw) == 4 and all(np.array_equal(a, b) for a, b in zip(lg, lw))
    assert all(same_bytes(a, b) for a, b in zip(got[0], want[0])) and all(same_bytes(a, b) for a, b in zip(got[1], want[1]))
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got[2], want[2]))


def test_both_executables_with_the_opt_in(ctx, tmp_path):
    """MSMHIP_FEATURES=gpu: tools/register_files.py and tools/cpp/newmsm write the files they write without it (one small --excl --VN case, ASCII output,
    a fresh child process per run)"""
    import __graft_entry__ as g

    exe = g.build_cpp_newmsm()
    xyz, tri, src, ref, inside = T.pairwise_case(order=4, D=2, cap=True)
    assert 0.05 * len(xyz) <= inside.sum() <= 0.95 * len(xyz)
    d = str(tmp_path) + "/"
    with open(d + "conf", "w") as f:
        f.write("--simval=2,2\n--sigma_in=2,0\n--sigma_ref=2,2\n--lambda=0.05,0.05\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=1,2\n--SGgrid=3,4\n--datagrid=3,4\n"
                "--regoption=3\n--dopt=HOCR\n--VN\n--excl\n--cutthr=0,0.0001\n")
    meshio.save_surface(d + "in.surf.gii", xyz + 0.25, tri)
    meshio.save_surface(d + "ref.surf.gii", xyz, tri)
    meshio.save_metric(d + "in.func.gii", src)
    meshio.save_metric(d + "ref.func.gii", ref)
    common = ["--inmesh=" + d + "in.surf.gii", "--refmesh=" + d + "ref.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "ref.func.gii", "--conf=" + d + "conf",
              "--format=ASCII"]
    plain = {k: v for k, v in os.environ.items() if k != "MSMHIP_FEATURES"}
    names = ["sphere.reg.asc", "sphere.LR.reg.asc", "transformed_and_reprojected.dpv"]
    for tag, cmd in (("py", [sys.executable, "tools/register_files.py"]), ("cpp", [exe])):
        for mode, env in (("host.", plain), ("gpu.", dict(plain, MSMHIP_FEATURES="gpu"))):
            run = subprocess.run(cmd + common + ["--out=" + d + tag + mode, "-v"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stderr
            assert ("Level features in one call on the GPU" in run.stdout) == (mode == "gpu."), run.stdout  # the opt-in was read, and only where it was set
        for n in names:
            with open(d + tag + "host." + n, "rb") as fa, open(d + tag + "gpu." + n, "rb") as fb:
                assert fa.read() == fb.read(), "%s of %s differs with MSMHIP_FEATURES=gpu" % (n, tag)


# ---------------------------------------------------------------- argument checks
def test_argument_checks(ctx):
    """each of these is MSM_ERR_INVALID with a message, and nothing is written"""
    xyz, tri, data = native(3, 12, 2)
    grid, mesh = M.Mesh(ctx, *M.make_mesh_from_icosa(2)), M.Mesh(ctx, xyz, tri)
    other = M.Context(0)
    foreign = M.Mesh(other, xyz, tri)
    d = np.ascontiguousarray(data)
    feat, mask = np.zeros((1, 2, grid.V)), np.zeros((1, grid.V))
    sigma = np.zeros(1)
    c_dp = _lib.c_dp

    def call(n=1, meshes=(mesh,), rows=(d,), D=2, exclude=1, with_mask=True):
        handles = (C.c_void_p * 1)(*[m.h for m in meshes])
        ptrs = (c_dp * 1)(*[None if r is None else r.ctypes.data_as(c_dp) for r in rows])
        p = _lib.LevelFeaturesParams(exclude, 0, 0, 0, 0.0, 0.0001)
        return M.lib().msm_level_features(grid.h, n, handles, ptrs, D, sigma.ctypes.data_as(c_dp), C.byref(p), feat.ctypes.data_as(c_dp),
                                          mask.ctypes.data_as(c_dp) if with_mask else None)

    assert call() == 0 and np.abs(feat).max() > 0
    feat[:] = 0.0
    for kw, text in ((dict(n=0), "0 data sets"), (dict(n=-3), "-3 data sets"), (dict(meshes=(foreign,)), "different contexts"), (dict(with_mask=False), "mask is NULL"),
                     (dict(D=0), "0 feature rows"), (dict(D=-1), "-1 feature rows"), (dict(rows=(None,)), "data of data set 0 is NULL")):
        assert call(**kw) == -1, kw
        assert text in M.lib().msm_last_error().decode(), (kw, M.lib().msm_last_error())
        assert not feat.any()
    assert call(exclude=0, with_mask=False) == 0  # without masks NULL is what the header asks for
    foreign.close()
    other.close()
