"""msm_resample_plan_*: weights built once, applied to many maps.  Everything is compared with np.array_equal -- the arithmetic contract of
include/msmhip.h (FP64 sums in stored order, one rounding for float32) leaves no room for a tolerance.  Cases: tests/test_resample_plan_cpu.py: case."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import _lib, meshio, synthetic
from oracle import oracle as O
from tests import resample_literal as RL
from tests.test_resample_plan_cpu import case, load_tool, tie_keys

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = M.PLAN_TILE
DS = (1, T - 1, T, T + 1, 70)
DMAX = max(DS)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case's inputs and the oracle's results for DMAX maps, computed once; every test takes the first D rows (the maps are independent)"""
    xin, tin, xnew, tnew, excl = case(name)
    oi, on = O.Mesh(xin, tin), O.Mesh(xnew, tnew)
    data = synthetic.features(xin, DMAX, seed=5)
    d32 = data.astype(np.float32)
    r = dict(xin=xin, tin=tin, xnew=xnew, tnew=tnew, excl=excl, data=data, d32=d32, weights=O.adaptive_barycentric_weights(oi, on, excl))
    if excl is None:
        r["want"] = O.metric_resample(oi, data, on)
        r["want32"] = O.metric_resample(oi, d32.astype(np.float64), on).astype(np.float32)
    else:
        r["want"], r["mask"] = O.metric_resample_excl(oi, data, on, excl)
        r["want32"] = O.metric_resample_excl(oi, d32.astype(np.float64), on, excl)[0].astype(np.float32)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def meshes(ctx, r):
    return M.Mesh(ctx, r["xin"], r["tin"]), M.Mesh(ctx, r["xnew"], r["tnew"])


@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_weights_are_the_oracle_s(ctx, name):
    r = reference(name)
    plan = M.ResamplePlan(*meshes(ctx, r), excl=r["excl"])
    rp, col, val = plan.weights()
    orp, ocol, oval = r["weights"]
    assert np.array_equal(rp, orp) and np.array_equal(col, ocol) and np.array_equal(val, oval)
    assert plan.sizes() == (len(r["xin"]), len(r["xnew"]), len(ocol), int(np.diff(orp).max()))
    assert np.all(np.isfinite(val))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_apply_float64(ctx, name):
    r = reference(name)
    min_, mnew = meshes(ctx, r)
    plan = M.ResamplePlan(min_, mnew)
    for D in DS:
        got = plan.apply(r["data"][:D])
        assert got.dtype == np.float64 and got.shape == (D, len(r["xnew"]))
        assert np.array_equal(got, r["want"][:D]), D
    assert np.array_equal(plan.apply(r["data"]), M.metric_resample(min_, r["data"], mnew))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_apply_float32(ctx, name):
    r = reference(name)
    plan = M.ResamplePlan(*meshes(ctx, r))
    for D in DS:
        got = plan.apply(r["d32"][:D])
        assert got.dtype == np.float32 and got.shape == (D, len(r["xnew"]))
        assert np.array_equal(got, r["want32"][:D]), D


def test_mask(ctx):
    r = reference("E")
    min_, mnew = meshes(ctx, r)
    plan = M.ResamplePlan(min_, mnew, excl=r["excl"])
    empty = np.diff(r["weights"][0]) == 0
    assert empty.sum() == 65
    for D in (1, DMAX):
        got, mask = plan.apply(r["data"][:D])
        assert np.array_equal(got, r["want"][:D]) and np.array_equal(mask, r["mask"])
        assert np.all(got[:, empty] == 0) and np.all(np.isfinite(got)) and np.all(np.isfinite(mask))
        got32, mask32 = plan.apply(r["d32"][:D])
        assert got32.dtype == np.float32 and np.array_equal(got32, r["want32"][:D]) and np.array_equal(mask32, r["mask"])
    m_out, m_mask = M.metric_resample(min_, r["data"], mnew, excl=r["excl"])
    got, mask = plan.apply(r["data"])
    assert np.array_equal(got, m_out) and np.array_equal(mask, m_mask)


CHUNK_KB = 100


def child(path):
    """run by test_slabs in a process of its own, with MSMHIP_PLAN_CHUNK_KB set: case A at D = 70 in both dtypes, and the staging blocks around it"""
    r = reference("A")
    ctx = M.Context(0)
    plan = M.ResamplePlan(*meshes(ctx, r))
    s0 = ctx.staging_stats()
    out64 = plan.apply(r["data"])
    s1 = ctx.staging_stats()
    out32 = plan.apply(r["d32"])
    s2 = ctx.staging_stats()
    keys = np.stack([tie_keys(r["xin"])] * 3 + [np.arange(len(r["xin"])) % 5]).astype(np.int32)
    np.savez(path, out64=out64, out32=out32, labels=plan.apply_labels(keys), stats=np.array([[s[k] for k in ("blocks", "bytes", "allocated", "waits")] for s in (s0, s1, s2)]))
    plan.close()
    ctx.close()


def test_slabs(ctx, tmp_path):
    """A budget of 100 KiB of maps holds 102400 // ((642 + 162) * 8) = 15 float64 maps or 31 float32 maps of case A: D = 70 goes in 5 slabs (15 x 4 + 10)
    and in 3 (31 + 31 + 8), each with a ragged last one; four rows of int32 keys (31 per slab) in one.  The bits do not depend on the slabs.

    Staging blocks (stager.cpp): a copy takes room in the open block; a block that is full is retired and a free or new block of at least
    max(MSMHIP_STAGE_MIN_KB = 4 MiB, 1.25 x the request) is opened.  Everything an apply of case A stages, 70 x (642 + 162) x 8 = 450 240 bytes in and
    out, is less than one block, so whatever the number of slabs an apply retires the open block at most once: at most ONE block more than before,
    of the smallest size, and no wait for a busy block."""
    r = reference("A")
    assert CHUNK_KB * 1024 // ((len(r["xin"]) + len(r["xnew"])) * 8) == 15 and CHUNK_KB * 1024 // ((len(r["xin"]) + len(r["xnew"])) * 4) == 31
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, MSMHIP_PLAN_CHUNK_KB=str(CHUNK_KB))
    env.pop("MSMHIP_STAGE_MIN_KB", None)
    run = subprocess.run([sys.executable, "-c", "import tests.test_gpu_resample_plan as t; t.child(%r)" % path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr + run.stdout
    got = np.load(path)
    plan = M.ResamplePlan(*meshes(ctx, r))  # this process: the default budget, one slab
    assert np.array_equal(got["out64"], plan.apply(r["data"])) and np.array_equal(got["out64"], r["want"])
    assert np.array_equal(got["out32"], plan.apply(r["d32"])) and np.array_equal(got["out32"], r["want32"])
    keys = np.stack([tie_keys(r["xin"])] * 3 + [np.arange(len(r["xin"])) % 5]).astype(np.int32)
    assert np.array_equal(got["labels"], plan.apply_labels(keys))
    s0, s1, s2 = got["stats"]
    for before, after in ((s0, s1), (s1, s2)):
        assert 0 <= after[2] - before[2] <= 1 and after[1] - before[1] <= (4 << 20) * (after[2] - before[2]) and after[3] == before[3], got["stats"]


def test_snapshot(ctx):
    """a plan owns its rows: later resampling on the context, new coordinates of its source and the end of its target change nothing"""
    r, rc = reference("A"), reference("C")
    min_, mnew = meshes(ctx, r)
    plan = M.ResamplePlan(min_, mnew)
    cin, cnew = meshes(ctx, rc)
    assert np.array_equal(M.metric_resample(cin, rc["data"][:2], cnew), rc["want"][:2])  # the context's weight scratch now holds case C's rows
    min_.set_coords(synthetic.known_warp(r["xin"], seed=3, rot_deg=20.0))
    mnew.close()
    assert np.array_equal(plan.apply(r["data"]), r["want"]) and np.array_equal(plan.apply(r["d32"]), r["want32"])
    rp, col, val = plan.weights()
    assert np.array_equal(rp, r["weights"][0]) and np.array_equal(col, r["weights"][1]) and np.array_equal(val, r["weights"][2])
    min_.close()
    assert np.array_equal(plan.apply(r["data"][:3]), r["want"][:3])


def test_nearest(ctx):
    r, re_ = reference("A"), reference("E")
    oin = O.Mesh(r["xin"], r["tin"])
    data = r["data"][:5]
    plan = M.ResamplePlan(*meshes(ctx, r), method="nearest")
    assert plan.sizes()[2:] == (len(r["xnew"]), 1)
    assert np.array_equal(plan.apply(data), O.nearest_neighbour(oin, data, r["xnew"]))
    assert np.array_equal(plan.apply(r["d32"][:5]), O.nearest_neighbour(oin, r["d32"][:5].astype(np.float64), r["xnew"]).astype(np.float32))
    masked = M.ResamplePlan(*meshes(ctx, re_), method="nearest", excl=re_["excl"])
    got, mask = masked.apply(data)
    want, wmask = O.nearest_neighbour_excl(oin, data, r["xnew"], re_["excl"])
    assert np.array_equal(got, want) and np.array_equal(mask, wmask)


def test_barycentric_is_surface_resample(ctx):
    r = reference("B")
    min_, mnew = meshes(ctx, r)
    anat = synthetic.anatomy(r["xin"])
    plan = M.ResamplePlan(min_, mnew, method="barycentric")
    got = plan.apply(np.ascontiguousarray(anat.T)).T
    assert np.array_equal(got, O.surface_resample(anat, O.Octree(O.Mesh(r["xin"], r["tin"])), r["xnew"]))
    assert np.array_equal(got, M.barycentric_coords_resample(min_, anat, r["xnew"]))
    rp, col, val = plan.weights()
    assert np.all(np.diff(rp) == 3) and np.all(np.diff(col.reshape(-1, 3), axis=1) > 0)  # ascending ids within a row


def label_rows(xyz):
    f = synthetic.features(xyz, 1, seed=11)[0]
    return np.stack([tie_keys(xyz), np.floor(3 * f).astype(np.int32), (np.arange(len(xyz)) % 5).astype(np.int32)])


@pytest.mark.parametrize("name", ["A", "C", "D", "E"])
def test_labels(ctx, name):
    xin, tin, xnew, tnew, excl = case(name)
    plan = M.ResamplePlan(M.Mesh(ctx, xin, tin), M.Mesh(ctx, xnew, tnew), excl=excl)
    rp, col, val = plan.weights()
    keys = label_rows(xin)
    want, tied = RL.label_vote(rp, col, val, keys, unassigned=-77, excl=excl)
    assert np.array_equal(plan.apply_labels(keys, unassigned=-77), want)
    want1, tied1 = RL.label_vote(rp, col, val, keys[:1], unassigned=-77, excl=excl)
    got1 = plan.apply_labels(keys[0], unassigned=-77)
    assert got1.dtype == np.int32 and np.array_equal(got1, want1)
    if name == "D":
        assert tied1 == 8  # the tie rule decided rows: it is exercised, not skipped
    if name == "E":
        empty = np.diff(rp) == 0
        kept = np.array([np.any(excl[col[rp[k]:rp[k + 1]]] != 0) for k in range(len(rp) - 1)])  # rows with an entry the mask keeps
        assert empty.sum() == 65 and not np.any(kept & empty) and np.all(want[:, ~kept] == -77) and np.all(want[:, kept] != -77)


def dev_child():
    """run by test_apply_dev in a process of its own that imported torch FIRST (the library then shares torch's HIP runtime; the other way round
    torch finds no device): case A at D = 33 in both dtypes, on tensors filled on torch's stream"""
    import torch

    r = reference("A")
    ctx = M.Context(0)
    plan = M.ResamplePlan(*meshes(ctx, r))
    D = 33
    for host, want in ((r["data"][:D], r["want"][:D]), (r["d32"][:D], r["want32"][:D])):
        t = torch.from_numpy(np.array(host)).to("cuda", non_blocking=True)  # a fill on torch's stream ...
        out = torch.full((D, len(r["xnew"])), float("nan"), dtype=t.dtype, device="cuda")
        ctx.wait_stream(torch.cuda.current_stream().cuda_stream)  # ... that the library's stream waits for
        res = plan.apply_dev(t, out)
        assert res is out
        got = out.cpu().numpy()
        assert got.dtype == host.dtype and np.array_equal(got, want) and np.array_equal(got, plan.apply(host))
        again = plan.apply_dev(t.data_ptr(), out=torch.empty_like(out), D=D, dtype=host.dtype)  # plain addresses
        assert np.array_equal(again.cpu().numpy(), want)
    plan.close()
    ctx.close()


def test_apply_dev():
    run = subprocess.run([sys.executable, "-c", "import torch; import tests.test_gpu_resample_plan as t; t.dev_child()"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout


def test_refusals(ctx):
    r = reference("A")
    min_, mnew = meshes(ctx, r)
    L = M.lib()

    def message():
        return L.msm_last_error().decode()

    other = M.Context(0)
    foreign = M.Mesh(other, r["xnew"], r["tnew"])
    assert not L.msm_resample_plan_create(min_.h, foreign.h, 0, None) and "context" in message()
    foreign.close()
    other.close()
    assert not L.msm_resample_plan_create(min_.h, mnew.h, 3, None) and "method" in message()
    with pytest.raises(ValueError):
        M.ResamplePlan(min_, mnew, method="linear")
    plan = M.ResamplePlan(min_, mnew)
    data, out = r["data"][:2], np.zeros((2, len(r["xnew"])))
    for status in (L.msm_resample_plan_apply(plan.h, data.ctypes.data, 2, 2, out.ctypes.data, None),          # unknown dtype
                   L.msm_resample_plan_apply(plan.h, data.ctypes.data, 0, -1, out.ctypes.data, None),         # D < 0
                   L.msm_resample_plan_apply(plan.h, None, 0, 2, out.ctypes.data, None),                      # NULL arrays with D > 0
                   L.msm_resample_plan_apply(plan.h, data.ctypes.data, 1, 2, None, None),
                   L.msm_resample_plan_apply_dev(plan.h, None, 0, 2, None),
                   L.msm_resample_plan_apply_dev(plan.h, None, 5, 0, None),
                   L.msm_resample_plan_apply_labels(plan.h, None, 1, 0, None),
                   L.msm_resample_plan_apply_labels(plan.h, None, -1, 0, None)):
        assert status == -1 and message()
    rp, col, val = (np.zeros(len(r["xnew"]) + 1, np.int32), np.zeros(plan.nnz, np.int32), np.zeros(plan.nnz))
    assert L.msm_resample_plan_weights(plan.h, rp.ctypes.data_as(_lib.c_ip), col.ctypes.data_as(_lib.c_ip), val.ctypes.data_as(_lib.c_dp), plan.nnz - 1) == -1
    assert "entries" in message()
    with pytest.raises(TypeError):
        plan.apply(r["data"].astype(np.float16))
    with pytest.raises(TypeError):
        plan.apply(np.zeros((1, len(r["xin"])), dtype=np.int32))
    # D == 0: a successful no-op
    for dt in (np.float64, np.float32):
        got = plan.apply(np.zeros((0, len(r["xin"])), dtype=dt))
        assert got.shape == (0, len(r["xnew"])) and got.dtype == dt
    assert plan.apply_labels(np.zeros((0, len(r["xin"])), dtype=np.int32)).shape == (0, len(r["xnew"]))
    assert L.msm_resample_plan_apply(plan.h, None, 0, 0, None, None) == 0 and L.msm_resample_plan_apply_dev(plan.h, None, 1, 0, None) == 0
    # a failed search fails the creation: one target vertex outside the source tree's box (its own tree is not needed by these two methods)
    xfar = r["xnew"].copy()
    xfar[0] = (0.0, 150.0, 0.0)
    far = M.Mesh(ctx, xfar, r["tnew"])
    for method in (1, 2):
        assert not L.msm_resample_plan_create(min_.h, far.h, method, None) and "bounding box" in message()
    with pytest.raises(M.MsmError) as e:
        M.ResamplePlan(min_, far, method="nearest")
    assert "bounding box" in str(e.value)
    assert np.array_equal(plan.apply(data), r["want"][:2])  # the context stays usable


def test_middle_size(ctx):
    """ico5 -> ico4, D = 64, float32: 641 workgroups of the row kernel, more than one per XCD"""
    xin, tin, xnew, tnew, _ = case("M")
    d32 = synthetic.features(xin, 4, seed=5).astype(np.float32)
    d32 = np.ascontiguousarray(np.tile(d32, (16, 1)) * np.arange(1, 65, dtype=np.float32)[:, None])
    want = O.metric_resample(O.Mesh(xin, tin), d32.astype(np.float64), O.Mesh(xnew, tnew)).astype(np.float32)
    got = M.ResamplePlan(M.Mesh(ctx, xin, tin), M.Mesh(ctx, xnew, tnew)).apply(d32)
    assert got.dtype == np.float32 and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ tools/resample_files.py
def tool_inputs(tmp_path):
    """files as meshio writes them: a warped ico3 sphere at radius 70 (the tool rescales), two metric files, a label file, an anatomy, a warp"""
    xin, tin = O.icosphere(3)
    xin = synthetic.known_warp(xin, seed=21, rot_deg=5.0, amp=1.0)
    p = {k: str(tmp_path / v) for k, v in dict(sphere="in.sphere.surf.gii", myelin="myelin.func.gii", rest="rest.func.gii", parc="parc.label.gii",
                                                anat="in.anat.surf.gii", warp="warp.sphere.surf.gii", target="ref.sphere.surf.gii").items()}
    meshio.save_surface(p["sphere"], xin * 0.7, tin)
    meshio.save_metric(p["myelin"], synthetic.features(xin, 2, seed=5))
    meshio.save_metric(p["rest"], synthetic.features(xin, 5, seed=9))
    meshio.save_label(p["parc"], label_rows(xin)[:2], '<LabelTable>\n<Label Key="1" Red="1" Green="0" Blue="0" Alpha="1"><![CDATA[one]]></Label>\n</LabelTable>')
    meshio.save_surface(p["anat"], synthetic.anatomy(xin), tin)
    meshio.save_surface(p["warp"], synthetic.known_warp(xin, seed=8, rot_deg=2.0, amp=0.5), tin)
    xt, tt = O.icosphere(2)
    meshio.save_surface(p["target"], synthetic.known_warp(xt, seed=2, rot_deg=1.0, amp=0.3) * 1.1, tt)
    return p, tin


def rescaled(path):
    xyz, tri = meshio.load_surface(path)
    xyz = np.ascontiguousarray(xyz)
    O.lib().orc_true_rescale(xyz.ctypes.data_as(O.c_dp), len(xyz), O.C.c_double(100.0))
    return xyz, tri


def f32(a):
    return np.asarray(a).astype(np.float32)


def test_tool_programs(ctx, tmp_path):
    tool = load_tool()
    p, tin = tool_inputs(tmp_path)
    xs, _ = rescaled(p["sphere"])
    oin = O.Mesh(xs, tin)
    myelin = meshio.load_metric(p["myelin"])
    base = str(tmp_path / "out")
    common = ["--current_sphere=" + p["sphere"], "--output=" + base]

    assert tool.main(["metric-resample", "--metric_in=" + p["myelin"], "--ico=2"] + common) == 0
    x2, t2 = O.icosphere(2)
    got = meshio.load_metric(base + "-resampled_data.func.gii", dtype=np.float32)
    assert np.array_equal(got, f32(O.metric_resample(oin, myelin, O.Mesh(x2, t2))))

    assert tool.main(["NN-resample", "--metric_in=" + p["myelin"], "--ico=3"] + common) == 0
    x3, t3 = O.icosphere(3)
    got = meshio.load_metric(base + "-resampled_data.func.gii", dtype=np.float32)
    assert np.array_equal(got, f32(O.nearest_neighbour(oin, myelin, x3)))
    sx, st = meshio.load_surface(base + "-sphere.surf.gii")
    assert np.array_equal(f32(sx), f32(x3)) and np.array_equal(st, t3)

    assert tool.main(["surface-resample", "--surface_in=" + p["anat"], "--ico=2"] + common) == 0
    anat, _ = meshio.load_surface(p["anat"])
    ax, at = meshio.load_surface(base + "-anat.surf.gii")
    assert np.array_equal(f32(ax), f32(O.surface_resample(anat, O.Octree(oin), x2))) and np.array_equal(at, t2)
    sx, st = meshio.load_surface(base + "-sphere.surf.gii")
    assert np.array_equal(f32(sx), f32(x2)) and np.array_equal(st, t2)

    assert tool.main(["smoothing", "--metric_in=" + p["myelin"], "--sigma=10"] + common) == 0
    got = meshio.load_metric(base + "-smoothed_data.func.gii", dtype=np.float32)
    assert np.array_equal(got, f32(O.smooth_data(oin, myelin, oin, 10.0)))

    assert tool.main(["applywarp", "--to_be_deformed=" + p["sphere"], "--warp=" + p["warp"], "--output=" + base]) == 0
    xw, _ = rescaled(p["warp"])
    wx, wt = meshio.load_surface(base + "warped.surf.gii")
    assert np.array_equal(f32(wx), f32(O.sphere_project_warp(xs, oin, xw))) and np.array_equal(wt, tin)


def test_tool_many_inputs_through_one_plan(ctx, tmp_path):
    tool = load_tool()
    p, tin = tool_inputs(tmp_path)
    both, one = str(tmp_path / "both"), str(tmp_path / "one")
    common = ["--current_sphere=" + p["sphere"], "--new_sphere=" + p["target"]]
    assert tool.main(["metric-resample", "--metric_in=" + p["myelin"], "--metric_in=" + p["rest"], "--label_in=" + p["parc"], "--output=" + both] + common) == 0
    for k in ("myelin", "rest"):
        assert tool.main(["metric-resample", "--metric_in=" + p[k], "--output=" + one + k] + common) == 0
        assert open(both + "-%s-resampled_data.func.gii" % k, "rb").read() == open(one + k + "-resampled_data.func.gii", "rb").read()
    assert tool.main(["metric-resample", "--label_in=" + p["parc"], "--output=" + one] + common) == 0
    assert open(both + "-resampled_data.label.gii", "rb").read() == open(one + "-resampled_data.label.gii", "rb").read()
    # and they are the oracle's composition
    xs, _ = rescaled(p["sphere"])
    xt, tt = rescaled(p["target"])
    oin, onew = O.Mesh(xs, tin), O.Mesh(xt, tt)
    got = meshio.load_metric(both + "-rest-resampled_data.func.gii", dtype=np.float32)
    assert got.shape == (5, len(xt)) and np.array_equal(got, f32(O.metric_resample(oin, meshio.load_metric(p["rest"]), onew)))
    keys, table = meshio.load_label(both + "-resampled_data.label.gii")
    src_keys, src_table = meshio.load_label(p["parc"])
    assert table == src_table and np.array_equal(keys, RL.label_vote(*O.adaptive_barycentric_weights(oin, onew), src_keys)[0])


def test_tool_exit_status():
    for argv, sentence in ((["metric-resample", "--current_sphere=s", "--ico=3", "--output=o"], "metric_in was not set, but required."),
                           (["applywarp", "--to_be_deformed=s", "--output=o"], "warp was not set, but required.")):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resample_files.py")] + argv, capture_output=True, text=True, timeout=60)
        assert run.returncode == 1 and run.stdout.strip() == sentence
