"""msm_resample_plan_create_smooth: Gaussian smoothing as the fourth kind of plan row -- the neighbourhood sweep once, on the device, and then any
number of maps.  Cases, literal and references: tests/test_smooth_plan_cpu.py.

Tolerances.  The rows' structure (row_ptr, col) is exact: the membership test sees the reference's bits.  The weights go through the device's asin and
exp, which may differ from glibc's in the last bit: rtol 1e-12, atol 1e-14, the figure tests/test_gpu_search.py::test_smooth_data has always used for
the same expressions.  Everything that is apply arithmetic alone -- the plan against its own read-back rows, against msm_smooth_data, one entry point
against another -- is compared with np.array_equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import _lib, meshio, synthetic
from oracle import oracle as O
from tests import smooth_plan_literal as SL
from tests.test_resample_plan_cpu import case, load_tool
from tests.test_smooth_plan_cpu import DMAX, reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = M.PLAN_TILE
TOL = dict(rtol=1e-12, atol=1e-14)
# a float32 result is an FP64 value rounded once; FP64 values that differ in their last bits round to the same float32 or, across a rounding boundary,
# to neighbouring ones: one unit in the last place, 2^-23 relative
TOL32 = dict(rtol=2.0 ** -23, atol=1e-14)


def meshes(ctx, r):
    """(orig, sphLow): one mesh where the case has one sphere"""
    orig = M.Mesh(ctx, r["xorig"], r["tri"])
    return orig, (orig if r["xlow"] is r["xorig"] else M.Mesh(ctx, r["xlow"], r["tri"]))


def make_plan(ctx, r):
    return M.ResamplePlan.smoothing(*meshes(ctx, r), r["sigma"], r["excl"])


def result(r, got):
    """the maps of an apply, and the mask where the case has one"""
    if r["excl"] is None:
        assert isinstance(got, np.ndarray)
        return got, None
    return got


@pytest.mark.parametrize("name", ["P", "Q", "R", "S", "PE", "RE", "T"])
def test_rows(ctx, name):
    r = reference(name)
    lrp, lcol, lval, ldiv, lmask = r["rows"]
    plan = make_plan(ctx, r)
    rp, col, val = plan.weights()
    assert np.array_equal(rp, lrp) and np.array_equal(col, lcol)
    assert np.allclose(val, lval, **TOL), np.max(np.abs(val - lval))
    div = plan.divisors()
    assert np.allclose(div, ldiv, **TOL) and np.array_equal(div == 0, ldiv == 0)
    assert plan.sizes() == (len(r["xorig"]), len(r["xlow"]), len(lcol), int(np.diff(lrp).max()))
    assert plan.method == "smoothing" and plan.masked == (r["excl"] is not None)
    if r["excl"] is not None:
        out, mask = plan.apply(r["data"][:1])
        assert np.allclose(mask, lmask, **TOL) and np.array_equal(mask == 0, lmask == 0)
    # the divisor is the stored-order sum of the row's stored weights, to the bit
    own = np.zeros(len(div))
    for j in range(int(np.diff(rp).max())):
        k = np.nonzero(np.diff(rp) > j)[0]
        own[k] += val[rp[k] + j]
    assert np.array_equal(div, own)


def check_apply(ctx, name, Ds):
    r = reference(name)
    orig, low = meshes(ctx, r)
    plan = M.ResamplePlan.smoothing(orig, low, r["sigma"], r["excl"])
    rp, col, val = plan.weights()
    div = plan.divisors()
    for D in Ds:
        for host, want in ((r["data"][:D], r["want"][:D]), (r["d32"][:D], r["want32"][:D])):
            got, mask = result(r, plan.apply(host))
            assert got.dtype == host.dtype and got.shape == (D, len(r["xlow"]))
            assert np.array_equal(got, SL.apply(rp, col, val, div, host)), (name, D, host.dtype)  # (a) its own rows: no tolerance
            assert np.allclose(got, want, **(TOL if host.dtype == np.float64 else TOL32)) and np.array_equal(got == 0, want == 0), (name, D, host.dtype)  # (c) the oracle
            if mask is not None:
                assert np.allclose(mask, r["mask"], **TOL)
                assert np.all(got[:, np.diff(rp) == 0] == 0)  # excluded centres: exactly 0
    # (b) the library's own smooth_data, bit for bit
    D = max(Ds)
    if r["excl"] is None:
        assert np.array_equal(plan.apply(r["data"][:D]), M.smooth_data(orig, r["data"][:D], low, r["sigma"]))
    else:
        got, mask = plan.apply(r["data"][:D])
        want, wmask = M.smooth_data(orig, r["data"][:D], low, r["sigma"], r["excl"])
        assert np.array_equal(got, want) and np.array_equal(mask, wmask)


@pytest.mark.parametrize("name", ["P", "R", "PE", "RE"])
def test_apply_every_tile_width(ctx, name):
    check_apply(ctx, name, (1, T - 1, T, T + 1, DMAX))


@pytest.mark.parametrize("name", ["Q", "S", "T", "TE"])
def test_apply_three_maps(ctx, name):
    check_apply(ctx, name, (3,))


def test_nan_meets_zero_weight(ctx):
    """a NaN under a stored weight of 0 (a masked neighbour of a centre that is kept) makes the row NaN, as in smooth_data: nothing is skipped"""
    r = reference("PE")
    rp, col, val, div, _ = r["rows"]
    zero = col[val == 0.0]
    assert len(zero)
    data = np.array(r["data"][:2])
    data[1, zero[0]] = np.nan
    orig, low = meshes(ctx, r)
    got, _ = M.ResamplePlan.smoothing(orig, low, r["sigma"], r["excl"]).apply(data)
    want, _ = M.smooth_data(orig, data, low, r["sigma"], r["excl"])
    assert np.isnan(got[1]).any() and not np.isnan(got[0]).any()
    assert np.array_equal(got, want, equal_nan=True)


def dev_child():
    """run by test_apply_dev in a process of its own that imported torch FIRST: case P at D = 70 in both dtypes"""
    import torch

    r = reference("P")
    ctx = M.Context(0)
    plan = make_plan(ctx, r)
    for host in (r["data"], r["d32"]):
        t = torch.from_numpy(np.array(host)).to("cuda", non_blocking=True)
        out = torch.full((DMAX, len(r["xlow"])), float("nan"), dtype=t.dtype, device="cuda")
        ctx.wait_stream(torch.cuda.current_stream().cuda_stream)
        assert plan.apply_dev(t, out) is out
        got = out.cpu().numpy()
        assert got.dtype == host.dtype and np.array_equal(got, plan.apply(host))
    plan.close()
    ctx.close()


def test_apply_dev():
    run = subprocess.run([sys.executable, "-c", "import torch; import tests.test_gpu_smooth_plan as t; t.dev_child()"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout


CHUNK_KB = 100


def child(path):
    """run by test_slabs in a process of its own, with MSMHIP_PLAN_CHUNK_KB set: case R at D = 70 in both dtypes"""
    r = reference("R")
    ctx = M.Context(0)
    plan = make_plan(ctx, r)
    np.savez(path, out64=plan.apply(r["data"]), out32=plan.apply(r["d32"]))
    plan.close()
    ctx.close()


def test_slabs(ctx, tmp_path):
    """100 KiB of maps hold 102400 // (2 x 2562 x 8) = 2 float64 maps or 4 float32 maps of case R: D = 70 goes in 35 slabs and in 18 (the last of 2).
    The bits do not depend on the slabs."""
    r = reference("R")
    V = len(r["xlow"])
    assert CHUNK_KB * 1024 // (2 * V * 8) == 2 and CHUNK_KB * 1024 // (2 * V * 4) == 4
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, MSMHIP_PLAN_CHUNK_KB=str(CHUNK_KB))
    run = subprocess.run([sys.executable, "-c", "import tests.test_gpu_smooth_plan as t; t.child(%r)" % path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr + run.stdout
    got = np.load(path)
    plan = make_plan(ctx, r)  # this process: the default budget, one slab
    assert np.array_equal(got["out64"], plan.apply(r["data"])) and np.array_equal(got["out32"], plan.apply(r["d32"]))


def test_snapshot(ctx):
    """a plan owns its rows: new coordinates of its meshes and their end change nothing"""
    r = reference("T")
    orig, low = meshes(ctx, r)
    plan = M.ResamplePlan.smoothing(orig, low, r["sigma"])
    before, rows, div = plan.apply(r["data"]), plan.weights(), plan.divisors()
    low.set_coords(synthetic.known_warp(r["xlow"], seed=3, rot_deg=20.0))
    orig.set_coords(synthetic.known_warp(r["xorig"], seed=4, rot_deg=30.0))
    assert np.array_equal(plan.apply(r["data"]), before) and np.array_equal(plan.apply(r["d32"]), SL.apply(*rows, div, r["d32"]))
    low.close()
    orig.close()
    assert np.array_equal(plan.apply(r["data"]), before)
    assert all(np.array_equal(a, b) for a, b in zip(plan.weights(), rows)) and np.array_equal(plan.divisors(), div)


def test_refusals(ctx):
    r, rbig = reference("P"), reference("R")
    orig, low = meshes(ctx, r)
    L = M.lib()

    def message():
        return L.msm_last_error().decode()

    for sigma in (0.0, -1.0, float("nan")):
        assert not L.msm_resample_plan_create_smooth(orig.h, low.h, sigma, None) and "sigma" in message()
    with pytest.raises(M.MsmError):
        M.ResamplePlan.smoothing(orig, low, 0.0)
    other = M.Context(0)
    foreign = M.Mesh(other, r["xlow"], r["tri"])
    assert not L.msm_resample_plan_create_smooth(orig.h, foreign.h, 2.0, None) and "context" in message()
    foreign.close()
    other.close()
    big = M.Mesh(ctx, rbig["xlow"], rbig["tri"])
    assert not L.msm_resample_plan_create_smooth(orig.h, big.h, 2.0, None) and "vertices" in message()  # V(orig) < V(sphlow)
    assert not L.msm_resample_plan_create_smooth(None, low.h, 2.0, None) and "null" in message()
    assert not L.msm_resample_plan_create(orig.h, low.h, 3, None) and "method" in message()  # MSM_RESAMPLE_SMOOTH has no sigma there
    with pytest.raises(ValueError):
        M.ResamplePlan.smoothing(orig, low, 2.0, excl=np.zeros(5))
    plan = M.ResamplePlan.smoothing(orig, low, r["sigma"])
    keys, out = np.zeros((1, plan.V_in), dtype=np.int32), np.zeros((1, plan.V_out), dtype=np.int32)
    assert L.msm_resample_plan_apply_labels(plan.h, keys.ctypes.data_as(_lib.c_ip), 1, 0, out.ctypes.data_as(_lib.c_ip)) == -1 and "smoothing" in message()
    with pytest.raises(ValueError):
        plan.apply_labels(keys)
    assert L.msm_resample_plan_divisors(plan.h, None) == -1 and L.msm_resample_plan_divisors(None, None) == -1
    assert np.array_equal(plan.apply(r["data"][:2]), M.smooth_data(orig, r["data"][:2], low, r["sigma"]))  # the context stays usable


def test_other_methods_are_not_divided(ctx):
    xin, tin, xnew, tnew, _ = case("A")
    min_, mnew = M.Mesh(ctx, xin, tin), M.Mesh(ctx, xnew, tnew)
    plan = M.ResamplePlan(min_, mnew)
    div = plan.divisors()
    assert div.shape == (len(xnew),) and np.all(div == 0.0)
    data = synthetic.features(xin, 5, seed=5)
    assert np.array_equal(plan.apply(data), M.metric_resample(min_, data, mnew))
    assert np.all(M.ResamplePlan(min_, mnew, method="nearest").divisors() == 0.0)


def test_file_tool(ctx, tmp_path):
    from tests.test_gpu_resample_plan import f32, rescaled, tool_inputs

    tool = load_tool()
    p, tin = tool_inputs(tmp_path)
    xs, _ = rescaled(p["sphere"])
    sphere = M.Mesh(ctx, xs, tin)
    both, one = str(tmp_path / "both"), str(tmp_path / "one")
    common = ["--current_sphere=" + p["sphere"], "--sigma=10"]
    plan = M.ResamplePlan.smoothing(sphere, sphere, 10.0)
    assert tool.main(["smoothing", "--metric_in=" + p["myelin"], "--metric_in=" + p["rest"], "--output=" + both] + common) == 0
    for k, D in (("myelin", 2), ("rest", 5)):
        got = meshio.load_metric(both + "-%s-smoothed_data.func.gii" % k, dtype=np.float32)
        assert got.shape == (D, len(xs)) and np.array_equal(got, plan.apply(meshio.load_metric(p[k], dtype=np.float32)))
    # one input, no mask: the bytes the tool wrote when it called smooth_data on the widened values
    assert tool.main(["smoothing", "--metric_in=" + p["myelin"], "--output=" + one] + common) == 0
    meshio.save_metric(str(tmp_path / "before.func.gii"), f32(M.smooth_data(sphere, meshio.load_metric(p["myelin"]), sphere, 10.0)))
    assert open(one + "-smoothed_data.func.gii", "rb").read() == open(str(tmp_path / "before.func.gii"), "rb").read()
    assert open(one + "-smoothed_data.func.gii", "rb").read() == open(both + "-myelin-smoothed_data.func.gii", "rb").read()
    # masked by the first input
    first = meshio.load_metric(p["myelin"])
    lo, hi = np.quantile(first, 0.2), np.quantile(first, 0.9)
    excl = M.create_exclusion(first, lo, hi)
    assert 0 < excl.sum() < len(excl)
    masked = str(tmp_path / "masked")
    assert tool.main(["smoothing", "--metric_in=" + p["myelin"], "--metric_in=" + p["rest"], "--output=" + masked, "--excl_thr=%r,%r" % (float(lo), float(hi))] + common) == 0
    want, _ = M.ResamplePlan.smoothing(sphere, sphere, 10.0, excl).apply(meshio.load_metric(p["rest"], dtype=np.float32))
    got = meshio.load_metric(masked + "-rest-smoothed_data.func.gii", dtype=np.float32)
    assert np.array_equal(got, want) and not np.array_equal(got, meshio.load_metric(both + "-rest-smoothed_data.func.gii", dtype=np.float32))
