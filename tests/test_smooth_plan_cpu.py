"""What the smoothing plan's GPU tests (tests/test_gpu_smooth_plan.py) rely on, checked without a GPU: the plain definition of the rows
(tests/smooth_plan_literal.py) gives the oracle's smooth_data bit for bit, the cases have the row lengths they were chosen for, the file tool's parser
takes what `smoothing` has learnt, and the two new entry points are bound."""
import functools

import numpy as np
import pytest

from newmsm_amd import _lib, synthetic
from oracle import oracle as O
from tests import smooth_plan_literal as SL
from tests.test_resample_plan_cpu import load_tool, refused

DMAX = 70
# name: (order of the meshes, sigma, masked, sphLow regular while orig is warped)
CASES = dict(P=(3, 10.0, False, False), Q=(3, 2.0, False, False), R=(4, 30.0, False, False), S=(5, 4.0, False, False), PE=(3, 10.0, True, False),
             RE=(4, 30.0, True, False), T=(3, 10.0, False, True), TE=(3, 10.0, True, True))
# rows: (shortest, longest, nnz, empty rows); the masked cases keep their unmasked rows or none
SHAPES = dict(P=(6, 7, 4482, 0), Q=(1, 1, 642, 0), R=(218, 233, 578412, 0), S=(13, 19, 179916, 0), PE=(6, 7, 3072, 202), RE=(218, 233, 398889, 796))
MAPS = dict(P=DMAX, R=DMAX, PE=DMAX, RE=DMAX)  # the others: 3


def mask_of(xyz):
    """deliberately not binary"""
    excl = (xyz[:, 2] > -20).astype(np.float64)
    excl[xyz[:, 0] > 50] = 0.5
    return excl


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case's inputs, the literal's rows and the oracle's results, computed once; the arrays are read-only"""
    order, sigma, masked, split = CASES[name]
    xlow, tri = O.icosphere(order)
    xorig = synthetic.known_warp(xlow, seed=21, rot_deg=5.0, amp=1.0)
    if not split:
        xlow = xorig
    excl = mask_of(xorig) if masked else None
    oorig, olow = O.Mesh(xorig, tri), O.Mesh(xlow, tri)
    cv = O.Octree(oorig).closest_vertex(xlow) if split else np.arange(len(xlow), dtype=np.int32)
    D = MAPS.get(name, 3)
    data = synthetic.features(xorig, D, seed=5)
    d32 = data.astype(np.float32)
    r = dict(xorig=xorig, xlow=xlow, tri=tri, sigma=sigma, excl=excl, cv=cv, data=data, d32=d32, rows=SL.rows(xlow, sigma, cv, excl))
    if masked:
        r["want"], r["mask"] = O.smooth_data(oorig, data, olow, sigma, excl)
        r["want32"] = O.smooth_data(oorig, d32.astype(np.float64), olow, sigma, excl)[0].astype(np.float32)
    else:
        r["want"], r["mask"] = O.smooth_data(oorig, data, olow, sigma), None
        r["want32"] = O.smooth_data(oorig, d32.astype(np.float64), olow, sigma).astype(np.float32)
    for v in list(r.values()) + list(r["rows"]):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@pytest.mark.parametrize("name", sorted(CASES))
def test_literal_is_the_oracle_s(built, name):
    r = reference(name)
    rp, col, val, div, eo = r["rows"]
    got = SL.apply(rp, col, val, div, r["data"])
    assert got.dtype == np.float64 and np.array_equal(got, r["want"])
    got32 = SL.apply(rp, col, val, div, r["d32"])
    assert got32.dtype == np.float32 and np.array_equal(got32, r["want32"])
    if r["excl"] is None:
        assert eo is None
    else:
        assert np.array_equal(eo, r["mask"])
        assert np.all(r["want"][:, np.diff(rp) == 0] == 0)
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    assert np.all(np.diff(col)[row[1:] == row[:-1]] > 0)  # ascending within a row


def test_case_shapes(built):
    for name, (lo, hi, nnz, empty) in SHAPES.items():
        n = np.diff(reference(name)["rows"][0])
        kept = n[n > 0]
        assert lo <= kept.min() and kept.max() <= hi and (n.sum(), (n == 0).sum()) == (nnz, empty), (name, kept.min(), kept.max(), n.sum(), (n == 0).sum())
        if empty == 0:
            assert (n.min(), n.max()) == (lo, hi), (name, n.min(), n.max())
    assert (len(reference("P")["xlow"]), len(reference("S")["xlow"])) == (642, 10242)  # 10 x 64 + 2: a ragged last chunk; 161 chunks
    t, te = reference("T"), reference("TE")
    n = np.diff(t["rows"][0])
    assert (n.min(), n.max()) == (6, 7) and np.sum(t["cv"] != np.arange(len(t["cv"]))) == 239
    assert np.sum(np.diff(te["rows"][0]) == 0) == 203
    # rows of one entry compute (x * g) / g, which is not always x: a plan that skipped the division would not pass
    q = reference("Q")
    assert q["data"].shape == (3, 642) and np.sum(q["want"] != q["data"]) == 250
    assert np.array_equal(q["rows"][3], q["rows"][2])  # one entry: the divisor is the weight
    # the mask takes the three kinds of value, and a fractional one reaches stored weights
    pe = reference("PE")
    assert sorted(set(pe["excl"])) == [0.0, 0.5, 1.0] and np.any(pe["excl"][pe["rows"][1]] == 0.5)


def test_tool_parser():
    tool = load_tool()
    prog, opt = tool.parse(["smoothing", "--metric_in=a.func.gii", "--metric_in", "b.func.gii", "--current_sphere=s", "--sigma=2.5", "--output=o",
                            "--excl_thr=-1,2.5"])
    assert prog == "smoothing" and opt.metric_in == ["a.func.gii", "b.func.gii"] and opt.sigma == 2.5 and opt.excl_thr == (-1.0, 2.5)
    assert tool.parse(["smoothing", "--metric_in=a.func.gii", "--current_sphere=s", "--sigma=1", "--output=o"])[1].excl_thr is None
    assert refused(tool, ["smoothing", "--metric_in=a.func.gii", "--metric_in=b.func.gii", "--current_sphere=s", "--excl_thr=0,1"]) == "sigma was not set, but required."
    assert refused(tool, ["smoothing", "--metric_in=a", "--current_sphere=s", "--sigma=1", "--output=o", "--excl_thr=3"]) == "excl_thr takes two numbers: lo,hi"
    assert "unrecognized" in refused(tool, ["smoothing", "--metric_in=a", "--current_sphere=s", "--sigma=1", "--output=o", "--method=nearest"])


def test_bindings():
    for name in ("msm_resample_plan_create_smooth", "msm_resample_plan_divisors"):
        assert name in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["msm_resample_plan_create_smooth"]
    assert len(argtypes) == 4 and argtypes[2] is _lib.C.c_double
