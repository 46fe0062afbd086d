"""What the resampling plan's GPU tests rely on, checked without a GPU: the inputs of the label vote's tie case, the label and float32 file routines,
and the file tool's parser (which refuses before it touches a file or a device)."""
import importlib.util
import os

import numpy as np
import pytest

from newmsm_amd import meshio, synthetic
from oracle import oracle as O
from tests import resample_literal as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("resample_files", os.path.join(ROOT, "tools", "resample_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case(name):
    """(source xyz, source tri, target xyz, target tri, excl or None) of the cases of tests/test_gpu_resample_plan.py:
    A warped ico3 -> ico2 (rows of 9-14 entries), B warped ico2 -> ico3 (rows of 3), C warped ico4 -> ico1 (rows of 151-200), D regular ico2 -> ico3
    (labels: exact vote ties), E = A with the mask z > -20 (65 of 162 rows empty), M warped ico5 -> ico4 (more than one workgroup per XCD)"""
    oin, onew = dict(A=(3, 2), B=(2, 3), C=(4, 1), D=(2, 3), E=(3, 2), M=(5, 4))[name]
    xin, tin = O.icosphere(oin)
    xnew, tnew = O.icosphere(onew)
    if name != "D":
        xin = synthetic.known_warp(xin, seed=21, rot_deg=5.0, amp=1.0)
    excl = (xin[:, 2] > -20).astype(np.float64) if name == "E" else None
    return xin, tin, xnew, tnew, excl


def tie_keys(xyz):
    """case D's keys: bands of z crossed with the sign of x, so that neighbouring vertices of a regular sphere hold different keys with equal weights"""
    return (3 * np.floor((xyz[:, 2] + 100) / 25) + (xyz[:, 0] > 0)).astype(np.int32)


def test_case_d_meets_exact_ties(built):
    xin, tin, xnew, tnew, _ = case("D")
    rp, col, val = O.adaptive_barycentric_weights(O.Mesh(xin, tin), O.Mesh(xnew, tnew))
    assert np.all(np.diff(rp) == 3)
    out, tied = RL.label_vote(rp, col, val, tie_keys(xin))
    assert tied == 8
    assert out.shape == (1, len(xnew)) and out.dtype == np.int32


def test_case_shapes(built):
    for name, lo, hi in (("A", 9, 14), ("B", 3, 3), ("C", 151, 200)):
        xin, tin, xnew, tnew, _ = case(name)
        n = np.diff(O.adaptive_barycentric_weights(O.Mesh(xin, tin), O.Mesh(xnew, tnew))[0])
        assert n.min() == lo and n.max() == hi, (name, n.min(), n.max())
    xin, tin, xnew, tnew, excl = case("E")
    rp, col, val = O.adaptive_barycentric_weights(O.Mesh(xin, tin), O.Mesh(xnew, tnew), excl)
    assert np.sum(np.diff(rp) == 0) == 65 and np.all(np.isfinite(val))


def test_literal_apply_is_the_oracle_s(built):
    xin, tin, xnew, tnew, _ = case("A")
    oi, on = O.Mesh(xin, tin), O.Mesh(xnew, tnew)
    rp, col, val = O.adaptive_barycentric_weights(oi, on)
    data = synthetic.features(xin, 2, seed=5)
    assert np.array_equal(RL.apply_rows(rp, col, val, data), O.metric_resample(oi, data, on))
    d32 = data.astype(np.float32)
    got = RL.apply_rows(rp, col, val, d32)
    assert got.dtype == np.float32 and np.array_equal(got, O.metric_resample(oi, d32.astype(np.float64), on).astype(np.float32))


TABLE = """<LabelTable>
      <Label Key="0" Red="1" Green="1" Blue="1" Alpha="0"><![CDATA[???]]></Label>
      <Label Key="7" Red="0.5" Green="0.25" Blue="0" Alpha="1"><![CDATA[L_V1 & "more"]]></Label>
   </LabelTable>"""


def test_label_file_round_trip(tmp_path):
    keys = np.array([[0, 7, 7, 0, 7], [7, 7, 0, 0, 0]], dtype=np.int32)
    p = str(tmp_path / "parc.label.gii")
    meshio.save_label(p, keys, TABLE)
    got, table = meshio.load_label(p)
    assert got.dtype == np.int32 and np.array_equal(got, keys) and table == TABLE
    assert [i for i, _ in meshio.read_gifti(p)] == ["NIFTI_INTENT_LABEL"] * 2
    assert all(a.dtype == np.int32 for _, a in meshio.read_gifti(p))
    q = str(tmp_path / "again.label.gii")
    meshio.save_label(q, got, table)
    assert open(p).read() == open(q).read()
    meshio.save_label(q, keys[0])  # no table: the empty element
    assert meshio.load_label(q)[1] == "<LabelTable/>" and np.array_equal(meshio.load_label(q)[0], keys[:1])
    with pytest.raises(meshio.MeshIOError):
        meshio.save_label(q, keys, "<MetaData/>")


def test_load_metric_dtype(tmp_path):
    data = np.random.default_rng(3).normal(size=(3, 40)).astype(np.float32)
    p = str(tmp_path / "m.func.gii")
    meshio.save_metric(p, data)
    got = meshio.load_metric(p, dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), data.view(np.uint32))
    default = meshio.load_metric(p)
    assert default.dtype == np.float64 and np.array_equal(default, data.astype(np.float64))
    assert np.array_equal(meshio.load_metric(p, 40), default)


def refused(tool, argv):
    with pytest.raises(tool.Refused) as e:
        tool.parse(argv)
    return str(e.value)


def test_tool_parser():
    tool = load_tool()
    assert sorted(tool.PROGRAMS) == sorted(["metric-resample", "NN-resample", "surface-resample", "smoothing", "applywarp"])
    full = ["--metric_in=a.func.gii", "--current_sphere=nowhere.surf.gii", "--ico=4", "--output=/nonexistent/o"]
    prog, opt = tool.parse(["metric-resample"] + full)
    assert prog == "metric-resample" and opt.metric_in == ["a.func.gii"] and opt.ico == 4 and opt.method == "adap_bary" and opt.new_sphere is None
    assert tool.parse(["NN-resample"] + full)[1].method == "nearest"
    # the programs' sentences, in their order of complaint
    for prog, names in (("metric-resample", ("metric_in", "current_sphere", "ico", "output")), ("NN-resample", ("metric_in", "current_sphere", "ico", "output")),
                        ("surface-resample", ("surface_in", "current_sphere", "ico", "output")), ("smoothing", ("metric_in", "current_sphere", "sigma", "output")),
                        ("applywarp", ("to_be_deformed", "warp", "output"))):
        value = dict(ico="4", sigma="0.5")
        given = []
        for n in names:
            assert refused(tool, [prog] + given) == "%s was not set, but required." % n
            given.append("--%s=%s" % (n, value.get(n, "x")))
        tool.parse([prog] + given)
    # --ico ranges: metric-resample 2..6, NN-resample 3..6
    for prog, bad, good in (("metric-resample", (1, 7), (2, 6)), ("NN-resample", (2, 7), (3, 6))):
        for n in bad:
            assert refused(tool, [prog] + full[:2] + ["--ico=%d" % n, full[3]]) == "Invalid ico dimension"
        for n in good:
            tool.parse([prog] + full[:2] + ["--ico=%d" % n, full[3]])
    # additions
    prog, opt = tool.parse(["metric-resample", "--metric_in=a.func.gii", "--metric_in", "b.func.gii", "--label_in=p.label.gii", "--current_sphere=s",
                            "--new_sphere=t.surf.gii", "--output=o", "--method=barycentric", "--excl_thr=-1,2.5"])
    assert opt.metric_in == ["a.func.gii", "b.func.gii"] and opt.label_in == "p.label.gii" and opt.new_sphere == "t.surf.gii" and opt.ico is None
    assert opt.method == "barycentric" and opt.excl_thr == (-1.0, 2.5)
    assert "both set" in refused(tool, ["metric-resample"] + full + ["--new_sphere=t.surf.gii"])
    tool.parse(["metric-resample", "--label_in=p.label.gii", "--current_sphere=s", "--ico=3", "--output=o"])  # labels alone
    assert "invalid choice" in refused(tool, ["metric-resample"] + full + ["--method=linear"])
    assert "unknown program" in refused(tool, ["label-resample"])
    assert tool.main(["metric-resample", "--current_sphere=s"]) == 1
    assert tool.gifti_name("o-resampled_data.func") == "o-resampled_data.func.gii" and tool.gifti_name("o-sphere.surf.gii") == "o-sphere.surf.gii"
    assert tool.stem("/x/rest.func.gii") == "rest" and tool.stem("thick.shape.gii") == "thick"


def test_tool_true_rescale_is_the_oracle_s(built):
    tool = load_tool()
    xyz = synthetic.random_sphere_points(500, seed=4) * np.random.default_rng(1).uniform(0.3, 2.0, size=(500, 1))
    xyz = xyz.astype(np.float32).astype(np.float64)
    want = xyz.copy()
    O.lib().orc_true_rescale(want.ctypes.data_as(O.c_dp), len(want), O.C.c_double(100.0))
    assert np.array_equal(tool.true_rescale(xyz), want)


def test_tile_width_is_the_kernels():
    import re

    import newmsm_amd as M

    text = open(os.path.join(ROOT, "newmsm_amd", "csrc", "resample_plan.hpp")).read()
    assert int(re.search(r"constexpr int kPlanTile = (\d+);", text).group(1)) == M.PLAN_TILE == 64
