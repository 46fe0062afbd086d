"""The rigid level's host side without a GPU: the schedules that start with a RIGID / AFFINE level (config.py and msmhip_config.hpp with
rigid=True), and the literal restatement of Rigid_cost_function (tests/rigid_literal.py) -- its fast mode against its literal mode, and a
recovery of a known rotation."""
import json
import os
import subprocess

import numpy as np
import pytest

import rigid_literal as RL
from newmsm_amd import config
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rigid_levels.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "rigid_levels")
LIBDIR = os.path.join(ROOT, "newmsm_amd")
F32_001 = float(np.float32(0.01))
MSMSULC = os.path.join(ROOT, "tests", "golden", "MSMSulcStrainFinalconf")  # config/HCP_multimodal_alignment/MSMSulcStrainFinalconf


def msmsulc_text():
    with open(MSMSULC) as f:
        return f.read()


def test_default_schedule_rigid_level():
    """no --conf: the 2014 sulc schedule's first level (M/mesh_registration.cpp:629-642) as a rigid level"""
    levels, _, skipped = config.levels_from_config(config.parse_config(None), 1, rigid=True)
    assert skipped == [] and len(levels) == 4
    assert levels[0] == dict(method="RIGID", data_order=4, sigma_in=2.0, sigma_ref=2.0, iters=50, simmeasure=1, stepsize=F32_001, gradsampling=0.5)
    assert [lv.get("method", "DISCRETE") for lv in levels[1:]] == ["DISCRETE"] * 3
    # without rigid=True nothing changes
    levels, _, skipped = config.levels_from_config(config.parse_config(None), 1)
    assert skipped == [(0, "RIGID")] and len(levels) == 3


def test_msmsulc_preset_rigid_level():
    """HCP MSMSulc: --opt=AFFINE,... --simval=3,... --it=50,...; NMI (3) becomes correlation (2)"""
    levels, _, skipped = config.levels_from_config(config.parse_config(msmsulc_text()), 1, rigid=True)
    assert skipped == []
    assert levels[0] == dict(method="RIGID", data_order=6, sigma_in=0.0, sigma_ref=0.0, iters=50, simmeasure=2, stepsize=F32_001, gradsampling=0.5)
    _, _, skipped = config.levels_from_config(config.parse_config(msmsulc_text()), 1)
    assert skipped == [(0, "AFFINE")]
    cfg = config.parse_config("--opt=AFFINE,DISCRETE\n--lambda=0,0.1\n--stepsize=0.02\n--gradsampling=0.3\n--dopt=HOCR\n--regoption=3\n")
    lv = config.levels_from_config(cfg, 1, rigid=True)[0][0]
    assert lv["stepsize"] == float(np.float32(0.02)) and lv["gradsampling"] == float(np.float32(0.3))


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as g

    g.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE, "-L", LIBDIR, "-lmsmhip",
                           "-Wl,-rpath," + LIBDIR])
    return EXE


@pytest.mark.parametrize("name", [None, "HCP_MSMSulc", "standard_MSM_strain", "standard_MSMpair", "HCP_MSMAll"])
def test_cpp_rigid_levels_match_python(exe, tmp_path, name):
    if name is None:
        arg, text = "NONE", None
    else:
        text = msmsulc_text() if name == "HCP_MSMSulc" else config.PRESETS[name]
        arg = str(tmp_path / "conf")
        (tmp_path / "conf").write_text(text)
    out = subprocess.run([exe, arg, "1"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    levels, _, skipped = config.levels_from_config(config.parse_config(text), 1, rigid=True)
    assert got["skipped"] == len(skipped) == 0
    assert len(got["levels"]) == len(levels)
    keys = ("data_order", "sigma_in", "sigma_ref", "iters", "simmeasure")
    for g, w in zip(got["levels"], levels):
        assert g["method"] == w.get("method", "DISCRETE")
        assert all(g[k] == w[k] for k in keys)
        if g["method"] == "RIGID":
            assert g["stepsize"] == w["stepsize"] and g["gradsampling"] == w["gradsampling"]


@pytest.mark.parametrize("D,sim", [(1, 1), (1, 2), (3, 1), (3, 2)])
def test_fast_mode_equals_literal_mode(D, sim):
    """the product's simplification (one query list per closest triangle, similarities computed where read) gives the reference's bits"""
    xyz, tri, A, B = RL.rigid_inputs(3, D, 5 + D)
    lit = RL.RigidLiteral(xyz, tri, A, B, sim).initialise()
    fast = RL.RigidLiteral(xyz, tri, A, B, sim, fast=True).initialise()
    src = RL.euler_rotate(xyz, 0.04, -0.03, 0.02)
    lit.update_source(src)
    fast.update_source(src)
    for e in [(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.0, 0.25, 0.0), (0.01, -0.02, 0.03)]:
        assert lit.rigid_cost_mesh(*e) == fast.rigid_cost_mesh(*e)
        assert np.array_equal(lit.current_sim, fast.current_sim)
    a = lit.run(3, F32_001, 0.5)
    b = fast.run(3, F32_001, 0.5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _axis_angle(R):
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


def test_literal_run_recovers_a_rotation():
    """simmeasure 1, D = 3, ico4: the input is the reference rotated by ~0.1 rad; the run improves the cost and shrinks the residual rotation"""
    xyz, tri, _, B = RL.rigid_inputs(4, 3, 11)
    w = (0.06, -0.05, 0.06)
    R = np.array(RL.euler_matrix(*w)).reshape(3, 3)
    # input data on the grid = reference data seen through the rotation: A(v) = B at the vertex nearest to R^T v
    rot = RL.euler_rotate(xyz, *w)
    tree = O.Octree(O.Mesh(xyz, tri))
    A = B[:, tree.closest_vertex(rot)]
    r = RL.RigidLiteral(xyz, tri, A, B, 1, fast=True).initialise()
    src, trace, summary = r.run(10, F32_001, 0.5)
    assert summary["RECfinal"] >= summary["RECinit"]
    # the rotation the run applied (src = P^T v per vertex), least squares over the vertices
    M = np.linalg.lstsq(xyz, src, rcond=None)[0]
    U, _, Vt = np.linalg.svd(M)
    P = U @ Vt
    # input vertex v carries the reference's data from R^T v: a perfect run moves v there (P^T = R^T), leaving R P^T = I
    before, after = _axis_angle(R), _axis_angle(R @ P.T)
    assert after < before - 0.005, (before, after, summary)
