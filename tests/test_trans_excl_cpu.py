"""--trans (a transformed input sphere as the starting point) and --excl (exclusion masks from the cut thresholds) without a GPU: the two
configuration front ends, and the level loops of newmsm_amd/registration.py / group_registration.py driven by the oracle alone
(tests/trans_excl_cases.py).  tests/test_gpu_trans_excl.py runs the same shapes over the MI355X path."""
import json
import os
import subprocess

import numpy as np
import pytest

import trans_excl_cases as C
from helpers import ulp_close
from newmsm_amd import config, group_registration, registration
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "excl_config.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "excl_config")
LIBDIR = os.path.join(ROOT, "newmsm_amd")
BASE = "--opt=DISCRETE,DISCRETE\n--lambda=0.1,0.2\n--regoption=3\n--sigma_in=3,1\n--dopt=HOCR\n"


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as g

    g.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE, "-L", LIBDIR, "-lmsmhip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def cpp(exe, tmp_path, text, groupwise=False):
    path = tmp_path / "conf"
    path.write_text(text)
    out = subprocess.run([exe, str(path), "2"] + (["groupwise"] if groupwise else []), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("groupwise", [False, True])
@pytest.mark.parametrize("extra,want", [("--excl\n--cutthr=0,0.0001\n", (True, 0.0, float(np.float32(0.0001)))), ("--excl\n", (True, 0.0, float(np.float32(0.0001)))),
                                        ("--excl\n--cutthr=-0.5,0.25\n", (True, -0.5, 0.25)), ("", (False, 0.0, float(np.float32(0.0001))))])
def test_excl_parses_the_same_in_python_and_cpp(exe, tmp_path, extra, want, groupwise):
    """--excl / --cutthr reach the level loops from both front ends with the same values (--cutthr through a float, as the reference's option holds it)"""
    cfg = config.parse_config(BASE + extra)
    levels, run_kw, _ = config.levels_from_config(cfg, 2, groupwise=groupwise)  # raised on --excl before the option was wired in
    opts = config.run_options(cfg)
    assert (opts["excl"], opts["cutthr"][0], opts["cutthr"][1]) == want and run_kw == dict(varnorm=False)
    got = cpp(exe, tmp_path, BASE + extra, groupwise)
    assert (got["excl"], got["cutthr"][0], got["cutthr"][1]) == want and got["levels"] == len(levels) == 2
    assert got["message"] == registration.EXCL_WITH_WEIGHTINGS


@pytest.mark.parametrize("flag", ["--IN\n", "--INc\n", "--excl\n--IN\n"])
def test_histogram_matching_is_still_refused(exe, tmp_path, flag):
    for groupwise in (False, True):
        with pytest.raises(config.ConfigError, match="--IN / --INc"):
            config.levels_from_config(config.parse_config(BASE + flag), 2, groupwise=groupwise)
        assert "--IN / --INc" in cpp(exe, tmp_path, BASE + flag, groupwise)["error"]


def test_cut_thresholds_need_two_values():
    with pytest.raises(config.ConfigError, match="cut threshold"):
        config.parse_config(BASE + "--excl\n--cutthr=0\n")


def test_excl_with_both_weightings_is_refused():
    """downsample_cfweighting would read the level grid's mask at vertex numbers of the weightings' meshes: an error that says so, before anything runs;
    one weighting alone is ignored by the reference (combine_weighting returns ones) and stays allowed"""
    case = C.pairwise_case(order=3, D=1)
    w = np.ones((1, len(case[0])))
    with pytest.raises(ValueError, match="downsample_cfweighting") as e:
        C.run(None, case, C.DISCRETE_PAIR[:1], excl=True, in_cfweight=w, ref_cfweight=w)  # no ops object is touched
    assert str(e.value) == registration.EXCL_WITH_WEIGHTINGS


# ---------------------------------------------------------------- --trans over the oracle
@pytest.mark.parametrize("levels", [C.DISCRETE_PAIR, C.RIGID_THEN_DISCRETE], ids=["discrete_discrete", "rigid_discrete"])
def test_trans_continues_a_run_exactly(levels):
    """check 1: [L2] started from the sphere.reg of [L1] is [L1, L2], bit for bit"""
    case = C.pairwise_case(order=4, D=2)
    a, lab_a2, reg1, b2, lab_b = C.composition(C.oracle_ops(), case, levels)
    C.assert_composition(a, lab_a2, b2, lab_b)
    assert not np.array_equal(reg1, case[0]) and not np.array_equal(b2[0], reg1)  # both stages moved the sphere


def test_trans_equal_to_the_input_sphere_warns_and_is_ignored(capfd):
    """check 2: operator== of the reference (every coordinate within 1e-8): its warning, then the run without the option"""
    case = C.pairwise_case(order=4, D=1)
    plain = C.run(C.oracle_ops(), case, C.DISCRETE_PAIR[:1])
    capfd.readouterr()
    same = C.run(C.oracle_ops(), case, C.DISCRETE_PAIR[:1], trans_xyz=case[0] + 5e-9)
    assert "WARNING: transformed mesh has the same coordinates as the input mesh" in capfd.readouterr().err
    assert np.array_equal(same[0], plain[0]) and np.array_equal(same[1][0], plain[1][0]) and same[2] == plain[2]


def test_trans_with_another_vertex_count_is_an_error():
    case = C.pairwise_case(order=4, D=1)
    with pytest.raises(ValueError, match="642 vertices, the input mesh has 2562"):
        C.run(C.oracle_ops(), case, C.DISCRETE_PAIR[:1], trans_xyz=O.icosphere(3)[0])


def test_trans_is_not_a_no_op():
    """an input mesh that is not the level's grid (ico4 input, ico3 data grid) started from a known smooth warp"""
    from newmsm_amd import synthetic

    case = C.pairwise_case(order=4, D=1)
    lab_t, lab_p = [], []
    moved = C.run(C.oracle_ops(), case, C.DISCRETE_PAIR[:1], lab_t, trans_xyz=synthetic.known_warp(case[0], seed=77, rot_deg=3.0, amp=2.0))
    plain = C.run(C.oracle_ops(), case, C.DISCRETE_PAIR[:1], lab_p)
    assert np.abs(moved[0] - plain[0]).max() > 1e-2 and np.allclose(np.linalg.norm(moved[0], axis=1), 100.0)


# ---------------------------------------------------------------- --excl over the oracle
def test_excl_prepares_the_features_in_the_reference_order():
    """check 4 without a GPU: per level and data set create_exclusion on the native data, the masked metric_resample whose mask replaces it, the masked
    smooth_data (sigma > 0) whose mask replaces it again, the masked variance_normalise -- restated here call by call; and the mask matters"""
    case = C.pairwise_case(order=4, D=2, cap=True)
    xyz, tri, src, ref, inside = case
    assert 0.05 * len(xyz) <= inside.sum() <= 0.15 * len(xyz) and inside.sum() == 256  # 9.99 % of the ico4 vertices
    with_mask = C.level_features(C.oracle_ops(), case, C.DISCRETE_PAIR, True)
    without = C.level_features(C.oracle_ops(), case, C.DISCRETE_PAIR, False)
    native = O.Mesh(xyz, tri)
    k = 0
    for lv in C.DISCRETE_PAIR:
        ico = O.Mesh(*O.icosphere(lv["data_order"]))
        for data, sigma in ((src, lv["sigma_in"]), (ref, lv["sigma_ref"])):
            mask = O.create_exclusion(data, *C.CUTTHR)
            assert np.array_equal(mask, 1.0 - inside)
            f, mask = O.metric_resample_excl(native, data, ico, mask)
            if sigma > 0.0:
                f, mask = O.smooth_data(ico, f, ico, sigma, excl=mask)
            f = O.variance_normalise(f, excl=mask)
            assert np.array_equal(with_mask[k][0], f) and np.array_equal(with_mask[k][1], mask)
            assert 0 < (mask > 0).sum() < len(mask)                              # the cap reaches the level's grid
            assert np.all(f[:, mask <= 0] == 0.0)                                # and holds nothing there
            kept = f[:, mask > 0]
            assert ulp_close(kept.mean(axis=1), 0.0, atol=1e-9)                  # the statistics ran over the kept vertices alone
            assert without[k][1] is None and not np.allclose(without[k][0], f, atol=1e-3)
            k += 1


def test_excl_changes_a_pairwise_run_and_leaves_the_default_alone():
    case = C.pairwise_case(order=4, D=2, cap=True)
    lab_e, lab_p, lab_d = [], [], []
    masked = C.run(C.oracle_ops(), case, C.DISCRETE_PAIR, lab_e, excl=True, cutthr=C.CUTTHR)
    plain = C.run(C.oracle_ops(), case, C.DISCRETE_PAIR, lab_p, excl=False)
    default = C.run(C.oracle_ops(), case, C.DISCRETE_PAIR, lab_d)
    assert not np.allclose(np.concatenate(masked[2]), np.concatenate(plain[2]), rtol=1e-6)
    assert np.array_equal(default[0], plain[0]) and all(np.array_equal(a, b) for a, b in zip(lab_p, lab_d))


def test_excl_in_a_groupwise_run():
    """the group loop prepares every subject's features with its own mask; without the option it calls ops that know nothing of masks (helpers.OracleOps)"""
    import newmsm_amd as M
    from helpers import OracleOps

    meshes, datas, txyz, tri, levels, mask, caps = C.group_case()
    levels = levels[:1]
    kw = dict(varnorm=True, fixnan=True)
    masked = group_registration.run_group_multiresolution(C.oracle_ops(), meshes, datas, txyz, tri, levels, excl=True, cutthr=C.CUTTHR, **kw)
    plain = group_registration.run_group_multiresolution(OracleOps(M.mcmc_optimise), meshes, datas, txyz, tri, levels, **kw)
    assert not np.allclose(masked[2][0], plain[2][0], rtol=1e-6)
