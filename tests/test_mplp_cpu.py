"""The MPLP optimiser's host literal (msm_mplp_optimise; newmsm_amd/csrc/mplp_host.hpp) against the numpy restatement of its definition
in mplp_literal.py, bit for bit, and against brute force on graphs small enough for it.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, config
from newmsm_amd._lib import c_dp, c_ip, lib

import mplp_literal as ML

SWEEPS = 25


def _run(case, sweeps=SWEEPS):
    U, tc, triplets, start = case
    return api.mplp_optimise(U, tc, triplets, start, sweeps=sweeps, bounds=True, messages=True)


def _everywhere(case, got):
    """the two promises, and the bound's monotonicity"""
    U, tc, triplets, start = case
    t = ML.tol(U, tc, triplets)
    steps = np.diff(got.bounds)
    print("start %.17g energy %.17g bound %.17g tol %.3g lowest step of the bound %.3g" % (ML.energy(U, tc, triplets, start), got.energy, got.bound, t,
                                                                                          steps.min() if len(steps) else 0.0))
    assert np.all(steps >= -t)
    assert got.energy <= ML.energy(U, tc, triplets, start)
    assert got.energy == ML.energy(U, tc, triplets, got.labeling)
    assert got.bound <= got.energy + t and got.bound == got.bounds[-1]


@pytest.mark.parametrize("name,case", [("ico0", (0, 19, 11, 0.0)), ("ico2", (2, 7, 11, 0.0)), ("ico2 shuffled", (2, 7, 12, 0.0, False, True)),
                                       ("ico0 with 1e7", (0, 19, 13, 0.05)), ("ico2 with 1e7", (2, 7, 13, 0.05))])
def test_literal_agrees_with_the_restatement(name, case):
    """T = 20 / L = 19 and T = 320 / L = 7, 25 sweeps: messages, labelling, energies and bounds; with and without 5 % of the entries at 1e7"""
    case = ML.ico_case(*case)
    got = _run(case)
    ML.same(got, ML.mplp(*case, SWEEPS), name)
    _everywhere(case, got)
    assert got.sweeps_run == SWEEPS and got.labeling.any()


def test_optional_outputs_do_not_change_the_others():
    case = ML.ico_case(0, 19, 11)
    full = _run(case)
    U, tc, triplets, start = case
    bare = api.mplp_optimise(U, tc, triplets, start, sweeps=SWEEPS, bound=False)
    assert bare.bound is None and bare.bounds is None and bare.messages is None
    ML.same(bare, full)
    ML.same(api.mplp_optimise(U, tc, triplets, start, sweeps=SWEEPS, bound=True), full)  # the bound alone: one pass after the last sweep


def _small(triplets, N, L, seed):
    triplets = np.asarray(triplets, dtype=np.int32)
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (L, N)), rng.uniform(0.0, 1.0, (len(triplets), L, L, L)), triplets, rng.integers(0, L, N).astype(np.int32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_single_triangle_is_solved_exactly(seed):
    """N = 3, L = 3: a fixed point within 3 sweeps, the brute-force optimum, the bound on it"""
    case = _small([[0, 1, 2]], 3, 3, seed)
    got = _run(case, sweeps=10)
    best, t = ML.brute_force(*case[:3]), ML.tol(*case[:3])
    print("sweeps_run %d energy %.17g optimum %.17g bound %.17g tol %.3g" % (got.sweeps_run, got.energy, best, got.bound, t))
    ML.same(got, ML.mplp(*case, 10))
    assert got.sweeps_run <= 3
    assert got.energy == best and abs(got.bound - best) <= t
    assert np.all(got.energies[got.sweeps_run:] == got.energies[got.sweeps_run - 1]) and np.all(got.bounds[got.sweeps_run:] == got.bound)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_triangles_sharing_a_node(seed):
    """N = 5: once the run has reached its fixed point (sweeps_run < sweeps) the labelling is optimal and the bound tight"""
    case = _small([[0, 1, 2], [2, 3, 4]], 5, 3, seed)
    sweeps = 200
    got = _run(case, sweeps=sweeps)
    best, t = ML.brute_force(*case[:3]), ML.tol(*case[:3])
    print("sweeps_run %d energy %.17g optimum %.17g bound %.17g tol %.3g" % (got.sweeps_run, got.energy, best, got.bound, t))
    assert got.sweeps_run < sweeps
    assert got.energy == best and abs(got.bound - best) <= t
    _everywhere(case, got)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_octahedron_bound_and_energy_bracket_the_optimum(seed):
    """N = 6, T = 8, L = 3: 729 labellings"""
    case = _small(ML.OCTAHEDRON, 6, 3, seed)
    got = _run(case)
    best, t = ML.brute_force(*case[:3]), ML.tol(*case[:3])
    print("energy %.17g optimum %.17g bound %.17g tol %.3g" % (got.energy, best, got.bound, t))
    ML.same(got, ML.mplp(*case, SWEEPS))
    assert got.bound <= best + t and best <= got.energy
    _everywhere(case, got)


def test_ties_take_the_lowest_label():
    """whole-number tables: exact ties between beliefs; the lowest label wins and the bits are the restatement's"""
    case = ML.ico_case(1, 4, 21, 0.0, True)
    U, tc, triplets, start = case
    got = _run(case, sweeps=6)
    ML.same(got, ML.mplp(*case, 6))
    inc = ML.incidence(triplets, U.shape[1])
    beliefs = np.stack([ML.node_sum(U, got.messages, inc, i) for i in range(U.shape[1])])
    tied = (beliefs == beliefs.min(axis=1, keepdims=True)).sum(axis=1) > 1
    decoded = beliefs.argmin(axis=1)
    print("nodes with tied beliefs after the last sweep: %d of %d" % (tied.sum(), len(tied)))
    assert tied.sum() >= 3
    assert ML.energy(U, tc, triplets, decoded) == got.energies[got.sweeps_run - 1]  # the last decode is the lowest-label one
    _everywhere(case, got)
    # one constant everywhere: every decode is label 0 at the start's energy, and the first of equal candidates is the start
    flat = (np.full_like(U, 1.5), np.full_like(tc, -0.25), triplets, start)
    same = _run(flat, sweeps=4)
    assert np.array_equal(same.labeling, start) and start.any() and np.all(same.energies == same.energy)


def test_zero_work_calls_leave_the_labelling():
    U, tc, triplets, start = ML.ico_case(0, 5, 31)
    none = api.mplp_optimise(U, tc, triplets, start, sweeps=0, bounds=True, messages=True)
    assert np.array_equal(none.labeling, start) and none.sweeps_run == 0 and none.energy == ML.energy(U, tc, triplets, start)
    assert not none.messages.any() and len(none.energies) == 0
    ML.same(none, ML.mplp(U, tc, triplets, start, 0))
    empty = api.mplp_optimise(U, np.zeros((0, 5, 5, 5)), np.zeros((0, 3), dtype=np.int32), start, sweeps=3, bounds=True)
    assert np.array_equal(empty.labeling, start) and empty.sweeps_run == 0
    assert empty.bound == ML.mplp(U, np.zeros((0, 5, 5, 5)), np.zeros((0, 3), dtype=np.int32), start, 3).bound


def _raw(U, tc, triplets, start, sweeps):
    """msm_mplp_optimise with every output pre-filled: (status, the outputs afterwards, what they were filled with)"""
    U, tc = np.ascontiguousarray(U, dtype=np.float64), np.ascontiguousarray(tc, dtype=np.float64)
    triplets = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    L, N = U.shape
    T = len(triplets)
    lab = np.array(start, dtype=np.int32)
    run, energy, bound = C.c_int32(-7), C.c_double(-7.0), C.c_double(-7.0)
    energies, bounds, messages = np.full(sweeps, -7.0), np.full(sweeps, -7.0), np.full((T, 3, L), -7.0)
    st = lib().msm_mplp_optimise(U.ctypes.data_as(c_dp), tc.ctypes.data_as(c_dp), triplets.ctypes.data_as(c_ip), N, L, T, sweeps, lab.ctypes.data_as(c_ip),
                                 C.byref(run), C.byref(energy), C.byref(bound), energies.ctypes.data_as(c_dp), bounds.ctypes.data_as(c_dp),
                                 messages.ctypes.data_as(c_dp))
    untouched = (np.array_equal(lab, start) and run.value == -7 and energy.value == -7.0 and bound.value == -7.0 and np.all(energies == -7.0)
                 and np.all(bounds == -7.0) and np.all(messages == -7.0))
    return st, untouched


def test_refusals_leave_the_outputs_untouched():
    U, tc, triplets, start = (np.array(a) for a in ML.ico_case(0, 5, 31))
    N = U.shape[1]
    bad_label, bad_node, twice = np.array(start), np.array(triplets), np.array(triplets)
    bad_label[7] = 5
    bad_node[11, 2] = N
    twice[4, 2] = twice[4, 0]
    nan_u, inf_t = np.array(U), np.array(tc)
    nan_u[2, 3] = np.nan
    inf_t[19, 4, 4, 4] = -np.inf
    cases = [((U, tc, triplets, bad_label), "MSM_ERR_INVALID.*msm_mcmc_optimise: label of node 7 out of range"),
             ((U, tc, bad_node, start), "MSM_ERR_INVALID.*msm_mcmc_optimise: triplet node out of range"),
             ((U, tc, twice, start), "MSM_ERR_INVALID.*triplet 4 names a node twice"),
             ((nan_u, tc, triplets, start), "MSM_ERR_INVALID.*the unary table holds a non-finite value.*--fixnan"),
             ((U, inf_t, triplets, start), "MSM_ERR_INVALID.*the triplet table holds a non-finite value.*--fixnan"),
             ((np.zeros((1025, 3)), np.zeros((0, 1, 1, 1)), np.zeros((0, 3), dtype=np.int32), np.zeros(3, dtype=np.int32)), "MSM_ERR_CAPACITY.*1025 labels")]
    for args, pattern in cases:
        st, untouched = _raw(*args, 3)
        assert st != 0 and untouched, pattern
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_optimise(*args, sweeps=3)
    st, untouched = _raw(U, tc, triplets, start, 3)
    assert st == 0 and not untouched


def test_every_non_finite_entry_is_refused_by_its_table():
    """-inf, +inf and NaN in the triplet table, -inf in the unary table, and the unary table named first where both hold one"""
    for args, pattern in ML.non_finite_refusals():
        st, untouched = _raw(*args, 3)
        assert st != 0 and untouched, pattern
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_optimise(*args, sweeps=3)


def test_host_literal_under_the_sanitizers(tmp_path):
    """tests/cpp/mplp_host_check.cpp: the incidence lists and the literal as a program of their own (no HIP, no Python), built with
    -fsanitize=address,undefined and run directly"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mplp_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(root, "tests", "cpp", "mplp_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


CONF = "--opt=DISCRETE\n--simval=2\n--it=2\n--sigma_in=2\n--sigma_ref=2\n--lambda=0.1\n--datagrid=4\n--CPgrid=2\n--SGgrid=4\n--regoption=3\n--mciters=5\n--dopt=%s\n"


def test_config_takes_mplp_only_when_asked():
    cfg = config.parse_config(CONF % "MPLP")
    with pytest.raises(config.ConfigError, match="Unrecognized optimiser"):
        config.levels_from_config(cfg, 1)
    levels, _, _ = config.levels_from_config(cfg, 1, mplp=True)
    assert [lv["optimiser"] for lv in levels] == ["mplp"] and levels[0]["mciters"] == 5
    pairwise = config.parse_config((CONF % "MPLP").replace("--regoption=3", "--regoption=1"))
    with pytest.raises(config.ConfigError, match="--regoption=1"):
        config.levels_from_config(pairwise, 1, mplp=True)
    # the other optimisers are what they were, with and without the option
    for dopt, name in (("HOCR", "fusion"), ("MCMC", "mcmc")):
        for kw in ({}, dict(mplp=True)):
            assert config.levels_from_config(config.parse_config(CONF % dopt), 1, **kw)[0][0]["optimiser"] == name
    with pytest.raises(config.ConfigError, match="Unrecognized optimiser"):
        config.levels_from_config(config.parse_config(CONF % "ELC"), 1, mplp=True)
