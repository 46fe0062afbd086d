"""MPLP over the pair tables on the host (msm_mplp_pairs_optimise / _polish / _colouring / _energy; newmsm_amd/csrc/mplp_pairs_host.hpp, DESIGN.md
5.20) against the numpy restatement of the definition in mplp_pairs_literal.py, bit for bit, against brute force on graphs small enough for it, on real
tables from the oracle, and the opt-in of the configuration in Python and C++.  No GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, config, problem
from newmsm_amd._lib import c_dp, c_ip, lib

import mplp_pairs_literal as PL
from tests.helpers import oracle_cost

pytestmark = pytest.mark.usefixtures("built")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = PL.SHARED
IDS = [name for name, _, _ in CASES]


def _run(case, sweeps):
    U, pc, pairs, start = case
    return api.mplp_pairs_optimise(U, pc, pairs, start, sweeps=sweeps, bounds=True, messages=True)


def _promises(case, got):
    """never worse than the start, every bound below every candidate's energy, the bound never falls (all up to tol)"""
    U, pc, pairs, start = case
    pc3 = np.asarray(pc).reshape(len(pairs), U.shape[0], U.shape[0])
    t = PL.tol(U, pc3, pairs)
    e0 = PL.energy(U, pc3, pairs, start)
    steps = np.diff(got.bounds)
    print("start %.17g energy %.17g bound %.17g tol %.3g lowest step of the bound %.3g" % (e0, got.energy, got.bound, t, steps.min() if len(steps) else 0.0))
    assert got.energy <= e0 and got.energy == PL.energy(U, pc3, pairs, got.labeling)
    if got.sweeps_run:
        assert got.energy == min(e0, got.energies.min()) and got.bound == got.bounds[-1]
        assert got.bounds.max() <= min(e0, got.energies.min()) + t
        assert np.all(steps >= -t)
    return t


@pytest.mark.parametrize("name,spec,sweeps", CASES, ids=IDS)
def test_literal_agrees_with_the_restatement(name, spec, sweeps):
    """labelling, sweeps run, energies, bounds and messages, bit for bit, and the promises"""
    case = PL.make(spec)
    got = _run(case, sweeps)
    PL.same(got, PL.mplp(*case, sweeps), name)
    _promises(case, got)
    assert api.mplp_pairs_energy(*case[:3], got.labeling) == got.energy


def test_optional_outputs_do_not_change_the_others():
    case = PL.ico_case(0, 19)
    full = _run(case, 10)
    bare = api.mplp_pairs_optimise(*case, sweeps=10, bound=False)
    assert bare.bound is None and bare.bounds is None and bare.messages is None
    PL.same(bare, full)
    PL.same(api.mplp_pairs_optimise(*case, sweeps=10, bound=True), full)  # the bound alone: one pass after the last sweep


@pytest.mark.parametrize("name,spec,sweeps", CASES, ids=IDS)
def test_colourings(name, spec, sweeps):
    """no two pairs of a class share a node, no two nodes of a class share a pair, every colour is the smallest admissible one"""
    U, pc, pairs, start = PL.make(spec)
    N = U.shape[1]
    pcol, pk, ncol, nk = api.mplp_pairs_colouring(pairs, N)
    want_p, _ = PL.pair_colouring(pairs)
    want_n, _ = PL.node_colouring(pairs, N)
    assert np.array_equal(pcol, want_p) and np.array_equal(ncol, want_n)
    assert pk == pcol.max() + 1 and nk == ncol.max() + 1
    for c in range(pk):
        nodes = np.asarray(pairs)[pcol == c].ravel()
        assert len(set(nodes.tolist())) == len(nodes)
    for A, B in np.asarray(pairs):
        assert ncol[A] != ncol[B]
    for p, (A, B) in enumerate(np.asarray(pairs)):  # smallest admissible: every lower colour is held by a lower pair on A or B
        lower = {int(pcol[q]) for q in range(p) if {int(pairs[q][0]), int(pairs[q][1])} & {int(A), int(B)}}
        assert pcol[p] not in lower and set(range(pcol[p])) <= lower
    nb = [set() for _ in range(N)]
    for A, B in np.asarray(pairs):
        nb[A].add(int(B)), nb[B].add(int(A))
    for i in range(N):
        lower = {int(ncol[j]) for j in nb[i] if j < i}
        assert ncol[i] not in lower and set(range(ncol[i])) <= lower


def test_star_colourings_and_the_isolated_node():
    U, pc, pairs, start = PL.star_case()
    pcol, pk, ncol, nk = api.mplp_pairs_colouring(pairs, U.shape[1])
    assert pk == 40 and np.array_equal(pcol, np.arange(40)) and nk == 2
    assert ncol[0] == 0 and ncol[41] == 0 and np.all(ncol[1:41] == 1)
    got = _run((U, pc, pairs, start), 3)
    assert got.labeling[41] == np.argmin(U[:, 41])  # a node in no pair decodes to the argmin of its unary costs
    pcol, pk, ncol, nk = api.mplp_pairs_colouring(np.zeros((0, 2), dtype=np.int32), 3)
    assert pk == 0 and nk == 1 and not ncol.any()


# seeds for which the numpy restatement alone reaches the optimum with a tight bound within 200 sweeps (checked in the test before the library is)
TREE_SEEDS = [1, 2, 3, 4, 5, 6]
STAR5 = np.array([[0, 1], [2, 0], [0, 3], [4, 0], [0, 5]], dtype=np.int32)


@pytest.mark.parametrize("seed", TREE_SEEDS)
@pytest.mark.parametrize("tree", ["chain of 6", "star of 5 leaves"])
def test_trees_are_solved_exactly(tree, seed):
    """L = 3, uniform random tables: the brute-force minimum, and the final bound within tol of it after at most 200 sweeps"""
    case = PL.chain_case(6, 3, seed) if tree == "chain of 6" else PL.random_case(STAR5, 6, 3, seed)
    best, t = PL.brute_force(*case[:3]), PL.tol(*case[:3])
    want = PL.mplp(*case, 200)
    assert want.energy == best and abs(want.bound - best) <= t, "the seed does not serve: the restatement itself misses"
    got = _run(case, 200)
    print("sweeps_run %d energy %.17g optimum %.17g bound %.17g tol %.3g" % (got.sweeps_run, got.energy, best, got.bound, t))
    PL.same(got, want)
    assert got.energy == best and abs(got.bound - best) <= t
    _promises(case, got)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("graph", ["triangle with a tail", "K4"])
def test_cycles_bracket_the_optimum(graph, seed):
    """graphs with cycles: the relaxation may leave a gap, so only bound <= minimum + tol <= returned + tol"""
    pairs, N = (PL.TRIANGLE_WITH_TAIL, 5) if graph == "triangle with a tail" else (PL.K4, 4)
    case = PL.random_case(pairs, N, 3, seed)
    got = _run(case, 50)
    best, t = PL.brute_force(*case[:3]), PL.tol(*case[:3])
    print("energy %.17g optimum %.17g bound %.17g tol %.3g" % (got.energy, best, got.bound, t))
    PL.same(got, PL.mplp(*case, 50))
    assert got.bound <= best + t and best <= got.energy + t
    _promises(case, got)


def test_ties_take_the_lowest_label():
    """whole-number tables: exact ties between beliefs; the lowest label wins"""
    case = PL.ico_case(1, 4, 21, 0.0, True)
    U, pc, pairs, start = case
    got = _run(case, 6)
    inc = PL.incidence(pairs, U.shape[1])
    beliefs = np.stack([PL.node_sum(U, got.messages, inc, i) for i in range(U.shape[1])])
    tied = (beliefs == beliefs.min(axis=1, keepdims=True)).sum(axis=1) > 1
    print("nodes with tied beliefs after the last sweep: %d of %d" % (tied.sum(), len(tied)))
    assert tied.sum() >= 3
    assert PL.energy(U, pc, pairs, beliefs.argmin(axis=1)) == got.energies[got.sweeps_run - 1]
    flat = (np.full_like(U, 1.5), np.full_like(pc, -0.25), pairs, start)  # one constant everywhere: the first of equal candidates is the start
    same = _run(flat, 4)
    assert np.array_equal(same.labeling, start) and start.any() and np.all(same.energies == same.energy)


def test_zero_work_calls_leave_the_labelling():
    U, pc, pairs, start = PL.ico_case(0, 5, 31)
    none = api.mplp_pairs_optimise(U, pc, pairs, start, sweeps=0, bounds=True, messages=True)
    assert np.array_equal(none.labeling, start) and none.sweeps_run == 0 and none.energy == PL.energy(U, pc, pairs, start)
    assert not none.messages.any() and len(none.energies) == 0
    PL.same(none, PL.mplp(U, pc, pairs, start, 0))
    no_pairs = (U, np.zeros((0, 5, 5)), np.zeros((0, 2), dtype=np.int32), start)
    empty = api.mplp_pairs_optimise(*no_pairs, sweeps=3, bounds=True)
    assert np.array_equal(empty.labeling, start) and empty.sweeps_run == 0 and empty.bound == PL.mplp(*no_pairs, 3).bound


# ---------------------------------------------------------------- the polish

@pytest.mark.parametrize("name,spec,sweeps", CASES, ids=IDS)
@pytest.mark.parametrize("passes", [0, 1, 8, 40])
def test_polish_agrees_with_the_restatement(name, spec, sweeps, passes):
    U, pc, pairs, start = PL.make(spec)
    got = api.mplp_pairs_polish(U, pc, pairs, start, polish=passes)
    PL.same_round(got, PL.polish(U, pc, pairs, start, passes), name)
    assert got.energy <= got.energies[0] == PL.energy(U, pc, pairs, start) and got.energy == got.energies.min()  # it never raises the energy
    assert got.energy == PL.energy(U, pc, pairs, got.labeling)
    if passes == 40:  # it ends at its fixed point, which no single node improves
        assert got.passes_run < passes
        again = api.mplp_pairs_polish(U, pc, pairs, got.labeling, polish=3)
        assert again.passes_run == 1 and np.array_equal(again.labeling, got.labeling)
        t = PL.tol(U, pc, pairs)
        for i in range(U.shape[1]):
            for x in range(U.shape[0]):
                lab = np.array(got.labeling)
                lab[i] = x
                assert PL.energy(U, pc, pairs, lab) >= got.energy - t


def test_polish_of_the_sweeps_winner_never_raises_it():
    case = PL.ico_case(2, 7)
    U, pc, pairs, start = case
    swept = _run(case, 5)
    got = api.mplp_pairs_polish(U, pc, pairs, swept.labeling, polish=8)
    assert got.energies[0] == swept.energy and got.energy <= swept.energy and got.energy >= swept.bound - PL.tol(U, pc, pairs)


# ---------------------------------------------------------------- refusals

_raw = PL.raw


def test_refusals_leave_the_outputs_untouched():
    for args, pattern in PL.refusals():
        st, st2, untouched = _raw(*args, 3)
        assert st != 0 and st2 != 0 and untouched, pattern
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_pairs_optimise(*args, sweeps=3)
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_pairs_polish(*args, polish=3)
    U, pc, pairs, start = PL.ico_case(0, 5, 31)
    st, st2, untouched = _raw(U, pc, pairs, start, -1)  # a negative count of sweeps, of passes
    assert st != 0 and st2 != 0 and untouched
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*polish passes"):
        api.mplp_pairs_polish(U, pc, pairs, start, polish=-1)
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*pair 0 names a node twice"):
        api.mplp_pairs_colouring(np.array([[2, 2]], dtype=np.int32), 3)
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*pair node out of range"):
        api.mplp_pairs_colouring(np.array([[0, 3]], dtype=np.int32), 3)
    for counts in (dict(N=0), dict(N=-3), dict(L=0), dict(L=-1), dict(P=-1)):  # negative counts, and no nodes or labels at all
        st, st2, untouched = _raw(U, pc, pairs, start, 3, **counts)
        assert st != 0 and st2 != 0 and untouched, counts
        N, L, P = (counts.get(k, v) for k, v in (("N", U.shape[1]), ("L", U.shape[0]), ("P", len(pairs))))
        e, k = C.c_double(-7.0), C.c_int32(-7)
        colour = np.full(len(pairs) + U.shape[1], -7, dtype=np.int32)
        assert lib().msm_mplp_pairs_energy(U.ctypes.data_as(c_dp), pc.ctypes.data_as(c_dp), pairs.ctypes.data_as(c_ip), N, L, P, start.ctypes.data_as(c_ip),
                                           C.byref(e)) != 0 and e.value == -7.0
        if "L" not in counts:  # (the colouring has no label count)
            assert lib().msm_mplp_pairs_colouring(pairs.ctypes.data_as(c_ip), N, P, colour.ctypes.data_as(c_ip), C.byref(k), colour.ctypes.data_as(c_ip),
                                                  C.byref(k)) != 0 and k.value == -7 and np.all(colour == -7)
    st, st2, untouched = _raw(U, pc, pairs, start, 3)
    assert st == 0 and st2 == 0 and not untouched


# ---------------------------------------------------------------- real tables

@functools.lru_cache(maxsize=None)
def _oracle_tables():
    """the oracle's unary and pair tables at data ico4 / control grid ico2, lambda 0.1, exponent 2"""
    inp = problem.pairwise_inputs(data_order=4, cp_order=2, D=1)
    oc = oracle_cost(inp, "univariate", rmode=1, lambda_=0.1, rexp=2.0)
    oc.get_source_data()
    U = oc.unary_table()
    L = U.shape[0]
    pairs = np.ascontiguousarray(inp["pairs"], dtype=np.int32)
    return U, oc.pairwise_table().reshape(len(pairs), L, L), pairs


def test_real_tables_from_the_oracle():
    """the promises hold, and the bound lies below the energy of the stand-in solve's labelling too"""
    U, pc, pairs = _oracle_tables()
    zero = np.zeros(U.shape[1], dtype=np.int32)
    got = _run((U, pc, pairs, zero), 30)
    t = _promises((U, pc, pairs, zero), got)
    icm = api.pairwise_icm(U, pc, pairs, passes=100)
    e_icm = PL.energy(U, pc, pairs, icm)
    polished = api.mplp_pairs_polish(U, pc, pairs, got.labeling, polish=8)
    print("zero %.17g icm %.17g decode after 1/5/10/20/30 %s polished %.17g bound %.17g" % (
        PL.energy(U, pc, pairs, zero), e_icm, " ".join("%.6g" % got.energies[k - 1] for k in (1, 5, 10, 20, 30)), polished.energy, got.bound))
    assert got.bounds.max() <= e_icm + t and polished.energy <= got.energy and got.bound <= polished.energy + t
    PL.same(got, PL.mplp(U, pc, pairs, zero, 30))


# ---------------------------------------------------------------- the stand-alone program and the configuration

def test_host_literal_under_the_sanitizers(tmp_path):
    """tests/cpp/mplp_pairs_host_check.cpp: the incidence, both colourings, the literal and the polish as a program of their own (no HIP, no Python),
    built with -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "mplp_pairs_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpp", "mplp_pairs_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


CONF = ("--opt=DISCRETE\n--simval=2\n--it=2\n--sigma_in=2\n--sigma_ref=2\n--lambda=0.1\n--datagrid=4\n--CPgrid=2\n--SGgrid=4\n--regoption=%s\n--mciters=5\n"
        "--dopt=%s\n")


def test_config_takes_mplp_over_pairs_only_when_asked():
    pairwise = config.parse_config(CONF % (1, "MPLP"))
    levels, _, _ = config.levels_from_config(pairwise, 1, mplp=True, mplp_pairs=True)
    assert [lv["optimiser"] for lv in levels] == ["mplp_pairs"] and levels[0]["mciters"] == 5 and levels[0]["rmode"] == 1
    with pytest.raises(config.ConfigError, match="--regoption=1"):
        config.levels_from_config(pairwise, 1, mplp=True)
    for kw in (dict(mplp_pairs=True), {}):
        with pytest.raises(config.ConfigError, match="Unrecognized optimiser"):
            config.levels_from_config(pairwise, 1, **kw)
    # the other optimisers, and MPLP over triplets, are what they were, with and without the options
    for kw in ({}, dict(mplp=True), dict(mplp=True, mplp_pairs=True)):
        for reg, dopt, name in ((3, "HOCR", "fusion"), (3, "MCMC", "mcmc"), (1, "FastPD", "fastpd")):
            assert config.levels_from_config(config.parse_config(CONF % (reg, dopt)), 1, **kw)[0][0]["optimiser"] == name
        with pytest.raises(config.ConfigError, match="--regoption=1"):
            config.levels_from_config(config.parse_config(CONF % (1, "HOCR")), 1, **kw)
        with pytest.raises(config.ConfigError, match="Unrecognized optimiser"):
            config.levels_from_config(config.parse_config(CONF % (3, "ELC")), 1, **kw)
    assert config.levels_from_config(config.parse_config(CONF % (3, "MPLP")), 1, mplp=True, mplp_pairs=True)[0][0]["optimiser"] == "mplp"
    assert config.levels_from_config(pairwise, 2, groupwise=True, mplp=True, mplp_pairs=True)[0][0]["optimiser"] == "mplp"  # a group run has its own model


def test_cpp_config_takes_mplp_over_pairs_only_when_asked(built, tmp_path):
    """include/msmhip_config.hpp's levels_from_config through tests/cpp/mplp_pairs_config_check.cpp"""
    exe, conf = str(tmp_path / "mplp_pairs_config_check"), tmp_path / "conf"
    conf.write_text(CONF % ("%REG%", "%DOPT%"))
    libdir = os.path.join(ROOT, "newmsm_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mplp_pairs_config_check.cpp"), "-o", exe, "-L", libdir, "-lmsmhip", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe, str(conf)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
