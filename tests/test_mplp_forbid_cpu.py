"""MPLP and its rounding under the forbidden-entry reading on the host (msm_mplp_classify, msm_mplp_optimise_forbid, msm_mplp_round_forbid;
newmsm_amd/csrc/mplp_host.hpp, DESIGN.md 5.19 "Forbidden entries") against the numpy restatement of the definition in mplp_forbid_literal.py, bit for
bit on every output, and the properties the definition promises.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api
from newmsm_amd._lib import c_dp, c_ip, c_lp, lib

import mplp_forbid_literal as FL
import mplp_literal as ML
import mplp_round_literal as RL

INF = np.inf


def _counts(tc):
    return [0, int(np.isnan(tc).sum()), int((tc == INF).sum()), int((tc == -INF).sum())]


@pytest.mark.parametrize("name", sorted(FL.CASES))
def test_literal_agrees_with_the_restatement(name):
    """sweeps, decode, energies, bounds and messages; then both modes of the rounding on those messages"""
    U, tc, triplets, start = case = FL.CASES[name]()
    counts = np.full(4, -1, dtype=np.int64)
    got = api.mplp_optimise(*case, sweeps=6, bound=True, bounds=True, messages=True, forbid=True, counts=counts)
    want = FL.mplp(*case, 6)
    ML.same(got, want, name)
    assert counts.tolist() == _counts(tc) == api.mplp_classify(U, tc).tolist()
    assert not np.isnan(got.messages).any() and not (got.messages == -INF).any()
    assert not np.isnan(got.energies).any() and not np.isnan(got.bounds).any()
    assert got.energy == FL.energy(U, tc, triplets, got.labeling) <= FL.energy(U, tc, triplets, start)
    ML.same(api.mplp_optimise(*case, sweeps=6, bound=True, forbid=True), want, name)  # the bound alone
    ML.same(api.mplp_optimise(*case, sweeps=0, bound=True, messages=True, forbid=True), FL.mplp(*case, 0), name)
    for mode in (0, 1):
        for polish in (0, 3):
            rc = np.full(4, -1, dtype=np.int64)
            r = api.mplp_round(U, tc, triplets, got.labeling, messages=got.messages, mode=mode, polish=polish, forbid=True, counts=rc)
            RL.same(r, FL.mplp_round(U, tc, triplets, got.labeling, messages=got.messages, mode=mode, polish=polish), (name, mode, polish))
            assert rc.tolist() == _counts(tc) and not np.isnan(r.energies).any()
            assert r.energy <= got.energy


def test_one_label_with_its_single_entry_forbidden():
    U, tc, triplets, start = case = FL.CASES["triplet L1 forbidden"]()
    got = api.mplp_optimise(*case, sweeps=3, bounds=True, messages=True, forbid=True)
    assert got.bound == INF and got.energy == INF and np.array_equal(got.labeling, start) and np.all(got.bounds == INF)
    assert np.all(got.messages == INF)
    r = api.mplp_round(*case, messages=got.messages, mode=0, polish=2, forbid=True)
    assert r.energy == INF and np.array_equal(r.labeling, start) and np.all(r.energies == INF)


def test_octahedron_bound_against_brute_force():
    """D <= the brute-force optimum + tol on every sweep, D non-decreasing within tol; at least one seed is infeasible (optimum +inf) and three are
    feasible.  tol = 64 (N + T) 2^-52 max(1, max|unary|, largest finite |message|)."""
    feasible = infeasible = 0
    for seed in FL.OCTAHEDRON_SEEDS:
        U, tc, triplets, start = case = FL.octahedron(seed)
        best = FL.brute_force(U, tc, triplets)
        got = api.mplp_optimise(*case, sweeps=30, bounds=True, messages=True, forbid=True)
        t = FL.tol(U, triplets, got.messages)
        print("seed %d optimum %.17g bound %.17g energy %.17g sweeps %d infinite messages %d tol %.3g" % (
            seed, best, got.bound, got.energy, got.sweeps_run, int(np.isinf(got.messages).sum()), t))
        feasible += best < INF
        infeasible += best == INF
        assert np.all(got.bounds <= best + t)
        assert not np.any(got.bounds[:-1] > got.bounds[1:] + t)  # never falls (a bound at +inf stays there)
        if best == INF:
            assert got.energy == INF
        else:
            assert got.energy >= best - t and got.bound < INF
    assert infeasible >= 1 and feasible >= 3


def test_fan_proves_the_forbidden_hub_label_infeasible():
    U, tc, triplets, start = case = FL.fan()
    assert np.isnan(tc[0, 1]).all() and (tc[5, :, 2, :] == INF).all() and U[1, 0] == U[:, 0].min()
    one = api.mplp_optimise(*case, sweeps=1, messages=True, forbid=True)
    assert one.messages[0, 0, 1] == INF
    for sweeps in (1, 2, 5, 12):
        got = api.mplp_optimise(*case, sweeps=sweeps, bounds=True, messages=True, forbid=True)
        ML.same(got, FL.mplp(*case, sweeps), sweeps)
        assert not np.isnan(got.messages).any() and not (got.messages == -INF).any()
    print("infinite messages per factor", np.isinf(got.messages).sum(axis=(1, 2)), "bound", got.bound, "energy", got.energy)
    assert np.isinf(got.messages[1:, 0, 1]).any()  # the hub's infeasible label reaches its other factors
    assert got.labeling[0] != 1 and got.energy < INF and not FL.uses_forbidden(tc, triplets, got.labeling)
    assert got.bound <= got.energy + FL.tol(U, triplets, got.messages)
    for mode in (0, 1):
        r = api.mplp_round(U, tc, triplets, start, messages=got.messages, mode=mode, polish=8, forbid=True)
        RL.same(r, FL.mplp_round(U, tc, triplets, start, messages=got.messages, mode=mode, polish=8), mode)
        assert r.labeling[0] != 1 and r.energy < INF


def test_ico0_starts_and_the_fixed_point():
    """a start on a forbidden entry is beaten; a finite start is never made worse; a run to its fixed point and past it"""
    on = FL.CASES["ico0 L19 start forbidden"]()
    off = FL.CASES["ico0 L19"]()
    assert FL.energy(on[0], on[1], on[2], on[3]) == INF and FL.energy(off[0], off[1], off[2], off[3]) < INF
    got = api.mplp_optimise(*on, sweeps=10, forbid=True)
    assert got.energy < INF and not FL.uses_forbidden(on[1], on[2], got.labeling)
    got = api.mplp_optimise(*off, sweeps=10, forbid=True)
    assert got.energy <= FL.energy(off[0], off[1], off[2], off[3])
    U, tc, triplets, start = case = FL.CASES["two triangles"]()
    long = api.mplp_optimise(*case, sweeps=100, bounds=True, messages=True, forbid=True)
    assert 3 < long.sweeps_run < 100, long.sweeps_run
    ML.same(long, FL.mplp(*case, 100), "fixed point")
    assert np.all(long.bounds[long.sweeps_run - 1:] == long.bound)


@pytest.mark.parametrize("args", [(0, 19, 11), (0, 19, 13, 0.05)])
def test_equivalence_on_tables_without_forbidden_entries(args):
    U, tc, triplets, start = case = ML.ico_case(*args)
    counts = np.full(4, -1, dtype=np.int64)
    plain = api.mplp_optimise(*case, sweeps=8, bounds=True, messages=True)
    ML.same(api.mplp_optimise(*case, sweeps=8, bounds=True, messages=True, forbid=True, counts=counts), plain)
    assert counts.tolist() == [0, 0, 0, 0]
    for mode in (0, 1):
        counts[:] = -1
        r = api.mplp_round(*case, messages=plain.messages, mode=mode, polish=4, forbid=True, counts=counts)
        RL.same(r, api.mplp_round(*case, messages=plain.messages, mode=mode, polish=4))
        assert counts.tolist() == [0, 0, 0, 0]


def _raw_optimise(U, tc, triplets, start):
    U, tc = np.ascontiguousarray(U, dtype=np.float64), np.ascontiguousarray(tc, dtype=np.float64)
    triplets = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    L, N = U.shape
    T = len(triplets)
    lab, run = np.array(start, dtype=np.int32), C.c_int32(-7)
    energy, bound, energies, bounds, m = C.c_double(-7.0), C.c_double(-7.0), np.full(3, -7.0), np.full(3, -7.0), np.full((T, 3, L), -7.0)
    counts = np.full(4, -7, dtype=np.int64)
    st = lib().msm_mplp_optimise_forbid(U.ctypes.data_as(c_dp), tc.ctypes.data_as(c_dp), triplets.ctypes.data_as(c_ip), N, L, T, 3, lab.ctypes.data_as(c_ip),
                                        C.byref(run), C.byref(energy), C.byref(bound), energies.ctypes.data_as(c_dp), bounds.ctypes.data_as(c_dp),
                                        m.ctypes.data_as(c_dp), counts.ctypes.data_as(c_lp))
    untouched = (np.array_equal(lab, start) and run.value == -7 and energy.value == -7.0 and bound.value == -7.0 and np.all(energies == -7.0)
                 and np.all(bounds == -7.0) and np.all(m == -7.0))
    return st, untouched


def _raw_round(U, tc, triplets, start, messages):
    U, tc = np.ascontiguousarray(U, dtype=np.float64), np.ascontiguousarray(tc, dtype=np.float64)
    triplets = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    L, N = U.shape
    lab, run, energy, energies = np.array(start, dtype=np.int32), C.c_int32(-7), C.c_double(-7.0), np.full(4, -7.0)
    pm = C.cast(None, c_dp) if messages is None else np.ascontiguousarray(messages).ctypes.data_as(c_dp)
    st = lib().msm_mplp_round_forbid(U.ctypes.data_as(c_dp), tc.ctypes.data_as(c_dp), triplets.ctypes.data_as(c_ip), N, L, len(triplets), pm, 0, 2,
                                     lab.ctypes.data_as(c_ip), C.byref(run), C.byref(energy), energies.ctypes.data_as(c_dp), C.cast(None, c_lp))
    return st, np.array_equal(lab, start) and run.value == -7 and energy.value == -7.0 and np.all(energies == -7.0)


def test_refusals_leave_the_outputs_untouched():
    ok, cases = FL.refusal_cases()
    for args, pattern in cases:
        st, untouched = _raw_optimise(*args)
        assert st != 0 and untouched, pattern
        st, untouched = _raw_round(*args, None)
        assert st != 0 and untouched, pattern
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_optimise(*args, sweeps=3, forbid=True)
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_round(*args, mode=1, polish=2, forbid=True)
    st, untouched = _raw_optimise(*ok)
    assert st == 0 and not untouched
    T, L = len(ok[2]), ok[0].shape[0]
    for value, pattern in ((np.nan, "MSM_ERR_INVALID.*the messages hold a NaN"), (-INF, "MSM_ERR_INVALID.*the messages hold -infinity")):
        m = np.zeros((T, 3, L))
        m[3, 1, 2] = value
        st, untouched = _raw_round(*ok, m)
        assert st != 0 and untouched, pattern
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_round(*ok, messages=m, mode=0, polish=2, forbid=True)
        api.mplp_round(*ok, messages=m, mode=1, polish=2, forbid=True)  # mode 1 reads no messages
    m = np.zeros((T, 3, L))
    m[3, 1, 2] = INF  # allowed
    st, untouched = _raw_round(*ok, m)
    assert st == 0 and not untouched
    RL.same(api.mplp_round(*ok, messages=m, mode=0, polish=2, forbid=True), FL.mplp_round(*ok, messages=m, mode=0, polish=2))
    # the plain entry points still refuse the table
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*the triplet table holds a non-finite value.*--fixnan"):
        api.mplp_optimise(*ok, sweeps=3)
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*the triplet table holds a non-finite value.*--fixnan"):
        api.mplp_round(*ok, mode=1, polish=2)


def test_the_last_entry_of_the_table_is_counted():
    U, tc, triplets, start = case = ML.last_entry_forbidden()
    assert api.mplp_classify(U, tc).tolist() == [0, 0, 1, 0]
    counts = np.full(4, -1, dtype=np.int64)
    got = api.mplp_optimise(*case, sweeps=3, bounds=True, messages=True, forbid=True, counts=counts)
    assert counts.tolist() == [0, 0, 1, 0]
    ML.same(got, FL.mplp(*case, 3))
    for mode in (0, 1):
        counts[:] = -1
        api.mplp_round(*case, messages=got.messages, mode=mode, polish=2, forbid=True, counts=counts)
        assert counts.tolist() == [0, 0, 1, 0]


def test_host_literal_under_the_sanitizers(tmp_path):
    """tests/cpp/mplp_forbid_host_check.cpp: the literal with forbid set as a program of its own (no HIP, no Python), built with
    -fsanitize=address,undefined and run directly"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mplp_forbid_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(root, "tests", "cpp", "mplp_forbid_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
