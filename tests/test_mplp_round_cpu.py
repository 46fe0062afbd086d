"""The rounding of MPLP's messages on the host (msm_mplp_colouring, msm_mplp_round; newmsm_amd/csrc/mplp_host.hpp, DESIGN.md 5.19 "Rounding") against the
numpy restatement of its definition in mplp_round_literal.py, bit for bit, its properties, and what it is for.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api
from newmsm_amd._lib import c_dp, c_ip, lib

import mplp_literal as ML
import mplp_round_literal as RL


def _proper(triplets, colour):
    tri = np.asarray(triplets).reshape(-1, 3)
    c = colour[tri]
    return bool(np.all((c[:, 0] != c[:, 1]) & (c[:, 0] != c[:, 2]) & (c[:, 1] != c[:, 2])))


@pytest.mark.parametrize("name", ["ico0 L16", "ico2 L8", "ico2 L8 shuffled", "fan", "octahedron"])
def test_colouring_is_proper_and_the_restatement(name):
    U, _, triplets, _ = RL.CASES[name]()
    N = U.shape[1]
    colour, classes = api.mplp_colouring(triplets, N)
    assert np.array_equal(colour, RL.colouring(triplets, N)) and classes == colour.max() + 1
    assert _proper(triplets, colour) and colour[0] == 0
    print(name, "classes", classes, np.bincount(colour))
    if name == "fan":
        assert colour[13] == 0  # the node in no triplet
        assert api.mplp_colouring(np.zeros((0, 3), dtype=np.int32), 4)[1] == 1


@pytest.mark.parametrize("name", sorted(RL.CASES))
def test_literal_agrees_with_the_restatement(name):
    """both modes, polish 0 / 1 / 8, messages after 0 / 1 / 5 sweeps, NULL against zeros"""
    U, tc, triplets, start = case = RL.CASES[name]()
    for sweeps in (0, 1, 5):
        m, _ = RL.messages_after(name, sweeps)
        for polish in (0, 1, 8):
            got = api.mplp_round(*case, messages=m, mode=0, polish=polish)
            RL.same(got, RL.mplp_round(*case, messages=m, mode=0, polish=polish), (name, sweeps, polish))
            assert len(got.energies) == 2 + polish and got.energy == got.energies.min() and got.energy == ML.energy(U, tc, triplets, got.labeling)
            if sweeps == 0:
                RL.same(api.mplp_round(*case, messages=None, mode=0, polish=polish), got, (name, "NULL", polish))
    for polish in (0, 1, 8):
        got = api.mplp_round(*case, mode=1, polish=polish)
        RL.same(got, RL.mplp_round(*case, mode=1, polish=polish), (name, "mode 1", polish))
        assert len(got.energies) == 1 + polish and got.energies[0] == ML.energy(U, tc, triplets, start)
        RL.same(api.mplp_round(*case, messages=np.full((len(triplets), 3, U.shape[0]), np.nan), mode=1, polish=polish), got)  # mode 1 reads no messages


def test_every_slot_and_fixed_subset_occurs():
    """the permuted case: all 3 x 4 combinations of (slot of the node, which of the two others are fixed) in the conditioned decode"""
    U, tc, triplets, start = RL.CASES["twelve"]()
    seen = RL.combinations(triplets, U.shape[1])
    assert len(seen) == 12, sorted(seen)
    assert len(RL.combinations(ML.ico_case(1, 5, 17)[2], U.shape[1])) < 12  # the mesh's own order does not show them all


def test_ties_lowest_label_in_the_decode_current_label_in_the_polish():
    U, tc, triplets, start = case = RL.CASES["ties"]()
    N, L = U.shape[1], U.shape[0]
    m, _ = RL.messages_after("ties", 5)
    got = api.mplp_round(*case, messages=m, mode=0, polish=0)
    tri = np.asarray(triplets).reshape(-1, 3)
    inc, colour = ML.incidence(tri, N), RL.colouring(tri, N)
    lab, tied = np.array(start), 0
    for k in range(colour.max() + 1):  # the decode again, asserting the first of equal minima
        for i in np.nonzero(colour == k)[0]:
            sc = RL.score(U, tc, tri, m, inc, colour, k, lab, int(i))
            tied += int((sc == sc.min()).sum() > 1)
            lab[i] = int(np.nonzero(sc == sc.min())[0][0])
    assert tied >= 3
    assert got.energies[1] == ML.energy(U, tc, triplets, lab)
    # one constant everywhere: every score ties, the decode is all zero, and a polish pass keeps whatever it is given
    flat = (np.full_like(U, 1.5), np.full_like(tc, -0.25), triplets, start)
    kept = api.mplp_round(*flat, mode=1, polish=3)
    assert start.any() and np.array_equal(kept.labeling, start) and kept.passes_run == 1
    dec = api.mplp_round(*flat, mode=0, polish=3)
    assert np.array_equal(dec.labeling, start) and np.all(dec.energies == dec.energy)  # the first of equal candidates is the one handed in
    ones = np.ones(N, dtype=np.int32)
    tied_polish = api.mplp_round(U, tc, triplets, ones, mode=1, polish=1)  # labels 1 and 2 cost the same everywhere: no node moves from 1 to 2
    assert not np.any((tied_polish.labeling == 2))


@pytest.mark.parametrize("name", ["ico2 L8", "ico0 with 1e7", "fan", "twelve"])
def test_properties(name):
    U, tc, triplets, start = case = RL.CASES[name]()
    t = ML.tol(U, tc, triplets)
    m, _ = RL.messages_after(name, 5)
    e0 = ML.energy(U, tc, triplets, start)
    for mode in (0, 1):
        got = api.mplp_round(*case, messages=m, mode=mode, polish=64)
        assert got.energy <= e0 and got.energies[0] == e0
        steps = np.diff(got.energies[(1 if mode == 0 else 0):])
        print(name, mode, "passes", got.passes_run, "energies", got.energies[:4], "largest rise", steps.max())
        assert np.all(steps <= t)
        assert 1 <= got.passes_run < 64  # a fixed point
        again = api.mplp_round(U, tc, triplets, got.labeling, mode=1, polish=8)
        assert again.passes_run == 1 and np.array_equal(again.labeling, got.labeling) and np.all(again.energies == got.energy)


@pytest.mark.parametrize("args", [(2, 7, 13, 0.05), (0, 19, 19, 0.05)])
def test_rounding_leaves_the_1e7_entries_where_the_naive_decode_does_not(args):
    """after 10 sweeps the rounded energy lies below every naive-decode energy of those sweeps and below 1e7; the numpy restatement shows it first.
    ico2 / L = 7 is the issue's seed 13.  ico0 / L = 19 with seed 13 does not satisfy the statement: there the naive decode itself leaves the 1e7
    entries in sweep 8, at 2.5377255334685254, and the rounding returns the same labelling, equal and not below.  Seed 19 is taken instead: its naive
    decodes stay at 1e7 through all ten sweeps and the rounding gives 3.097."""
    U, tc, triplets, start = case = ML.ico_case(*args)
    r = api.mplp_optimise(U, tc, triplets, start, sweeps=10, bound=True, messages=True)
    got = api.mplp_round(*case, messages=r.messages, mode=0, polish=8)
    want = RL.mplp_round(*case, messages=r.messages, mode=0, polish=8)
    RL.same(got, want)
    print("naive decodes %s\nrounded %.6g polished %.6g bound %.6g" % (r.energies, got.energies[1], got.energies[-1], r.bound))
    for e in (want.energies[1], got.energies[1], got.energy):
        assert e < r.energies.min() and e < 1e7
    assert r.bound <= got.energy + ML.tol(U, tc, triplets)


@pytest.mark.parametrize("shape,seed", [("one", 1), ("one", 2), ("one", 3), ("two", 1), ("two", 2), ("two", 3)])
def test_tight_cases_round_to_the_optimum(shape, seed):
    """where the literal's bound meets the brute-force minimum within tol(), the rounded labelling has that energy within tol()"""
    triplets = [[0, 1, 2]] if shape == "one" else [[0, 1, 2], [2, 3, 4]]
    U, tc, triplets, start = case = RL._small(triplets, 3 if shape == "one" else 5, 3, seed)
    r = api.mplp_optimise(U, tc, triplets, start, sweeps=200, bound=True, messages=True)
    best, t = ML.brute_force(U, tc, triplets), ML.tol(U, tc, triplets)
    assert abs(r.bound - best) <= t  # the case is tight (test_mplp_cpu.py shows it for these seeds)
    got = api.mplp_round(*case, messages=r.messages, mode=0, polish=0)
    print("rounded %.17g optimum %.17g bound %.17g" % (got.energies[1], best, r.bound))
    assert abs(got.energies[1] - best) <= t and abs(got.energy - best) <= t


def _raw(U, tc, triplets, start, messages, mode, polish):
    U, tc = np.ascontiguousarray(U, dtype=np.float64), np.ascontiguousarray(tc, dtype=np.float64)
    triplets = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    L, N = U.shape
    lab = np.array(start, dtype=np.int32)
    run, energy = C.c_int32(-7), C.c_double(-7.0)
    energies = np.full(2 + max(polish, 0) + 2000 * (polish > 1024), -7.0)
    pm = C.cast(None, c_dp) if messages is None else np.ascontiguousarray(messages).ctypes.data_as(c_dp)
    st = lib().msm_mplp_round(U.ctypes.data_as(c_dp), tc.ctypes.data_as(c_dp), triplets.ctypes.data_as(c_ip), N, L, len(triplets), pm, mode, polish,
                              lab.ctypes.data_as(c_ip), C.byref(run), C.byref(energy), energies.ctypes.data_as(c_dp))
    return st, np.array_equal(lab, start) and run.value == -7 and energy.value == -7.0 and np.all(energies == -7.0)


def test_refusals_leave_the_outputs_untouched():
    ok, cases = RL.refusal_cases()
    for args, pattern in cases:
        st, untouched = _raw(*args)
        assert st != 0 and untouched, pattern
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_round(*args[:4], messages=args[4], mode=args[5], polish=args[6])
    st, untouched = _raw(*ok)
    assert st == 0 and not untouched
    with pytest.raises(M.MsmError, match="triplet 4 names a node twice"):
        api.mplp_colouring(cases[2][0][2], 12)
    with pytest.raises(M.MsmError, match="triplet node out of range"):
        api.mplp_colouring(cases[1][0][2], 12)


def test_mode_1_reads_no_messages():
    """the messages mode 0 refuses change nothing in mode 1"""
    ok, _ = RL.refusal_cases()
    want = api.mplp_round(*ok[:4], mode=1, polish=2)
    for m in RL.unread_messages():
        st, untouched = _raw(*ok[:4], m, 1, 2)
        assert st == 0 and not untouched
        RL.same(api.mplp_round(*ok[:4], messages=m, mode=1, polish=2), want)


def test_host_literal_under_the_sanitizers(tmp_path):
    """tests/cpp/mplp_round_host_check.cpp: the colouring and the rounding's literal as a program of their own (no HIP, no Python), built with
    -fsanitize=address,undefined and run directly"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mplp_round_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(root, "tests", "cpp", "mplp_round_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
