"""gMSM with the Monte Carlo optimiser, subject by subject: what needs no GPU.  The incidence of a pair list against the literal, the
conditional identity on random tables, the acceptance and the seed rule, a literal pass over the host optimiser, the host pieces under the sanitizers as a
program of their own, and the executables' refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api
from tests import group_mcmc_literal as lit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def group_pairs(S, N, rng, spread=None):
    """estimate_pairs' shape: for a < b and every node v of a, (a N + v, b N + some node of b); spread < N leaves nodes of b without an incoming pair"""
    spread = N if spread is None else spread
    return np.array([(a * N + v, b * N + int(rng.integers(0, spread))) for a in range(S) for v in range(N) for b in range(a + 1, S)], dtype=np.int32).reshape(-1, 2)


@pytest.mark.parametrize("S,N,spread", [(2, 42, 42), (2, 42, 9), (3, 42, 30), (4, 17, 1), (1, 5, 5)])
def test_incidence_against_the_literal(built, S, N, spread):
    rng = np.random.default_rng(100 * S + spread)
    pairs = group_pairs(S, N, rng, spread)
    ptr, idx = api.group_mcmc_incidence(pairs, S * N)
    wptr, widx = lit.incidence(pairs, S * N)
    assert np.array_equal(ptr, wptr) and np.array_equal(idx, widx)
    if 1 < spread < N:
        assert np.any(np.diff(ptr)[(S - 1) * N:] == 0)  # nodes of the last subject without a pair
    assert len(idx) == 2 * len(pairs)


def test_incidence_of_random_lists_and_its_refusals(built):
    rng = np.random.default_rng(3)
    pairs = rng.integers(0, 25, size=(200, 2)).astype(np.int32)  # any list: repeated nodes, nodes named twice by one pair, nodes never named
    pairs[7] = (4, 4)
    ptr, idx = api.group_mcmc_incidence(pairs, 31)
    wptr, widx = lit.incidence(pairs, 31)
    assert np.array_equal(ptr, wptr) and np.array_equal(idx, widx) and np.all(np.diff(ptr)[25:] == 0)
    for bad in ((0, 31), (-1, 2)):
        with pytest.raises(M.MsmError) as e:
            api.group_mcmc_incidence(np.array([bad], dtype=np.int32), 31)
        assert e.value.code == -1


def random_problem(S=3, N=12, L=4, Tc=9, seed=0):
    rng = np.random.default_rng(seed)
    pairs = group_pairs(S, N, rng, spread=max(2, N // 2))
    PT = rng.normal(size=(len(pairs), L, L))
    tri_local = np.array([sorted(rng.choice(N, 3, replace=False)) for _ in range(Tc)], dtype=np.int32)
    triplets = np.concatenate([tri_local + s * N for s in range(S)])
    tc = rng.normal(size=(S * Tc, L, L, L))
    return rng, pairs, PT, tri_local, triplets, tc


@pytest.mark.parametrize("s", [0, 1, 2])
def test_conditional_identity_on_random_tables(s):
    """the group energy with subject s relabelled x, minus E_s(x), does not depend on x: every incident pair appears once in U_s"""
    S, N, L, Tc = 3, 12, 4, 9
    rng, pairs, PT, tri_local, triplets, tc = random_problem(S, N, L, Tc, seed=11 + s)
    lab = rng.integers(0, L, S * N).astype(np.int32)
    ptr, idx = lit.incidence(pairs, S * N)
    U = lit.conditional_unary(PT, pairs, ptr, idx, lab, s, N, L)
    tc_s = tc[s * Tc:(s + 1) * Tc]
    rest = []
    for _ in range(20):
        x = rng.integers(0, L, N).astype(np.int32)
        full = lab.copy()
        full[s * N:(s + 1) * N] = x
        rest.append(lit.group_energy(PT, tc, pairs, triplets, full) - lit.block_energy(U, tc_s, tri_local, x))
    rest = np.array(rest)
    scale = np.sum(np.abs(PT[:, 0, 0])) + np.sum(np.abs(tc[:, 0, 0, 0]))  # the size of the sums the difference is taken of
    assert np.max(np.abs(rest - rest[0])) <= 1e-12 * scale


def test_acceptance_rule_on_crafted_energies(built):
    nan, inf = float("nan"), float("inf")
    cases = [(1.0, 1.0, False), (1.0, np.nextafter(1.0, 0.0), True), (1.0, np.nextafter(1.0, 2.0), False), (1.0, nan, False), (nan, 1.0, False),
             (nan, nan, False), (inf, 1e7, True), (inf, inf, False), (0.0, -0.0, False), (-1.0, -2.0, True)]
    for start, best, want in cases:
        assert api.group_mcmc_accept(start, best) is want and lit.accept(start, best) is want, (start, best)


def test_seed_rule(built):
    assert list(api.group_mcmc_seeds(42, 3, 4, 5, 0)) == list(api.chain_seeds(42, 3, 4))  # subject 0 in pass 0: the pairwise loops' seeds
    for seed0, it, K, S, s, p in [(0, 0, 1, 2, 1, 0), (7, 2, 5, 4, 3, 1), ((1 << 64) - 1, 1, 3, 64, 63, 2)]:
        got = api.group_mcmc_seeds(seed0, it, K, S, s, pass_=p)
        assert [int(x) for x in got] == [lit.seed(seed0, it, k, p, S, s) for k in range(K)]
    assert int(api.group_mcmc_seeds(1, 2, 4, 4, 2, pass_=1)[3]) == 1 + 2 + 3 * 1000003 + 15485863 * 6
    for K in (0, 257):
        with pytest.raises(M.MsmError):
            api.group_mcmc_seeds(0, 0, K, 2, 0)
    with pytest.raises(M.MsmError):
        api.group_mcmc_seeds(0, 0, 1, 2, 2)


@pytest.mark.parametrize("K,passes", [(1, 1), (3, 2)])
def test_a_literal_pass_over_the_host_optimiser_never_raises_the_energy(built, K, passes):
    S, N, L, Tc = 3, 12, 4, 9
    rng, pairs, PT, tri_local, triplets, tc = random_problem(S, N, L, Tc, seed=5)
    ptr, idx = lit.incidence(pairs, S * N)

    def tables(s, lab):
        return lit.conditional_unary(PT, pairs, ptr, idx, lab, s, N, L), tc[s * Tc:(s + 1) * Tc], tri_local

    def chains(U, tcs, tri, start, seeds, mcparam, iters):
        return api.mcmc_optimise_chains(U, tcs, tri, start, seeds, mcparam=mcparam, iters=iters)

    lab0 = np.zeros(S * N, dtype=np.int32)
    lab, recs = lit.run_pass(chains, api.mcmc_energy, tables, lab0, S, N, 0.5, 30, 9, 1, K, passes)
    assert len(recs) == passes * S and any(r[2] for r in recs)
    energy = lit.group_energy(PT, tc, pairs, triplets, lab0)
    scale = np.sum(np.abs(PT[:, 0, 0])) + np.sum(np.abs(tc[:, 0, 0, 0]))
    for e0, kept, take, best in recs:
        assert kept <= e0 and (kept < e0) == take and 0 <= best < K
    # the change of the group energy over the pass is the sum of the accepted blocks' changes
    assert abs((lit.group_energy(PT, tc, pairs, triplets, lab) - energy) - sum(r[1] - r[0] for r in recs)) <= 1e-11 * scale
    assert lit.group_energy(PT, tc, pairs, triplets, lab) <= energy
    # no sweeps: nothing is accepted, nothing changes
    lab2, recs2 = lit.run_pass(chains, api.mcmc_energy, tables, lab, S, N, 0.5, 0, 9, 1, K, 1)
    assert np.array_equal(lab2, lab) and not any(r[2] for r in recs2)


def test_host_pieces_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/group_mcmc_host_check.cpp: the incidence, the seed rule and the acceptance rule without HIP -- a program of its own, run directly"""
    exe = str(tmp_path / "group_mcmc_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpp", "group_mcmc_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def groupwise_command(tool, tmp_path, dopt):
    import __graft_entry__ as g

    (tmp_path / "meshes.txt").write_text("none-0.surf.gii\nnone-1.surf.gii\n")
    (tmp_path / "data.txt").write_text("none-0.func.gii\nnone-1.func.gii\n")
    (tmp_path / "conf").write_text("--opt=DISCRETE\n--simval=2\n--it=2\n--lambda=0.1\n--datagrid=3\n--CPgrid=1\n--SGgrid=3\n--sigma_in=0\n--sigma_ref=0\n--dopt=%s\n" % dopt)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_files.py")] if tool == "py" else [g.build_cpp_newmsm()]
    return cmd + ["--groupwise", "--meshes=" + str(tmp_path / "meshes.txt"), "--data=" + str(tmp_path / "data.txt"), "--template=none.surf.gii",
                  "--conf=" + str(tmp_path / "conf"), "--out=" + str(tmp_path) + "/"]


def run_tool(cmd, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MSMHIP_GROUP_MCMC") and k not in ("MSMHIP_MCMC_CHAINS", "MSMHIP_MCMC_DRAW")}
    return subprocess.run(cmd, cwd=ROOT, env=dict(clean, **env), capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("tool", ["py", "cpp"])
def test_the_executables_refuse_groupwise_mcmc_without_the_variable(built, tool, tmp_path):
    """as before: the reference's message (M/group_mesh_registration.cpp:87) and exit status 1; FastPD gets it with the variable too"""
    for dopt, env in (("MCMC", {}), ("FastPD", {}), ("FastPD", dict(MSMHIP_GROUP_MCMC="on"))):
        run = run_tool(groupwise_command(tool, tmp_path, dopt), **env)
        assert run.returncode == 1 and "Groupwise mode is only supported in the HOCR version of MSM." in run.stderr, run.stdout + run.stderr


@pytest.mark.parametrize("tool", ["py", "cpp"])
def test_the_executables_refuse_bad_settings_of_groupwise_mcmc(built, tool, tmp_path):
    cmd = groupwise_command(tool, tmp_path, "MCMC")
    for value in ("off", "1", "ON", ""):
        run = run_tool(cmd, MSMHIP_GROUP_MCMC=value)
        assert run.returncode == 1 and "MSMHIP_GROUP_MCMC=%s: the groupwise Monte Carlo optimiser is switched on with MSMHIP_GROUP_MCMC=on" % value in run.stderr, run.stderr
    for value in ("0", "65", "two", ""):
        run = run_tool(cmd, MSMHIP_GROUP_MCMC="on", MSMHIP_GROUP_MCMC_PASSES=value)
        assert run.returncode == 1 and "MSMHIP_GROUP_MCMC_PASSES=%s: the number of passes over the subjects must be a whole number from 1 to 64" % value in run.stderr, run.stderr
    run = run_tool(cmd, MSMHIP_GROUP_MCMC="on", MSMHIP_MCMC_CHAINS="257")
    assert run.returncode == 1 and "MSMHIP_MCMC_CHAINS=257: the number of Monte Carlo chains must be a whole number from 1 to 256" in run.stderr, run.stderr
    run = run_tool(cmd, MSMHIP_GROUP_MCMC="on", MSMHIP_MCMC_DRAW="device")
    assert run.returncode == 1 and "MSMHIP_MCMC_DRAW=device: the proposals are drawn on the host (host, or unset) or on the device (gpu)" in run.stderr, run.stderr
