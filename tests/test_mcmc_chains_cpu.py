"""Several Monte Carlo optimiser chains from one start, the host half (newmsm_amd/csrc/mcmc.cpp, mcmc_host.hpp; DESIGN.md 5.16 "Chains"): the energy of a
labelling over the two tables, the choice of the best chain, msm_mcmc_optimise_chains against K runs of the optimiser, the level loops' seed rule, and the
threaded drawing of K proposal streams as a program of its own under the sanitizers.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, registration

import mcmc_chain_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("order,L", [(0, 19), (2, 19), (1, 1)])
def test_energy_is_the_plain_serial_sum(order, L):
    U, tc, triplets, _ = cases.tables(order, L)
    rng = np.random.default_rng(order)
    for _ in range(3):
        lab = rng.integers(0, L, U.shape[1]).astype(np.int32)
        assert api.mcmc_energy(U, tc, triplets, lab) == cases.serial_energy(U, tc, triplets, lab)
    # no triplets: the unary sum alone
    lab = rng.integers(0, L, U.shape[1]).astype(np.int32)
    none = np.zeros((0, 3), dtype=np.int32)
    assert api.mcmc_energy(U, np.zeros((0, L, L, L)), none, lab) == cases.serial_energy(U, tc[:0], none, lab)


def test_energy_keeps_the_order_of_the_sums():
    """1e16 + 1 + 1 - 1e16 is 0 summed from the left (numpy's pairwise sum of the same values is not)"""
    U = np.array([[1e16, 1.0, 1.0, -1e16]])
    tc = np.array([1e16, 1.0, 1.0, -1e16]).reshape(4, 1, 1, 1)
    triplets = np.array([[0, 1, 2], [1, 2, 3], [0, 0, 0], [3, 2, 1]], dtype=np.int32)
    assert api.mcmc_energy(U, tc, triplets, np.zeros(4, dtype=np.int32)) == 0.0 + 0.0 + 0.0
    assert api.mcmc_energy(U[:, :3], tc[1:], triplets[:3] % 3, np.zeros(3, dtype=np.int32)) == 1e16 + 0.0 + (2.0 - 1e16)


def test_energy_refuses_what_the_optimiser_refuses():
    U, tc, triplets, start = cases.tables(0)
    bad = np.array(start)
    bad[7] = cases.LABELS
    with pytest.raises(M.MsmError, match="label of node 7 out of range"):
        api.mcmc_energy(U, tc, triplets, bad)
    bad_t = np.array(triplets)
    bad_t[3, 1] = U.shape[1]
    with pytest.raises(M.MsmError, match="triplet node out of range"):
        api.mcmc_energy(U, tc, bad_t, start)


def test_best_follows_min_elements_rule():
    nan, inf = float("nan"), float("inf")
    assert api.mcmc_best([4.0]) == 0                         # K = 1
    assert api.mcmc_best([3.0, 1.0, 2.0, 1.0, 1.0]) == 1     # ties go to the lower index
    assert api.mcmc_best([7.5, 7.5]) == 0
    assert api.mcmc_best([nan, -5.0, 1.0]) == 0              # nothing beats a NaN in slot 0
    assert api.mcmc_best([2.0, nan, 1.0, nan]) == 2          # a NaN never beats anything
    assert api.mcmc_best([inf, -inf, -inf]) == 1
    rng = np.random.default_rng(4)
    for _ in range(20):
        E = rng.integers(0, 4, 9).astype(float)
        E[rng.integers(0, 9)] = nan
        assert api.mcmc_best(E) == cases.best_rule(E)
    with pytest.raises(M.MsmError, match="msm_mcmc_best"):
        api.mcmc_best(np.zeros(0))


@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("K", [1, 2, 5, 17])
def test_host_chains_are_k_runs_of_the_optimiser(order, K):
    """50 sweeps, 19 labels; the seeds are the GPU test's: all energies distinct and, from two chains on, a chain other than 0 wins"""
    U, tc, triplets, start = cases.tables(order)
    seeds, labs, E, best = cases.icosphere_chains(order, K)
    assert len(set(E.tolist())) == K and (best != 0) == (K > 1)
    cases.check_chains(api.mcmc_optimise_chains(U, tc, triplets, start, seeds, mcparam=cases.MCPARAM, iters=cases.SWEEPS), labs, E, best)


def test_host_chains_do_not_depend_on_the_host_threads(monkeypatch):
    U, tc, triplets, start = cases.tables(0)
    seeds, labs, E, best = cases.icosphere_chains(0, 17)
    for threads in ("1", "3", "16"):
        monkeypatch.setenv("MSMHIP_HOST_THREADS", threads)
        cases.check_chains(api.mcmc_optimise_chains(U, tc, triplets, start, seeds, mcparam=cases.MCPARAM, iters=cases.SWEEPS), labs, E, best)


def test_host_chains_equal_seeds_no_sweeps_and_refusals():
    U, tc, triplets, start = cases.tables(0)
    kw = dict(mcparam=cases.MCPARAM, iters=cases.SWEEPS)
    lab, labs, E, best = api.mcmc_optimise_chains(U, tc, triplets, start, [9, 9, 4], **kw)
    assert np.array_equal(labs[0], labs[1]) and E[0] == E[1]
    assert best == cases.best_rule(E) and best != 1  # of two equal chains the lower index
    # no sweeps, no triplets: every chain is the start
    e0 = cases.serial_energy(U, tc, triplets, start)
    lab, labs, E, best = api.mcmc_optimise_chains(U, tc, triplets, start, [1, 2, 3], mcparam=0.3, iters=0)
    assert best == 0 and np.array_equal(lab, start) and np.array_equal(labs, np.tile(start, (3, 1))) and np.array_equal(E, [e0] * 3)
    none = np.zeros((0, 3), dtype=np.int32)
    lab, labs, E, best = api.mcmc_optimise_chains(U, tc[:0], none, start, [1, 2], mcparam=0.3, iters=5)
    assert best == 0 and np.array_equal(labs, np.tile(start, (2, 1))) and np.array_equal(E, [cases.serial_energy(U, tc[:0], none, start)] * 2)
    for seeds in ([], list(range(257)), None):
        with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*msm_mcmc_optimise_chains"):
            api.mcmc_optimise_chains(U, tc, triplets, start, seeds, **kw)
    bad = np.array(start)
    bad[7] = cases.LABELS
    with pytest.raises(M.MsmError, match="msm_mcmc_optimise: label of node 7 out of range"):
        api.mcmc_optimise_chains(U, tc, triplets, bad, [1, 2], **kw)
    with pytest.raises(M.MsmError, match=r"the geometric distribution parameter must be in \(0, 1\]"):
        api.mcmc_optimise_chains(U, tc, triplets, start, [1, 2], mcparam=0.0, iters=3)
    assert len(api.mcmc_optimise_chains(U, tc, triplets, start, list(range(256)), mcparam=0.3, iters=1)[2]) == 256


def test_seed_rule_of_the_level_loops():
    """chain k of iteration it: seed + it + 1000003 k -- chain 0 is the single run's seed, and the 32 bits the engine keeps stay distinct for k < 256"""
    assert api.chain_seeds(5, 0, 1) == [5] and api.chain_seeds(5, 3, 3) == [8, 8 + 1000003, 8 + 2000006]
    for seed in (0, 5, 2 ** 32 - 1, 2 ** 63):
        low = {s & 0xFFFFFFFF for it in range(4) for s in api.chain_seeds(seed, it, 256)[:1]}
        assert len(low) == 4
        for it in (0, 49):
            s = api.chain_seeds(seed, it, 256)
            assert s[0] == (seed + it) % 2 ** 64 and len({v & 0xFFFFFFFF for v in s}) == 256 and all(0 <= v < 2 ** 64 for v in s)
    # seeds that agree in their low 32 bits are one chain to the engine
    U, tc, triplets, start = cases.tables(0)
    a = api.mcmc_optimise(U, tc, triplets, start, mcparam=0.3, iters=5, seed=7)
    assert np.array_equal(api.mcmc_optimise(U, tc, triplets, start, mcparam=0.3, iters=5, seed=7 + 2 ** 32), a)


class _RecordingOps:
    """what the MCMC branch of run_discrete_level hands to the optimiser: ProductOps' methods over recorded arguments (no context is made)"""

    def __init__(self):
        self.single, self.chains = [], []

    def mcmc(self, unary, tcosts, triplets, labeling, mcparam, iters, seed):
        self.single.append(seed)
        return registration.ProductOps.mcmc(self, unary, tcosts, triplets, labeling, mcparam, iters, seed)

    def mcmc_chains(self, unary, tcosts, triplets, labeling, mcparam, iters, seeds):
        self.chains.append(list(seeds))
        return registration.ProductOps.mcmc_chains(self, unary, tcosts, triplets, labeling, mcparam, iters, seeds)


def test_the_level_loops_host_branch_keeps_the_best_chain():
    """ProductOps.mcmc_chains is msm_mcmc_optimise_chains over the fetched tables: the labelling of the chain with the lowest energy"""
    U, tc, triplets, start = cases.tables(2)
    seeds, labs, E, best = cases.icosphere_chains(2, 5)
    ops = _RecordingOps()
    got = ops.mcmc_chains(U, tc, triplets, start, cases.MCPARAM, cases.SWEEPS, seeds)
    assert np.array_equal(got, labs[best]) and not np.array_equal(got, labs[0]) and ops.chains == [seeds]
    assert np.array_equal(ops.mcmc(U, tc, triplets, start, cases.MCPARAM, cases.SWEEPS, seeds[0]), labs[0])
    import inspect
    assert inspect.signature(registration.run_discrete_level).parameters["mcmc_chains"].default == 1


@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], ["-fsanitize=thread"]],
                         ids=["address_undefined", "thread"])
def test_host_pieces_alone_under_the_sanitizers(tmp_path, flags):
    """tests/cpp/mcmc_chains_host_check.cpp: K = 1, 5, 17 streams drawn on 1, 4, 16 threads in chunks of 1, 3 and the whole run into the kernel's layout
    against McmcProposals drawn serially, the chunk length, the energy, the selection -- a program of its own, run directly"""
    exe = str(tmp_path / "mcmc_chains_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "mcmc_chains_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


@pytest.mark.parametrize("tool", ["py", "cpp"])
def test_the_executables_refuse_a_chain_count_outside_1_to_256(tool, tmp_path):
    import __graft_entry__ as g

    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_files.py")] if tool == "py" else [g.build_cpp_newmsm()]
    cmd += ["--inmesh=none.surf.gii", "--indata=none.func.gii", "--refdata=none.func.gii", "--out=" + str(tmp_path) + "/"]
    for value in ("0", "257", "three", ""):
        run = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, MSMHIP_MCMC_CHAINS=value), capture_output=True, text=True, timeout=120)
        assert run.returncode == 1 and "MSMHIP_MCMC_CHAINS" in run.stderr and "1 to 256" in run.stderr, (value, run.stdout, run.stderr)
