"""Shared by test_mcmc_chains_cpu.py and test_gpu_mcmc_chains.py: random cost tables on icosphere faces, the host optimiser's chains over them (computed
once, never written), the energy as a plain serial sum and the selection rule in plain Python."""
import functools

import numpy as np

import newmsm_amd as M
from newmsm_amd import api

MCPARAM, SWEEPS, LABELS = 0.3, 50, 19
# base seeds (chain k takes api.chain_seeds(base, 0, K)[k]) for which the host optimiser alone gives, over the tables below, seventeen distinct energies with
# chain 1 below chain 0 -- so best != 0 for every K >= 2: best is 1, 3, 9 at ico0 and 1, 2, 11 at ico2 for K = 2, 5, 17 (found by trying 1, 2, 3, ... on the
# host; test_mcmc_chains_cpu.py asserts the properties)
BASE_SEED = {0: 1, 2: 6}


@functools.lru_cache(maxsize=None)
def faces(order):
    xyz, tri = M.make_mesh_from_icosa(order)
    return len(xyz), np.ascontiguousarray(api.estimate_triplets(tri), dtype=np.int32)


@functools.lru_cache(maxsize=None)
def tables(order, L=LABELS, rng_seed=None):
    """(U, tc, triplets, start): random tables over the faces of an icosphere, the start labelling all zero"""
    N, triplets = faces(order)
    rng = np.random.default_rng(100 + order if rng_seed is None else rng_seed)
    U, tc = rng.normal(size=(L, N)), rng.normal(size=(len(triplets), L, L, L))
    start = np.zeros(N, dtype=np.int32)
    for a in (U, tc, triplets, start):
        a.setflags(write=False)
    return U, tc, triplets, start


def serial_energy(U, tc, triplets, lab):
    """(sum over i ascending from 0.0 of U[lab[i], i]) + 0.0 + (sum over t ascending from 0.0 of tc[t, la, lb, lc]) in Python floats, one addition at a time"""
    U, tc = np.asarray(U), np.asarray(tc)
    triplets = np.asarray(triplets).reshape(-1, 3)
    u = 0.0
    for i in range(U.shape[1]):
        u += float(U[lab[i], i])
    t3 = 0.0
    for t, (a, b, c) in enumerate(triplets):
        t3 += float(tc[t, lab[a], lab[b], lab[c]])
    return u + 0.0 + t3


def best_rule(energies):
    """std::min_element: the first index no later energy is strictly smaller than"""
    best = 0
    for k in range(1, len(energies)):
        if energies[k] < energies[best]:
            best = k
    return best


def host_chains(U, tc, triplets, start, seeds, mcparam, iters):
    """K runs of api.mcmc_optimise, their serial energies and the rule's choice: (labelings K x N, energies K, best)"""
    labs = np.stack([api.mcmc_optimise(U, tc, triplets, start, mcparam=mcparam, iters=iters, seed=int(s)) for s in seeds])
    E = np.array([serial_energy(U, tc, triplets, lab) for lab in labs])
    return labs, E, best_rule(E)


@functools.lru_cache(maxsize=None)
def icosphere_chains(order, K):
    """the host reference of the ico0 / ico2 cases: (seeds, labelings, energies, best) for K chains of 50 sweeps over tables(order)"""
    U, tc, triplets, start = tables(order)
    seeds = api.chain_seeds(BASE_SEED[order], 0, K)
    labs, E, best = host_chains(U, tc, triplets, start, seeds, MCPARAM, SWEEPS)
    labs.setflags(write=False)
    E.setflags(write=False)
    return seeds, labs, E, best


def check_chains(got, labs, E, best):
    """a chains call's (labeling, labelings, energies, best) against the host reference, exactly"""
    lab, got_labs, got_E, got_best = got
    assert got_labs.dtype == np.int32 and np.array_equal(got_labs, labs)
    assert np.array_equal(got_E, E, equal_nan=True), (got_E, E)
    assert got_best == best and np.array_equal(lab, labs[best])
