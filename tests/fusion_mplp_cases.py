"""Shared by test_fusion_mplp_cpu.py and test_gpu_fusion_mplp.py: seeded numpy tables of one label step's binary problem (unary2 N x 2, octets T x 8 over
the faces of an icosphere), the composition msm_fusion_mplp_step is defined as (api.mplp_optimise, then api.mplp_round mode 0, at L = 2
on the transposed unary), and the comparison of two results bit for bit."""
import functools
import itertools

import numpy as np

from newmsm_amd import api

import mplp_literal as ML


@functools.lru_cache(maxsize=None)
def case(order, kind="smooth", seed=3, shuffled=False, lone_node=False):
    """(unary2, octets, triplets) on the faces of the icosphere of that order; never written.
    smooth: uniform unary costs and, per triplet, a random weight times the number of unequal label pairs (an attractive step: it settles early);
    rough: uniform unary costs in [0, 1) against octets drawn from [-2, 2) entry by entry (frustrated: no fixed point within a dozen sweeps);
    settled: no unary costs under the smooth octets -- x = 0 is optimal and the first sweep leaves the messages at a fixed point (bitwise fixed points
    are rare otherwise: the last bits of the messages keep oscillating).
    shuffled: the triplet list in a seeded random order (another level count); lone_node: one more node, in no triplet."""
    N, triplets = ML.faces(order)
    rng = np.random.default_rng(1000 * order + seed)
    if shuffled:
        triplets = np.ascontiguousarray(triplets[rng.permutation(len(triplets))])
    N += int(lone_node)
    T = len(triplets)
    unary2 = rng.uniform(0.0, 1.0, (N, 2)) * (kind != "settled")
    x = np.arange(2.0)
    a, b, c = x[:, None, None], x[None, :, None], x[None, None, :]
    if kind == "rough":
        octets = rng.uniform(-2.0, 2.0, (T, 8))
    else:
        pairs = ((a != b) * 1.0 + (b != c) * 1.0 + (a != c) * 1.0).reshape(1, 8)
        octets = pairs * rng.uniform(0.0, 0.4, (T, 1))
    octets = np.ascontiguousarray(octets, dtype=np.float64)
    for arr in (unary2, octets, triplets):
        arr.setflags(write=False)
    return unary2, octets, triplets


def tables_at_two_labels(unary2, octets, triplets, N=None):
    """(U 2 x N, tcosts T x 2 x 2 x 2) of DESIGN.md 5.19's layout"""
    T = len(np.asarray(triplets).reshape(-1, 3))
    U = np.zeros((2, N)) if unary2 is None else np.ascontiguousarray(np.asarray(unary2, dtype=np.float64).T)
    return U, np.asarray(octets, dtype=np.float64).reshape(T, 2, 2, 2)


def composition(unary2, octets, triplets, sweeps, polish, N=None):
    """what the step is defined as, through the existing host entry points: api.FusionMplp"""
    U, tc = tables_at_two_labels(unary2, octets, triplets, N)
    N = U.shape[1]
    start = np.zeros(N, dtype=np.int32)
    e0 = ML.energy(U, tc, triplets, start)
    r = api.mplp_optimise(U, tc, triplets, start, sweeps=sweeps, bound=True, bounds=True, messages=True)
    energies = [np.array([e0]), r.energies]
    x, energy, passes = r.labeling, r.energy, 0
    if polish > 0:
        rr = api.mplp_round(U, tc, triplets, r.labeling, messages=r.messages, mode=0, polish=polish)
        assert rr.energies[0] == r.energy  # candidate 0 of the rounding is the handed-in winner
        energies.append(rr.energies[1:])
        x, energy, passes = rr.labeling, rr.energy, rr.passes_run
    return api.FusionMplp(x, r.sweeps_run, passes, energy, r.bound, np.concatenate(energies), r.bounds)


def same(got, want, what=""):
    """every output of two FusionMplp results, bit for bit"""
    assert np.array_equal(got.x, want.x), (what, "x")
    assert (got.sweeps_run, got.passes_run) == (want.sweeps_run, want.passes_run), (what, got.sweeps_run, got.passes_run, want.sweeps_run, want.passes_run)
    for name in ("energy", "bound", "energies", "bounds"):
        a, b = (np.atleast_1d(np.asarray(getattr(r, name), dtype=np.float64)) for r in (got, want))
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, a[:4], b[:4])


def energy(unary2, octets, triplets, x):
    U, tc = tables_at_two_labels(unary2, octets, triplets, len(x))
    return ML.energy(U, tc, triplets, x)


def brute_force(unary2, octets, triplets):
    """the lowest energy over all 2^N labellings (ico0: 4 096), vectorised: exact to a few ulps, which the caller's slack covers"""
    N = len(unary2)
    X = np.array(list(itertools.product(range(2), repeat=N)), dtype=np.int64)
    E = unary2[np.arange(N)[None, :], X].sum(axis=1)
    for t, (a, b, c) in enumerate(np.asarray(triplets).reshape(-1, 3)):
        E = E + octets[t][4 * X[:, a] + 2 * X[:, b] + X[:, c]]
    return float(E.min())


def slack(unary2, octets, triplets):
    """DESIGN.md 5.19's own: 64 (N + T) 2^-52 max(1, max |theta|)"""
    big = max(1.0, float(np.abs(unary2).max()), float(np.abs(octets).max()) if np.size(octets) else 0.0)
    return 64.0 * (len(unary2) + len(triplets)) * 2.0 ** -52 * big
