"""Shared by test_mplp_cpu.py and test_gpu_mplp.py: a numpy restatement of the MPLP definition, written here from the definition and
not from the library's code, the cases both files run, brute force over small graphs, and the tolerance of the issue.

Every floating-point operation below is one IEEE double operation in the order the definition gives: additions of whole label vectors element by
element, exact minima, one division and one subtraction per message, Python-float sums one term at a time."""
import functools
import itertools

import numpy as np

import newmsm_amd as M
from newmsm_amd import api


def incidence(triplets, N):
    """per node the list of its (t, s) slots, ascending"""
    inc = [[] for _ in range(N)]
    for t, tri in enumerate(np.asarray(triplets).reshape(-1, 3)):
        for s in range(3):
            inc[int(tri[s])].append((t, s))
    return inc


def node_sum(U, m, inc, i, skip=None):
    d = np.array(U[:, i], dtype=np.float64)
    for (t, s) in inc[i]:
        if (t, s) != skip:
            d = d + m[t, s]
    return d


def energy(U, tc, triplets, lab):
    u = 0.0
    for i in range(U.shape[1]):
        u += float(U[lab[i], i])
    t3 = 0.0
    for t, (a, b, c) in enumerate(np.asarray(triplets).reshape(-1, 3)):
        t3 += float(tc[t, lab[a], lab[b], lab[c]])
    return u + 0.0 + t3


def bound(U, tc, triplets, m, inc):
    D = 0.0
    for i in range(U.shape[1]):
        D += float(node_sum(U, m, inc, i).min())
    for t in range(len(tc)):
        D += float((((tc[t] - m[t, 0][:, None, None]) - m[t, 1][None, :, None]) - m[t, 2][None, None, :]).min())
    return D


def decode(U, m, inc):
    return np.array([int(np.argmin(node_sum(U, m, inc, i))) for i in range(U.shape[1])], dtype=np.int32)  # argmin: the first of equal minima


def sweep(U, tc, triplets, m, inc):
    for t, (A, B, C) in enumerate(np.asarray(triplets).reshape(-1, 3)):
        d = [node_sum(U, m, inc, int(n), skip=(t, s)) for s, n in enumerate((A, B, C))]
        v = ((tc[t] + d[0][:, None, None]) + d[1][None, :, None]) + d[2][None, None, :]
        mins = (v.min(axis=(1, 2)), v.min(axis=(0, 2)), v.min(axis=(0, 1)))
        for s in range(3):
            m[t, s] = (mins[s] + 0.0) / 3.0 - d[s]  # + 0.0: a zero minimum is +0.0 whatever the order it was found in


def mplp(U, tc, triplets, start, sweeps):
    """the definition: MplpResult with bounds and messages"""
    U, tc = np.asarray(U, dtype=np.float64), np.asarray(tc, dtype=np.float64)
    triplets = np.asarray(triplets, dtype=np.int32).reshape(-1, 3)
    L, N = U.shape
    T = len(triplets)
    inc = incidence(triplets, N)
    m = np.zeros((T, 3, L))
    best_lab, best_e = np.array(start, dtype=np.int32), energy(U, tc, triplets, start)
    energies, bounds = np.full(sweeps, np.nan), np.full(sweeps, np.nan)
    run = 0
    for k in range(sweeps if T else 0):
        before = m.copy()
        sweep(U, tc, triplets, m, inc)
        run = k + 1
        lab = decode(U, m, inc)
        energies[k] = energy(U, tc, triplets, lab)
        bounds[k] = bound(U, tc, triplets, m, inc)
        if energies[k] < best_e:
            best_lab, best_e = lab, energies[k]
        if before.tobytes() == m.tobytes():
            break
    if run:
        energies[run:], bounds[run:] = energies[run - 1], bounds[run - 1]
    return api.MplpResult(best_lab, run, best_e, bounds[run - 1] if run else bound(U, tc, triplets, m, inc), energies, bounds, m)


def same(got, want, what=""):
    """two MplpResults, bit for bit (what one side did not ask for is not compared)"""
    assert got.labeling.dtype == np.int32 and np.array_equal(got.labeling, want.labeling), what
    assert got.sweeps_run == want.sweeps_run, (what, got.sweeps_run, want.sweeps_run)
    for name in ("energy", "bound", "energies", "bounds", "messages"):
        a, b = getattr(got, name), getattr(want, name)
        if a is None or b is None:
            continue
        a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, a.ravel()[:4], b.ravel()[:4])


def tol(U, tc, triplets):
    """64 (N + T) 2^-52 max(1, max|unary|, max|tcosts|): a few ulps of the largest magnitude per summed term"""
    big = max(1.0, float(np.abs(U).max()), float(np.abs(tc).max()) if np.size(tc) else 0.0)
    return 64.0 * (U.shape[1] + len(triplets)) * 2.0 ** -52 * big


def brute_force(U, tc, triplets):
    """the lowest energy over all L^N labellings (small graphs only)"""
    L, N = U.shape
    return min(energy(U, tc, triplets, lab) for lab in itertools.product(range(L), repeat=N))


@functools.lru_cache(maxsize=None)
def faces(order):
    xyz, tri = M.make_mesh_from_icosa(order)
    return len(xyz), np.ascontiguousarray(api.estimate_triplets(tri), dtype=np.int32)


def smooth_tables(N, triplets, L, seed, big=0.0, integer=False):
    """a uniform random unary table and a smooth triplet cost (the squared differences of the three labels, scaled per triplet), as in the issue's
    prototype; big: that share of the entries of both tables set to 1e7; integer: small whole numbers instead, with exact ties (L >= 3)"""
    rng = np.random.default_rng(seed)
    T = len(triplets)
    x = np.arange(L, dtype=np.float64)
    a, b, c = x[:, None, None], x[None, :, None], x[None, None, :]
    if integer:
        # labels 1 and 2 cost the same at every node and the triplet cost counts unequal label pairs, which no renaming of labels changes: the beliefs
        # of labels 1 and 2 are equal bit for bit at every node and after every sweep
        U = 1.0 * rng.integers(0, 3, (L, N))
        U[2] = U[1]
        tc = np.stack([(1.0 * (a != b) + 1.0 * (b != c) + 1.0 * (a != c)) * float(w) for w in rng.integers(0, 2, T)]) if T else np.zeros((0, L, L, L))
    else:
        U = rng.uniform(0.0, 1.0, (L, N))
        tc = np.stack([((a - b) ** 2 + (b - c) ** 2 + (a - c) ** 2) * w for w in rng.uniform(0.0, 0.02, T)]) if T else np.zeros((0, L, L, L))
    tc = np.array(np.broadcast_to(tc, (T, L, L, L)), dtype=np.float64)
    if big:
        U[rng.random(U.shape) < big] = 1e7
        tc[rng.random(tc.shape) < big] = 1e7
    start = rng.integers(0, L, N).astype(np.int32)
    return U, tc, start


@functools.lru_cache(maxsize=None)
def ico_case(order, L, seed=11, big=0.0, integer=False, shuffled=False):
    """(U, tc, triplets, start) on the faces of an icosphere, the triplet list in a seeded random order when shuffled; never written"""
    N, triplets = faces(order)
    if shuffled:
        triplets = np.ascontiguousarray(triplets[np.random.default_rng(seed + 1).permutation(len(triplets))])
    U, tc, start = smooth_tables(N, triplets, L, seed, big=big, integer=integer)
    for arr in (U, tc, triplets, start):
        arr.setflags(write=False)
    return U, tc, triplets, start


def fan_case(L=4, seed=5):
    """twelve triangles round hub 0 (rim 1 .. 12, closed), and node 13 in no triplet"""
    triplets = np.array([[0, 1 + k, 1 + (k + 1) % 12] for k in range(12)], dtype=np.int32)
    U, tc, start = smooth_tables(14, triplets, L, seed)
    return U, tc, triplets, start


OCTAHEDRON = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)


def non_finite_refusals():
    """((U, tc, triplets, start), the message) of the plain reading's refusals over tables with a non-finite entry, on the T = 20 / L = 5 case: every
    class of triplet entry is named as the triplet table's non-finite value (-inf too: "holds -infinity" is the forbidden-entry reading's text), an
    infinite unary entry as the unary table's, and the unary table is named first where both tables hold one"""
    U, tc, triplets, start = (np.array(a) for a in ico_case(0, 5, 31))
    unary, triplet = "MSM_ERR_INVALID.*the unary table holds a non-finite value.*--fixnan", "MSM_ERR_INVALID.*the triplet table holds a non-finite value.*--fixnan"
    minus_t, plus_t, nan_t, minus_u, nan_u = np.array(tc), np.array(tc), np.array(tc), np.array(U), np.array(U)
    minus_t[7, 0, 3, 1] = -np.inf
    plus_t[19, 4, 4, 4] = np.inf
    nan_t[0, 0, 0, 0] = np.nan
    minus_u[4, 11] = -np.inf
    nan_u[2, 3] = np.nan
    return [((U, minus_t, triplets, start), triplet), ((U, plus_t, triplets, start), triplet), ((U, nan_t, triplets, start), triplet),
            ((minus_u, tc, triplets, start), unary), ((nan_u, plus_t, triplets, start), unary)]


def last_entry_forbidden():
    """the T = 20 / L = 5 case whose only non-finite entry is +inf in the last element of the last triplet: the forbidden-entry reading counts
    (0, 0, 1, 0), the last thing a pass over the table reads"""
    U, tc, triplets, start = (np.array(a) for a in ico_case(0, 5, 31))
    tc[-1, -1, -1, -1] = np.inf
    return U, tc, triplets, start
