"""Shared by test_mplp_pairs_cpu.py and test_gpu_mplp_pairs.py: a numpy restatement of MPLP over the pair tables, written here from
the definition and not from the library's code, the cases both files run, brute force over small graphs, and the tolerance of the issue.

Tables: U[x, i] = theta_i(x); pc[p, b, a] = theta_p(a, b), pair p on A = pairs[p, 0] (label a, slot 0) and B = pairs[p, 1] (label b, slot 1).  Every
floating-point operation below is one IEEE double operation in the order the definition gives: additions of whole label vectors element by element,
exact minima, one division and one subtraction per message, Python-float sums one term at a time."""
import functools
import itertools

import numpy as np

import newmsm_amd as M
from newmsm_amd import api


def incidence(pairs, N):
    """per node the list of its (p, s) slots, ascending"""
    inc = [[] for _ in range(N)]
    for p, pr in enumerate(np.asarray(pairs).reshape(-1, 2)):
        for s in range(2):
            inc[int(pr[s])].append((p, s))
    return inc


def pair_colouring(pairs):
    """(colour per pair, the sweep's order): pairs ascending, each the smallest colour no lower pair sharing a node holds"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    colour = []
    for p, (A, B) in enumerate(pairs):
        held = {colour[q] for q in range(p) if {int(pairs[q, 0]), int(pairs[q, 1])} & {int(A), int(B)}}
        c = 0
        while c in held:
            c += 1
        colour.append(c)
    order = sorted(range(len(pairs)), key=lambda p: (colour[p], p))
    return np.array(colour, dtype=np.int32), order


def node_colouring(pairs, N):
    """(colour per node, the polish's order): nodes ascending, each the smallest colour no lower node sharing a pair holds"""
    nb = [set() for _ in range(N)]
    for A, B in np.asarray(pairs).reshape(-1, 2):
        nb[int(A)].add(int(B))
        nb[int(B)].add(int(A))
    colour = []
    for i in range(N):
        held = {colour[j] for j in nb[i] if j < i}
        c = 0
        while c in held:
            c += 1
        colour.append(c)
    order = sorted(range(N), key=lambda i: (colour[i], i))
    return np.array(colour, dtype=np.int32), order


def node_sum(U, m, inc, i, skip=None):
    d = np.array(U[:, i], dtype=np.float64)
    for (p, s) in inc[i]:
        if (p, s) != skip:
            d = d + m[p, s]
    return d


def energy(U, pc, pairs, lab):
    u = 0.0
    for i in range(U.shape[1]):
        u += float(U[lab[i], i])
    e2 = 0.0
    for p, (A, B) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        e2 += float(pc[p, lab[B], lab[A]])
    return u + 0.0 + e2


def bound(U, pc, m, inc):
    D = 0.0
    for i in range(U.shape[1]):
        D += float(node_sum(U, m, inc, i).min())
    for p in range(len(pc)):
        D += float(((pc[p] - m[p, 0][None, :]) - m[p, 1][:, None]).min())
    return D


def decode(U, m, inc):
    return np.array([int(np.argmin(node_sum(U, m, inc, i))) for i in range(U.shape[1])], dtype=np.int32)  # argmin: the first of equal minima


def sweep(U, pc, pairs, m, inc, order):
    for p in order:
        A, B = int(pairs[p, 0]), int(pairs[p, 1])
        d0, d1 = node_sum(U, m, inc, A, skip=(p, 0)), node_sum(U, m, inc, B, skip=(p, 1))
        v = (pc[p] + d0[None, :]) + d1[:, None]  # v[b, a]
        m[p, 0] = (v.min(axis=0) + 0.0) / 2.0 - d0  # + 0.0: a zero minimum is +0.0 whatever the order it was found in
        m[p, 1] = (v.min(axis=1) + 0.0) / 2.0 - d1


def _tables(U, pc, pairs):
    U = np.asarray(U, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    L = U.shape[0]
    return U, np.asarray(pc, dtype=np.float64).reshape(len(pairs), L, L), pairs


def mplp(U, pc, pairs, start, sweeps):
    """the definition: MplpResult with bounds and messages"""
    U, pc, pairs = _tables(U, pc, pairs)
    L, N = U.shape
    P = len(pairs)
    inc = incidence(pairs, N)
    _, order = pair_colouring(pairs)
    m = np.zeros((P, 2, L))
    best_lab, best_e = np.array(start, dtype=np.int32), energy(U, pc, pairs, start)
    energies, bounds = np.full(sweeps, np.nan), np.full(sweeps, np.nan)
    run = 0
    for k in range(sweeps if P else 0):
        before = m.copy()
        sweep(U, pc, pairs, m, inc, order)
        run = k + 1
        lab = decode(U, m, inc)
        energies[k] = energy(U, pc, pairs, lab)
        bounds[k] = bound(U, pc, m, inc)
        if energies[k] < best_e:
            best_lab, best_e = lab, energies[k]
        if before.tobytes() == m.tobytes():
            break
    if run:
        energies[run:], bounds[run:] = energies[run - 1], bounds[run - 1]
    return api.MplpResult(best_lab, run, best_e, bounds[run - 1] if run else bound(U, pc, m, inc), energies, bounds, m)


def polish(U, pc, pairs, start, passes):
    """the definition's polish: MplpRound with 1 + passes energies"""
    U, pc, pairs = _tables(U, pc, pairs)
    L, N = U.shape
    inc = incidence(pairs, N)
    _, order = node_colouring(pairs, N)
    lab = np.array(start, dtype=np.int32)
    best_lab, best_e = lab.copy(), energy(U, pc, pairs, lab)
    energies = np.full(1 + passes, np.nan)
    energies[0] = best_e
    run = 0
    for k in range(passes):
        changed = False
        for i in order:
            s = np.array(U[:, i], dtype=np.float64)
            for (p, slot) in inc[i]:
                s = s + (pc[p, lab[pairs[p, 1]], :] if slot == 0 else pc[p, :, lab[pairs[p, 0]]])
            x = int(np.argmin(s))
            if s[x] < s[lab[i]]:
                lab[i] = x
                changed = True
        run = k + 1
        energies[run] = energy(U, pc, pairs, lab)
        if energies[run] < best_e:
            best_lab, best_e = lab.copy(), energies[run]
        if not changed:
            break
    energies[run + 1:] = energies[run]
    return api.MplpRound(best_lab, run, best_e, energies)


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


def same_round(got, want, what=""):
    """two MplpRounds, bit for bit"""
    assert got.labeling.dtype == np.int32 and np.array_equal(got.labeling, want.labeling), what
    assert got.passes_run == want.passes_run, (what, got.passes_run, want.passes_run)
    assert np.float64(got.energy).tobytes() == np.float64(want.energy).tobytes(), (what, got.energy, want.energy)
    a, b = np.asarray(got.energies, dtype=np.float64), np.asarray(want.energies, dtype=np.float64)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, a, b)


def tol(U, pc, pairs):
    """64 (N + P) 2^-52 max(1, max|unary|, max|paircosts|): mplp_literal.tol with P in T's place"""
    big = max(1.0, float(np.abs(U).max()), float(np.abs(pc).max()) if np.size(pc) else 0.0)
    return 64.0 * (U.shape[1] + len(np.asarray(pairs).reshape(-1, 2))) * 2.0 ** -52 * big


def brute_force(U, pc, pairs):
    """the lowest energy over all L^N labellings (small graphs only)"""
    L, N = U.shape
    return min(energy(U, pc, pairs, lab) for lab in itertools.product(range(L), repeat=N))


@functools.lru_cache(maxsize=None)
def edges(order):
    """(N, the edge list of an icosphere in estimate_pairs order)"""
    xyz, tri = M.make_mesh_from_icosa(order)
    return len(xyz), np.ascontiguousarray(api.estimate_pairs(tri, len(xyz)), dtype=np.int32)


def smooth_tables(N, pairs, L, seed, big=0.0, integer=False):
    """a uniform random unary table and a smooth pair cost (the squared difference of the two labels, weighted per pair), as in the issue's
    prototype; big: that share of the entries of both tables set to 1e7; integer: small whole numbers instead, with exact ties (L >= 3)"""
    rng = np.random.default_rng(seed)
    P = len(pairs)
    x = np.arange(L, dtype=np.float64)
    b, a = x[:, None], x[None, :]
    if integer:
        # labels 1 and 2 cost the same at every node and the pair cost counts unequal labels, which no renaming of labels changes: the beliefs of
        # labels 1 and 2 are equal bit for bit at every node and after every sweep
        U = 1.0 * rng.integers(0, 3, (L, N))
        U[2] = U[1]
        pc = np.stack([1.0 * (a != b) * float(w) for w in rng.integers(0, 2, P)]) if P else np.zeros((0, L, L))
    else:
        U = rng.uniform(0.0, 1.0, (L, N))
        pc = np.stack([(a - b) ** 2 * w for w in rng.uniform(0.0, 0.05, P)]) if P else np.zeros((0, L, L))
    pc = np.array(np.broadcast_to(pc, (P, L, L)), dtype=np.float64)
    if big:
        U[rng.random(U.shape) < big] = 1e7
        pc[rng.random(pc.shape) < big] = 1e7
    start = rng.integers(0, L, N).astype(np.int32)
    return U, pc, start


def _frozen(U, pc, pairs, start):
    for arr in (U, pc, pairs, start):
        arr.setflags(write=False)
    return U, pc, pairs, start


@functools.lru_cache(maxsize=None)
def ico_case(order, L, seed=11, big=0.0, integer=False, shuffled=False):
    """(U, pc, pairs, start) on the edges of an icosphere; shuffled: the list in a seeded random order with a seeded half of the pairs reversed
    (B < A); never written"""
    N, pairs = edges(order)
    if shuffled:
        rng = np.random.default_rng(seed + 1)
        pairs = np.array(pairs[rng.permutation(len(pairs))])
        flip = rng.random(len(pairs)) < 0.5
        pairs[flip] = pairs[flip][:, ::-1]
        pairs = np.ascontiguousarray(pairs)
    U, pc, start = smooth_tables(N, pairs, L, seed, big=big, integer=integer)
    return _frozen(U, pc, pairs, start)


@functools.lru_cache(maxsize=None)
def one_pair(L, seed=3):
    """one pair on nodes (1, 0) -- B below A -- with random tables"""
    rng = np.random.default_rng(seed)
    pairs = np.array([[1, 0]], dtype=np.int32)
    return _frozen(rng.uniform(0.0, 1.0, (L, 2)), rng.uniform(0.0, 1.0, (1, L, L)), pairs, rng.integers(0, L, 2).astype(np.int32))


@functools.lru_cache(maxsize=None)
def star_case(L=5, leaves=40, seed=5):
    """hub 0 with `leaves` leaves, every other pair written leaf-first, and node leaves + 1 in no pair: as many pair classes as leaves, one pair each"""
    pairs = np.array([[0, 1 + k] if k % 2 == 0 else [1 + k, 0] for k in range(leaves)], dtype=np.int32)
    U, pc, start = smooth_tables(leaves + 2, pairs, L, seed)
    return _frozen(U, pc, pairs, start)


@functools.lru_cache(maxsize=None)
def doubled_case(L=4, seed=9):
    """a triangle whose edge (0, 1) is listed twice, once in each direction, with different tables"""
    pairs = np.array([[0, 1], [1, 2], [1, 0], [2, 0]], dtype=np.int32)
    rng = np.random.default_rng(seed)
    return _frozen(rng.uniform(0.0, 1.0, (L, 3)), rng.uniform(0.0, 1.0, (4, L, L)), pairs, rng.integers(0, L, 3).astype(np.int32))


def chain_case(n, L, seed):
    """a chain of n nodes with uniform random tables"""
    pairs = np.array([[k, k + 1] for k in range(n - 1)], dtype=np.int32)
    return random_case(pairs, n, L, seed)


def random_case(pairs, N, L, seed):
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (L, N)), rng.uniform(0.0, 1.0, (len(pairs), L, L)), pairs, rng.integers(0, L, N).astype(np.int32)


TRIANGLE_WITH_TAIL = np.array([[0, 1], [1, 2], [2, 0], [2, 3], [3, 4]], dtype=np.int32)
K4 = np.array([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]], dtype=np.int32)


# (name, (maker, its arguments), sweeps) of the cases both the host and the device are held to; make() builds one (nothing is built at import)
SHARED = [("one pair L=1", (one_pair, (1,)), 4), ("one pair L=2", (one_pair, (2,)), 6), ("one pair L=3", (one_pair, (3,)), 6),
          ("ico0 L=19", (ico_case, (0, 19)), 10), ("ico2 L=7", (ico_case, (2, 7)), 5), ("ico2 L=7 shuffled", (ico_case, (2, 7, 12, 0.0, False, True)), 5),
          ("star of 40", (star_case, ()), 6), ("doubled pair", (doubled_case, ()), 8), ("whole-number ties", (ico_case, (1, 4, 21, 0.0, True)), 6),
          ("ico0 with 1e7", (ico_case, (0, 19, 13, 0.05)), 10)]


def make(spec):
    maker, args = spec
    return maker(*args)


def raw(U, pc, pairs, start, sweeps, ctx=None, N=None, L=None, P=None):
    """msm_mplp_pairs_optimise and msm_mplp_pairs_polish (ctx: their _gpu forms on that context) through ctypes with every output pre-filled, `sweeps`
    read as the passes by the polish; N / L / P override the counts the arrays have.  Returns (the two statuses, whether every output is still what it
    was filled with)."""
    import ctypes as C

    from newmsm_amd._lib import c_dp, c_ip, lib

    U, pc = np.ascontiguousarray(U, dtype=np.float64), np.ascontiguousarray(pc, dtype=np.float64)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    lab = np.array(start, dtype=np.int32)
    run, energy, bound = C.c_int32(-7), C.c_double(-7.0), C.c_double(-7.0)
    energies, bounds, messages = np.full(max(sweeps, 1), -7.0), np.full(max(sweeps, 1), -7.0), np.full((len(pairs), 2, U.shape[0]), -7.0)
    polished = np.full(1 + max(sweeps, 0), -7.0)  # 1 + passes energies
    head = (U.ctypes.data_as(c_dp), pc.ctypes.data_as(c_dp), pairs.ctypes.data_as(c_ip), U.shape[1] if N is None else N, U.shape[0] if L is None else L,
            len(pairs) if P is None else P, sweeps, lab.ctypes.data_as(c_ip), C.byref(run), C.byref(energy))
    tail = (C.byref(bound), energies.ctypes.data_as(c_dp), bounds.ctypes.data_as(c_dp), messages.ctypes.data_as(c_dp))
    if ctx is None:
        st, st2 = lib().msm_mplp_pairs_optimise(*head, *tail), lib().msm_mplp_pairs_polish(*head, polished.ctypes.data_as(c_dp))
    else:
        st, st2 = lib().msm_mplp_pairs_optimise_gpu(ctx.h, *head, *tail), lib().msm_mplp_pairs_polish_gpu(ctx.h, *head, polished.ctypes.data_as(c_dp))
    untouched = (np.array_equal(lab, start) and run.value == -7 and energy.value == -7.0 and bound.value == -7.0 and np.all(energies == -7.0)
                 and np.all(bounds == -7.0) and np.all(messages == -7.0) and np.all(polished == -7.0))
    return st, st2, untouched


def refusals():
    """((U, pc, pairs, start), the message) of everything refused, on the ico0 / L = 5 case; the unary table is named first where both hold a
    non-finite value"""
    U, pc, pairs, start = (np.array(a) for a in ico_case(0, 5, 31))
    N = U.shape[1]
    bad_label, bad_node, low_node, twice = np.array(start), np.array(pairs), np.array(pairs), np.array(pairs)
    bad_label[7] = 5
    bad_node[11, 1] = N
    low_node[3, 0] = -1
    twice[4, 1] = twice[4, 0]
    nan_u, inf_u, nan_p, inf_p, minus_p = np.array(U), np.array(U), np.array(pc), np.array(pc), np.array(pc)
    nan_u[2, 3] = np.nan
    inf_u[4, 11] = -np.inf
    nan_p[0, 0, 0] = np.nan
    inf_p[-1, -1, -1] = np.inf
    minus_p[7, 3, 1] = -np.inf
    unary, pair = "MSM_ERR_INVALID.*the unary table holds a non-finite value", "MSM_ERR_INVALID.*the pair table holds a non-finite value"
    return [((U, pc, pairs, bad_label), "MSM_ERR_INVALID.*label of node 7 out of range"),
            ((U, pc, bad_node, start), "MSM_ERR_INVALID.*pair node out of range"),
            ((U, pc, low_node, start), "MSM_ERR_INVALID.*pair node out of range"),
            ((U, pc, twice, start), "MSM_ERR_INVALID.*pair 4 names a node twice"),
            ((nan_u, pc, pairs, start), unary), ((inf_u, pc, pairs, start), unary), ((nan_u, inf_p, pairs, start), unary),
            ((U, nan_p, pairs, start), pair), ((U, inf_p, pairs, start), pair), ((U, minus_p, pairs, start), pair),
            ((np.zeros((1025, 2)), np.zeros((1, 1025, 1025)), np.array([[0, 1]], dtype=np.int32), np.zeros(2, dtype=np.int32)), "MSM_ERR_CAPACITY.*1025 labels")]
