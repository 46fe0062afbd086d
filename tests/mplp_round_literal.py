"""Shared by test_mplp_round_cpu.py and test_gpu_mplp_round.py: a numpy restatement of the rounding of MPLP's messages (DESIGN.md 5.19 "Rounding"),
written here from the definition and not from the library's code, and the cases both files run on top of those of mplp_literal.py.

Every floating-point operation is one IEEE double operation in the order the definition gives: (theta - m1) - m2 element by element, exact minima,
`+ 0.0` on every minimum, the scores summed slot by slot in list order, the energies as mplp_literal.energy sums them."""
import functools

import numpy as np

from newmsm_amd import api

import mplp_literal as ML

ALL_FIXED = 2 ** 31 - 1


def colouring(triplets, N):
    """colour per node: ascending, the smallest colour no lower-index node sharing a triplet holds"""
    inc = ML.incidence(triplets, N)
    tri = np.asarray(triplets).reshape(-1, 3)
    colour = np.zeros(N, dtype=np.int32)
    for i in range(N):
        held = {int(colour[j]) for (t, _) in inc[i] for j in tri[t] if j < i}
        c = 0
        while c in held:
            c += 1
        colour[i] = c
    return colour


def score(U, tc, tri, m, inc, colour, frontier, lab, i):
    sc = np.array(U[:, i], dtype=np.float64)
    for (t, s) in inc[i]:
        s1, s2 = [q for q in range(3) if q != s]
        j1, j2 = int(tri[t, s1]), int(tri[t, s2])
        f1, f2 = colour[j1] < frontier, colour[j2] < frontier
        th = np.moveaxis(tc[t], s, 0)  # (x, y1, y2): the remaining axes keep their order, s1 < s2
        if f1 and f2:
            g = th[:, lab[j1], lab[j2]]
        elif f1:
            g = (th[:, lab[j1], :] - m[t, s2][None, :]).min(axis=1) + 0.0
        elif f2:
            g = (th[:, :, lab[j2]] - m[t, s1][None, :]).min(axis=1) + 0.0
        else:
            g = ((th - m[t, s1][None, :, None]) - m[t, s2][None, None, :]).min(axis=(1, 2)) + 0.0
        sc = sc + g
    return sc


def walk(U, tc, tri, m, inc, colour, lab, polish):
    """one pass over the classes, in place; whether a label changed"""
    changed = False
    for k in range(int(colour.max()) + 1 if len(colour) else 0):
        for i in np.nonzero(colour == k)[0]:
            sc = score(U, tc, tri, m, inc, colour, ALL_FIXED if polish else k, lab, int(i))
            best = int(np.argmin(sc))  # the first of equal minima
            if polish and not sc[best] < sc[lab[i]]:
                best = int(lab[i])
            changed |= best != lab[i]
            lab[i] = best
    return changed


def mplp_round(U, tc, triplets, start, messages=None, mode=0, polish=8):
    """the definition: api.MplpRound"""
    U, tc = np.asarray(U, dtype=np.float64), np.asarray(tc, dtype=np.float64)
    tri = np.asarray(triplets, dtype=np.int32).reshape(-1, 3)
    L, N = U.shape
    m = np.zeros((len(tri), 3, L)) if messages is None else np.asarray(messages, dtype=np.float64).reshape(len(tri), 3, L)
    inc = ML.incidence(tri, N)
    colour = colouring(tri, N)
    lab = np.array(start, dtype=np.int32)
    cands = [(lab.copy(), ML.energy(U, tc, tri, lab))]
    if mode == 0:
        walk(U, tc, tri, m, inc, colour, lab, False)
        cands.append((lab.copy(), ML.energy(U, tc, tri, lab)))
    run = 0
    for p in range(polish):
        changed = walk(U, tc, tri, m, inc, colour, lab, True)
        run = p + 1
        cands.append((lab.copy(), ML.energy(U, tc, tri, lab)))
        if not changed:
            break
    energies = np.array([e for _, e in cands] + [cands[-1][1]] * (polish - run))
    best = 0
    for k in range(1, len(cands)):
        if cands[k][1] < cands[best][1]:
            best = k
    return api.MplpRound(cands[best][0], run, cands[best][1], energies)


def same(got, want, what=""):
    assert got.labeling.dtype == np.int32 and np.array_equal(got.labeling, want.labeling), what
    assert got.passes_run == want.passes_run, (what, got.passes_run, want.passes_run)
    assert np.float64(got.energy).tobytes() == np.float64(want.energy).tobytes(), (what, got.energy, want.energy)
    a, b = np.asarray(got.energies, dtype=np.float64), np.asarray(want.energies, dtype=np.float64)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, a, b)


@functools.lru_cache(maxsize=None)
def messages_after(case_key, sweeps):
    """the host literal's messages after `sweeps` sweeps of a case of CASES, and the winner of those sweeps; never written"""
    U, tc, triplets, start = CASES[case_key]()
    r = api.mplp_optimise(U, tc, triplets, start, sweeps=sweeps, bound=False, messages=True)
    r.messages.setflags(write=False)
    r.labeling.setflags(write=False)
    return r.messages, r.labeling


def _small(triplets, N, L, seed):
    triplets = np.asarray(triplets, dtype=np.int32)
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (L, N)), rng.uniform(0.0, 1.0, (len(triplets), L, L, L)), triplets, rng.integers(0, L, N).astype(np.int32)


def permuted(case, seed):
    """the three nodes of every triplet permuted by a seeded rule, the table's axes with them: every (slot of a node, which others are fixed) occurs"""
    U, tc, triplets, start = case
    rng = np.random.default_rng(seed)
    tri, tab = np.array(triplets), np.array(tc)
    for t in range(len(tri)):
        p = rng.permutation(3)
        tri[t] = tri[t][p]
        tab[t] = np.transpose(tab[t], p)
    return U, np.ascontiguousarray(tab), tri, start


def combinations(triplets, N):
    """the (slot, other s1 fixed, other s2 fixed) triples that occur in the conditioned decode"""
    tri = np.asarray(triplets).reshape(-1, 3)
    colour = colouring(tri, N)
    seen = set()
    for t in range(len(tri)):
        for s in range(3):
            s1, s2 = [q for q in range(3) if q != s]
            k = colour[tri[t, s]]
            seen.add((s, bool(colour[tri[t, s1]] < k), bool(colour[tri[t, s2]] < k)))
    return seen


def unread_messages():
    """messages of the T = 20 / L = 5 case with one +inf, one -inf, one NaN: the plain reading's mode 0 refuses each with the same words (not the
    forbidden-entry reading's, which allows the first), and mode 1 reads none of them"""
    out = []
    for value in (np.inf, -np.inf, np.nan):
        m = np.zeros((20, 3, 5))
        m[3, 1, 2] = value
        out.append(m)
    return out


def refusal_cases():
    """(arguments of mplp_round, the message); shared with the GPU tests"""
    U, tc, triplets, start = (np.array(a) for a in ML.ico_case(0, 5, 31))
    N = U.shape[1]
    bad_label, bad_node, twice = np.array(start), np.array(triplets), np.array(triplets)
    bad_label[7] = 5
    bad_node[11, 2] = N
    twice[4, 2] = twice[4, 0]
    nan_u, inf_t, nan_m = np.array(U), np.array(tc), np.zeros((len(triplets), 3, 5))
    nan_u[2, 3] = np.nan
    inf_t[19, 4, 4, 4] = -np.inf
    nan_m[3, 1, 2] = np.inf
    ok = (U, tc, triplets, start, None, 0, 2)
    plain = [(args + (None, 1, 2), pattern) for args, pattern in ML.non_finite_refusals()]  # the tables are looked at in either mode
    plain += [((U, tc, triplets, start, m, 0, 2), "MSM_ERR_INVALID.*the messages hold a non-finite value") for m in unread_messages()]
    return ok, [((U, tc, triplets, bad_label, None, 0, 2), "MSM_ERR_INVALID.*msm_mcmc_optimise: label of node 7 out of range"),
                ((U, tc, bad_node, start, None, 0, 2), "MSM_ERR_INVALID.*msm_mcmc_optimise: triplet node out of range"),
                ((U, tc, twice, start, None, 0, 2), "MSM_ERR_INVALID.*triplet 4 names a node twice"),
                ((nan_u, tc, triplets, start, None, 0, 2), "MSM_ERR_INVALID.*the unary table holds a non-finite value.*--fixnan"),
                ((U, inf_t, triplets, start, None, 1, 2), "MSM_ERR_INVALID.*the triplet table holds a non-finite value.*--fixnan"),
                ((U, tc, triplets, start, nan_m, 0, 2), "MSM_ERR_INVALID.*the messages hold a non-finite value"),
                ((U, tc, triplets, start, None, 2, 2), "MSM_ERR_INVALID.*mode 2"),
                ((U, tc, triplets, start, None, -1, 2), "MSM_ERR_INVALID.*mode -1"),
                ((U, tc, triplets, start, None, 0, -1), "MSM_ERR_INVALID.*-1 polish passes"),
                ((U, tc, triplets, start, None, 1, 1025), "MSM_ERR_INVALID.*1025 polish passes"),
                ((np.zeros((1025, 3)), np.zeros((0, 1, 1, 1)), np.zeros((0, 3), dtype=np.int32), np.zeros(3, dtype=np.int32), None, 0, 2),
                 "MSM_ERR_CAPACITY.*1025 labels")] + plain


CASES = {
    "triplet L1": lambda: _small([[0, 1, 2]], 3, 1, 1),
    "triplet L2": lambda: _small([[0, 1, 2]], 3, 2, 2),
    "triplet L3": lambda: _small([[2, 0, 1]], 3, 3, 3),
    "octahedron": lambda: _small(ML.OCTAHEDRON, 6, 3, 2),
    "ico0 L16": lambda: ML.ico_case(0, 16, 11),
    "ico0 L19": lambda: ML.ico_case(0, 19, 11),
    "ico0 L20": lambda: ML.ico_case(0, 20, 11),
    "fan": lambda: ML.fan_case(),
    "ico2 L8": lambda: ML.ico_case(2, 8, 11),
    "ico2 L8 shuffled": lambda: ML.ico_case(2, 8, 12, 0.0, False, True),
    "ico0 with 1e7": lambda: ML.ico_case(0, 19, 13, 0.05),
    "ico2 with 1e7": lambda: ML.ico_case(2, 7, 13, 0.05),
    "ties": lambda: ML.ico_case(1, 4, 21, 0.0, True),
    "twelve": lambda: permuted(ML.ico_case(1, 5, 17), 3),
}
