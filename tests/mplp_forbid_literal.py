"""Shared by test_mplp_forbid_cpu.py and test_gpu_mplp_forbid.py: a numpy restatement of MPLP and its rounding under the forbidden-entry reading
(DESIGN.md 5.19 "Forbidden entries"), written here from the definition and not from the library's code, and the cases both files run.

theta^ is the entry where that is below +inf and +inf where it is NaN or +inf.  Every operand of a sum lies in (-inf, +inf], so numpy's plain IEEE
arithmetic forms no NaN where the definition says none arises; where the definition selects +inf instead of computing (a message of an infeasible
label, a combination with a +inf message) the restatement selects with np.where over values computed under errstate(invalid="ignore")."""
import functools
import itertools

import numpy as np

from newmsm_amd import api

import mplp_literal as ML
import mplp_round_literal as RL

INF = np.inf


def hat(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(v < INF, v, INF)


def energy(U, tc, tri, lab):
    """E^: every term through the mapping, summed as mplp_literal.energy sums"""
    u = 0.0
    for i in range(U.shape[1]):
        u += float(hat(U[lab[i], i]))
    t3 = 0.0
    for t, (a, b, c) in enumerate(tri):
        t3 += float(hat(tc[t, lab[a], lab[b], lab[c]]))
    return u + 0.0 + t3


def sweep(U, th, tri, m, inc):
    for t, (A, B, C) in enumerate(tri):
        d = [ML.node_sum(U, m, inc, int(n), skip=(t, s)) for s, n in enumerate((A, B, C))]
        v = ((th[t] + d[0][:, None, None]) + d[1][None, :, None]) + d[2][None, None, :]
        mins = (v.min(axis=(1, 2)), v.min(axis=(0, 2)), v.min(axis=(0, 1)))
        for s in range(3):
            with np.errstate(invalid="ignore"):
                new = (mins[s] + 0.0) / 3.0 - d[s]
            m[t, s] = np.where(mins[s] < INF, new, INF)


def bound(U, th, m, inc):
    D = 0.0
    for i in range(U.shape[1]):
        D += float(ML.node_sum(U, m, inc, i).min())
    for t in range(len(th)):
        ok = (th[t] < INF) & (m[t, 0] < INF)[:, None, None] & (m[t, 1] < INF)[None, :, None] & (m[t, 2] < INF)[None, None, :]
        with np.errstate(invalid="ignore"):
            v = ((th[t] - m[t, 0][:, None, None]) - m[t, 1][None, :, None]) - m[t, 2][None, None, :]
        D += float(np.where(ok, v, INF).min())
    return D


def mplp(U, tc, triplets, start, sweeps):
    """the definition: MplpResult with bounds and messages"""
    U, tc = np.asarray(U, dtype=np.float64), np.asarray(tc, dtype=np.float64)
    tri = np.asarray(triplets, dtype=np.int32).reshape(-1, 3)
    th = hat(tc)
    L, N = U.shape
    T = len(tri)
    inc = ML.incidence(tri, N)
    m = np.zeros((T, 3, L))
    best_lab, best_e = np.array(start, dtype=np.int32), energy(U, tc, tri, start)
    energies, bounds = np.full(sweeps, np.nan), np.full(sweeps, np.nan)
    run = 0
    for k in range(sweeps if T else 0):
        before = m.copy()
        sweep(U, th, tri, m, inc)
        run = k + 1
        lab = ML.decode(U, m, inc)
        energies[k] = energy(U, tc, tri, lab)
        bounds[k] = bound(U, th, m, inc)
        if energies[k] < best_e:
            best_lab, best_e = lab, energies[k]
        if before.tobytes() == m.tobytes():
            break
    if run:
        energies[run:], bounds[run:] = energies[run - 1], bounds[run - 1]
    return api.MplpResult(best_lab, run, best_e, bounds[run - 1] if run else bound(U, th, m, inc), energies, bounds, m)


def score(U, th, tri, m, inc, colour, frontier, lab, i):
    sc = np.array(U[:, i], dtype=np.float64)
    for (t, s) in inc[i]:
        s1, s2 = [q for q in range(3) if q != s]
        j1, j2 = int(tri[t, s1]), int(tri[t, s2])
        f1, f2 = colour[j1] < frontier, colour[j2] < frontier
        x = np.moveaxis(th[t], s, 0)  # (x, y1, y2), s1 < s2
        m1, m2 = m[t, s1], m[t, s2]
        with np.errstate(invalid="ignore"):
            if f1 and f2:
                g = x[:, lab[j1], lab[j2]]
            elif f1:
                e = x[:, lab[j1], :]
                g = np.where((e < INF) & (m2 < INF)[None, :], e - m2[None, :], INF).min(axis=1) + 0.0
            elif f2:
                e = x[:, :, lab[j2]]
                g = np.where((e < INF) & (m1 < INF)[None, :], e - m1[None, :], INF).min(axis=1) + 0.0
            else:
                ok = (x < INF) & (m1 < INF)[None, :, None] & (m2 < INF)[None, None, :]
                g = np.where(ok, (x - m1[None, :, None]) - m2[None, None, :], INF).min(axis=(1, 2)) + 0.0
        sc = sc + g
    return sc


def walk(U, th, tri, m, inc, colour, lab, polish):
    changed = False
    for k in range(int(colour.max()) + 1 if len(colour) else 0):
        for i in np.nonzero(colour == k)[0]:
            sc = score(U, th, tri, m, inc, colour, RL.ALL_FIXED if polish else k, lab, int(i))
            best = int(np.argmin(sc))  # the first of equal minima: label 0 where every score is +inf
            if polish and not sc[best] < sc[lab[i]]:
                best = int(lab[i])
            changed |= best != lab[i]
            lab[i] = best
    return changed


def mplp_round(U, tc, triplets, start, messages=None, mode=0, polish=8):
    """the definition: api.MplpRound"""
    U, tc = np.asarray(U, dtype=np.float64), np.asarray(tc, dtype=np.float64)
    tri = np.asarray(triplets, dtype=np.int32).reshape(-1, 3)
    th = hat(tc)
    L, N = U.shape
    zero = np.zeros((len(tri), 3, L))
    m = zero if messages is None else np.asarray(messages, dtype=np.float64).reshape(len(tri), 3, L)
    inc = ML.incidence(tri, N)
    colour = RL.colouring(tri, N)
    lab = np.array(start, dtype=np.int32)
    cands = [(lab.copy(), energy(U, tc, tri, lab))]
    if mode == 0:
        walk(U, th, tri, m, inc, colour, lab, False)
        cands.append((lab.copy(), energy(U, tc, tri, lab)))
    run = 0
    for p in range(polish):
        changed = walk(U, th, tri, zero, inc, colour, lab, True)
        run = p + 1
        cands.append((lab.copy(), energy(U, tc, tri, lab)))
        if not changed:
            break
    energies = np.array([e for _, e in cands] + [cands[-1][1]] * (polish - run))
    best = 0
    for k in range(1, len(cands)):
        if cands[k][1] < cands[best][1]:
            best = k
    return api.MplpRound(cands[best][0], run, cands[best][1], energies)


def brute_force(U, tc, triplets):
    """the lowest E^ over all L^N labellings (small graphs only); +inf: no labelling avoids the forbidden entries"""
    L, N = U.shape
    tri = np.asarray(triplets).reshape(-1, 3)
    return min(energy(U, tc, tri, lab) for lab in itertools.product(range(L), repeat=N))


def tol(U, triplets, messages):
    """the issue's: 64 (N + T) 2^-52 max(1, max|unary|, largest finite |message|)"""
    m = np.asarray(messages, dtype=np.float64)
    finite = np.abs(m[np.isfinite(m)])
    big = max(1.0, float(np.abs(U).max()), float(finite.max()) if finite.size else 0.0)
    return 64.0 * (U.shape[1] + len(triplets)) * 2.0 ** -52 * big


def uses_forbidden(tc, triplets, lab):
    tri = np.asarray(triplets).reshape(-1, 3)
    return any(not tc[t, lab[a], lab[b], lab[c]] < INF for t, (a, b, c) in enumerate(tri))


def forbid_share(case, share, seed):
    """the case with a seeded random `share` of its triplet entries forbidden, half NaN and half +inf"""
    U, tc, triplets, start = case
    rng = np.random.default_rng(seed)
    tc = np.array(tc)
    hit = rng.random(tc.shape) < share
    tc[hit] = np.where(rng.random(int(hit.sum())) < 0.5, np.nan, INF)
    return np.array(U), tc, np.array(triplets), np.array(start)


def octahedron(seed):
    return forbid_share(RL._small(ML.OCTAHEDRON, 6, 3, seed), 0.3, 100 + seed)


# 1 .. 6 are feasible; 470042 is the first seed at which no labelling avoids the forbidden entries (at share 0.3 such tables are rare: two among the
# first 634474 seeds)
OCTAHEDRON_SEEDS = (1, 2, 3, 4, 5, 6, 470042)


def fan():
    """mplp_literal.fan_case at L = 4: factor 0 forbids hub label 1 outright (NaN), factor 5 a whole label of its first rim node (+inf), and the hub's
    unary is lowered at label 1 so that the forbidden label tempts"""
    U, tc, triplets, start = (np.array(a) for a in ML.fan_case(4))
    tc[0, 1, :, :] = np.nan
    tc[5, :, 2, :] = INF
    U[1, 0] = -5.0
    return U, tc, triplets, start


def single(L, forbidden):
    """one triplet; `forbidden`: flat indices of its table set to NaN (even) or +inf (odd)"""
    U, tc, triplets, start = RL._small([[0, 1, 2]], 3, L, 40 + L)
    flat = tc.reshape(-1)
    for j, e in enumerate(forbidden):
        flat[e] = np.nan if j % 2 == 0 else INF
    return U, tc, triplets, start


@functools.lru_cache(maxsize=None)
def ico(order, L, seed=11, share=0.05, shuffled=False):
    case = forbid_share(ML.ico_case(order, L, seed, 0.0, False, shuffled), share, 1000 + seed)
    for a in case:
        a.setflags(write=False)
    return case


def start_feasible(case):
    """the case with a start whose E^ is finite: the first of a seeded sequence of random labellings that uses no forbidden entry"""
    U, tc, triplets, _ = case
    rng = np.random.default_rng(77)
    while True:
        start = rng.integers(0, U.shape[0], U.shape[1]).astype(np.int32)
        if not uses_forbidden(tc, triplets, start):
            return U, tc, triplets, start


def start_on_forbidden(case):
    """the case with a start whose E^ is +inf: the labels of triplet 0's nodes moved onto its first forbidden entry"""
    U, tc, triplets, start = case
    a, b, c = np.argwhere(~(tc[0] < INF))[0]
    start = np.array(start)
    start[triplets[0]] = (a, b, c)
    return U, tc, triplets, start


CASES = {
    "triplet L1 forbidden": lambda: single(1, [0]),
    "triplet L1": lambda: single(1, []),
    "triplet L2": lambda: single(2, [0, 3, 5]),
    "triplet L3": lambda: single(3, [0, 1, 4, 13, 20, 26]),
    "fan": fan,
    "two triangles": lambda: forbid_share(RL._small([[0, 1, 2], [2, 3, 4]], 5, 3, 1), 0.3, 201),  # a fixed point after 46 sweeps
    "ico0 L19": lambda: start_feasible(ico(0, 19)),
    "ico0 L19 start forbidden": lambda: start_on_forbidden(ico(0, 19)),
}
CASES.update({"octahedron %d" % s: functools.partial(octahedron, s) for s in OCTAHEDRON_SEEDS})

# the cases only the GPU tests run: label counts round the kernels' thresholds, many levels
GPU_CASES = {
    "ico0 L20": lambda: ico(0, 20),
    "ico0 L61": lambda: ico(0, 61),
    "ico0 L67": lambda: ico(0, 67),
    "ico2 L7 shuffled": lambda: ico(2, 7, 12, 0.05, True),
}

# (case, replacement of one value, message pattern): the refusals of the forbid entry points
def refusal_cases():
    U, tc, triplets, start = (np.array(a) for a in ico(0, 5, 31))
    minus_t, nan_u, inf_u = np.array(tc), np.array(U), np.array(U)
    minus_t[19, 4, 4, 4] = -INF
    nan_u[2, 3] = np.nan
    inf_u[1, 1] = INF
    return (U, tc, triplets, start), [((U, minus_t, triplets, start), "MSM_ERR_INVALID.*the triplet table holds -infinity"),
                                      ((nan_u, tc, triplets, start), "MSM_ERR_INVALID.*the unary table holds a non-finite value"),
                                      ((inf_u, tc, triplets, start), "MSM_ERR_INVALID.*the unary table holds a non-finite value")]
