"""gMSM with the Monte Carlo optimiser, subject by subject, written out literally in numpy: the incidence of a pair list, the conditional
unary table and the triplet table of a subject from given cost tables, the seed rule, the acceptance rule, and a pass over any chain optimiser.  No GPU."""
import numpy as np

M64 = (1 << 64) - 1


def incidence(pairs, nodes):
    """for node n the pair indices p with pairs[p][0] == n or pairs[p][1] == n, ascending: (ptr nodes + 1, idx)"""
    lists = [[] for _ in range(nodes)]
    for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        lists[a].append(p)
        if b != a:
            lists[b].append(p)
    ptr = np.zeros(nodes + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    return ptr, np.array([p for x in lists for p in x], dtype=np.int32)


def conditional_queries(pairs, ptr, idx, lab, s, N, L):
    """the (pair, la, lb) queries of subject s in segment order -- node v, label l, incident pair ascending -- and the N L + 1 segment offsets"""
    qp, qa, qb, seg = [], [], [], [0]
    for v in range(N):
        n = s * N + v
        inc = idx[ptr[n]:ptr[n + 1]]
        for l in range(L):
            for p in inc:
                a, b = pairs[p]
                qp.append(p)
                qa.append(l if a == n else lab[a])
                qb.append(lab[b] if a == n else l)
            seg.append(len(qp))
    return np.array(qp, dtype=np.int32), np.array(qa, dtype=np.int32), np.array(qb, dtype=np.int32), np.array(seg, dtype=np.int64)


def segment_sums(vals, seg, N, L):
    """U[l][v]: the segment (v, l) added in order from 0.0, each addition rounded"""
    U = np.zeros((L, N))
    for v in range(N):
        for l in range(L):
            acc = 0.0
            for x in vals[seg[v * L + l]:seg[v * L + l + 1]]:
                acc = acc + float(x)
            U[l, v] = acc
    return U


def conditional_unary(PT, pairs, ptr, idx, lab, s, N, L):
    """U_s from a pair table PT[p][la][lb]"""
    qp, qa, qb, seg = conditional_queries(pairs, ptr, idx, lab, s, N, L)
    return segment_sums(PT[qp, qa, qb] if len(qp) else np.zeros(0), seg, N, L)


def group_energy(PT, tc, pairs, triplets, lab):
    """pairs then triplets at the labelling (math.fsum: the identity is checked to 1e-12, not to the bit)"""
    import math

    pairs, triplets = np.asarray(pairs), np.asarray(triplets)
    e = [PT[p, lab[a], lab[b]] for p, (a, b) in enumerate(pairs)]
    e += [tc[t, lab[a], lab[b], lab[c]] for t, (a, b, c) in enumerate(triplets)]
    return math.fsum(e)


def block_energy(U, tc_s, tri_s, x):
    import math

    return math.fsum([U[x[v], v] for v in range(len(x))] + [tc_s[t, x[a], x[b], x[c]] for t, (a, b, c) in enumerate(tri_s)])


def seed(seed0, it, k, p, S, s):
    return (seed0 + it + 1000003 * k + 15485863 * (p * S + s)) & M64


def accept(start, best):
    return bool(best < start)


def run_pass(optimise_chains, energy, tables, lab, S, N, mcparam, iters, seed0, it, K, passes):
    """tables(s, lab) -> (U_s, tc_s, local triplets); optimise_chains(U, tc, tri, start, seeds, mcparam, iters) -> (best labelling, labelings, energies, best);
    energy(U, tc, tri, x).  Returns (labelling, records [(start, kept, accepted, best)] per block)."""
    lab = np.array(lab, dtype=np.int32)
    recs = []
    for p in range(passes):
        for s in range(S):
            U, tc, tri = tables(s, lab)
            start = lab[s * N:(s + 1) * N].copy()
            e0 = energy(U, tc, tri, start)
            seeds = np.array([seed(seed0, it, k, p, S, s) for k in range(K)], dtype=np.uint64)
            got, _, E, best = optimise_chains(U, tc, tri, start, seeds, mcparam, iters)
            take = accept(e0, E[best])
            if take:
                lab[s * N:(s + 1) * N] = got
            recs.append((e0, E[best] if take else e0, take, best))
    return lab, recs
