"""Crafted groups for the gMSM pair-cost kernel (k_group_pairwise): patch lists whose lengths sit on and beside every threshold the kernel
branches on, handed to the library exactly as written through import_subject (a real set-up cannot put a patch on a threshold), and a
literal of DiscreteGroupCostFunction::computePairwiseCost (M/DiscreteGroupCostFunction.cpp:54-98) over the same arrays.

Shape: S = 2, control grid ico1 (N = 42 control points, P = 42 pairs: both subjects keep the regular grid, so pair p joins control point p
of subject 0 to control point p of subject 1), 19 labels, template ico4 (Vt = 2 562).  Row (subject s, control point v, label l) holds
SIZES[(5 v + 3 l + 11 s) mod 29] ascending template vertex ids: half of them a prefix of control point v's own random ranking of the
template, the rest drawn from a window behind that prefix, so that members and non-members of an intersection interleave.  Label
FAR_LABEL of subject 1 draws from the other end of the ranking: non-empty patches without a common vertex.

Shared by tests/test_group_pairs_cpu.py (the cases meet their conditions; no GPU) and tests/test_gpu_group_pair_routes.py."""
import functools

import numpy as np

from oracle import oracle as O

S, N, L, VT = 2, 42, 19, 2562
P = N  # pairs of the two regular control grids
SIZES = (0, 1, 2, 15, 16, 17, 33, 63, 64, 65, 79, 80, 81, 97, 127, 128, 129, 200, 255, 256, 257, 300, 511, 1023, 1024, 1025, 1300, 2049, 2100)
FAR_LABEL = 7  # of subject 1
ROWS = S * N * L  # 1 596
SMALL, LARGE = 40, 100  # the lane-choice cases: rows of at most kPairSmallPatch = 80 entries, and longer ones
KB = 1024
DICE_STATIC_LDS = 4 * (256 + 8) * 4  # k_group_pairwise<true, 64>: s_ids[4][kGroupStage + 8] ints (LDS Size 4 224 in the build's resource usage)


def threshold_sizes():
    s, v, l = np.meshgrid(np.arange(S), np.arange(N), np.arange(L), indexing="ij")
    return np.asarray(SIZES)[(5 * v + 3 * l + 11 * s) % len(SIZES)]


def lane_sizes(nsmall):
    """the first nsmall rows (subject, control point, label order) hold SMALL entries, the others LARGE"""
    return np.where(np.arange(ROWS) < nsmall, SMALL, LARGE).reshape(S, N, L)


def capped_sizes(cap):
    """the threshold list with every longer row cut to cap entries (cap is itself the largest patch)"""
    sizes = np.minimum(threshold_sizes(), cap)
    assert sizes.max() == cap
    return sizes


def with_one_row(n):
    sizes = threshold_sizes().copy()
    sizes[0, 0, 0] = n
    return sizes


def with_empty_last_rows():
    """the threshold list with the last row (control point N - 1, label L - 1) of both subjects empty: nothing follows an empty patch in its list"""
    sizes = threshold_sizes().copy()
    sizes[:, N - 1, L - 1] = 0
    return sizes


EMPTY_LAST_QUERIES = [(N - 1, L - 1, L - 1), (N - 1, L - 1, 0), (N - 1, 0, L - 1)]  # pair 41: both patches empty, patch A, patch B


# name -> row sizes (S x N x L)
CASES = {
    "thresholds": threshold_sizes,
    "lanes16": lambda: lane_sizes(1437),  # 10 * 1 437 >= 9 * 1 596 > 10 * 1 436: the two sides of msm_group_finalize's choice
    "lanes32": lambda: lane_sizes(1436),
    "dice958": lambda: capped_sizes(958),    # 64 * 958 + 4 224 = 64 KB exactly: the last patch size that needs no attribute
    "dice1000": lambda: capped_sizes(1000),  # 64 000 dynamic bytes stay below 64 KB, the sum does not
    "dice2100": threshold_sizes,             # 138 624 bytes: the attribute path
    "dice2500": lambda: with_one_row(2500),  # 164 224 bytes: refused (the dynamic bytes alone, 160 000, would have passed)
    "dice2561": lambda: with_one_row(2561),
    "empty_last": lambda: with_empty_last_rows(),  # the clamped loads of the register path then start behind the subject's lists
}


def dice_lds(patch_max):
    """bytes of the DICE launch for a largest patch: four wavefronts x two rows of doubles, and the kernel's static variables"""
    return 4 * 2 * 8 * max(patch_max, 1) + DICE_STATIC_LDS


@functools.lru_cache(maxsize=None)
def rankings():
    rng = np.random.default_rng(2024)
    r = np.stack([rng.permutation(VT) for _ in range(N)])
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def csr(name):
    """(pptr, pidx) of both subjects: pptr[s] N * L + 1 row offsets, pidx[s] the rows' ascending template vertex ids"""
    sizes = CASES[name]()
    rank = rankings()
    rng = np.random.default_rng(7)
    pptr, pidx = [], []
    for s in range(S):
        rows = []
        for v in range(N):
            for l in range(L):
                n = int(sizes[s, v, l])
                order = rank[v][::-1] if (s == 1 and l == FAR_LABEL) else rank[v]
                h = (n + 1) // 2
                window = order[h: h + max(2 * (n - h), 1)]
                assert len(window) >= n - h
                ids = np.concatenate([order[:h], rng.choice(window, n - h, replace=False)])
                rows.append(np.sort(ids).astype(np.int32))
        pp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        pi = np.concatenate(rows).astype(np.int32)
        pp.setflags(write=False), pi.setflags(write=False)
        pptr.append(pp), pidx.append(pi)
    return pptr, pidx


def row(name, s, v, l):
    pptr, pidx = csr(name)
    k = v * L + l
    return pidx[s][pptr[s][k]: pptr[s][k + 1]]


@functools.lru_cache(maxsize=None)
def features(D):
    """F[s]: L x D x Vt seeded random doubles, the resampled maps of subject s"""
    rng = np.random.default_rng(100 + D)
    F = [rng.standard_normal((L, D, VT)) for _ in range(S)]
    for f in F:
        f.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def mask(kind):
    """none, or dyadic weights 0, 1/4, 1/2, 1 with about a tenth of them zero"""
    if kind == "none":
        return None
    m = np.random.default_rng(5).choice([0.0, 0.25, 0.5, 1.0], VT, p=[0.1, 0.3, 0.3, 0.3])
    m.setflags(write=False)
    return m


def pairs():
    return np.stack([np.arange(N), N + np.arange(N)], axis=1).astype(np.int32)


def all_queries():
    """every (pair, label A, label B): 42 * 19 * 19 = 15 162"""
    p, la, lb = np.meshgrid(np.arange(P), np.arange(L), np.arange(L), indexing="ij")
    return p.ravel().astype(np.int32), la.ravel().astype(np.int32), lb.ravel().astype(np.int32)


# ---------------------------------------------------------------- the literal
def literal(idsA, dataA, idsB, dataB, maskv, sim, percentile=0.75, fixnan=False, reverse=False):
    """computePairwiseCost from the arrays themselves.  ids: ascending template vertex ids of the two patches, data: their values (entries x D),
    maskv: the template mask or None.  The common ids in A's order (reverse: backwards), get_sim_for_min per feature row, the sum over D.
    Returns (cost, number of common entries)."""
    at = np.searchsorted(idsB, idsA)
    at[at == len(idsB)] = 0
    hit = np.flatnonzero(idsB[at] == idsA) if len(idsB) else np.zeros(0, dtype=np.int64)
    if len(hit) == 0:
        return (1e7 if fixnan else np.nan), 0
    if reverse:
        hit = hit[::-1]
    w = np.ones(len(hit)) if maskv is None else np.abs(maskv[idsA[hit]])
    D = dataA.shape[1]
    cost = 0.0
    for d in range(D):
        cost += O.sim_for_min(sim, dataA[hit, d], dataB[at[hit], d], w, percentile)
    cost /= D
    return (1e7 if fixnan and cost != cost else cost), len(hit)


def literal_batch(name, D, sim, mask_kind, p, la, lb, percentile=0.75, fixnan=False, reverse=False):
    """the literal for queries of a crafted group: (costs, common entries per query)"""
    pptr, pidx = csr(name)
    F, m, pr = features(D), mask(mask_kind), pairs()
    out, nc = np.zeros(len(p)), np.zeros(len(p), dtype=np.int64)
    for i, (q, a, b) in enumerate(zip(p, la, lb)):
        va, vb = pr[q, 0] % N, pr[q, 1] % N
        ia, ib = row(name, 0, va, a), row(name, 1, vb, b)
        out[i], nc[i] = literal(ia, F[0][a][:, ia].T, ib, F[1][b][:, ib].T, m, sim, percentile, fixnan, reverse)
    return out, nc


@functools.lru_cache(maxsize=None)
def reference(name, D, sim, mask_kind, percentile=0.75):
    """All 15 162 queries of a crafted group through the literal, computed once and left unchanged: dict(want, ncommon, unstable).
    unstable: correlation over one or two common entries is ill-conditioned (r is +-1 or 0 / 0) -- a query whose literal changes with the
    common entries reversed is compared by its NaN pattern only."""
    p, la, lb = all_queries()
    want, nc = literal_batch(name, D, sim, mask_kind, p, la, lb, percentile)
    unstable = np.zeros(len(p), dtype=bool)
    if sim == 2:
        few = np.flatnonzero((nc == 1) | (nc == 2))
        back, _ = literal_batch(name, D, sim, mask_kind, p[few], la[few], lb[few], percentile, reverse=True)
        unstable[few] = want[few].view(np.uint64) != back.view(np.uint64)
    for a in (want, nc, unstable):
        a.setflags(write=False)
    return dict(want=want, ncommon=nc, unstable=unstable)


def query_sizes(name):
    """(cntA, cntB) of every query of all_queries()"""
    sizes = CASES[name]()
    p, la, lb = all_queries()
    pr = pairs()
    return sizes[0, pr[p, 0] % N, la], sizes[1, pr[p, 1] % N, lb]


def query_routes(name, D, sim, lanes):
    """the route name of every query (DiscreteGroupCostFunction.pair_route: the function the kernel calls)"""
    from newmsm_amd import api

    ca, cb = query_sizes(name)
    table = {}
    for a, b in set(zip(ca.tolist(), cb.tolist())):
        table[(a, b)] = api.DiscreteGroupCostFunction.pair_route(a, b, D, sim, lanes)["name"]
    return np.array([table[k] for k in zip(ca.tolist(), cb.tolist())])


def expected_routes(lanes, D, sim):
    """the routes that exist for (lanes, D, measure): the table of DESIGN.md section 5.6"""
    general = ["staged", "unstaged", "staged_beyond", "unstaged_beyond"]
    return (["fast64", "fast128", "fast256"] if D <= 2 and sim in (1, 2) else []) + general


# ---------------------------------------------------------------- the product's side
def empty_group(ctx, D, sim, mask_kind="none", fixnan=False, percentile=0.75):
    """the crafted group's frame in the library: set_template / Initialize / the subjects' (small) data meshes as usual and an empty set-up for the pair
    list -- ready for its subjects to be imported"""
    import newmsm_amd as M

    txyz, ttri = M.make_mesh_from_icosa(4)
    cxyz, ctri = M.make_mesh_from_icosa(1)
    dxyz, dtri = M.make_mesh_from_icosa(2)
    assert (len(txyz), len(cxyz)) == (VT, N)
    _, mvd = M.cp_spacings(cxyz, ctri)
    samples, _ = M.label_sampling_grid(3, 0.5 * mvd)
    assert len(samples) == L
    g = M.DiscreteGroupCostFunction(ctx, S, simmeasure=sim, fixnan=fixnan, lambda_=0.2, percentile=percentile)
    keep = [M.Mesh(ctx, txyz, ttri)]
    g.set_template(keep[0], mask(mask_kind))
    g.Initialize(cxyz, ctri)
    rng = np.random.default_rng(3)
    for s in range(S):
        m = M.Mesh(ctx, dxyz, dtri)
        g.reset_meshspace(s, m, rng.standard_normal((D, len(dxyz))))
        g.reset_CPgrid(s, cxyz)
        keep.append(m)
    g.set_labels(samples)
    g.setup_subjects([])
    return g, keep


def product_group(ctx, name, D, sim, mask_kind="none", fixnan=False, percentile=0.75):
    """the crafted group in the library: its frame, then the rows and maps exactly as written through import_subject, and finalize"""
    g, keep = empty_group(ctx, D, sim, mask_kind, fixnan, percentile)
    pptr, pidx = csr(name)
    for s in range(S):
        g.import_subject(s, features(D)[s], pptr[s], pidx[s])
    g.finalize()
    return g, keep
