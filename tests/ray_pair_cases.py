"""Cases of the tests of the lane pairs of k_unary_rays (csrc/unary_kernels.hip: lanes 2j and 2j + 1 fetch the vertex pieces of their two first candidates
together and hand each other half of them): pairs in which one lane or neither has a first candidate, pairs whose second lane has no sample, and pairs
that hold the same triangle twice.  What meets what in a pair follows from the sampling kernels' mapping, restated here (unary.hpp:
unary_workgroup_share): a workgroup takes the labels [l_beg, l_end) of one control point, sample q = (l - l_beg) * P + i of its P patch points goes to
thread q % 256, and 256 is even, so the pairs are (q, q + 1) for even q, and an odd number of samples leaves the last one alone."""
import numpy as np

import newmsm_amd as M
from helpers import oracle_cost
from ray_retry_cases import inputs, mesh

# case 1 (target, control grid order): patches of 5 to 6 points under 19 labels (95 or 114 samples a workgroup) and of about 65
OUT_OF_RANGE_GRIDS = [("ico3_strongly_warped", 3), ("ico4_warped", 2)]
# case 2: ico3 / ico3 at this range_ has patches of 1 to 5 points (at 1.0: 5 to 6; at 0.82 and below every patch is its control point's own vertex)
SMALL_RANGE = 0.88
EMPTIED = 24  # control points whose only patch point is moved away


def radius_range(target):
    """(r2lo, r2hi) of the direction table of a target of ray_retry_cases.mesh, from the table's signature (host code, no GPU)"""
    sig = M.ray_table_signature(*mesh(target))
    assert sig["G"] > 0
    return tuple(float(np.array([sig[k]], dtype=np.uint64).view(np.float64)[0]) for k in ("r2lo_bits", "r2hi_bits"))


def moved_vertices(n):
    """a scattered third of n vertices (a multiplicative hash of the vertex number: runs of one to a few vertices, no period in the patch lists)"""
    v = np.arange(n, dtype=np.uint64)
    return ((v * np.uint64(2654435761)) >> np.uint64(9)) % np.uint64(3) == 0


def out_of_range_inputs(target, cp_order):
    """inputs(target, cp_order) with a scattered third of the source vertices moved radially inwards to twice the table's margin below the sphere: their
    samples have a squared radius below r2lo whatever the label's rotation does to the last bits, so ray_cell_of gives them no first candidate"""
    inp = inputs(target, cp_order, D=1)
    r2lo, _ = radius_range(target)
    src = np.array(inp["source_xyz"], dtype=np.float64)
    r = np.linalg.norm(src, axis=1)
    assert np.all(r * r > r2lo)  # (the source lies on the sphere: every sample is in range before the move)
    moved = moved_vertices(len(src))
    r_in = np.sqrt(r2lo) - (r.mean() - np.sqrt(r2lo))
    src[moved] *= (r_in / r[moved])[:, None]
    assert np.all((src[moved] ** 2).sum(axis=1) < r2lo * (1 - 1e-9))
    return dict(inp, source_xyz=src), moved


def pair_census(pptr, pidx, flagged, L, nsplit):
    """how the samples of a table meet in lane pairs: counts of pairs by (even lane, odd lane), each 'in' (a sample whose source vertex is not flagged),
    'out' (flagged) or 'none' (no sample: the odd lane behind an odd number of samples)"""
    out = {}
    lper = (L + nsplit - 1) // nsplit
    for n in range(len(pptr) - 1):
        f = np.asarray(flagged)[pidx[pptr[n]:pptr[n + 1]]]
        for l_beg in range(0, L, lper):
            q = np.tile(f, min(L, l_beg + lper) - l_beg)
            names = np.where(q, "out", "in")
            if len(names) % 2:
                names = np.append(names, "none")
            for pair in zip(names[0::2], names[1::2]):
                out[pair] = out.get(pair, 0) + 1
    return out


def emptied_inputs():
    """case 2: inputs("ico3_strongly_warped", 3) whose patches at range_ = SMALL_RANGE include sizes 0 and 1.  A control point of ico3 / ico3 coincides with a
    source vertex, which is in range at every range_ > 0 (the reference's test is distance < range_ * spacing), so no range_ gives an empty patch by
    itself: the lone vertices of EMPTIED one-point patches are moved next to the vertex half-way round the vertex list, 0.3 of a spacing from it."""
    inp = inputs("ico3_strongly_warped", 3, D=1)
    oc = oracle_cost(inp, "univariate", range_=SMALL_RANGE)
    oc.get_source_data()
    pptr, pidx = oc.patches()
    sizes = np.diff(pptr)
    lone = np.flatnonzero(sizes == 1)[:: max(1, (sizes == 1).sum() // EMPTIED)][:EMPTIED]
    src = np.array(inp["source_xyz"], dtype=np.float64)
    n = len(src)
    for k in lone:
        v = int(pidx[pptr[k]])
        w = (v + n // 2) % n
        nb = (w + 1) % n
        p = src[w] + 0.3 * np.min(inp["maxsep"]) * (src[nb] - src[w]) / np.linalg.norm(src[nb] - src[w])
        src[v] = p / np.linalg.norm(p) * np.linalg.norm(src[w])
    return dict(inp, source_xyz=src), lone
