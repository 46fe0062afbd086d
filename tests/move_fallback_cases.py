"""Shared by tests/test_move_fallbacks_cpu.py (the oracle and the host entry points alone: is the direction table built, is the oracle finite
everywhere, how much folds?) and tests/test_gpu_move_fallbacks.py (the MI355X path against the oracle): star-shaped targets -- the data sphere's
vertices moved radially (problem.pairwise_inputs(..., target_radial=r)), still one triangle per ray, so the direction table is built and the fused
move applies, but off the shell of radius 100 the queries descend the octree on.  There some samples the direction table leaves open find no
candidate in their octree leaf: the fused move hands their evaluations to k_ho_move_tail, the three-kernel path and the unary table theirs to
k_ho_octets_fix / k_unary_fixup.

RADIAL: of the amplitudes 3e-3, 1e-2 and 3e-2 the one at which the fused move defers most on the smallest shape (ico4 data / ico2 control grid,
320 control triangles; evaluations deferred by the two labelings of move_labelings(., SEED), measured on an MI355X: 1 and 0 at 3e-3, 20 and 16 at
1e-2, 354 and 318 at 3e-2)."""
import functools
import types

import numpy as np

from newmsm_amd import problem
from helpers import HCP, move_labelings, oracle_cost

LAMBDA = 0.0075    # --lambda of the ico3 level of the HCP configuration (HCP: its regulariser options, from helpers)
MAX_FOLDED = 0.05  # of a move's evaluations: the cap of tests/test_gpu_feature_widths.py
SEED = 534         # of move_labelings
RADIAL = 3e-2
MOVE_SHAPE = (4, 2)     # the fused move and the unary tables: 320 control triangles with bins of 3 to 15 points, 162 patches of 50 to 68
BIG_BIN_SHAPE = (5, 1)  # the three-kernel path: 80 control triangles with bins of 105 to 150 points
MANY_LABELS = 6         # sampling-grid order under the ico2 control grid: 277 labels, beyond the 256 the kernel arguments carry

# (kind, D, simmeasure, route) of every mode of k_ho_move
FUSED = [("ho_univariate", 1, 2, "fused0"), ("ho_univariate", 1, 1, "fused0"), ("ho_multivariate", 13, 2, "fused1"), ("ho_multivariate", 16, 4, "fused1"),
         ("ho_multivariate", 12, 2, "fused3"), ("ho_multivariate", 12, 1, "fused3"), ("ho_multivariate", 34, 2, "fused2")]
WEIGHTED = [("ho_univariate", 1), ("ho_multivariate", 12), ("ho_multivariate", 34)]  # fused0, fused3, fused2; each with one weight row and with D
SINGLE = [("ho_univariate", 1, "fused0"), ("ho_multivariate", 34, "fused2")]          # evaluateTotalCostSum
DEVICE_LABELS = [("ho_univariate", 1, "fused0"), ("ho_multivariate", 12, "fused3")]   # the labeling as a device array (MANY_LABELS)
THREE_KERNEL = [(11, "octets_sample"), (12, "octets_sample_mv8")]
UNARY = [("multivariate", 11, "features"), ("multivariate", 12, "mv8"), ("patchwise", 12, "pw8<4>"), ("patchwise", 33, "pw8<8>")]


@functools.lru_cache(maxsize=None)
def star(shape, D, sg_order=None, radial=RADIAL):
    """the inputs of one shape and row count (read only)"""
    return problem.pairwise_inputs(shape[0], shape[1], D=D, sg_order=sg_order, target_radial=radial)


def weights(inp, rows):
    return np.random.default_rng(200 + inp["D"]).uniform(0.1, 1.0, size=(rows, len(inp["source_xyz"])))


def labelings(N, L, seed=SEED):
    return move_labelings(types.SimpleNamespace(N=N, L=L), seed)


def total_labelings(N, L):
    """evaluateTotalCostSum: all control points on the centre label, and a random labeling"""
    return [np.zeros(N, dtype=np.int32), np.random.default_rng(SEED + 1).integers(0, L, N).astype(np.int32)]


def other_label(N, L):
    """a label that the mixed labeling's move does not propose (the call that drops its prefetch)"""
    return (labelings(N, L)[1][1] + 1) % L


@functools.lru_cache(maxsize=None)
def oracle(kind, D, sim=2, rows=0, shape=MOVE_SHAPE, sg_order=None, radial=RADIAL):
    """the oracle's cost function of a move case after get_source_data (its pair list emptied: the product side is built with triplets only)"""
    inp = star(shape, D, sg_order, radial)
    oc = oracle_cost(inp, kind, simmeasure=sim, lambda_=LAMBDA, **HCP)
    if rows:
        oc.set_cfweight(weights(inp, rows))
    oc.get_source_data()
    oc.set_pairs(np.zeros((0, 2), dtype=np.int32))
    return oc


@functools.lru_cache(maxsize=None)
def octets(which, *case, **kw):
    """the oracle's move of labeling `which` of labelings() (0: all zero, 1: mixed; 2: the mixed labeling with other_label) -- computed once, shared
    by the tests of a case (read only)"""
    oc = oracle(*case, **kw)
    labeling, label = labelings(oc.N, oc.L)[min(which, 1)]
    E = oc.triplet_octets(labeling, other_label(oc.N, oc.L) if which == 2 else label, threads=8)
    E.setflags(write=False)
    return E


@functools.lru_cache(maxsize=None)
def unary_oracle(kind, D, sim=2):
    inp = star(MOVE_SHAPE, D)
    oc = oracle_cost(inp, kind, simmeasure=sim)
    oc.get_source_data()
    U = oc.unary_table(threads=8)
    U.setflags(write=False)
    return oc, U


def move_cases():
    """(case, keywords) of every oracle() the GPU file evaluates a move of"""
    out = [((k, D, sim), {}) for k, D, sim, _ in FUSED]
    out += [((k, D, 2, rows), {}) for k, D in WEIGHTED for rows in sorted({1, D})]
    out += [((k, D), dict(sg_order=MANY_LABELS)) for k, D, _ in DEVICE_LABELS]
    out += [(("ho_multivariate", D), dict(shape=BIG_BIN_SHAPE)) for D, _ in THREE_KERNEL]
    return out
