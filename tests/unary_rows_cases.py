"""Shared by tests/test_unary_rows_cpu.py (the oracle alone, no GPU), tests/test_gpu_unary_rows.py (the MI355X path) and tools/record_unary_tables.py:
unary tables over patches of 1 to 101 points, the sizes around which k_unary_reduce_rows (csrc/unary_reduce_kernels.hip) can go
wrong -- an 8-lane group per table row with twelve register slots per lane, behind a prepare step whose statistics stride 64 lanes -- and the
threshold of 96 points above which k_unary_reduce_flat runs instead.

Every shape is problem.pairwise_inputs(data, cp) with the default seed, univariate, and the cost's range_ parameter.  Measured on the oracle, where every
table is finite in every entry:

  one    3 / 1  range 0.2   19 x 42    1         one point per row: the zero-variance branch; a constant table
  few    3 / 1  range 0.3   19 x 42    6..7      fewer points than a group has lanes (the patches are disjoint)
  slot2  3 / 1  range 0.5   19 x 42    12..19    second register slot partly filled
  wave   3 / 1  range 1.0   19 x 42    50, 60    below one 64-lane stride of the statistics
  wave2  4 / 2  range 1.0   19 x 162   50..68    statistics lanes with a second element; 3 078 rows, the last workgroup partly filled
  full   3 / 1  range 1.24  19 x 42    71..95    all twelve register slots; the largest patch just under the threshold
  over   3 / 1  range 1.25  19 x 42    74..101   just over it: the staged kernel
  many   3 / 1  range 1.0   57 x 42    50, 60    sg_order 4, L > 32: a control point's rows spread over wavefronts and workgroups

Inputs, oracle objects and oracle tables are cached and shared between the tests of a session: read only."""
import functools

import numpy as np

from newmsm_amd import problem
from helpers import oracle_cost

ROWS_PMAX = 96  # kRowsPmax: the largest patch of the row form
# name: data order, control-grid order, range_, sg_order, labels, control points, smallest and largest patch
CASES = dict(
    one=(3, 1, 0.2, None, 19, 42, 1, 1),
    few=(3, 1, 0.3, None, 19, 42, 6, 7),
    slot2=(3, 1, 0.5, None, 19, 42, 12, 19),
    wave=(3, 1, 1.0, None, 19, 42, 50, 60),
    wave2=(4, 2, 1.0, None, 19, 162, 50, 68),
    full=(3, 1, 1.24, None, 19, 42, 71, 95),
    over=(3, 1, 1.25, None, 19, 42, 74, 101),
    many=(3, 1, 1.0, 4, 57, 42, 50, 60),
)
SIMS = (2, 1)  # correlation, SSD
ZEROED = (0, 17, 41)  # the control points of `few` whose patches the "zero" weight row switches off
# the weight rows of a case: none, unary_patch_cases.weights, and for `few` that row with zeros on every point of the ZEROED patches
WEIGHTINGS = {name: ("", "row") + (("zero",) if name == "few" else ()) for name in CASES}


def form_of(name):
    return "rows" if CASES[name][7] <= ROWS_PMAX else "staged"


def range_of(name):
    return CASES[name][2]


@functools.lru_cache(maxsize=None)
def inputs(name):
    data, cp, _, sg = CASES[name][:4]
    return problem.pairwise_inputs(data, cp, sg_order=sg)


@functools.lru_cache(maxsize=None)
def weights(name, weighting):
    """None, or the 1 x Nsrc weight row of a weighting"""
    if not weighting:
        return None
    import unary_patch_cases

    w = unary_patch_cases.weights(inputs(name), 1)
    if weighting == "zero":
        ptr, idx = oracle(name).patches()
        for node in ZEROED:
            w[0, idx[ptr[node]:ptr[node + 1]]] = 0.0
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def oracle(name, sim=2, weighting=""):
    """the oracle's cost function of a case after get_source_data()"""
    oc = oracle_cost(inputs(name), "univariate", simmeasure=sim, range_=range_of(name))
    if weighting:
        oc.set_cfweight(np.array(weights(name, weighting)))
    oc.get_source_data()
    return oc


@functools.lru_cache(maxsize=None)
def oracle_table(name, sim=2, weighting=""):
    U = oracle(name, sim, weighting).unary_table()
    U.setflags(write=False)
    return U


def key(name, sim, weighting):
    """the table's name in tests/golden/unary_rows_parent.npz"""
    return "%s-sim%d-%s" % (name, sim, weighting or "plain")


def all_tables():
    return [(name, sim, weighting) for name in CASES for sim in SIMS for weighting in WEIGHTINGS[name]]


def product(ctx, name, sim=2, weighting=""):
    """the product's cost function of a case after get_source_data(), its target's direction table built"""
    cf, keep = problem.build_cost(ctx, inputs(name), kind="univariate", simmeasure=sim, range_=range_of(name))
    if weighting:
        cf.set_dataaffintyweighting(np.array(weights(name, weighting)))
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)
    cf._keep_meshes = keep
    return cf
