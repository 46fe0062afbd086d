"""Shared by tests/test_unary_patches_cpu.py (the oracle and the launch plan alone, no GPU) and tests/test_gpu_unary_patches.py (the MI355X path against
the oracle): unary tables over patches of hundreds to thousands of source points -- coarse control grids under fine data grids, as in the first levels
of a multiresolution schedule -- where the launch decisions that depend on the largest patch pmax (unary_plan.cpp: unary_plan) leave the values
they have at the workload's 40 to 90 points.

Every shape is problem.pairwise_inputs(data, cp, D=...) with its default seed and warp, and the cost's range_ parameter.  Measured on the oracle
(patch sizes min..max; oracle table on 8 threads):

  A  4 / 1  range 1.0   42 x 19    200..253     0.7 s
  B  4 / 0  range 1.0   12 x 15    722..726     0.5 s
  C  5 / 1  range 1.0   42 x 19    776..1012    3.2 s
  D  5 / 1  range 1.1   42 x 19    929..1230    4.4 s (patchwise D = 3, DICE)
  E  4 / 0  range 2.5   12 x 15    2471..2478   1.7 s
  F  5 / 0  range 1.0   12 x 15    2856..2875   2.2 to 2.6 s (D = 1, 3, 12)
  G  5 / 0  range 1.3   12 x 15    4484..4511   3.4 s
  H  5 / 0  range 1.5   12 x 15    5596..5618   4.3 s
  X  6 / 0  range 1.0   12 x 15    11435..11512 patches only (4 s of set-up): no table

The oracle's tables of A to H are finite in every entry with a spread (np.ptp) of 0.19 to 0.87, so a test compares every entry and a constant table
cannot pass.  Inputs, oracle objects and oracle tables are cached and shared between the tests of a session: read only."""
import functools

import numpy as np

from newmsm_amd import problem
from helpers import oracle_cost

# name: data order, control-grid order, range_, control points, labels, smallest and largest patch (bounds: the measured sizes above)
CASES = dict(
    A=(4, 1, 1.0, 42, 19, 200, 253),
    B=(4, 0, 1.0, 12, 15, 722, 726),
    C=(5, 1, 1.0, 42, 19, 776, 1012),
    D=(5, 1, 1.1, 42, 19, 929, 1230),
    E=(4, 0, 2.5, 12, 15, 2471, 2478),
    F=(5, 0, 1.0, 12, 15, 2856, 2875),
    G=(5, 0, 1.3, 12, 15, 4484, 4511),
    H=(5, 0, 1.5, 12, 15, 5596, 5618),
    X=(6, 0, 1.0, 12, 15, 11435, 11512),
)
TABLES = "ABCDEFGH"  # X is beyond every kernel's LDS: refused, no table

KB = 1024
LDS_DEFAULT, LDS_WORKGROUP = 64 * KB, 160 * KB  # dynamic LDS without / with the kernel's attribute raised
CHUNK = 768      # kChunk: samples per LDS pass of k_unary_samples
FLAT_REGS = 96   # kRedKeep * kRedLanes: target values per label that k_unary_reduce_flat keeps in registers
SEGMENTS = 64    # MSM_UNARY_FIX_SEGMENTS


def range_of(name):
    return CASES[name][2]


@functools.lru_cache(maxsize=None)
def inputs(name, D=1, sg_order=None):
    data, cp = CASES[name][:2]
    return problem.pairwise_inputs(data, cp, D=D, sg_order=sg_order)


def weights(inp, rows, seed=31):
    """cost-function weights in [0.2, 1): one row (sW of the univariate kernels, every channel of the others) or a row per dimension"""
    return np.random.default_rng(seed).uniform(0.2, 1.0, size=(rows, len(inp["source_xyz"])))


@functools.lru_cache(maxsize=None)
def oracle(name, kind="univariate", D=1, sim=2, rows=0, sg_order=None):
    """the oracle's cost function of a case after get_source_data()"""
    inp = inputs(name, D, sg_order)
    oc = oracle_cost(inp, kind, simmeasure=sim, range_=range_of(name))
    if rows:
        oc.set_cfweight(weights(inp, rows))
    oc.get_source_data()
    return oc


@functools.lru_cache(maxsize=None)
def oracle_table(name, kind="univariate", D=1, sim=2, rows=0, sg_order=None):
    U = oracle(name, kind, D, sim, rows, sg_order).unary_table(threads=8)
    U.setflags(write=False)
    return U


@functools.lru_cache(maxsize=None)
def patches(name):
    """(pptr, sizes) of a case from the oracle; the patches depend on the meshes and range_ only"""
    ptr, _ = oracle(name).patches()
    ptr = np.asarray(ptr, dtype=np.int32)
    return ptr, np.diff(ptr)


def workgroup_shares(N, L, nsplit, pptr, order):
    """(segment, samples) of every workgroup of the sampling kernels, from the sampling kernels' mapping (unary.hpp: unary_workgroup_share), restated: workgroup b takes
    label range b // slots of the control point at launch position (slot & 7) * per + (slot >> 3), and appends to fix-up segment b % 64"""
    per = (N + 7) >> 3
    slots = 8 * per
    lper = (L + nsplit - 1) // nsplit
    out = []
    for b in range(nsplit * slots):
        part, slot = divmod(b, slots)
        at = (slot & 7) * per + (slot >> 3)
        if at >= N:
            continue
        l_beg, l_end = part * lper, min(L, part * lper + lper)
        if l_beg >= l_end:
            continue
        node = int(order[at])
        out.append((b % SEGMENTS, (l_end - l_beg) * int(pptr[node + 1] - pptr[node])))
    return out
