"""The lane pairs of k_unary_rays (csrc/unary_kernels.hip): lanes 2j and 2j + 1 fetch the six vertex pieces of their two first
candidates together -- each load instruction has both lanes read adjacent pieces of one record -- and hand each other half of what they loaded.  A lane
without a first candidate loads for its partner, so the cases are the pairs the existing suites do not make on purpose: one lane or neither with a
first candidate at either parity, an odd lane without a sample behind patches of one point, of none and of odd sizes, and two lanes with the same triangle.

Every table follows tests/test_gpu_unary_retries.py: computed plainly, without certificates and through the complete sampler, the three equal bit for
bit, each computed twice bit-equal with every fix-up counter zero afterwards, and within the suite's bars of the oracle wherever the oracle's table is
finite (elsewhere the complete sampler is the reference: the bit-equality covers those entries, NaN for NaN)."""
import numpy as np
import pytest

import newmsm_amd as M
import ray_pair_cases as cases
from ray_retry_cases import inputs
from tests.helpers import oracle_cost

pytestmark = pytest.mark.gpu


def table(ctx, inp, kind, sampler="rays", **params):
    """tests/test_gpu_unary_retries.py: table, with NaN equal to NaN and the cost's parameters passed on"""
    from newmsm_amd import problem

    cf, keep = problem.build_cost(ctx, inp, kind=kind, **params)
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)
    U = cf.computeUnaryCosts().copy()
    plan = cf.unary_launch()
    assert plan["sampler"] == sampler
    assert not cf.unary_fix_counters().any()
    assert np.array_equal(U, cf.computeUnaryCosts(), equal_nan=True)
    assert not cf.unary_fix_counters().any()
    return U, plan


def three_tables(ctx, monkeypatch, inp, kind, **params):
    plain, plan = table(ctx, inp, kind, **params)
    monkeypatch.setenv("MSMHIP_RAY_CERTS", "off")
    without_certs, _ = table(ctx, inp, kind, **params)
    monkeypatch.delenv("MSMHIP_RAY_CERTS")
    monkeypatch.setenv("MSMHIP_RAYTABLE", "off")
    complete, _ = table(ctx, inp, kind, sampler="samples", **params)
    assert np.array_equal(plain, complete, equal_nan=True)
    assert np.array_equal(plain, without_certs, equal_nan=True)
    return plain, plan


def against_oracle(U, Uo, rtol, atol):
    finite = np.isfinite(Uo)
    assert U.shape == Uo.shape and finite.any()
    print("max |table - oracle| = %.3e over %d of %d entries" % (np.max(np.abs(U[finite] - Uo[finite])), finite.sum(), Uo.size))
    assert np.allclose(U[finite], Uo[finite], rtol=rtol, atol=atol), np.max(np.abs(U[finite] - Uo[finite]))


@pytest.mark.parametrize("target,cp_order", cases.OUT_OF_RANGE_GRIDS, ids=["%s-ico%d" % g for g in cases.OUT_OF_RANGE_GRIDS])
def test_partner_without_a_first_candidate(ctx, monkeypatch, target, cp_order):
    """A scattered third of the source vertices lies 2e-4 inside the sphere, below the table's radius range: their samples get no first candidate from
    ray_cell_of and go to the fix-up list, and their lanes load for their partners.  On the CPU first: the oracle's table is finite in every entry (19 x 642
    with a spread of 0.75, 19 x 162 with 0.69), and the samples meet in every way -- ico3 / ico3, one workgroup per control point: 10 179 pairs in / out,
    10 253 out / in, 3 995 out / out, 135 + 78 lone even lanes; ico4 / ico2, two: 26 298, 26 061, 6 444, 38 + 18."""
    inp, moved = cases.out_of_range_inputs(target, cp_order)
    oc = oracle_cost(inp, "univariate")
    oc.get_source_data()
    pptr, pidx = oc.patches()
    Uo = oc.unary_table()
    assert np.isfinite(Uo).all() and np.ptp(Uo) > 0.5
    nsplit = M.unary_launch_plan("univariate", 2, 1, Uo.shape[0], int(np.diff(pptr).max()), True)["nsplit"]
    census = cases.pair_census(pptr, pidx, moved, Uo.shape[0], nsplit)
    print(target, cp_order, "nsplit", nsplit, {"%s/%s" % k: v for k, v in census.items()})
    for pair in [("in", "out"), ("out", "in"), ("out", "out"), ("in", "in"), ("in", "none"), ("out", "none")]:
        assert census.get(pair, 0) > 0, pair
    U, plan = three_tables(ctx, monkeypatch, inp, "univariate")
    assert plan["nsplit"] == nsplit  # (the pairs counted above are the pairs the kernel made)
    against_oracle(U, Uo, 1e-10, 1e-12)
    # the in-range partners are untouched and the others went through the fix-up: with the moved vertices alone out of the table's reach the table is
    # still the oracle's, and it is not the table of the unmoved source (whose patches differ: every entry of the comparison would pass a stale table)
    oc0 = oracle_cost(inputs(target, cp_order, D=1), "univariate")
    oc0.get_source_data()
    assert not np.allclose(U, oc0.unary_table(), rtol=1e-10, atol=1e-12)


def test_patches_of_one_point_and_of_none(ctx, monkeypatch):
    """ico3 / ico3 at range_ = 0.88: patches of 1 to 5 points.  No range_ above zero empties a patch there (a control point coincides with a source vertex), so
    the lone vertices of some one-point patches are moved away (ray_pair_cases.emptied_inputs).  On the CPU first: 23 patches of no point, 51 of one, 119,
    287, 94, 57 and 11 of two to six; the oracle's table is finite but for 57 entries, the 19 labels of three control points, where the complete sampler
    is the reference."""
    inp, lone = cases.emptied_inputs()
    oc = oracle_cost(inp, "univariate", range_=cases.SMALL_RANGE)
    oc.get_source_data()
    sizes = np.diff(oc.patches()[0])
    print("patches by size:", np.bincount(sizes))
    assert {0, 1, 3, 5} <= set(sizes.tolist()) and (sizes == 0).sum() >= 16 and (sizes == 1).sum() >= 16 and sizes.max() <= 8
    Uo = oc.unary_table()
    print("oracle: %d of %d entries not finite" % ((~np.isfinite(Uo)).sum(), Uo.size))
    assert np.isfinite(Uo).mean() > 0.99
    U, _ = three_tables(ctx, monkeypatch, inp, "univariate", range_=cases.SMALL_RANGE)
    against_oracle(U, Uo, 1e-10, 1e-12)


def test_pairs_with_one_triangle_twice(ctx, monkeypatch):
    """ico4 / ico2 on the unwarped target, D = 3: neighbouring patch points often fall into one target triangle, so both lanes of a pair name the same record,
    and the multivariate class reads the vertex words alone (the three feature words of the record stay unread) and writes stri / sw3.  On the CPU first:
    the oracle's table (19 x 162) is finite in every entry, with a spread of 0.55."""
    inp = inputs("ico4", 2, D=3)
    oc = oracle_cost(inp, "multivariate")
    oc.get_source_data()
    Uo = oc.unary_table()
    assert np.isfinite(Uo).all() and np.ptp(Uo) > 0.25
    U, _ = three_tables(ctx, monkeypatch, inp, "multivariate")
    against_oracle(U, Uo, 1e-9, 1e-11)
