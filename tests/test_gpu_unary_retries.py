"""k_unary_rays behind a first-candidate miss (csrc/unary_kernels.hip): round A -- the second candidate's planes and the cell's further
candidates in one batch -- round T, in which the wavefront tests the remaining candidates of up to eight unsettled lanes together, eight lanes each, and
runs again while more than eight are unsettled, and the reload of the vertex pieces of what either round accepted.

The targets are warped, so their cells hold the answer at every position of their lists (tests/test_ray_depth_cpu.py); the control grids give patches of
about 65 points (partial last wavefront rounds), about 7 (most lanes of a wavefront idle in round T) and several hundred.  Every decision is the rolled
loop's, so each table is the oracle's within the suite's bars, the same bit for bit through the complete sampler (MSMHIP_RAYTABLE=off: it feeds the same
reduction kernel) and without certificates (MSMHIP_RAY_CERTS=off: 2.3 times as many lanes retry, and wavefronts with more than eight unsettled lanes
occur), and computed twice it is bit-equal with every fix-up counter zero again."""
import numpy as np
import pytest

from newmsm_amd import problem
from ray_retry_cases import GRIDS, inputs
from tests.helpers import oracle_cost

pytestmark = pytest.mark.gpu


def table(ctx, inp, kind, sampler="rays"):
    """the table of a freshly built cost function whose target has its search structures ready, twice: bit-equal, every fix-up counter zero again;
    `sampler`: the sampling kernel the launch plan names (DiscreteCostFunction.unary_launch())"""
    cf, keep = problem.build_cost(ctx, inp, kind=kind)
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)  # (the table is otherwise built in the background, and a first launch may not have it yet)
    U = cf.computeUnaryCosts().copy()
    assert cf.unary_launch()["sampler"] == sampler
    assert not cf.unary_fix_counters().any()
    assert np.array_equal(U, cf.computeUnaryCosts())
    assert not cf.unary_fix_counters().any()
    return U


def three_tables(ctx, monkeypatch, inp, kind):
    plain = table(ctx, inp, kind)
    monkeypatch.setenv("MSMHIP_RAY_CERTS", "off")
    without_certs = table(ctx, inp, kind)
    monkeypatch.delenv("MSMHIP_RAY_CERTS")
    monkeypatch.setenv("MSMHIP_RAYTABLE", "off")
    complete = table(ctx, inp, kind, sampler="samples")
    return plain, without_certs, complete


@pytest.mark.parametrize("target,cp_order", GRIDS, ids=["%s-ico%d" % g for g in GRIDS])
def test_univariate_table_through_both_retry_rounds(ctx, monkeypatch, target, cp_order):
    inp = inputs(target, cp_order, D=1)
    plain, without_certs, complete = three_tables(ctx, monkeypatch, inp, "univariate")
    oc = oracle_cost(inp, "univariate")
    oc.get_source_data()
    sizes = np.diff(oc.patches()[0])
    print(target, cp_order, "patches of", sizes.min(), "to", sizes.max(), "points")
    assert {2: 40 <= sizes.min() and sizes.max() <= 96, 3: sizes.max() <= 8, 1: sizes.min() > 128}[cp_order]  # (50 .. 68, 5 .. 6 and 200 .. 253 points)
    Uo = oc.unary_table()
    assert np.isfinite(Uo).all() and plain.shape == Uo.shape
    print("max |table - oracle| = %.3e" % np.max(np.abs(plain - Uo)))
    assert np.allclose(plain, Uo, rtol=1e-10, atol=1e-12), np.max(np.abs(plain - Uo))
    assert np.array_equal(plain, complete)
    assert np.array_equal(plain, without_certs)


def test_multivariate_table_through_both_retry_rounds(ctx, monkeypatch):
    # D = 3 at ico4 / ico2: the sampler stores (triangle, raw weights) per sample -- the stri / sw3 outputs of a lane settled in round A or round T
    inp = inputs("ico4_warped", 2, D=3)
    plain, without_certs, complete = three_tables(ctx, monkeypatch, inp, "multivariate")
    oc = oracle_cost(inp, "multivariate")
    oc.get_source_data()
    Uo = oc.unary_table()
    assert np.isfinite(Uo).all() and plain.shape == Uo.shape
    assert np.allclose(plain, Uo, rtol=1e-9, atol=1e-11), np.max(np.abs(plain - Uo))
    assert np.array_equal(plain, complete) and np.array_equal(plain, without_certs)
