"""k_unary_reduce_rows (csrc/unary_reduce_kernels.hip) and the prepare blocks of the fix-up launch that feed it, on the shapes of
tests/unary_rows_cases.py (tests/test_unary_rows_cpu.py keeps them honest on the oracle): patches of 1 to 101 points, around every size at which a row's
8-lane group, its twelve register slots, the 64-lane statistics or the choice between the two reductions change what runs.

Every table follows tests/test_gpu_unary_pairs.py: computed plainly, without certificates and through the complete sampler, the three equal bit for
bit, each computed twice bit-equal with all 65 fix-up counters zero afterwards (the row kernel clears them as the staged one does), the form asserted
through routes(), and within the suite's bars of the oracle in every entry (rtol 1e-10, atol 1e-12; the oracle's tables are finite everywhere).

tests/golden/unary_rows_parent.npz holds the same tables from the commit before the row form (tools/record_unary_tables.py, on an MI355X): the new
reduction keeps k_unary_reduce_flat's statements in their order, so every table that takes the row form equals its predecessor bit for bit."""
import os

import numpy as np
import pytest

import unary_rows_cases as R

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unary_rows_parent.npz")


@pytest.fixture(scope="module")
def parent_tables():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def table(ctx, name, sim, weighting, sampler="rays"):
    cf = R.product(ctx, name, sim, weighting)
    U = cf.computeUnaryCosts().copy()
    plan, routes = cf.unary_launch(), cf.routes()
    assert plan["sampler"] == sampler and plan["reduce"] == routes["unary"] == "flat"
    assert plan["pmax"] == R.CASES[name][7] and routes["unary_form"] == R.form_of(name)
    assert not cf.unary_fix_counters().any()
    assert np.array_equal(U, cf.computeUnaryCosts())
    assert not cf.unary_fix_counters().any() and cf.routes() == routes
    return U


def three_tables(ctx, monkeypatch, name, sim, weighting):
    plain = table(ctx, name, sim, weighting)
    monkeypatch.setenv("MSMHIP_RAY_CERTS", "off")
    without_certs = table(ctx, name, sim, weighting)
    monkeypatch.delenv("MSMHIP_RAY_CERTS")
    monkeypatch.setenv("MSMHIP_RAYTABLE", "off")
    complete = table(ctx, name, sim, weighting, sampler="samples")
    assert np.array_equal(plain, complete)
    assert np.array_equal(plain, without_certs)
    return plain


@pytest.mark.parametrize("name,sim,weighting", R.all_tables(), ids=[R.key(*t) for t in R.all_tables()])
def test_table(ctx, monkeypatch, parent_tables, name, sim, weighting):
    Uo = R.oracle_table(name, sim, weighting)
    assert np.isfinite(Uo).all()
    U = three_tables(ctx, monkeypatch, name, sim, weighting)
    assert U.shape == Uo.shape
    err = np.abs(U - Uo)
    print("%s: max |table - oracle| = %.3e, form %s" % (R.key(name, sim, weighting), err.max(), R.form_of(name)))
    assert np.allclose(U, Uo, rtol=RTOL, atol=ATOL), err.max()
    if weighting:  # the weights matter
        assert not np.allclose(U, R.oracle_table(name, sim), rtol=1e-3, atol=0)
    if R.form_of(name) == "rows":
        assert np.array_equal(U, parent_tables[R.key(name, sim, weighting)])


def test_the_fixture_holds_every_table(parent_tables):
    assert sorted(parent_tables) == sorted(R.key(*t) for t in R.all_tables())


def test_zero_weight_patches(ctx):
    """`few` with a weight row that is zero on every point of three patches: sw == 0 there, so the means and moments stay undivided (correlation: r = 0,
    half the AbsoluteWeights; SSD: 0) while every other control point divides by its sum of weights"""
    for sim in R.SIMS:
        U = R.product(ctx, "few", sim, "zero").computeUnaryCosts()
        zeroed = U[:, list(R.ZEROED)]
        assert np.allclose(zeroed, R.oracle_table("few", sim, "zero")[:, list(R.ZEROED)], rtol=RTOL, atol=ATOL)
        assert (zeroed > 0.1).all() if sim == 2 else (zeroed == 0).all()
