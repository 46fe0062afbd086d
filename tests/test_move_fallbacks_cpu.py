"""The star-shaped cases of tests/move_fallback_cases.py on the oracle and the host entry points alone, no GPU: the direction table is built on
every target (so the fused route applies), the oracle is finite in every entry (so tests/test_gpu_move_fallbacks.py compares every entry and a
tail kernel that returned NaN could not hide behind a NaN of the oracle), and little of a move folds (so the similarity is what is compared).
MAX_FOLDED is a condition; the measured shares are in the docstrings."""
import numpy as np
import pytest

import move_fallback_cases as C
from newmsm_amd import api
from helpers import oracle_cost

FOLD = 1e6 * C.LAMBDA  # a folded proposal costs MSM_FOLDING * lambda = 1e7 * lambda


@pytest.mark.parametrize("shape,radial", [(C.MOVE_SHAPE, C.RADIAL), (C.BIG_BIN_SHAPE, C.RADIAL), ((5, 3), 3e-3), ((5, 3), 1e-4)])
def test_direction_table_is_built_on_every_target(shape, radial):
    """the ico4 and ico5 data spheres at RADIAL, and ico5 at the amplitudes of test_fused_move_star_shaped_target_d34 and
    test_non_spherical_star_shaped_targets: simple surfaces, no violation of the table's guarantee at 20 000 points"""
    inp = C.star(shape, 1, None, radial)
    rep = api.ray_table_check(inp["target_xyz"], inp["target_tri"])
    assert rep["simple"] and rep["violations"] == 0 and rep["points"] == 20000


@pytest.mark.parametrize("case,kw", C.move_cases(), ids=["-".join(str(x) for x in case + tuple(kw)) for case, kw in C.move_cases()])
def test_moves_are_finite_and_fold_little(case, kw):
    """both labelings of labelings() and the label that drops a prefetch: every octet finite.  Folded share (all-zero labeling / mixed / mixed with the
    other label), measured, the same for every class, measure and weight matrix of a shape: ico4 / ico2 0.0004 / 0.0273 / 0.0254, with 277 labels
    0 / 0.0223 / 0.0133, ico5 / ico1 0 / 0.0125 / 0.0094."""
    oc = C.oracle(*case, **kw)
    assert oc.T == (80 if kw.get("shape") == C.BIG_BIN_SHAPE else 320) and (oc.L > 256) == ("sg_order" in kw)
    for which in (0, 1, 2):
        E = C.octets(which, *case, **kw)
        assert E.shape == (oc.T, 8) and np.isfinite(E).all() and (E >= FOLD).mean() <= C.MAX_FOLDED


@pytest.mark.parametrize("kind,D,route", C.SINGLE)
def test_totals_are_finite(kind, D, route):
    """evaluateTotalCostSum's labelings: finite sums; 0 of the 320 control triangles fold under the all-zero labeling, 3 under the random one"""
    oc = C.oracle(kind, D)
    for labeling in C.total_labelings(oc.N, oc.L):
        tot, parts = oc.total(labeling)
        assert np.isfinite(tot) and np.isfinite(parts).all() and parts[0] == 0.0 and parts[1] == 0.0
        E = oc.triplet_octets(labeling, 3, threads=8)
        assert np.isfinite(E).all() and (E[:, 0] >= FOLD).mean() <= C.MAX_FOLDED


@pytest.mark.parametrize("kind,D,route", C.UNARY)
def test_unary_tables_are_finite(kind, D, route):
    """the 19 x 162 tables of the multivariate and patchwise classes on the ico4 star-shaped target"""
    _, U = C.unary_oracle(kind, D)
    assert U.shape == (19, 162) and np.isfinite(U).all()


def test_existing_star_shaped_cases_are_finite():
    """what tests/test_gpu_feature_widths.py::test_fused_move_star_shaped_target_d34 (ico5 / ico3, 34 rows, 3e-3, the mixed labeling: 0.0154 folded) and
    tests/test_gpu_unary.py::test_non_spherical_star_shaped_targets (the univariate table at 1e-4 and 3e-3) compare against: finite in every entry"""
    oc = C.oracle("ho_multivariate", 34, shape=(5, 3), radial=3e-3)
    labeling, label = C.labelings(oc.N, oc.L)[1]
    E = oc.triplet_octets(labeling, label, threads=8)
    assert E.shape == (1280, 8) and np.isfinite(E).all() and (E >= FOLD).mean() <= C.MAX_FOLDED
    for radial in (1e-4, 3e-3):
        ou = oracle_cost(C.star((5, 3), 1, None, radial), "univariate")
        ou.get_source_data()
        assert np.isfinite(ou.unary_table(threads=8)).all()
