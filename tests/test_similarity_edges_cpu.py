"""The degenerate-input cases of tests/similarity_edge_cases.py on the oracle alone, no GPU: each case must reach the branch it is named for
(`sum > 0` and `varA == 0 || varB == 0` of sparsesimkernel::corr, M/similarities.cpp:129-158), so that tests/test_gpu_similarity_edges.py
cannot pass by accident.  FLOOR (0.05) is a condition, about half of what the oracle gives; the measured shares are in the docstrings."""
import types

import numpy as np
import pytest

import similarity_edge_cases as C
from helpers import move_labelings, oracle_cost

SIMS = [2, 1]


def table(kind, D, case, sim):
    inp, w = C.case_inputs(C.base(4, 2, D), case)
    oc = oracle_cost(inp, kind, simmeasure=sim)
    if w is not None:
        oc.set_cfweight(w)
    oc.get_source_data()
    U = oc.unary_table(threads=8)
    assert U.shape == (19, 162)
    return U, oc.absolute_weights()


def test_cap_covers_a_fifth_of_both_meshes():
    """z > 60 on the ico4 sphere: 20.3 % of the vertices"""
    inp = C.base(4, 2, 2)
    assert 0.19 < C.source_cap(inp).mean() < 0.22 and 0.19 < (inp["target_xyz"][:, 2] > C.CAP_Z).mean() < 0.22
    c = C.cap(inp)
    assert (c["src_feat"][:, C.source_cap(inp)] == 0.0).all() and (c["src_feat"][:, ~C.source_cap(inp)] != 0.0).all()


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("case", ["cap", "cap_zero_weights"])
@pytest.mark.parametrize("kind,D", [("univariate", 1), ("multivariate", 2), ("multivariate", 13), ("multivariate", 34), ("multivariate", 65),
                                    ("patchwise", 2), ("patchwise", 13), ("patchwise", 34), ("patchwise", 65)])
def test_unary_cases_reach_the_degenerate_value(kind, D, case, sim):
    """ico4 / ico2, 19 x 162 table, every entry finite.  Share of entries that are bit for bit 0.5 * AbsoluteWeights (correlation) / 0 (SSD):
    cap 0.103 / 0.083 for every class at D = 1, 13, 34, 65 (multivariate D = 2: 0.105 / 0.083); cap + zero_weights 0.103 to 0.108 / 0.083 to
    0.086 (largest at D = 65)."""
    U, absw = table(kind, D, case, sim)
    assert np.isfinite(U).all() and (absw > 0).all()
    assert C.degenerate_unary(U, absw, sim).mean() >= C.FLOOR


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("case", ["pow2_sum", "pow2_sum_small"])
@pytest.mark.parametrize("kind", ["multivariate", "patchwise"])
def test_pow2_weight_sums_are_finite(kind, case, sim):
    """D = 34 with two zero rows: a vertex's weights sum to 32 or 2^-5; AbsoluteWeights is the weight resampled (the same up to rounding)"""
    U, absw = table(kind, 34, case, sim)
    assert np.isfinite(U).all() and np.allclose(absw, 1.0 if case == "pow2_sum" else 2.0 ** -10, rtol=1e-12, atol=0)


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("kind", ["multivariate", "patchwise"])
def test_weight_cap_zeroes_whole_columns(kind, sim):
    """AbsoluteWeights is 0 at 0.117 of the control points; exactly those columns of the table are 0 (not 0 * NaN), no other entry is"""
    U, absw = table(kind, 13, "weight_cap", sim)
    zero = absw == 0.0
    assert np.isfinite(U).all() and zero.mean() >= C.FLOOR
    assert np.array_equal((U == 0.0).all(axis=0), zero) and (U[:, ~zero] != 0.0).all()


@pytest.mark.parametrize("sim", SIMS)
def test_weight_cap_zeroes_whole_patches_of_the_univariate_table(sim):
    """D = 1: the weights of 0.093 of the 162 patches sum to exactly 0 (with cap_zero_weights none does), AbsoluteWeights is 0 at 0.117 of the
    control points, and exactly those columns are 0"""
    inp, w = C.case_inputs(C.base(4, 2, 1), "weight_cap")
    oc = oracle_cost(inp, "univariate", simmeasure=sim)
    oc.set_cfweight(w)
    oc.get_source_data()
    assert C.bins_inside(*oc.patches(), w[0] == 0.0) >= C.FLOOR
    U, zero = oc.unary_table(threads=8), oc.absolute_weights() == 0.0
    assert np.isfinite(U).all() and zero.mean() >= C.FLOOR and np.array_equal((U == 0.0).all(axis=0), zero)
    ptr, idx = oc.patches()
    assert C.bins_inside(ptr, idx, C.zero_weights(inp)[0] == 0.0) == 0.0


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("order", [(5, 3), (5, 1)])
def test_move_bins_of_weight_zero(order, sim):
    """the univariate triclique class with weight_cap's row on smooth data.  ico5 / ico3: the weights of 0.187 of the 1280 bins sum to exactly 0
    (the false side of `sum > 0`), 0.133 of the control triangles have AbsoluteWeights 0 at all three corners; ico5 / ico1: 0.075 of the 80 bins,
    no such triangle.  The binary row of cap_binary_row (10 % independent zeros) zeroes no bin at all.  With lambda = 0 every octet is finite, and
    the share that is exactly 0.5 * (mean AbsoluteWeights) (correlation) / 0 (SSD) is 0.192 / 0.187 at ico3 and 0.075 at ico1."""
    inp, w = C.case_inputs(C.base(order[0], order[1], 1), "weight_cap")
    oc = oracle_cost(inp, "ho_univariate", simmeasure=sim, lambda_=0.0, **C.HCP)
    oc.set_cfweight(w)
    oc.get_source_data()
    ptr, idx = oc.patches()
    assert C.bins_inside(ptr, idx, w[0] == 0.0) >= C.FLOOR and C.bins_inside(ptr, idx, C.binary_row(inp)[0] == 0.0) == 0.0
    absw, t = oc.absolute_weights(), inp["triplets"]
    weight = (absw[t[:, 0]] + absw[t[:, 1]] + absw[t[:, 2]]) / 3.0
    for labeling, label in move_labelings(types.SimpleNamespace(N=oc.N, L=oc.L), 301):
        E = oc.triplet_octets(labeling, label, threads=8)
        assert np.isfinite(E).all() and (E == (0.5 * weight if sim == 2 else 0.0 * weight)[:, None]).mean() >= C.FLOOR
        assert (E[weight == 0.0] == 0.0).all() and (order != (5, 3) or (weight == 0.0).mean() >= C.FLOOR)


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("kind,D", [("univariate", 1), ("multivariate", 2), ("multivariate", 32), ("patchwise", 13)])
def test_nan_case_marks_a_part_of_the_table(kind, D, sim):
    """two NaN target vertices and two NaN source vertices: 0.102 of the entries NaN for univariate, 0.108 for the other classes (five and
    five gave 0.24)"""
    U, _ = table(kind, D, "nan", sim)
    assert 0.02 <= np.isnan(U).mean() <= 0.5 and not np.isinf(U).any()


@pytest.mark.parametrize("kind,D,case", [("ho_multivariate", 12, "cap"), ("ho_univariate", 1, "cap_binary_row")])
def test_move_bins_lie_inside_the_cap(kind, D, case):
    """the `varA == 0` branch (test_move_bins_of_weight_zero has the `sum > 0` one).  ico5 / ico3: 0.189 of the 1280 control triangles have every
    bin point inside the source cap (ico5 / ico2: 0.163 of 320, ico5 / ico1: 0.075 of 80), so their likelihood is the degenerate one at every label.  Both labelings of move_labelings give finite octets, about 1 % folded at
    the most (measured: 0 and 1.01 % at D = 12, 0 and 0.28 % univariate)."""
    inp, w = C.case_inputs(C.base(5, 3, D), case)
    oc = oracle_cost(inp, kind, lambda_=C.LAMBDA, **C.HCP)
    if w is not None:
        oc.set_cfweight(w)
    oc.get_source_data()
    assert C.bins_inside(*oc.patches(), C.source_cap(inp)) >= C.FLOOR
    for order in ((5, 2, 34), (5, 1, 11)):
        other = C.base(*order)
        o2 = oracle_cost(other, "ho_multivariate", lambda_=C.LAMBDA, **C.HCP)
        o2.get_source_data()
        assert C.bins_inside(*o2.patches(), C.source_cap(other)) >= C.FLOOR
    for labeling, label in move_labelings(types.SimpleNamespace(N=oc.N, L=oc.L), 300 + D):
        E = oc.triplet_octets(labeling, label, threads=8)
        assert np.isfinite(E).all() and (E >= 1e6 * C.LAMBDA).mean() <= 0.05  # (the bar of tests/test_gpu_feature_widths.py)


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("mask", C.GROUP_MASKS)
def test_group_pair_costs_reach_the_degenerate_value(mask, sim):
    """1 500 random (pair, label, label) queries, all finite.  Share equal to 0.5 (correlation) / 0 (SSD): no mask 0.105 / 0.080, binary mask
    0.285 / 0.248, a mask of zeros 1 / 1 (every common entry has weight 0: the reference divides by nothing)."""
    og, _ = C.oracle_group(C.group_parts(mask), sim)
    want = og.pairwise_batch(*C.group_queries(og.P, og.L), threads=8)
    share = (want == (0.5 if sim == 2 else 0.0)).mean()
    assert np.isfinite(want).all() and share >= C.FLOOR and (mask != "zeros" or share == 1.0)


@pytest.mark.parametrize("sim", SIMS)
def test_group_long_patches_reach_the_degenerate_value(sim):
    """S = 2 under an ico1 control grid, binary mask (patches of 195 to 249 template vertices): 600 queries, all finite, 0.147 equal to 0.5
    (correlation) / 0.108 equal to 0 (SSD)"""
    og, _ = C.oracle_group(C.group_parts("binary", 2, 1), sim)
    want = og.pairwise_batch(*C.group_queries(og.P, og.L, 600), threads=8)
    sizes = [len(og.patch(s, v, l)[0]) for s in range(2) for v in (0, 20, 41) for l in (0, 5)]
    assert min(sizes) > 128 and np.isfinite(want).all() and (want == (0.5 if sim == 2 else 0.0)).mean() >= C.FLOOR
