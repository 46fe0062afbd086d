"""What the similarity kernels do at the edges of the measure: the degenerate-input cases of tests/similarity_edge_cases.py (exact-zero caps,
zero and dyadic weights, power-of-two weight sums, zero-weight patches, NaN vertices) through every route of DESIGN.md section 5.3 and both lane
widths of k_group_pairwise, against the oracle.  tests/test_similarity_edges_cpu.py shows on the oracle alone that the cases reach the
reference's two branches (`sum > 0`, `varA == 0 || varB == 0`, M/similarities.cpp:129-158).

Assertions: NaN where the oracle has NaN; the project's tolerances for the class (rtol 1e-10 / atol 1e-12 for the univariate unary table, rtol
1e-9 / atol 1e-11 for everything else); and bit for bit the oracle's entry wherever that entry is exactly the degenerate value -- 0.5 *
AbsoluteWeights for correlation tables, 0 for SSD tables and weight-0 columns, 0.5 (correlation) or 0 (SSD) for the group pair costs.  With
exact-zero inputs every sum is exact in any order, so bit equality is the contract there: it catches a kernel that takes the other branch and
happens to land within the tolerance.  A fusion move's entries carry the strain term, which is not bit-exact; the fused `cap` cases are
therefore run a second time with lambda = 0, where an entry is the likelihood alone and the degenerate value is 0.5 * (the mean of the three
AbsoluteWeights)."""
import functools

import numpy as np
import pytest

import similarity_edge_cases as C
from helpers import check_moves, close, move_labelings, oracle_cost
from newmsm_amd import problem

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-11
MAX_FOLDED = 0.05  # of a move's evaluations, as tests/test_gpu_feature_widths.py: the similarity is what is compared


def pair(ctx, inp, kind, w=None, **kw):
    cf, keep = problem.build_cost(ctx, inp, kind=kind, **kw)
    oc = oracle_cost(inp, kind, **kw)
    if w is not None:
        cf.set_dataaffintyweighting(w)
        oc.set_cfweight(w)
    cf.get_source_data()
    oc.get_source_data()
    ptr, idx = cf.patches()
    optr, oidx = oc.patches()
    assert np.array_equal(ptr, optr) and np.array_equal(idx, oidx)
    assert np.array_equal(cf.absolute_weights(), oc.absolute_weights())
    return cf, oc, keep


# ------------------------------------------------------------------ unary tables: ico4 data, ico2 control grid
def unary_route(kind, D):
    if kind == "univariate":
        return "flat"
    if D < 12 or D > 64:
        return "features"
    if kind == "multivariate":
        return "mv8"
    return "pw8<4>" if D <= 32 else "pw8<8>"


def check_unary(ctx, kind, D, case, sim):
    inp, w = C.case_inputs(C.base(4, 2, D), case)
    cf, oc, _ = pair(ctx, inp, kind, w, simmeasure=sim)
    assert cf.routes()["unary"] == "none"
    U, Uo = cf.computeUnaryCosts(), oc.unary_table(threads=8)
    assert cf.routes()["unary"] == unary_route(kind, D)
    assert U.shape == Uo.shape == (19, 162)
    assert np.array_equal(np.isnan(U), np.isnan(Uo))
    rtol, atol = (1e-10, 1e-12) if kind == "univariate" else (RTOL, ATOL)
    assert np.allclose(U, Uo, rtol=rtol, atol=atol, equal_nan=True), np.nanmax(np.abs(U - Uo))
    absw = oc.absolute_weights()
    deg = C.degenerate_unary(Uo, absw, sim) | (absw == 0.0)[None, :]
    assert np.array_equal(U[deg], Uo[deg]), (int(deg.sum()), np.abs(U[deg] - Uo[deg]).max())
    if case == "nan":
        assert np.isnan(Uo).any()
    elif case.startswith("cap"):
        assert np.isfinite(U).all() and deg.mean() >= C.FLOOR
    else:
        assert np.isfinite(U).all()
    return U, absw


@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("case", ["cap", "cap_zero_weights", "nan"])
@pytest.mark.parametrize("search", ["raytable", "complete"])
def test_univariate_table(ctx, monkeypatch, search, case, sim):
    """the wavefront patch_similarity behind both search paths"""
    if search == "complete":
        monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")  # read when the target's search structures are built
    check_unary(ctx, "univariate", 1, case, sim)


@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("case", ["cap", "cap_zero_weights", "nan"])
@pytest.mark.parametrize("D", [2, 13, 32, 34, 64, 65])
@pytest.mark.parametrize("kind", ["multivariate", "patchwise"])
def test_feature_tables_at_every_route(ctx, kind, D, case, sim):
    """features (D = 2, 65), mv8 / pw8<4> (13, 32), mv8 / pw8<8> (34, 64)"""
    check_unary(ctx, kind, D, case, sim)


@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("case", ["pow2_sum", "pow2_sum_small"])
@pytest.mark.parametrize("kind", ["multivariate", "patchwise"])
def test_feature_tables_with_power_of_two_weight_sums(ctx, kind, case, sim):
    """D = 34, weights of 1 (or 2^-10) with two zero rows: div_exact multiplies by the reciprocal of 32 (2^-5), zero-weight lanes in the group"""
    check_unary(ctx, kind, 34, case, sim)


@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("kind", ["multivariate", "patchwise"])
def test_feature_tables_with_zero_weight_patches(ctx, kind, sim):
    """D = 13, one weight row that is 0 on a cap: AbsoluteWeights 0 there, and those columns exactly 0 (not 0 * NaN)"""
    U, absw = check_unary(ctx, kind, 13, "weight_cap", sim)
    zero = absw == 0.0
    assert zero.mean() >= C.FLOOR and (U[:, zero] == 0.0).all() and (U[:, ~zero] != 0.0).all()


@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("search", ["raytable", "complete"])
def test_univariate_table_with_zero_weight_patches(ctx, monkeypatch, search, sim):
    """the same row on the univariate table: 9.3 % of the patches have weights that sum to exactly 0 (the false side of patch_similarity's
    `sum > 0`; cap_zero_weights has zero-weight points in every patch but no such patch), AbsoluteWeights 0 at 11.7 % of the control points"""
    if search == "complete":
        monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")  # read when the target's search structures are built
    U, absw = check_unary(ctx, "univariate", 1, "weight_cap", sim)
    zero = absw == 0.0
    assert zero.mean() >= C.FLOOR and (U[:, zero] == 0.0).all() and (U[:, ~zero] != 0.0).all()


# ------------------------------------------------------------------ the fusion move
def move_route(D):
    if D % 2 == 0 and 12 <= D <= 32:
        return "fused3"
    if D % 2 == 0 and 34 <= D <= 64:
        return "fused2"
    return "fused1"


def ho(ctx, order, D, case, sim=2, lam=C.LAMBDA):
    inp, w = C.case_inputs(C.base(order[0], order[1], D), case)
    cf, oc, _ = pair(ctx, inp, "ho_univariate" if D == 1 else "ho_multivariate", w, simmeasure=sim, lambda_=lam, **C.HCP)
    assert cf.routes()["move"] == "none"
    return inp, cf, oc


def check_move(ctx, order, D, case, route, sim=2, seed=None):
    """both labelings of move_labelings, the whole move, against the oracle's replay"""
    inp, cf, oc = ho(ctx, order, D, case, sim)
    seed = 300 + D if seed is None else seed
    if case == "nan":
        for labeling, label in move_labelings(cf, seed):
            E, want = cf.tripletOctets(labeling, label), oc.triplet_octets(labeling, label, threads=8)
            assert np.isnan(want).any() and np.array_equal(np.isnan(E), np.isnan(want)) and not np.isinf(E).any()
            assert close(E, want), np.nanmax(np.abs(E - want))
            assert np.array_equal(E >= 1e6 * C.LAMBDA, want >= 1e6 * C.LAMBDA)
    else:
        check_moves(cf, oc, inp["triplets"], seed=seed, full=True)
    for labeling, label in move_labelings(cf, seed):
        assert (cf.tripletOctets(labeling, label) >= 1e6 * C.LAMBDA).mean() <= MAX_FOLDED
    r = cf.routes()
    assert r["move"] == route and r["move_tails"] == 0
    return r, oc


def check_likelihood_bits(ctx, order, D, case, route, sim=2):
    """lambda = 0: an entry is the likelihood alone (folded triangles: 0), and where the oracle's is the degenerate value -- the bin or its samples
    inside a cap, or a bin whose weights sum to 0 -- the move's is the same bit for bit.  weight_cap: where the three AbsoluteWeights are 0 as
    well the entry is exactly 0, not 0 * NaN"""
    inp, cf, oc = ho(ctx, order, D, case, sim, lam=0.0)
    absw = oc.absolute_weights()
    t = inp["triplets"]
    weight = (absw[t[:, 0]] + absw[t[:, 1]] + absw[t[:, 2]]) / 3.0
    deg_value = 0.5 * weight if sim == 2 else np.zeros(len(t))
    for labeling, label in move_labelings(cf, 300 + D):
        E, want = cf.tripletOctets(labeling, label), oc.triplet_octets(labeling, label, threads=8)
        deg = want == deg_value[:, None]
        assert deg.mean() >= C.FLOOR and np.array_equal(E[deg], want[deg]), np.abs(E[deg] - want[deg]).max()
        assert np.isfinite(E).all() and close(E, want), np.abs(E - want).max()
        if case == "weight_cap" and order == (5, 3):
            assert (weight == 0.0).mean() >= C.FLOOR and (E[weight == 0.0] == 0.0).all()
    assert cf.routes()["move"] == route


@pytest.mark.parametrize("case", ["cap", "cap_binary_row"])
def test_fused_move_univariate(ctx, case):
    """ico5 / ico3, fused0: move_likelihood's `varA == 0` on bins inside the cap, without weights and with a binary weight row (10 % zeros: zero-weight
    points in a bin, but no bin whose weights sum to 0)"""
    check_likelihood_bits(ctx, (5, 3), 1, case, "fused0")
    check_move(ctx, (5, 3), 1, case, "fused0")


@pytest.mark.parametrize("sim", [2, 1])
def test_fused_move_univariate_zero_weight_bins(ctx, sim):
    """ico5 / ico3, fused0, one weight row that is 0 below z = -60 on smooth data: 18.7 % of the bins have weights that sum to exactly 0 -- the
    false side of `sum > 0` in k_move_prepare and move_likelihood -- and 13.3 % of the control triangles AbsoluteWeights 0 at all three corners"""
    check_likelihood_bits(ctx, (5, 3), 1, "weight_cap", "fused0", sim=sim)
    check_move(ctx, (5, 3), 1, "weight_cap", "fused0", sim=sim)


@pytest.mark.parametrize("case", ["cap", "cap_zero_weights"])
@pytest.mark.parametrize("D", [13, 32, 34])
def test_fused_move_multivariate(ctx, D, case):
    """ico5 / ico3: fused1 (13), fused3 (32), fused2 (34); one sampling round"""
    check_likelihood_bits(ctx, (5, 3), D, case, move_route(D))
    r, _ = check_move(ctx, (5, 3), D, case, move_route(D))
    assert r["move_maxtri"] == 2 and r["move_cap"] == 16


@pytest.mark.parametrize("D,sim", [(32, 1), (34, 1)])
def test_fused_move_ssd_on_the_cap(ctx, D, sim):
    check_likelihood_bits(ctx, (5, 3), D, "cap", move_route(D), sim=sim)
    check_move(ctx, (5, 3), D, "cap", move_route(D), sim=sim)


@pytest.mark.parametrize("case", ["pow2_sum", "pow2_sum_small"])
def test_fused_move_with_power_of_two_weight_sums(ctx, case):
    """on smooth data, and (lambda = 0, bit for bit) on the cap"""
    check_likelihood_bits(ctx, (5, 3), 34, "cap_" + case, "fused2")
    check_move(ctx, (5, 3), 34, case, "fused2")


def test_fused_move_with_nan_vertices_d32(ctx):
    check_move(ctx, (5, 3), 32, "nan", "fused3")


def test_fused_move_two_sampling_rounds_d34(ctx):
    """ico5 / ico2: bins of 21 to 44 points, one control triangle per workgroup, a second partly filled round"""
    check_likelihood_bits(ctx, (5, 2), 34, "cap", "fused2")
    r, _ = check_move(ctx, (5, 2), 34, "cap", "fused2")
    assert r["move_maxtri"] == 1 and r["move_cap"] == 44


@pytest.mark.parametrize("D,case,route", [(11, "cap", "octets_sample"), (16, "cap_zero_weights", "octets_sample_mv8"), (1, "weight_cap", "octets_sample")])
def test_three_kernel_path(ctx, D, case, route):
    """ico5 / ico1: bins of 105 to 150 points; D = 1: the univariate class off the fused path (ho_likelihood_core, the serial restatement of the two
    decisions), 7.5 % of its bins with weights that sum to 0"""
    check_likelihood_bits(ctx, (5, 1), D, case, route)
    _, oc = check_move(ctx, (5, 1), D, case, route)
    bins = np.diff(oc.patches()[0])
    assert bins.min() == 105 and bins.max() == 150


@pytest.mark.parametrize("D,case", [(34, "cap"), (1, "cap"), (1, "weight_cap")])
def test_complete_search(ctx, monkeypatch, D, case):
    """k_triplet_octets_ho; D = 1: ho_likelihood_core on bins inside the cap and on bins whose weights sum to 0"""
    monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")  # read when the target's search structures are built
    check_likelihood_bits(ctx, (5, 3), D, case, "octets_ho")
    check_move(ctx, (5, 3), D, case, "octets_ho")


# ------------------------------------------------------------------ gMSM pair costs
@functools.lru_cache(maxsize=None)
def group_oracle(mask, sim, S=3, cp_order=2, n=1500):
    """the oracle's side of a group case, shared by the lane widths (read only)"""
    og, keep = C.oracle_group(C.group_parts(mask, S, cp_order), sim)
    want = og.pairwise_batch(*C.group_queries(og.P, og.L, n), threads=8)
    want.setflags(write=False)
    return og, keep, want


def assert_pair_costs(got, want, sim):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True), np.nanmax(np.abs(got - want))
    deg = want == (0.5 if sim == 2 else 0.0)
    assert np.array_equal(got[deg], want[deg]), np.abs(got[deg] - want[deg]).max()
    return deg


@pytest.mark.parametrize("lanes", [None, 16, 32])
@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("mask", C.GROUP_MASKS)
def test_group_pair_costs(ctx, monkeypatch, mask, sim, lanes):
    """S = 3, ico4 / ico2, D = 2, every subject's data exactly 0 above the cap; a quarter and half a wavefront per pair cost, and the default.
    A template mask of all zeros: every common entry has weight 0, the oracle gives 0.5 (correlation) or 0 (SSD) everywhere."""
    if lanes is not None:
        monkeypatch.setenv("MSMHIP_GROUP_PAIR_LANES", str(lanes))  # read when the set-up is finalised
    og, _, want = group_oracle(mask, sim)
    g, _ = C.product_group(ctx, C.group_parts(mask), sim)
    assert (g.P, g.L) == (og.P, og.L) and np.array_equal(g.getPairs(), og.pairs())
    deg = assert_pair_costs(g.computePairwiseCost(*C.group_queries(g.P, g.L)), want, sim)
    assert np.isfinite(want).all() and deg.mean() >= C.FLOOR and (mask != "zeros" or deg.all())


@pytest.mark.parametrize("lanes", [16, 32])
@pytest.mark.parametrize("sim", [2, 1])
def test_group_pair_costs_of_long_patches(ctx, monkeypatch, sim, lanes):
    """S = 2 under an ico1 control grid, binary mask: patches of 195 to 249 template vertices, beyond the 80 | 128 entries the butterfly keeps in
    registers -- the scalar tail of k_group_pairwise<false, 16 | 32>"""
    monkeypatch.setenv("MSMHIP_GROUP_PAIR_LANES", str(lanes))
    og, _, want = group_oracle("binary", sim, 2, 1, 600)
    g, _ = C.product_group(ctx, C.group_parts("binary", 2, 1), sim)
    assert min(len(g.patch(s, v, l)[0]) for s in range(2) for v in (0, 20, 41) for l in (0, 5)) > 128
    deg = assert_pair_costs(g.computePairwiseCost(*C.group_queries(g.P, g.L, 600)), want, sim)
    assert np.isfinite(want).all() and deg.mean() >= C.FLOOR


@pytest.mark.parametrize("lanes", [16, 32])
def test_group_fusion_move_binary_mask(ctx, monkeypatch, lanes):
    """one label step on the binary-mask case: the four pair costs of every pair and the eight triplet costs of every triplet"""
    monkeypatch.setenv("MSMHIP_GROUP_PAIR_LANES", str(lanes))
    og, _, _ = group_oracle("binary", 2)
    g, _ = C.product_group(ctx, C.group_parts("binary"), 2)
    labeling, label = np.random.default_rng(5).integers(0, g.L, g.num_nodes).astype(np.int32), 7
    quads, octets = g.fusionMove(labeling, label)
    pairs, trips = og.pairs(), og.triplets()
    p, k = np.repeat(np.arange(og.P, dtype=np.int32), 4), np.tile(np.arange(4), og.P)
    la = np.where(k & 2, label, labeling[pairs[p, 0]]).astype(np.int32)
    lb = np.where(k & 1, label, labeling[pairs[p, 1]]).astype(np.int32)
    deg = assert_pair_costs(quads.ravel(), og.pairwise_batch(p, la, lb, threads=8), 2)
    assert deg.mean() >= C.FLOOR
    t, k = np.repeat(np.arange(og.T, dtype=np.int32), 8), np.tile(np.arange(8), og.T)
    lab3 = [np.where(k >> (2 - j) & 1, label, labeling[trips[t, j]]).astype(np.int32) for j in range(3)]
    want = og.triplet_batch(t, *lab3, threads=8)
    assert np.allclose(octets.ravel(), want, rtol=RTOL, atol=ATOL), np.abs(octets.ravel() - want).max()
