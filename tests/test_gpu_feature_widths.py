"""Every feature-count route of the multivariate, patchwise and triclique multivariate classes against the oracle, with the route
asserted through DiscreteCostFunction.routes() (msm_cost_routes: what the launchers recorded where they chose the kernel).

unary table (unary_plan.cpp: unary_plan)                        features for D < 12, D > 64 or DICE; mv8 for 12 <= D <= 64 (multivariate);
                                                                pw8<4> for 12 <= D <= 32, pw8<8> for 33 <= D <= 64 (patchwise)
fused fusion move (move_kernels.hip: move_mode)                 fused3 for even D in 12..32, fused2 for even D in 34..64, fused1 otherwise
three-kernel path (clique_kernels.hip: launch_triplet_octets)   octets_sample_mv8 for 12 <= D <= 64 (odd D included), octets_sample otherwise
complete search (MSMHIP_DISABLE_RAYTABLE=1)                     octets_ho

The D values sit on both sides of every threshold and on odd counts inside the lane-group ranges, where the last lane's d < D guard
decides between dropping a dimension and reading past the row.  Tolerance: the project's for these classes, rtol 1e-9 / atol 1e-11, NaN
for NaN (tests/test_gpu_cost_kinds.py)."""
import functools

import numpy as np
import pytest

from newmsm_amd import problem
from tests.helpers import HCP, check_moves, close, move_labelings, oracle_cost

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-11
LAMBDA = 0.0075  # --lambda of the ico3 level of the HCP configuration
MAX_FOLDED = 0.05  # of a move's evaluations; the oracle folds 0.4 to 0.6 % on the shapes below: the similarity is what is compared


@functools.lru_cache(maxsize=4)
def inputs(data_order, cp_order, D, **kw):
    """shared by the cases of one shape (read only)"""
    return problem.pairwise_inputs(data_order, cp_order, D=D, **kw)


def weights(inp, rows, seed):
    return np.random.default_rng(seed).uniform(0.1, 1.0, size=(rows, len(inp["source_xyz"])))


def pair(ctx, inp, kind, w=None, **kw):
    cf, keep = problem.build_cost(ctx, inp, kind=kind, **kw)
    oc = oracle_cost(inp, kind, **kw)
    if w is not None:
        cf.set_dataaffintyweighting(w)
        oc.set_cfweight(w)
    cf.get_source_data()
    oc.get_source_data()
    return cf, oc, keep


# ------------------------------------------------------------------ unary tables: ico4 data, ico2 control grid
def unary_route(kind, D, sim):
    if sim in (4, 5) or D < 12 or D > 64:
        return "features"
    if kind == "multivariate":
        return "mv8"
    return "pw8<4>" if D <= 32 else "pw8<8>"


def check_unary(ctx, kind, D, sim, rows=0, range_=1.0):
    inp = inputs(4, 2, D)
    w = weights(inp, rows, 100 + D) if rows else None
    cf, oc, _ = pair(ctx, inp, kind, w, simmeasure=sim, range_=range_)
    assert cf.routes()["unary"] == "none"
    ptr, idx = cf.patches()
    optr, oidx = oc.patches()
    assert np.array_equal(ptr, optr) and np.array_equal(idx, oidx)
    if rows:
        assert np.array_equal(cf.absolute_weights(), oc.absolute_weights())
    U, Uo = cf.computeUnaryCosts(), oc.unary_table(threads=8)
    assert cf.routes()["unary"] == unary_route(kind, D, sim)
    assert U.shape == Uo.shape == (19, 162)
    assert np.array_equal(np.isnan(U), np.isnan(Uo))
    assert np.allclose(U, Uo, rtol=RTOL, atol=ATOL, equal_nan=True), np.nanmax(np.abs(U - Uo))
    return np.diff(ptr), U


@pytest.mark.parametrize("D", [11, 12, 13, 31, 32, 33, 63, 64, 65])
@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("kind", ["multivariate", "patchwise"])
def test_unary_table_at_every_width(ctx, kind, sim, D):
    """162 control points, patches of 50 to 68 points (no multiple of the 8 lanes of a group), 19 labels: the whole table"""
    sizes, U = check_unary(ctx, kind, D, sim)
    assert sizes.min() == 50 and sizes.max() == 68 and np.isfinite(U).all()


@pytest.mark.parametrize("kind", ["multivariate", "patchwise"])
def test_unary_table_dice_keeps_the_features_kernel(ctx, kind):
    check_unary(ctx, kind, 16, 4)


@pytest.mark.parametrize("D,sim", [(13, 2), (64, 2), (65, 2), (13, 1)])
@pytest.mark.parametrize("rows", ["one", "D"])
@pytest.mark.parametrize("kind", ["multivariate", "patchwise"])
def test_unary_table_with_cost_function_weights(ctx, kind, rows, D, sim):
    """set_dataaffintyweighting with one weight row (used by every dimension: the cfw_rows >= d + 1 rule) and with a row per dimension.
    With D rows the oracle's multivariate table moves by 8 % of its largest entry: a kernel that ignores them fails."""
    check_unary(ctx, kind, D, sim, rows=1 if rows == "one" else D)


@pytest.mark.parametrize("range_", [0.0, 0.12])
@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("kind", ["multivariate", "patchwise"])
def test_unary_table_empty_and_single_point_patches(ctx, kind, sim, range_):
    """the lane-group kernels on patches of no point (range 0) and of the one point the control point sits on (0.12), D = 12"""
    sizes, _ = check_unary(ctx, kind, 12, sim, range_=range_)
    assert sizes.max() == (0 if range_ == 0.0 else 1)


# ------------------------------------------------------------------ the fused fusion move
def move_route(D):
    if D % 2 == 0 and 12 <= D <= 32:
        return "fused3"
    if D % 2 == 0 and 34 <= D <= 64:
        return "fused2"
    return "fused1"


def ho(ctx, inp, sim=2, rows=0):
    w = weights(inp, rows, 200 + inp["D"]) if rows else None
    cf, oc, keep = pair(ctx, inp, "ho_multivariate", w, simmeasure=sim, lambda_=LAMBDA, **HCP)
    assert cf.routes()["move"] == "none"
    ptr, idx = cf.patches()
    optr, oidx = oc.patches()
    assert np.array_equal(ptr, optr) and np.array_equal(idx, oidx)
    if rows:
        assert np.array_equal(cf.absolute_weights(), oc.absolute_weights())
    return cf, oc, np.diff(ptr)


def check_folded(cf, seed):
    for labeling, label in move_labelings(cf, seed):
        assert (cf.tripletOctets(labeling, label) >= 1e6 * LAMBDA).mean() <= MAX_FOLDED


def check_fused(ctx, data_order, cp_order, D, sim=2, rows=0):
    inp = inputs(data_order, cp_order, D)
    cf, oc, bins = ho(ctx, inp, sim, rows)
    check_moves(cf, oc, inp["triplets"], seed=300 + D, full=True)
    check_folded(cf, 300 + D)
    r = cf.routes()
    assert r["move"] == move_route(D) and r["move_tails"] == 0
    return r, bins


@pytest.mark.parametrize("D,sim", [(D, 2) for D in (11, 12, 13, 14, 32, 33, 34, 62, 63, 64, 65, 66)] + [(12, 1), (34, 1), (64, 1)])
def test_fused_move_at_every_width(ctx, D, sim):
    """ico5 / ico3: 1280 control triangles, bins of 3 to 15 points, two control triangles per workgroup, one sampling round"""
    r, bins = check_fused(ctx, 5, 3, D, sim)
    assert len(bins) == 1280 and bins.min() == 3 and bins.max() == 15
    assert r["move_maxtri"] == 2 and r["move_cap"] == 16 and r["move_nblk"] >= 640  # 8 x 16 samples: one round of 256


@pytest.mark.parametrize("D", [13, 32, 34, 64])
def test_fused_move_ragged_second_round(ctx, D):
    """ico5 / ico2: 320 control triangles, bins of 21 to 44 points, one triangle per workgroup; 8 x (more than 32) samples need a second,
    partly filled round of 256"""
    r, bins = check_fused(ctx, 5, 2, D)
    assert len(bins) == 320 and bins.min() == 21 and bins.max() == 44
    assert r["move_maxtri"] == 1 and r["move_cap"] == 44 and r["move_nblk"] == 320


def test_fused_move_mode2_six_triangles_two_rounds_ico6(ctx):
    """ico6 / ico4 with 34 rows: k_ho_move<., 2> at the shape of the last level of the HCP configuration -- six control triangles and 48 bin
    slots per workgroup, two sampling rounds -- one mixed labeling, the whole move"""
    inp = inputs(6, 4, 34)
    cf, oc, bins = ho(ctx, inp)
    assert cf.T == 5120 and cf.L == 19
    labeling, label = move_labelings(cf, 33)[1]
    E, want = cf.tripletOctets(labeling, label), oc.triplet_octets(labeling, label, threads=8)
    assert np.isfinite(E).all() and close(E, want), np.abs(E - want).max()
    folded = want >= 1e6 * LAMBDA
    assert np.array_equal(E >= 1e6 * LAMBDA, folded) and folded.mean() <= MAX_FOLDED
    r = cf.routes()
    assert r["move"] == "fused2" and r["move_maxtri"] == 6 and r["move_cap"] == 48 and r["move_tails"] == 0


@pytest.mark.parametrize("D", [13, 32, 34])
@pytest.mark.parametrize("rows", ["one", "D"])
def test_fused_move_with_cost_function_weights(ctx, rows, D):
    check_fused(ctx, 5, 3, D, rows=1 if rows == "one" else D)


def test_triplet_queries_and_total_cost_d34(ctx):
    """computeTripletCost on random queries (the assertions of test_triclique_likelihood) and evaluateTotalCostSum, the move's `single` form
    (those of test_total_cost_of_the_triclique_classes, with its long label moves: some proposals fold), with 34 rows"""
    inp = inputs(5, 3, 34, labeldist=1.2)
    cf, oc, _ = ho(ctx, inp)
    assert np.array_equal(cf.absolute_weights(), oc.absolute_weights())
    assert np.all(cf.computeUnaryCosts() == 0.0) and cf.routes()["unary"] == "none"
    rng = np.random.default_rng(3)
    t = rng.integers(0, cf.T, 1500).astype(np.int32)
    la, lb, lc = [rng.integers(0, cf.L, 1500).astype(np.int32) for _ in range(3)]
    got = cf.computeTripletCost(t, la, lb, lc)
    want = np.array([oc.triplet(*q) for q in zip(t, la, lb, lc)])
    assert np.isfinite(got).all()
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL), np.max(np.abs(got - want))
    oc.set_pairs(np.zeros((0, 2), dtype=np.int32))
    for labeling in (np.zeros(cf.N, dtype=np.int32), rng.integers(0, cf.L, cf.N).astype(np.int32)):
        tot, parts = cf.evaluateTotalCostSum(labeling)
        assert cf.routes()["move"] == "fused2"
        otot, oparts = oc.total(labeling)
        assert parts[0] == 0.0 and parts[1] == 0.0
        assert abs(parts[2] - oparts[2]) <= 1e-9 * abs(oparts[2]) and abs(tot - otot) <= 1e-9 * abs(otot), (parts, oparts)
        E = cf.tripletOctets(labeling, 3)
        assert abs(parts[2] - E[:, 0].sum()) <= 1e-9 * abs(parts[2])
    assert (E[:, 0] >= 1e6 * LAMBDA).any()  # the random labeling folds some control triangles


def test_complete_search_d34(ctx, monkeypatch):
    """without the direction table the general on-demand kernel evaluates the move: same numbers"""
    monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")  # read when the target's search structures are built
    inp = inputs(5, 3, 34)
    cf, oc, _ = ho(ctx, inp)
    check_moves(cf, oc, inp["triplets"], seed=334, full=True)
    check_folded(cf, 334)
    assert cf.routes()["move"] == "octets_ho"


# ------------------------------------------------------------------ the three-kernel path
@pytest.mark.parametrize("D,rows", [(D, 0) for D in (11, 12, 13, 63, 64, 65)] + [(16, 16)])
def test_three_kernel_path_at_every_width(ctx, D, rows):
    """ico5 / ico1: 80 control triangles with bins of 105 to 150 points, beyond the 128 a workgroup of the fused move holds; at D = 16 with
    a weight row per dimension"""
    inp = inputs(5, 1, D)
    cf, oc, bins = ho(ctx, inp, rows=rows)
    assert len(bins) == 80 and bins.min() == 105 and bins.max() == 150
    check_moves(cf, oc, inp["triplets"], seed=400 + D, full=True)
    check_folded(cf, 400 + D)
    assert cf.routes()["move"] == ("octets_sample_mv8" if 12 <= D <= 64 else "octets_sample")


# ------------------------------------------------------------------ the move's tail kernel
def test_fused_move_star_shaped_target_d34(ctx):
    """a star-shaped target (vertices moved radially by 3e-3, the shape test_non_spherical_star_shaped_targets uses to defeat leaf
    membership): one move with 34 rows, every entry against the oracle (finite everywhere on this input: tests/test_move_fallbacks_cpu.py).  On
    this target some open samples find no candidate in their octree leaf, so the move hands their evaluations (49 of 10 240, measured) to
    k_ho_move_tail.  tests/test_gpu_move_fallbacks.py runs the tail kernel on every route."""
    inp = inputs(5, 3, 34, target_radial=3e-3)
    cf, oc, _ = ho(ctx, inp)
    labeling, label = move_labelings(cf, 534)[1]
    r = cf.routes()
    assert r["move_tails"] == 0 and r["move_deferred"] == 0
    E, want = cf.tripletOctets(labeling, label), oc.triplet_octets(labeling, label, threads=8)
    assert np.isfinite(want).all() and np.isfinite(E).all()
    assert close(E, want), np.abs(E - want).max()
    folded = want >= 1e6 * LAMBDA
    assert np.array_equal(E >= 1e6 * LAMBDA, folded) and folded.mean() <= MAX_FOLDED
    r = cf.routes()
    assert r["move"] == "fused2" and r["move_tails"] == 1 and r["move_deferred"] > 0
