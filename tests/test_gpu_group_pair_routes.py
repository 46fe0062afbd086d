"""k_group_pairwise on every route it can take by patch size and feature rows, against a literal of computePairwiseCost.

The crafted groups of tests/group_pair_cases.py put patches on and beside every threshold of the kernel (lanes per query,
the register path and the length of its search, staged or unstaged ids of B, the membership bits, pval / dir or gathers from F, D = 1 / 2 / >= 3,
the DICE launch's LDS); tests/test_group_pairs_cpu.py shows on the CPU that they do and that the literal is the oracle's group.  Bars: those of
tests/test_gpu_group.py, NaN for NaN, exact where the literal gives exactly 0.5 (correlation) or 0 (SSD), exact for DICE.  Measured on an MI355X:
the largest relative difference of any route is 4.2e-15 (correlation, unstaged general path) and 1.6e-15 for SSD, the largest absolute one 2.2e-16;
DESIGN.md section 5.6 has the figure of every route (test_every_query_of_the_threshold_group prints them before it asserts)."""
import numpy as np
import pytest

import group_pair_cases as C
import newmsm_amd as M
from test_gpu_group import ATOL, RTOL, build

pytestmark = pytest.mark.gpu
MSM_ERR_CAPACITY = -7


def table(g):
    """every (pair, label A, label B) of the group through the explicit batch: P x L x L"""
    return g.computePairwiseCost(*C.all_queries()).reshape(C.P, C.L, C.L)


def assert_against_literal(got, ref, sim, names=None, tag=None):
    """got: all 15 162 costs; ref: C.reference().  Prints the largest relative difference per route before it asserts."""
    want, skip = ref["want"], ref["unstable"]
    got = got.ravel()
    ok = np.isfinite(want) & ~skip
    rel = np.zeros(len(want))
    rel[ok] = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
    rel[ok & (got == want)] = 0.0
    if names is not None:
        for name in sorted(set(names.tolist())):
            sel = ok & (names == name)
            print("PAIR-ROUTE-DIFF %s %-16s queries %5d  max rel %.3e  max abs %.3e" % (tag, name, sel.sum(), rel[sel].max() if sel.any() else 0.0,
                                                                                       np.abs(got[sel] - want[sel]).max() if sel.any() else 0.0))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.allclose(got[ok], want[ok], rtol=RTOL, atol=ATOL), np.abs(got[ok] - want[ok]).max()
    deg = ok & (want == (0.5 if sim == 2 else 0.0))
    assert np.array_equal(got[deg], want[deg]), np.abs(got[deg] - want[deg]).max()
    return deg


@pytest.mark.parametrize("mask", ["none", "dyadic"])
@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("lanes", [16, 32])
def test_every_query_of_the_threshold_group(ctx, monkeypatch, lanes, D, sim, mask):
    """All 42 x 19 x 19 queries: fast64 / fast128 / fast256 (D <= 2), staged and unstaged general path with and without entries beyond the membership
    bits, empty intersections and intersections of one and two entries.  Right after finalize() an imported group has no value copies: the register
    path runs in its gather form here (the compact form: test_gather_and_compact_forms).  fixnan: the same costs, 1e7 for the empty intersections."""
    monkeypatch.setenv("MSMHIP_GROUP_PAIR_LANES", str(lanes))
    ref = C.reference("thresholds", D, sim, mask)
    g, _ = C.product_group(ctx, "thresholds", D, sim, mask)
    assert np.array_equal(g.getPairs(), C.pairs()) and (g.P, g.L, g.D) == (C.P, C.L, D)
    launch = g.pair_launch()
    assert (launch["lanes"], launch["patch_max"], launch["npatch"]) == (lanes, 2100, C.ROWS) and not launch["pval"] and not launch["dir"]
    got = table(g)
    deg = assert_against_literal(got, ref, sim, C.query_routes("thresholds", D, sim, lanes), "lanes %d D %d sim %d mask %-6s" % (lanes, D, sim, mask))
    assert (ref["ncommon"] == 0).sum() > 1000 and deg.sum() >= (500 if sim == 2 else 0)
    gf, _ = C.product_group(ctx, "thresholds", D, sim, mask, fixnan=True)
    fixed = table(gf).ravel()
    empty = ref["ncommon"] == 0
    assert (fixed[empty] == 1e7).all()
    assert np.array_equal(fixed[~empty], got.ravel()[~empty])


@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("lanes", [16, 32])
def test_gather_and_compact_forms(ctx, monkeypatch, lanes, D, sim):
    """An imported group evaluates from F by vertex id until its first whole label step has built the value copies and the patch directory; a sliced
    step builds them for its slice only.  Same bits either way, and a slice of a step equals the rows of the whole step."""
    monkeypatch.setenv("MSMHIP_GROUP_PAIR_LANES", str(lanes))
    ref = C.reference("thresholds", D, sim, "dyadic")
    g, _ = C.product_group(ctx, "thresholds", D, sim, "dyadic")
    assert not g.pair_launch()["pval"] and not g.pair_launch()["dir"]
    gathered = table(g)
    labeling, label = np.random.default_rng(5).integers(0, g.L, g.num_nodes).astype(np.int32), 11
    p0, p1 = g.P // 3, 2 * g.P // 3
    part = ctx.host_array((4 * (p1 - p0),))
    part[:] = -7.0
    g.fusionMove_dev(labeling, label, (p0, p1), (0, 0), part.ctypes.data, 0)
    assert not g.pair_launch()["pval"]  # the copies of a slice serve that slice's label steps only
    assert np.array_equal(table(g), gathered, equal_nan=True)
    quads, _ = g.fusionMove(labeling, label)
    assert np.array_equal(part.reshape(-1, 4), quads[p0:p1], equal_nan=True)
    assert g.pair_launch()["pval"] and g.pair_launch()["dir"]
    compact = table(g)
    assert np.array_equal(compact, gathered, equal_nan=True)
    assert_against_literal(compact, ref, sim)
    assert np.array_equal(quads, step_from(gathered, labeling, label), equal_nan=True)


@pytest.mark.parametrize("lanes", [16, 32])
def test_empty_last_row_of_a_subject(ctx, monkeypatch, lanes):
    """Both subjects' lists end with an empty row: the register path's loads, clamped to the patch, start at the element behind the list (ids in the
    gather form, ids and values in the compact form -- the lists carry one element of padding for it).  All 15 162 queries in both forms against
    the literal; pair 41 with the empty row as patch A, as patch B and as both has no cost."""
    monkeypatch.setenv("MSMHIP_GROUP_PAIR_LANES", str(lanes))
    ref = C.reference("empty_last", 2, 2, "none")
    g, _ = C.product_group(ctx, "empty_last", 2, 2, "none")
    assert g.pair_launch()["npatch"] == C.ROWS and not g.pair_launch()["pval"]
    gathered = table(g)
    assert_against_literal(gathered, ref, 2)
    g.fusionMove(np.zeros(g.num_nodes, dtype=np.int32), C.L - 1)  # a whole step builds the value copies
    assert g.pair_launch()["pval"] and g.pair_launch()["dir"]
    compact = table(g)
    assert np.array_equal(compact, gathered, equal_nan=True)
    for p, la, lb in C.EMPTY_LAST_QUERIES:
        assert np.isnan(ref["want"].reshape(C.P, C.L, C.L)[p, la, lb]) and np.isnan(compact[p, la, lb])


def step_from(tab, labeling, label):
    """the P x 4 pair costs of a label step (I/Fusion/Fusion.h:170-173) out of the table of all queries"""
    pr, k = C.pairs(), np.arange(4)
    la = np.where(k[None, :] & 2, label, labeling[pr[:, 0]][:, None])
    lb = np.where(k[None, :] & 1, label, labeling[pr[:, 1]][:, None])
    return tab[np.arange(C.P)[:, None], la, lb]


@pytest.mark.parametrize("lanes,D,sim", [(16, 1, 2), (32, 1, 2), (16, 2, 2), (32, 2, 2), (16, 3, 2), (32, 3, 2), (16, 2, 1), (32, 2, 1), (64, 2, 4), (64, 3, 5)])
def test_label_steps_on_the_threshold_group(ctx, monkeypatch, lanes, D, sim):
    """Eight steps with a changing labeling, then two sweeps over all labels: the kept (current, current) and (label, label) costs and the
    four-at-a-time enumeration with its tail (42 pairs: count & ~3 = 40), on patches of every tier.  DICE: the single pass."""
    if lanes != 64:
        monkeypatch.setenv("MSMHIP_GROUP_PAIR_LANES", str(lanes))
    ref = C.reference("thresholds", D, sim, "none")
    g, _ = C.product_group(ctx, "thresholds", D, sim, "none")
    tab = table(g)
    if sim in (4, 5):
        ok = np.isfinite(ref["want"])
        assert np.array_equal(np.isnan(tab.ravel()), ~ok) and np.array_equal(tab.ravel()[ok], ref["want"][ok])
    else:
        assert_against_literal(tab, ref, sim)
    rng = np.random.default_rng(23)
    labeling = rng.integers(0, g.L, g.num_nodes).astype(np.int32)
    steps = [int(l) for l in rng.integers(0, g.L, 8)] + 2 * list(range(g.L))
    for i, label in enumerate(steps):
        quads, _ = g.fusionMove(labeling, label)
        assert np.array_equal(quads, step_from(tab, labeling, label), equal_nan=True), (i, label)
        if i < 8:
            labeling = np.where(rng.random(g.num_nodes) < 0.2, rng.integers(0, g.L, g.num_nodes), labeling).astype(np.int32)
        elif i % 5 == 0:  # within the sweeps a few nodes take the proposed label, as after an accepted move
            labeling = np.where(rng.random(g.num_nodes) < 0.1, label, labeling).astype(np.int32)


@pytest.mark.parametrize("cp_order", [2, 1])
@pytest.mark.parametrize("D", [1, 3])
def test_one_and_three_feature_rows_on_a_real_set_up(ctx, monkeypatch, D, cp_order):
    """The ordinary path (set-up pipeline, value copies built by finalize for D = 1, none for D = 3) at the row counts the other group tests never use:
    ico4 under ico2 (patches of ~65 entries) and under ico1 (~220), pair costs and one label step against the oracle"""
    monkeypatch.delenv("MSMHIP_GROUP_PAIR_LANES", raising=False)
    g, og, _ = build(ctx, S=2, data_order=4, cp_order=cp_order, D=D, mask=True)
    assert g.pair_launch()["pval"] == (D <= 2) and g.pair_launch()["lanes"] == (16 if cp_order == 2 else 32)
    rng = np.random.default_rng(1)
    p, la, lb = (rng.integers(0, hi, 400).astype(np.int32) for hi in (g.P, g.L, g.L))
    got, want = g.computePairwiseCost(p, la, lb), og.pairwise_batch(p, la, lb, threads=8)
    assert np.isfinite(want).sum() > 300
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True), np.nanmax(np.abs(got - want))
    labeling, label = rng.integers(0, g.L, g.num_nodes).astype(np.int32), 7
    quads, _ = g.fusionMove(labeling, label)
    pairs = og.pairs()
    q, k = np.repeat(np.arange(og.P, dtype=np.int32), 4), np.tile(np.arange(4), og.P)
    la = np.where(k & 2, label, labeling[pairs[q, 0]]).astype(np.int32)
    lb = np.where(k & 1, label, labeling[pairs[q, 1]]).astype(np.int32)
    want = og.pairwise_batch(q, la, lb, threads=8)
    assert np.allclose(quads.ravel(), want, rtol=RTOL, atol=ATOL, equal_nan=True), np.nanmax(np.abs(quads.ravel() - want))
    assert np.array_equal(quads.ravel(), g.computePairwiseCost(q, la, lb), equal_nan=True)


@pytest.mark.parametrize("name,auto", [("lanes16", 16), ("lanes32", 32)])
def test_lane_choice(ctx, monkeypatch, name, auto):
    """1 437 of 1 596 patches with at most 80 entries: a quarter wavefront per query; 1 436: half a wavefront (10 nsmall >= 9 npatch).
    MSMHIP_GROUP_PAIR_LANES overrides both."""
    monkeypatch.delenv("MSMHIP_GROUP_PAIR_LANES", raising=False)
    rng = np.random.default_rng(9)
    p, la, lb = (rng.integers(0, hi, 300).astype(np.int32) for hi in (C.P, C.L, C.L))
    want, _ = C.literal_batch(name, 2, 2, "dyadic", p, la, lb)
    for forced in (None, 16, 32):
        if forced is not None:
            monkeypatch.setenv("MSMHIP_GROUP_PAIR_LANES", str(forced))
        g, _ = C.product_group(ctx, name, 2, 2, "dyadic")
        launch = g.pair_launch()
        assert (launch["npatch"], launch["nsmall"], launch["patch_max"]) == (C.ROWS, 1437 if auto == 16 else 1436, C.LARGE)
        assert launch["lanes"] == (forced or auto), launch
        got = g.computePairwiseCost(p, la, lb)
        assert np.allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True), np.nanmax(np.abs(got - want))


@pytest.mark.parametrize("sim,percentile", [(4, 0.75), (5, 0.75), (4, 0.3), (5, 0.3)])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("name,fit", [("dice958", "default"), ("dice1000", "attribute"), ("dice2100", "attribute")])
def test_dice_at_the_lds_limits(ctx, name, fit, D, sim, percentile):
    """DICE / genDICE pack the common entries into LDS rows of the largest patch: 64 KB in all at 958 entries (no attribute), 68 224 bytes at 1 000
    (the dynamic bytes alone would not ask for the attribute, the sum does) and 138 624 at 2 100.  Ratios of counts: exactly the literal's."""
    ref = C.reference(name, D, sim, "none", percentile)
    g, _ = C.product_group(ctx, name, D, sim, "none", percentile=percentile)
    launch = g.pair_launch()
    patch_max = int(C.CASES[name]().max())
    assert (launch["lanes"], launch["patch_max"], launch["dice_lds"], launch["dice_fit"]) == (64, patch_max, C.dice_lds(patch_max), fit), launch
    got, want = table(g).ravel(), ref["want"]
    ok = np.isfinite(want)
    assert np.array_equal(np.isnan(got), ~ok) and ok.sum() > 13000 and np.unique(want[ok]).size > 20
    assert np.array_equal(got[ok], want[ok]), np.abs(got[ok] - want[ok]).max()


@pytest.mark.parametrize("name", ["dice2500", "dice2561"])
def test_dice_refuses_a_patch_that_does_not_fit(ctx, name):
    """One patch of 2 500 (2 561) entries: 64 n + 4 224 bytes pass the 160 KB of a workgroup.  Every pair evaluation says so; the triplets of the group
    and a correlation group on the same context go on working."""
    n = int(C.CASES[name]().max())
    g, _ = C.product_group(ctx, name, 2, 4, "none")
    launch = g.pair_launch()
    assert (launch["patch_max"], launch["dice_lds"], launch["dice_fit"]) == (n, C.dice_lds(n), "refused")
    p, la, lb = (a[:500] for a in C.all_queries())
    labeling = np.zeros(g.num_nodes, dtype=np.int32)
    for call in (lambda: g.computePairwiseCost(p, la, lb), lambda: g.fusionMove(labeling, 3)):
        with pytest.raises(M.MsmError, match="group patch of %d entries does not fit in LDS" % n) as e:
            call()
        assert e.value.code == MSM_ERR_CAPACITY
    t = np.arange(g.T, dtype=np.int32)
    assert np.isfinite(g.computeTripletCost(t, 0 * t, 0 * t + 1, 0 * t + 2)).all()
    gc, _ = C.product_group(ctx, name, 2, 2, "none")
    want, _ = C.literal_batch(name, 2, 2, "none", p, la, lb)
    got = gc.computePairwiseCost(p, la, lb)
    assert np.isfinite(want).sum() > 400 and np.allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True)
