"""The strain regulariser's triplet costs where triangles collapse, kernel by kernel against the oracle.

The inputs of tests/strain_collapse_cases.py -- a regular control grid under unrescaled labels -- put NaN, +inf, folded and nearly collapsed finite
entries into every producer of triplet costs; tests/test_strain_collapse_cpu.py pins how many.  Here every route must give the oracle's class
for every entry (SC.compare: the four masks array_equal) and its value within the 1e-9 / 1e-11 of tests/test_gpu_cost_kinds.py elsewhere, the
nearly collapsed entries included; deliveries of one evaluator must agree bit for bit, NaN pattern included.  The consumers (Monte Carlo
optimiser, MPLP) then take the real table with its 211 NaN and 248 +inf.

Measured worst relative difference on the nearly collapsed entries (MI355X; every route prints its own in SC.compare): k_triplet_table 2.9e-16
(k_exponent 1.5: 2.6e-16), the anatomical batch 1.7e-16, k_group_triplet over a subject's whole table 6.2e-16, 0 on the batch samples, on every octet
route and on the triclique routes -- the kernels spell the oracle's operations in the oracle's order and the build does not contract them.  No class
differed anywhere.

What a wrong kernel looks like here (each tried once on a build of its own, then dropped): a `fixnan` that tests `!isfinite(e)` rewrites the 248
infinities too and fails the three group tests under fixnan.  `I1st <= 2` written `!(I1st > 2)` in triangle_strain_from, and the folding test written
`<= 0.0`, change NOT ONE entry of the near-coincidences above -- there the NaN come from the square root of a negative residue, not from 0/0, and no
normal is exactly zero; test_exact_coincidence is the case that sees them (NaN turned into +inf, into the sentinel)."""
import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api
from newmsm_amd._lib import lib
from tests import strain_collapse_cases as SC

pytestmark = pytest.mark.gpu
FOLD = 1e7 * SC.BASE["lambda_"]


def fold_of(setting):
    return 1e7 * SC.params(setting)["lambda_"]


# ------------------------------------------------------------------------------------------------ pairwise registration, strain only
@pytest.mark.parametrize("setting", list(SC.SETTINGS))
def test_full_table(ctx, setting):
    """k_triplet_table: the whole table in one call, and in ranges that cut between triplets holding non-finite entries (0 and 2 do)"""
    oc, want = SC.oracle_table(setting)
    assert SC.counts(want, fold_of(setting)) == SC.COUNTS[("cp1", setting)]
    cf, _ = SC.product_cost(ctx, setting=setting)
    assert (cf.N, cf.T, cf.L) == (42, 80, 19)
    full = np.array(cf.computeTripletCosts())
    SC.compare(full, want, fold_of(setting), "k_triplet_table %s" % setting)
    assert SC.counts(full, fold_of(setting)) == SC.COUNTS[("cp1", setting)]
    parts = [np.array(cf.computeTripletCosts(t0, t1)) for t0, t1 in ((0, 1), (1, 3), (3, cf.T))]
    assert SC.same_bits(np.concatenate(parts), full)
    cf.close()


@pytest.mark.parametrize("setting", ["k2_r2", "k1.5_r1"])
def test_batch_queries(ctx, setting):
    """k_triplet_batch: all 459 non-finite entries, their neighbours that differ in one label, 2 000 random queries"""
    _, tab = SC.oracle_table(setting)
    t, la, lb, lc = SC.collapse_queries(SC.oracle_table()[1])
    want = tab[t, la, lb, lc]
    assert SC.has_every_class(want, FOLD) and int((~np.isfinite(want[:459])).sum()) == 459
    cf, _ = SC.product_cost(ctx, setting=setting)
    SC.compare(cf.computeTripletCost(t, la, lb, lc), want, FOLD, "k_triplet_batch %s" % setting)
    cf.close()


@pytest.mark.parametrize("setting", ["k2_r2", "k1.5_r1"])
def test_octets(ctx, monkeypatch, setting):
    """k_triplet_octets_packed (staged and into the caller's mapped array) and k_triplet_octets (MSMHIP_OCTETS=copy) on the three label steps that
    meet the most collapsed triangles: the oracle's classes, one evaluator behind the three deliveries, and the batch evaluator's bits"""
    oc, tab = SC.oracle_table(setting)
    inp = SC.inputs()
    moves = SC.collapse_moves(SC.oracle_table()[1], inp["triplets"], 42)
    assert len(moves) == 3 and all(n >= 20 for _, _, n in moves)
    cf, _ = SC.product_cost(ctx, setting=setting)
    run = SC.octets_all_ways(ctx, cf, monkeypatch)
    every = []
    for labeling, label, n in moves:
        want = oc.triplet_octets(labeling, label, threads=8)
        assert int((~np.isfinite(want)).sum()) == n and np.array_equal(want, SC.octets_from_table(tab, inp["triplets"], labeling, label), equal_nan=True)
        got = run(labeling, label)
        assert cf.routes()["move"] == "strain"
        for how, E in got.items():
            assert E.shape == (cf.T, 8)
            SC.compare(E, want, FOLD, "octets %s %s label %d" % (setting, how, label))
        assert SC.same_bits(got["pageable"], got["mapped"]) and SC.same_bits(got["pageable"], got["copy"])
        assert SC.same_bits(got["pageable"].ravel(), cf.computeTripletCost(*SC.octet_queries(inp["triplets"], labeling, label)))
        every.append(want)
    assert SC.has_every_class(np.concatenate(every), FOLD)
    cf.close()


def test_exact_coincidence(ctx, monkeypatch):
    """Two nodes of a triplet on bitwise the same point (SC.coincident_inputs): a normal of exactly (0, 0, 0) is not a fold (`< 0`), and I1st = 0/0
    fails `I1st <= 2`: NaN on all 15 x 19 x 19 equal-label entries, from the table, the batch and the label step's kernels"""
    inp, shared = SC.coincident_inputs()
    oc, want = SC.oracle_coincident()
    assert SC.counts(want, FOLD) == SC.COUNTS[("coincident", "k2_r2")]
    cf, _ = SC.product_cost(ctx, inp=inp)
    full = np.array(cf.computeTripletCosts())
    SC.compare(full, want, FOLD, "k_triplet_table, exact coincidence")
    i = np.arange(cf.L)
    assert sum(int(np.isnan(full[t][i, i, :]).sum()) for t, _, _ in shared) == 15 * 19 * 19
    t = np.repeat(np.array([t for t, _, _ in shared], dtype=np.int32), cf.L * cf.L)
    la = np.tile(np.repeat(i, cf.L), len(shared)).astype(np.int32)
    lc = np.tile(i, len(shared) * cf.L).astype(np.int32)
    assert np.isnan(cf.computeTripletCost(t, la, la, lc)).all()
    labeling = np.full(cf.N, 3, dtype=np.int32)  # every shared pair on label 3: combinations 000, 001 (and 110, 111) of its triplet are NaN
    got = SC.octets_all_ways(ctx, cf, monkeypatch)(labeling, 5)
    wantE = oc.triplet_octets(labeling, 5, threads=8)
    assert all(np.isnan(wantE[t, [0, 1, 6, 7]]).all() for t, _, _ in shared)
    for how, E in got.items():
        SC.compare(E, wantE, FOLD, "octets %s, exact coincidence" % how)
    cf.close()


# ------------------------------------------------------------------------------------------------ the triclique classes
def test_triclique_table_and_batch(ctx):
    """k_triplet_table_ho and k_triplet_batch_ho over the first six triplets that hold non-finite entries: a NaN or infinite strain term added to a
    finite likelihood"""
    ts, want, strain = SC.oracle_ho_tables()
    assert SC.counts(want, FOLD) == SC.COUNTS[("ho", "k2_r2")] and SC.has_every_class(want, FOLD)
    cf, _ = SC.product_cost(ctx, kind="ho_univariate")
    got = np.stack([np.array(cf.computeTripletCosts(t, t + 1))[0] for t in ts])
    SC.compare(got, want, FOLD, "k_triplet_table_ho")
    # the likelihood is finite wherever the triangle is not folded; where the sum is not finite, that is the strain term's class
    lost = ~np.isfinite(strain)
    assert lost.sum() == 54 and np.array_equal(np.isnan(got[lost]), np.isnan(strain[lost])) and np.array_equal(got[lost] == np.inf, strain[lost] == np.inf)
    assert np.isfinite(got[~lost]).all()
    run = np.array(cf.computeTripletCosts(2, 5))  # one call over triplets 2, 3, 4
    assert SC.same_bits(run, got[1:4])
    q, la, lb, lc = SC.collapse_queries(want, extra=2000, seed=1)  # (indices into the six)
    t = np.array(ts, dtype=np.int32)[q]
    batch = cf.computeTripletCost(t, la, lb, lc)
    assert SC.has_every_class(want[q, la, lb, lc], FOLD)
    SC.compare(batch, want[q, la, lb, lc], FOLD, "k_triplet_batch_ho")
    assert SC.same_bits(batch, got[q, la, lb, lc])  # ho_group_eval behind both
    cf.close()


@pytest.mark.parametrize("route,data_order", [("fused0", 4), ("octets_ho", 4), ("octets_sample", 5)])
def test_triclique_octets(ctx, monkeypatch, route, data_order):
    """One label step of the triclique classes on its three routes: the fused move (bins of up to 39 points), k_triplet_octets_ho (no direction table)
    and, with bins of 111 to 140 points under the same control grid, k_ho_octets_sample / _fix / _reduce"""
    if route == "octets_ho":
        monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")  # read when the target's search structures are built
    inp = SC.inputs(1, data_order)
    oc = SC.oracle_ho(data_order)
    moves = SC.collapse_moves(SC.oracle_table()[1], inp["triplets"], 42)  # (the control grid and the labels do not depend on the data grid)
    cf, _ = SC.product_cost(ctx, kind="ho_univariate", data_order=data_order)
    ptr, _ = cf.patches()
    assert (np.diff(ptr).max() > 128) == (route == "octets_sample")
    every = []
    for labeling, label, n in moves:
        want = oc.triplet_octets(labeling, label, threads=8)
        assert int((~np.isfinite(want)).sum()) == n >= 20
        E = np.array(cf.tripletOctets(labeling, label))
        assert cf.routes()["move"] == route
        SC.compare(E, want, FOLD, "%s label %d" % (route, label))
        # the batch evaluator samples the same points through the same search and runs the same serial likelihood: its bits, NaN pattern included
        assert SC.same_bits(E, cf.computeTripletCost(*SC.octet_queries(inp["triplets"], labeling, label)).reshape(cf.T, 8))
        every.append(want)
    assert SC.has_every_class(np.concatenate(every), FOLD)
    cf.close()


# ------------------------------------------------------------------------------------------------ anatomical regulariser
def test_anatomical_regulariser(ctx):
    """k_triplet_batch<true>, regoption 5: every fourth triplet's whole table.  A collapsed control triangle is not a failed search: the status word
    stays clear (a raised one makes computeTripletCost raise)"""
    oc, want = SC.oracle_anat()
    fold = 1e7 * SC.ANAT["lambda_"]
    assert SC.counts(want, fold) == SC.COUNTS[("anat", "step4")] and SC.has_every_class(want, fold)
    cf, keep = SC.product_anat(ctx)
    L = cf.L
    q = np.arange(L ** 3)
    got = np.stack([cf.computeTripletCost(np.full(L ** 3, t, dtype=np.int32), q // L ** 2, q // L % L, q % L).reshape(L, L, L) for t in SC.anat_triplets(cf.T)])
    SC.compare(got, want, fold, "k_triplet_batch<anatomical>")
    cf.close()


# ------------------------------------------------------------------------------------------------ groupwise
@pytest.fixture(scope="module")
def groups(ctx):
    made = {}

    def get(fixnan):
        if fixnan not in made:
            made[fixnan] = SC.product_group(ctx, fixnan)
        return made[fixnan][0]

    yield get
    for g, _ in made.values():
        g.close()


@pytest.mark.parametrize("fixnan", [False, True])
def test_group_queries(groups, fixnan):
    """k_group_triplet in query mode: subject 0 (regular control grid) over its whole table, subject 1 (warped) over 20 000 queries.  FIX_NAN replaces
    the NaN and nothing else: no NaN, the 248 infinities, 8 136 + 211 entries at 1e7"""
    g = groups(fixnan)
    assert (g.num_nodes, g.T, g.Tc, g.L) == (84, 160, 80, 19)
    want = SC.oracle_group_table(fixnan, 0)
    assert SC.counts(want, SC.GROUP_FOLD) == SC.COUNTS[("group", fixnan, 0)]
    got = g.computeTripletCost(*SC.subject_queries(0, g.Tc, g.L)).reshape(want.shape)
    SC.compare(got, want, SC.GROUP_FOLD, "k_group_triplet fixnan=%s subject 0" % fixnan)
    assert SC.counts(got, SC.GROUP_FOLD) == SC.COUNTS[("group", fixnan, 0)]
    if fixnan:
        assert SC.counts(got, SC.GROUP_FOLD)[:4] == (0, 248, 0, 8347)
    else:
        assert SC.has_every_class(want, SC.GROUP_FOLD)
    rng = np.random.default_rng(7)
    pick = rng.choice(want.size, 20000, replace=False)
    t, la, lb, lc = (x[pick] for x in SC.subject_queries(1, g.Tc, g.L))
    want1 = SC.oracle_group_table(fixnan, 1)
    assert SC.counts(want1, SC.GROUP_FOLD)[:3] == (0, 0, 0)
    SC.compare(g.computeTripletCost(t, la, lb, lc), want1[t - g.Tc, la, lb, lc], SC.GROUP_FOLD, "k_group_triplet fixnan=%s subject 1" % fixnan)


@pytest.mark.parametrize("fixnan", [False, True])
def test_group_label_step(groups, fixnan):
    """k_group_triplet in move mode: the label steps that meet the most collapsed triangles of subject 0, subject 1 on random labels"""
    g = groups(fixnan)
    trips = g.getTriplets()
    tabs = [SC.oracle_group_table(fixnan, s) for s in range(2)]
    moves = SC.collapse_moves(SC.oracle_group_table(False, 0), trips[: g.Tc], g.N)
    rng = np.random.default_rng(9)
    every = []
    for lab0, label, n in moves:
        assert n >= 20
        labeling = np.concatenate([lab0, rng.integers(0, g.L, g.N)]).astype(np.int32)
        _, octets = g.fusionMove(labeling, label)
        octets = np.array(octets)
        want = np.concatenate([SC.octets_from_table(tabs[s], trips[s * g.Tc:(s + 1) * g.Tc] - s * g.N, labeling[s * g.N:(s + 1) * g.N], label) for s in range(2)])
        assert int((~np.isfinite(want)).sum()) == (n if not fixnan else int(np.isinf(want).sum())) > 0
        SC.compare(octets, want, SC.GROUP_FOLD, "k_group_triplet move mode fixnan=%s label %d" % (fixnan, label))
        assert SC.same_bits(octets.ravel(), g.computeTripletCost(*SC.octet_queries(trips, labeling, label)))
        every.append(want)
    n = SC.counts(np.concatenate(every), SC.GROUP_FOLD)
    assert n[1] > 0 and n[3] > 0 and n[4] > 0 and (n[0] > 0) == (not fixnan)


@pytest.mark.parametrize("fixnan", [False, True])
def test_group_subject_table(groups, fixnan):
    """the subject's triplet table of the group Monte Carlo path is the batch evaluator's, bit for bit, with its non-finite entries"""
    from tests.test_gpu_group_mcmc import same_bits

    g = groups(fixnan)
    tc = g.subject_triplet_table(0)
    assert same_bits(tc.ravel(), g.computeTripletCost(*SC.subject_queries(0, g.Tc, g.L)))
    assert int((~np.isfinite(tc)).sum()) == (248 if fixnan else 459)
    SC.compare(tc, SC.oracle_group_table(fixnan, 0), SC.GROUP_FOLD, "subject triplet table fixnan=%s" % fixnan)
    assert np.array_equal(g.subject_triplets(0), SC.oracle_group(fixnan).triplets()[: g.Tc])


# ------------------------------------------------------------------------------------------------ the consumers, on the real table
@pytest.fixture(scope="module")
def real_tables(ctx):
    cf, keep = SC.product_cost(ctx)
    U, tc = np.array(cf.computeUnaryCosts()), np.array(cf.computeTripletCosts())
    assert np.isfinite(U).all() and SC.counts(tc, FOLD) == SC.COUNTS[("cp1", "k2_r2")]
    yield cf, U, tc, SC.inputs()["triplets"]
    cf.close()


@pytest.mark.parametrize("K", [1, 4])
def test_monte_carlo_optimiser_on_the_real_table(ctx, real_tables, K):
    """MCMC::optimise branches on these values (a NaN is never smaller, nothing beats a NaN in slot 0): the GPU sweeps take the host literal's
    decisions on the table with its 211 NaN and 248 +inf, from the fetched tables and from the tables left on the device"""
    cf, U, tc, triplets = real_tables
    collapsed, n = SC.collapsed_start(tc, triplets, cf.N)
    assert n == 13 and np.isnan(api.mcmc_energy(U, tc, triplets, collapsed))  # 6 triplets start on a NaN, 7 on +inf
    seeds = api.chain_seeds(5, 0, K)
    for start, iters in ((np.zeros(cf.N, dtype=np.int32), 3), (collapsed, 1), (collapsed, 3)):
        kw = dict(mcparam=0.5, iters=iters)
        want = api.mcmc_optimise_chains(U, tc, triplets, start, seeds, **kw)
        print("K = %d, %d sweeps from %d collapsed triplets: %s labels changed, energies %s" % (K, iters, n if start.any() else 0, (want[1] != start).sum(axis=1), want[2]))
        for name, got in (("tables", api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, **kw)), ("cost function", cf.mcmc_optimise_chains(start, seeds, **kw))):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
            assert SC.same_bits(got[2], want[2]) and got[3] == want[3], (name, got[2], want[2])
        if K == 1:
            one = api.mcmc_optimise(U, tc, triplets, start, seed=seeds[0], **kw)
            assert np.array_equal(one, want[1][0])
            assert np.array_equal(api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, seed=seeds[0], **kw), one)
            assert np.array_equal(cf.mcmc_optimise(start, seed=seeds[0], **kw), one)
    assert not np.array_equal(want[0], collapsed)  # the sweeps left the collapsed triangles


def test_mplp_refuses_the_real_table(ctx, real_tables):
    """MPLP has no reading for a NaN or an infinity: MSM_ERR_INVALID naming the triplet table, from the host literal, from the GPU route over fetched
    tables and from the cost function's own tables, and nothing is written"""
    cf, U, tc, triplets = real_tables
    start = np.random.default_rng(3).integers(0, cf.L, cf.N).astype(np.int32)
    pattern = "MSM_ERR_INVALID.*the triplet table holds a non-finite value"
    for call in (lambda: api.mplp_optimise(U, tc, triplets, start, sweeps=3), lambda: api.mplp_optimise_gpu(ctx, U, tc, triplets, start, sweeps=3),
                 lambda: cf.mplp_optimise(start, sweeps=3)):
        with pytest.raises(M.MsmError, match=pattern):
            call()
    _, head = api._mplp_tables(U, tc, triplets)
    for route in ("host", "gpu", "cost function"):
        out, tail = api._mplp_outputs(cf.N, cf.L, cf.T, 3, start, True, True, True)
        st = {"host": lambda: lib().msm_mplp_optimise(*head, 3, *tail), "gpu": lambda: lib().msm_mplp_optimise_gpu(ctx.h, *head, 3, *tail),
              "cost function": lambda: lib().msm_cost_mplp_optimise(cf.h, 3, *tail)}[route]()
        assert st == -1, route  # MSM_ERR_INVALID
        assert np.array_equal(out["lab"], start) and out["run"].value == -1 and np.isnan(out["energy"].value) and np.isnan(out["bound"].value), route
        assert np.isnan(out["energies"]).all() and np.isnan(out["bounds"]).all() and not out["messages"].any(), route
