"""The crafted groups of tests/group_pair_cases.py on the CPU alone: their literal of computePairwiseCost equals the oracle's group bit for bit
on a real set-up, the route predicate the pair kernel calls (msm_group_pair_route) gives the table of DESIGN.md section 5.6 on both sides of
every threshold, and the cases reach what tests/test_gpu_group_pair_routes.py claims to compare -- no GPU.  The bounds are conditions;
measured counts are in the docstrings."""
import collections

import numpy as np
import pytest

import group_pair_cases as C
import newmsm_amd as M
from newmsm_amd import api, synthetic
from oracle import oracle as O

route = api.DiscreteGroupCostFunction.pair_route


# ------------------------------------------------------------------ the literal against the oracle's group
def real_group(D, sim, percentile=0.75):
    """S = 2, ico3 data and template under an ico1 control grid with a template mask: the oracle's half of tests/test_gpu_group.py's builder"""
    dxyz, dtri = M.make_mesh_from_icosa(3)
    cxyz, ctri = M.make_mesh_from_icosa(1)
    _, mvd = M.cp_spacings(cxyz, ctri)
    samples, _ = M.label_sampling_grid(3, 0.5 * mvd)
    mk = np.cos(dxyz[:, 0] / 30.0)
    og = O.Group(2, simmeasure=sim, lambda_=0.2, percentile=percentile)
    keep = [O.Mesh(dxyz, dtri), O.Mesh(cxyz, ctri)]
    og.set_template(keep[0], mk)
    og.set_controlgrid(keep[1])
    for s in range(2):
        sph = synthetic.known_warp(dxyz, seed=40 + s, rot_deg=1.0 + s, amp=0.5)
        feat = synthetic.features(synthetic.known_warp(dxyz, seed=90 + s, rot_deg=2.0, amp=1.0), D, seed=5)
        om = O.Mesh(dxyz, dtri)
        og.set_subject(s, om, feat)
        om.set_coords(sph)
        og.set_subject(s, om, feat)
        og.reset_cpgrid(s, synthetic.known_warp(cxyz, seed=40 + s, rot_deg=1.0 + s, amp=0.5))
        keep.append(om)
    og.set_labels(samples)
    og.setup()
    return og, mk, keep


@pytest.mark.parametrize("sim,percentile", [(1, 0.75), (2, 0.75), (4, 0.75), (5, 0.3)])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_literal_equals_the_oracle_group(D, sim, percentile):
    """300 queries of a real group: the literal over og.patch()'s arrays gives og.pairwise()'s bits, NaN for NaN"""
    og, mk, _ = real_group(D, sim, percentile)
    pairs = og.pairs()
    rng = np.random.default_rng(17)
    n = 300
    finite = 0
    for p, la, lb in zip(rng.integers(0, og.P, n), rng.integers(0, og.L, n), rng.integers(0, og.L, n)):
        (sa, va), (sb, vb) = divmod(int(pairs[p, 0]), og.N), divmod(int(pairs[p, 1]), og.N)
        ia, da = og.patch(sa, va, la)
        ib, db = og.patch(sb, vb, lb)
        got, _ = C.literal(ia, da, ib, db, mk, sim, percentile)
        want = og.pairwise(p, la, lb)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64) or (np.isnan(got) and np.isnan(want)), (p, la, lb, got, want)
        finite += np.isfinite(want)
    assert finite > 200


# ------------------------------------------------------------------ the route table
THRESHOLD_SIDES = [0, 1, 63, 64, 65, 79, 80, 81, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097]


@pytest.mark.parametrize("sim", [1, 2, 4, 5])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_route_table(D, sim):
    """DESIGN.md section 5.6, written out again from the text (not from the code): every (cntA, cntB) of both sides of every threshold"""
    for lanes in ((64,) if sim in (4, 5) else (16, 32)):
        reg = {16: 80, 32: 128, 64: -1}[lanes]  # entries of A the register path holds
        for a in THRESHOLD_SIDES:
            for b in THRESHOLD_SIDES:
                r = route(a, b, D, sim, lanes)
                staged = b <= 256
                fast = sim in (1, 2) and D <= 2 and staged and a <= reg
                want = dict(fast=fast, staged=staged, padded=(64 if b <= 64 else 128 if b <= 128 else 256) if staged else 0,
                            beyond=(not fast) and a > 64 * lanes)
                want["name"] = "fast%d" % want["padded"] if fast else ("staged" if staged else "unstaged") + ("_beyond" if want["beyond"] else "")
                assert r == want, (lanes, a, b, r, want)


def test_route_rejects_what_no_launch_uses():
    for bad in [(-1, 5, 1, 2, 16), (5, 5, 0, 2, 16), (5, 5, 1, 3, 16), (5, 5, 1, 2, 64), (5, 5, 1, 4, 32), (5, 5, 1, 2, 8)]:
        with pytest.raises(M.MsmError, match="msm_group_pair_route"):
            route(*bad)


# ------------------------------------------------------------------ the cases meet their conditions
def test_threshold_case_holds_every_ordered_pair_of_sizes():
    ca, cb = C.query_sizes("thresholds")
    assert len(set(zip(ca.tolist(), cb.tolist()))) == len(C.SIZES) ** 2
    pptr, pidx = C.csr("thresholds")
    for s in range(C.S):
        assert np.array_equal(np.diff(pptr[s]), C.threshold_sizes()[s].ravel())
        for k in range(C.N * C.L):
            assert (np.diff(pidx[s][pptr[s][k]: pptr[s][k + 1]]) > 0).all()  # ascending within every row, no id twice
        assert pidx[s].min() >= 0 and pidx[s].max() < C.VT
    assert 600_000 < len(pidx[0]) + len(pidx[1]) < 640_000  # 619 672 index entries


@pytest.mark.parametrize("sim", [1, 2, 4])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_threshold_case_reaches_every_route(D, sim):
    """counted through pair_route: every route that exists for (lanes, D, measure) by at least 100 queries (fewest: 316, unstaged_beyond at 32
    lanes), and both cntA < cntB and cntA > cntB inside fast64 and fast128 (fast256 admits only cntA < cntB)"""
    ca, cb = C.query_sizes("thresholds")
    for lanes in ((64,) if sim == 4 else (16, 32)):
        names = C.query_routes("thresholds", D, sim, lanes)
        count = collections.Counter(names.tolist())
        want = ["staged", "unstaged"] if lanes == 64 else C.expected_routes(lanes, D, sim)  # (DICE: no patch passes 64 x 64 entries)
        assert sorted(count) == sorted(want), count
        assert min(count.values()) >= 100, count
        for name in want:
            if name.startswith("fast"):
                a, b = ca[names == name], cb[names == name]
                assert (a < b).any()
                if name == "fast256":  # cntA <= 80 | 128 < 129 <= cntB: no query of this route can have the longer patch first
                    assert a.max() <= 128 < b.min()
                else:
                    assert (a > b).any()


@pytest.mark.parametrize("mask", ["none", "dyadic"])
def test_threshold_case_intersections(mask):
    """1 661 of the 15 162 intersections are empty (11 %), 959 hold one entry and 887 two; no correlation over one or two entries changes
    with the order of the entries (0 queries left out of the closeness comparison; the bound is 1 %)"""
    ref = C.reference("thresholds", 1, 2, mask)
    nc, want = ref["ncommon"], ref["want"]
    assert len(nc) == C.P * C.L * C.L == 15162
    assert np.array_equal(np.isnan(want), nc == 0)
    assert (nc == 0).mean() <= 0.15 and (nc == 0).sum() > 1000
    assert (nc == 1).sum() >= 500 and (nc == 2).sum() >= 500
    assert ref["unstable"].mean() < 0.01
    assert (want[nc == 1] == 0.5).all()  # one entry has no variance
    ca, cb = C.query_sizes("thresholds")
    assert ((nc == 0) & (ca > 0) & (cb > 0)).sum() > 500  # non-empty patches without a common vertex (FAR_LABEL)


def test_empty_last_row_case():
    """both subjects' lists end with an empty row (control point 41, label 18), the row before it does not; all queries hold pair 41 with that row as patch A,
    as patch B and as both, and the literal has no cost for them"""
    pptr, pidx = C.csr("empty_last")
    for s in range(C.S):
        assert pptr[s][-1] == pptr[s][-2] == len(pidx[s]) and pptr[s][-2] > pptr[s][-3]
        assert np.array_equal(np.diff(pptr[s]), C.with_empty_last_rows()[s].ravel())
    p, la, lb = C.all_queries()
    ca, cb = C.query_sizes("empty_last")
    for q, want_sizes in zip(C.EMPTY_LAST_QUERIES, [(0, 0), (0, None), (None, 0)]):
        at = np.flatnonzero((p == q[0]) & (la == q[1]) & (lb == q[2]))
        assert len(at) == 1
        assert all(w is None or w == got for w, got in zip(want_sizes, (ca[at[0]], cb[at[0]])))
        cost, ncommon = C.literal_batch("empty_last", 2, 2, "none", p[at], la[at], lb[at])
        assert np.isnan(cost[0]) and ncommon[0] == 0
    assert C.CASES["thresholds"]()[0, C.N - 1, 0] > 0 and C.CASES["thresholds"]()[1, C.N - 1, 0] > 0  # the other patch of the one-sided queries is not empty


def test_lane_choice_cases_sit_on_the_boundary():
    small = {n: int((C.CASES[n]() <= 80).sum()) for n in ("lanes16", "lanes32")}
    assert small == {"lanes16": 1437, "lanes32": 1436} and C.ROWS == 1596
    assert 10 * small["lanes16"] >= 9 * C.ROWS > 10 * small["lanes32"]


def test_dice_cases_sit_on_the_lds_limits():
    """64 n + 4 224 bytes for a largest patch of n entries: 958 is the last below 64 KB, 1 000 passes it with its dynamic bytes alone below, 2 494 is
    the last below 160 KB"""
    big = {n: int(C.CASES[n]().max()) for n in C.CASES if n.startswith("dice")}
    assert big == dict(dice958=958, dice1000=1000, dice2100=2100, dice2500=2500, dice2561=2561)
    assert C.dice_lds(958) == 64 * C.KB < C.dice_lds(959)
    assert C.dice_lds(1000) - C.DICE_STATIC_LDS < 64 * C.KB < C.dice_lds(1000)
    assert C.dice_lds(2100) < 160 * C.KB
    assert C.dice_lds(2494) == 160 * C.KB < C.dice_lds(2500) and C.dice_lds(2500) - C.DICE_STATIC_LDS < 160 * C.KB < C.dice_lds(2561) - C.DICE_STATIC_LDS
