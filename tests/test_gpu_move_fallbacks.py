"""The fused fusion move's lower levels -- the leaf search of the samples the direction table leaves open (group8_find inside k_ho_move) and the
evaluations deferred to k_ho_move_tail -- on every route, against the oracle, on the star-shaped targets of tests/move_fallback_cases.py
(tests/test_move_fallbacks_cpu.py shows on the oracle alone that every entry compared here is finite).  The tail kernel has its own copy of nearly
every decision of the main kernel: the value of a sample (ho_value_on, one lane through all rows, against the table record of mode 0 and the
eight-lane moments of modes 2 and 3), the cost-function weights (from global memory, not LDS), the single form's output index, the labeling as
kernel arguments or as a device array, the arguments of a prefetched move.  Every case that claims to reach it asserts that it did:
routes()["move_tails"] rises by one for the move and routes()["move_deferred"], the evaluations the move handed over, is positive.

Every comparison is over all T x 8 entries at the project's tolerance for these classes (helpers.MOVE_RTOL / MOVE_ATOL = 1e-9 / 1e-11), every entry
finite, the folded pattern equal to the oracle's.

Deferred evaluations, measured on an MI355X (ico4 / ico2 at 3e-2, of 2 560): 354 for the all-zero labeling, 318 for the mixed one, in every mode
of the kernel -- more than the 256 the tail kernel's 64 workgroups x 4 wavefronts take in one pass, so its grid-stride loop runs a second time;
with 277 labels 360 and 342; evaluateTotalCostSum (of 320) 45 and 41."""
import numpy as np
import pytest

import move_fallback_cases as C
from newmsm_amd import problem
from helpers import HCP, close

pytestmark = pytest.mark.gpu
FOLD = 1e6 * C.LAMBDA


def build(ctx, kind, D, sim=2, rows=0, shape=C.MOVE_SHAPE, sg_order=None):
    """the product's cost function of C.oracle(the same arguments), with the patches and the absolute weights of the oracle's"""
    inp = C.star(shape, D, sg_order)
    cf, _ = problem.build_cost(ctx, inp, kind=kind, simmeasure=sim, lambda_=C.LAMBDA, **HCP)
    if rows:
        cf.set_dataaffintyweighting(C.weights(inp, rows))
    cf.get_source_data()
    oc = C.oracle(kind, D, sim, rows, shape, sg_order)
    ptr, idx = cf.patches()
    optr, oidx = oc.patches()
    assert np.array_equal(ptr, optr) and np.array_equal(idx, oidx)
    assert np.array_equal(cf.absolute_weights(), oc.absolute_weights())  # bit-equal, weighted or not
    r = cf.routes()
    assert r["move"] == "none" and r["move_tails"] == 0 and r["move_deferred"] == 0
    return cf, oc  # (cf holds its meshes)


def want_of(which, kind, D, sim=2, rows=0, shape=C.MOVE_SHAPE, sg_order=None):
    return C.octets(which, kind, D, sim, rows, shape, sg_order)


def same(E, want):
    """the full comparison"""
    assert E.shape == want.shape and np.isfinite(E).all()
    assert close(E, want), np.abs(E - want).max()
    assert np.array_equal(E >= FOLD, want >= FOLD)


def tail_move(cf, route, call):
    """call() is one fused move that must reach the tail kernel: its result and the evaluations it deferred"""
    before = cf.routes()["move_tails"]
    got = call()
    r = cf.routes()
    assert r["move"] == route
    assert r["move_tails"] == before + 1 and r["move_deferred"] > 0, r
    return got, r["move_deferred"]


def both_moves(cf, route, *case):
    for which, (labeling, label) in enumerate(C.labelings(cf.N, cf.L)):
        E, n = tail_move(cf, route, lambda: cf.tripletOctets(labeling, label))
        print("deferred", case, which, n)
        same(E, want_of(which, *case))


@pytest.mark.parametrize("kind,D,sim,route", C.FUSED)
def test_every_fused_route_through_the_tail(ctx, kind, D, sim, route):
    """both labelings; 354 and 318 evaluations deferred on every route"""
    cf, oc = build(ctx, kind, D, sim)
    assert cf.T == 320 and cf.L == 19
    both_moves(cf, route, kind, D, sim)
    cf.close()


@pytest.mark.parametrize("rows", ["one", "D"])
@pytest.mark.parametrize("kind,D,route", [(k, D, r) for (k, D), r in zip(C.WEIGHTED, ("fused0", "fused3", "fused2"))])
def test_cost_function_weights_in_the_tail(ctx, kind, D, route, rows):
    """set_dataaffintyweighting with one row and with a row per dimension (the same thing at D = 1): the tail reads the weights of a bin from global
    memory where the main kernel has them in LDS; 354 and 318 deferred"""
    rows = 1 if rows == "one" else D
    cf, oc = build(ctx, kind, D, rows=rows)
    both_moves(cf, route, kind, D, 2, rows)
    assert not close(want_of(1, kind, D, 2, rows), want_of(1, kind, D))  # the weights matter
    cf.close()


@pytest.mark.parametrize("kind,D,route", C.SINGLE)
def test_single_form_through_the_tail(ctx, kind, D, route):
    """evaluateTotalCostSum: combination 000 only, T values; the tail writes out[t] instead of out[8 * t + k].  45 (all-zero labeling) and 41
    (random) of the 320 evaluations deferred"""
    cf, oc = build(ctx, kind, D)
    for labeling in C.total_labelings(cf.N, cf.L):
        (tot, parts), n = tail_move(cf, route, lambda: cf.evaluateTotalCostSum(labeling))
        print("deferred single", kind, D, n)
        otot, oparts = oc.total(labeling)
        assert parts[0] == 0.0 and parts[1] == 0.0 and np.isfinite(tot)
        assert abs(parts[2] - oparts[2]) <= 1e-9 * abs(oparts[2]) and abs(tot - otot) <= 1e-9 * abs(otot), (parts, oparts)
        E = cf.tripletOctets(labeling, 3)
        assert np.isfinite(E).all() and abs(parts[2] - E[:, 0].sum()) <= 1e-9 * abs(parts[2])
    cf.close()


@pytest.mark.parametrize("kind,D,route", C.DEVICE_LABELS)
def test_labeling_as_a_device_array(ctx, kind, D, route):
    """277 labels: the labeling no longer fits the kernel arguments (L > 256), so the move takes k_ho_move<false, .> and
    k_ho_move_tail<false> -- the only case of the suite that runs the latter.  The mixed labeling: 342 deferred"""
    cf, oc = build(ctx, kind, D, sg_order=C.MANY_LABELS)
    assert cf.L == 277 and cf.T == 320
    labeling, label = C.labelings(cf.N, cf.L)[1]
    assert labeling.max() > 255
    E, n = tail_move(cf, route, lambda: cf.tripletOctets(labeling, label))
    print("deferred device labels", kind, D, n)
    same(E, want_of(1, kind, D, sg_order=C.MANY_LABELS))
    cf.close()


@pytest.mark.parametrize("kind,D,route", C.DEVICE_LABELS)
def test_mapped_output_and_prefetch(ctx, kind, D, route):
    """the caller's mapped array as the output, and a prefetched move: the tail launched from take_pending_move runs with the arguments stored
    with the queued move; a dropped prefetch of a deferring move leaves nothing behind for the next one.  The mixed labeling: 318 deferred"""
    cf, oc = build(ctx, kind, D)
    labeling, label = C.labelings(cf.N, cf.L)[1]
    other = C.other_label(cf.N, cf.L)
    plain, _ = tail_move(cf, route, lambda: cf.tripletOctets(labeling, label))
    same(plain, want_of(1, kind, D))
    A, B = ctx.host_array((cf.T, 8)), ctx.host_array((cf.T, 8))
    # synchronous, into mapped memory
    A[:] = -1.0
    got, _ = tail_move(cf, route, lambda: cf.tripletOctets(labeling, label, A))
    assert got is A and np.array_equal(A, plain)
    # prefetched and taken
    taken, dropped = cf.prefetch_stats()
    A[:] = -1.0
    cf.prefetchTripletOctets(labeling, label, A)
    got, _ = tail_move(cf, route, lambda: cf.tripletOctets(labeling, label, A))
    assert got is A and np.array_equal(A, plain) and cf.prefetch_stats() == (taken + 1, dropped)
    # prefetched and dropped by a call with another label
    fresh, _ = build(ctx, kind, D)
    want, _ = tail_move(fresh, route, lambda: fresh.tripletOctets(labeling, other))
    same(want, want_of(2, kind, D))
    cf.prefetchTripletOctets(labeling, label, A)
    got, _ = tail_move(cf, route, lambda: cf.tripletOctets(labeling, other, B))
    assert cf.prefetch_stats() == (taken + 1, dropped + 1)
    assert np.array_equal(B, want)
    fresh.close()
    cf.close()


def test_six_deferring_moves_in_a_row(ctx):
    """two (labeling, label) pairs in turn on one cost function: the counter of a move is cleared by the next move's first workgroup, the list
    and the handed-over values are reused.  354 and 318 deferred in turn"""
    kind, D, route = "ho_multivariate", 12, "fused3"
    cf, oc = build(ctx, kind, D)
    pairs = C.labelings(cf.N, cf.L)
    first, counts = [], []
    before = cf.routes()["move_tails"]
    for step in range(6):
        labeling, label = pairs[step % 2]
        E, n = tail_move(cf, route, lambda: cf.tripletOctets(labeling, label))
        if step < 2:
            same(E, want_of(step, kind, D))
            first.append(E)
            counts.append(n)
        assert np.array_equal(E, first[step % 2]) and n == counts[step % 2]
    assert cf.routes()["move_tails"] == before + 6
    cf.close()


@pytest.mark.parametrize("D,route", C.THREE_KERNEL)
def test_three_kernel_path_on_the_star_shaped_target(ctx, D, route):
    """ico5 / ico1: bins of 105 to 150 points, beyond what a workgroup of the fused move holds; the same two lower levels inside k_ho_octets_fix"""
    cf, oc = build(ctx, "ho_multivariate", D, shape=C.BIG_BIN_SHAPE)
    bins = np.diff(cf.patches()[0])
    assert len(bins) == 80 and bins.min() == 105 and bins.max() == 150
    for which, (labeling, label) in enumerate(C.labelings(cf.N, cf.L)):
        same(cf.tripletOctets(labeling, label), want_of(which, "ho_multivariate", D, shape=C.BIG_BIN_SHAPE))
        r = cf.routes()
        assert r["move"] == route and r["move_tails"] == 0 and r["move_deferred"] == 0
    cf.close()


@pytest.mark.parametrize("kind,D,route", C.UNARY)
def test_unary_table_behind_the_fixup_kernel(ctx, kind, D, route):
    """the lane-group reductions of the multivariate and patchwise tables behind k_unary_fixup: 19 x 162, the project's tolerance for these
    classes (rtol 1e-9 / atol 1e-11, tests/test_gpu_feature_widths.py)"""
    cf, _ = problem.build_cost(ctx, C.star(C.MOVE_SHAPE, D), kind=kind)
    cf.get_source_data()
    oc, Uo = C.unary_oracle(kind, D)
    ptr, idx = cf.patches()
    optr, oidx = oc.patches()
    assert np.array_equal(ptr, optr) and np.array_equal(idx, oidx)
    U = cf.computeUnaryCosts()
    assert cf.routes()["unary"] == route
    assert U.shape == Uo.shape == (19, 162) and np.isfinite(U).all()
    assert np.allclose(U, Uo, rtol=1e-9, atol=1e-11), np.abs(U - Uo).max()
    cf.close()
