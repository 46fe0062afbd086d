"""The bookkeeping around a label step (msm_cost_triplet_octets, csrc/label_step.cpp) in each of its three launch forms -- the fused triclique move, the
strain-only packed move and the general copy route --: where the costs are delivered, the timing slot a step takes (enable_timing / kernel_times), the
evaluations it counts (counters()["triplet"]), and what a hint (msm_cost_triplet_octets_prefetch) does to both when it is queued, taken, dropped or ignored.

Every case is ico4 data under the ico2 control grid: 162 control points, 320 control triangles.  The univariate class takes the same kernel family
("strain") in the packed form and on the general route, so routes()["move"] cannot tell the two apart: the general route shows in the hint, which it ignores.

The timing slots of a queued step are the parent's (the commit before label_step.cpp existed, on which this file was first run): the slot is taken when the
step is queued, the call that takes the step adds none, and a dropped step keeps the slot it took (so a prefetch and the other step that drops it make two)."""
import functools

import numpy as np
import pytest

import move_fallback_cases as C
import newmsm_amd as M
from newmsm_amd import problem
from helpers import HCP

pytestmark = pytest.mark.gpu

# (form, kind, D, MSMHIP_OCTETS=copy)
FORMS = [("fused", "ho_univariate", 1, False), ("fused", "ho_multivariate", 16, False), ("strain", "univariate", 1, False), ("general", "univariate", 1, True)]
QUEUED = [f for f in FORMS if f[0] != "general"]


@functools.lru_cache(maxsize=None)
def inputs(D):
    return problem.pairwise_inputs(4, 2, D=D)


def make(ctx, kind, inp, **params):
    cf, _ = problem.build_cost(ctx, inp, kind=kind, **dict(HCP, **params))
    cf.get_source_data()
    assert cf.N == 162 and cf.T == 320
    return cf  # (holds its meshes)


def labelings(cf):
    """a mixed labeling, the label of its step, and another label"""
    rng = np.random.default_rng(77)
    lab = rng.integers(0, cf.L, cf.N).astype(np.int32)
    return lab, 4, 7


def is_form(cf, form):
    move = cf.routes()["move"]
    return move.startswith("fused") if form == "fused" else move == "strain"


class Ledger:
    """what a call adds: timing slots, counted triplet evaluations, (taken, dropped).  kernel_times() resolves a queued step, so it is read around
    whole sequences only"""

    def __init__(self, cf):
        self.cf = cf

    def read(self):
        return self.cf.counters()["triplet"], np.array(self.cf.prefetch_stats())  # neither touches a queued step

    def run(self, call, slots, evals, taken=0, dropped=0):
        n0 = len(self.cf.kernel_times())
        e0, s0 = self.read()
        got = call()
        n1 = len(self.cf.kernel_times())  # (drops a step that call() left queued)
        e1, s1 = self.read()
        print("slots %+d evaluations %+d stats %s" % (n1 - n0, e1 - e0, s1 - s0))
        assert n1 - n0 == slots and e1 - e0 == evals and tuple(s1 - s0) == (taken, dropped), (n1 - n0, e1 - e0, s1 - s0)
        return got


@pytest.mark.parametrize("form,kind,D,copy", FORMS)
def test_deliveries_slots_and_counters(ctx, monkeypatch, form, kind, D, copy):
    if copy:
        monkeypatch.setenv("MSMHIP_OCTETS", "copy")
    cf = make(ctx, kind, inputs(D))
    lab, label, other = labelings(cf)
    A, B = ctx.host_array((cf.T, 8)), ctx.host_array((cf.T, 8))
    T8 = 8 * cf.T
    cf.enable_timing(True)
    led = Ledger(cf)
    # the three deliveries: a pageable array, the caller's mapped array, (below) prefetched and taken
    plain = led.run(lambda: cf.tripletOctets(lab, label), 1, T8)
    assert is_form(cf, form) and np.isfinite(plain).all()
    A[:] = -1.0
    assert led.run(lambda: cf.tripletOctets(lab, label, A), 1, T8) is A and np.array_equal(A, plain)
    assert is_form(cf, form)
    plain_other = led.run(lambda: cf.tripletOctets(lab, other), 1, T8)
    assert not np.array_equal(plain, plain_other)
    # a hint into a pageable array is ignored in every form: nothing launched, nothing counted
    led.run(lambda: cf.prefetchTripletOctets(lab, label, np.zeros((cf.T, 8))), 0, 0)
    if form == "general":
        # the general route is never queued ahead, the caller's mapped array or not
        A[:] = -1.0
        led.run(lambda: cf.prefetchTripletOctets(lab, label, A), 0, 0)
        assert (A == -1.0).all()
        assert np.array_equal(led.run(lambda: cf.tripletOctets(lab, label, A), 1, T8), plain)
        # the variable is read by every call: without it the packed form is back, and its hint is honoured
        monkeypatch.delenv("MSMHIP_OCTETS")
    # queued: counted (and its slot taken) at launch; the call that takes it adds neither
    A[:] = -1.0
    e0, s0 = led.read()

    def queue_and_take():
        cf.prefetchTripletOctets(lab, label, A)
        e1, s1 = led.read()
        assert e1 - e0 == T8 and tuple(s1 - s0) == (0, 0)
        got = cf.tripletOctets(lab, label, A)
        assert led.read()[0] == e1
        return got

    assert led.run(queue_and_take, 1, T8, taken=1) is A
    if form == "general":
        assert np.isfinite(A).all() and (A != -1.0).any()  # (the packed kernel's sums: not compared with the general kernel's bit for bit)
        cf.close()
        return
    assert np.array_equal(A, plain)
    # dropped by a step with another label: both launched, both counted, two slots
    def queue_and_drop():
        cf.prefetchTripletOctets(lab, label, A)
        return cf.tripletOctets(lab, other, B)

    assert np.array_equal(led.run(queue_and_drop, 2, 2 * T8, dropped=1), plain_other)
    # dropped by an entry point that launches nothing (kernel_times itself): the queued step keeps its slot and its count
    led.run(lambda: cf.prefetchTripletOctets(lab, label, A), 1, T8, dropped=1)
    assert np.array_equal(led.run(lambda: cf.tripletOctets(lab, label, A), 1, T8), plain)
    cf.close()


@pytest.mark.parametrize("kind,form", [("ho_univariate", "fused"), ("univariate", "strain")])
def test_labeling_too_wide_for_the_kernel_arguments(ctx, kind, form):
    """277 labels: the labeling travels as a device array (k_ho_move<false, .>; the strain class takes the general route).  Into the caller's mapped
    array the costs are those of the pageable delivery bit for bit, and a hint is ignored because the labeling is not packed"""
    cf = make(ctx, kind, C.star(C.MOVE_SHAPE, 1, C.MANY_LABELS), lambda_=C.LAMBDA)
    assert cf.L == 277
    lab, label = C.labelings(cf.N, cf.L)[1]
    assert lab.max() > 255
    A = ctx.host_array((cf.T, 8))
    T8 = 8 * cf.T
    cf.enable_timing(True)
    led = Ledger(cf)
    plain = led.run(lambda: cf.tripletOctets(lab, label), 1, T8)
    assert is_form(cf, form) and np.isfinite(plain).all()
    A[:] = -1.0
    assert led.run(lambda: cf.tripletOctets(lab, label, A), 1, T8) is A and np.array_equal(A, plain)
    A[:] = -1.0
    led.run(lambda: cf.prefetchTripletOctets(lab, label, A), 0, 0)
    assert (A == -1.0).all()
    assert np.array_equal(led.run(lambda: cf.tripletOctets(lab, label, A), 1, T8), plain)
    cf.close()


@pytest.mark.parametrize("form,kind,D,copy", QUEUED)
def test_labeling_out_of_range(ctx, form, kind, D, copy):
    """an entry == L: the step and the hint both refuse it (the hint also where it would have been ignored), nothing is launched or queued, and the next
    valid step is the one from before"""
    cf = make(ctx, kind, inputs(D))
    lab, label, _ = labelings(cf)
    A = ctx.host_array((cf.T, 8))
    cf.enable_timing(True)
    led = Ledger(cf)
    before = led.run(lambda: cf.tripletOctets(lab, label, A), 1, 8 * cf.T).copy()
    bad = lab.copy()
    bad[7] = cf.L
    calls = [lambda: cf.tripletOctets(bad, label), lambda: cf.tripletOctets(bad, label, A), lambda: cf.prefetchTripletOctets(bad, label, A),
             lambda: cf.prefetchTripletOctets(bad, label, np.zeros((cf.T, 8)))]

    def refused(call):
        with pytest.raises(M.MsmError, match=r"labeling\[7\] out of range"):
            call()

    for call in calls:
        led.run(lambda: refused(call), 0, 0)
    assert np.array_equal(led.run(lambda: cf.tripletOctets(lab, label, A), 1, 8 * cf.T), before)
    assert is_form(cf, form)
    cf.close()


@pytest.mark.parametrize("kind,D", [("ho_univariate", 1), ("ho_multivariate", 16)])
def test_single_form_after_a_queued_step(ctx, kind, D):
    """evaluateTotalCostSum drops the queued step and runs the single-combination move: T evaluations and one slot of its own, its triplet part
    combination 000 of the label step"""
    cf = make(ctx, kind, inputs(D))
    lab, label, _ = labelings(cf)
    A = ctx.host_array((cf.T, 8))
    cf.enable_timing(True)
    led = Ledger(cf)

    def queue_then_total():
        cf.prefetchTripletOctets(lab, label, A)
        return cf.evaluateTotalCostSum(lab)

    tot, parts = led.run(queue_then_total, 2, 8 * cf.T + cf.T, dropped=1)
    assert cf.routes()["move"].startswith("fused") and np.isfinite(tot)
    E = led.run(lambda: cf.tripletOctets(lab, label), 1, 8 * cf.T)
    assert abs(parts[2] - E[:, 0].sum()) <= 1e-9 * abs(parts[2])
    cf.close()
