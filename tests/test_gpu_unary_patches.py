"""The unary table over patches of hundreds to thousands of points (tests/unary_patch_cases.py: coarse control grids under fine data grids) against the
oracle: the WHOLE table, every entry finite (tests/test_unary_patches_cpu.py), computed twice and bit-equal, the fix-up counters zero afterwards, and
the route the test is about asserted through the launch plan the launchers acted on (DiscreteCostFunction.unary_launch(), msm_cost_unary_launch) and
routes(), so that a change of a threshold makes the test say that it no longer covers what it claims.

Launch decisions that depend on the largest patch pmax (unary_plan.cpp: unary_plan) and the test that pins each:
  pmax > 96          k_unary_reduce_flat's tail loops behind the 96 values per label kept in registers      test_flat_reduction_tails, _with_weights, _many_labels
  nsplit 4 -> L      label ranges per control point (L = 19: 4 up to 571 points, one label per workgroup from 817) test_complete_sampler
  lper * P > 768     several kChunk passes of k_unary_samples, its queue, its fused DICE reduction + redo list  test_complete_sampler, test_fused_dice
  samples LDS        > 64 KB: attribute (C; F: 157.5 KB); > 160 KB: refused (G)                                 test_complete_sampler, test_complete_sampler_near_and_beyond_a_workgroups_lds
  rays LDS           > 64 KB: attribute (F, G, H); > 160 KB: refused (X)                                        test_flat_reduction_tails, test_beyond_64_kb, test_too_large_everywhere
  reduction LDS      16 pmax > 64 KB: attribute (G, H; DICE too)                                                 test_beyond_64_kb
  64 pmax            patchwise DICE: <= 64 KB (A), attribute (D), one wavefront with a quarter of it (F)         test_patchwise_dice_lds_tiers
  eight-point walks  k_unary_reduce_features / _mv8 / _pw8<4> / _pw8<8> over 2 875 points                        test_multivariate_reductions

Tolerance: the module's bar for the univariate class, rtol 1e-10 / atol 1e-12 (tests/test_gpu_unary.py), and 1e-9 / 1e-11 for the multivariate and
patchwise classes (test_many_labels_and_a_single_label).  DICE costs are ratios of counts and keep the bar.  Measured on an MI355X, largest relative
difference to the oracle: 8.5e-13 (correlation, case H), 3.5e-15 (SSD), 1.5e-13 (patchwise), 4.7e-15 (multivariate), 0 (DICE): the sums over thousands
of points in another order need no wider bar."""
import numpy as np
import pytest

import unary_patch_cases as P
import unary_table_pin
from newmsm_amd import problem
from newmsm_amd._lib import MsmError

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-12
MV_RTOL, MV_ATOL = 1e-9, 1e-11
MSM_ERR_CAPACITY = -7


def complete_search(monkeypatch):
    """from here to the end of the test, targets take the complete sampler, k_unary_samples (the switch is read when a target's search structures
    are built, at its first table)"""
    monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")


def product(ctx, name, kind="univariate", D=1, sim=2, rows=0, sg_order=None):
    """the product's cost function of a case after get_source_data(), with the oracle's patches"""
    inp = P.inputs(name, D, sg_order)
    cf, keep = problem.build_cost(ctx, inp, kind=kind, simmeasure=sim, range_=P.range_of(name))
    oc = P.oracle(name, kind, D, sim, rows, sg_order)
    if rows:
        cf.set_dataaffintyweighting(P.weights(inp, rows))
    cf.get_source_data()
    ptr, idx = cf.patches()
    optr, oidx = oc.patches()
    assert np.array_equal(ptr, optr) and np.array_equal(idx, oidx)
    if rows:
        assert np.array_equal(cf.absolute_weights(), oc.absolute_weights())
    cf._keep_meshes = keep
    return cf


def table(cf):
    """the table, twice: bit-equal, and every fix-up counter zero again"""
    U = cf.computeUnaryCosts().copy()
    assert not cf.unary_fix_counters().any()
    assert np.array_equal(U, cf.computeUnaryCosts())
    assert not cf.unary_fix_counters().any()
    return U


def check(U, name, kind="univariate", D=1, sim=2, rows=0, sg_order=None, sampler="rays"):
    """against the oracle to the module's tolerance, and bit for bit against the pinned build (unary_table_pin.py)"""
    Uo = P.oracle_table(name, kind, D, sim, rows, sg_order)
    rtol, atol = (RTOL, ATOL) if kind == "univariate" else (MV_RTOL, MV_ATOL)
    assert U.shape == Uo.shape and np.isfinite(U).all()
    err = np.abs(U - Uo)
    print("%s %s D=%d sim=%d rows=%d: max abs err %.3e, max rel err %.3e" % (name, kind, D, sim, rows, err.max(), (err / np.abs(Uo).clip(1e-300)).max()))
    assert np.allclose(U, Uo, rtol=rtol, atol=atol), err.max()
    unary_table_pin.assert_pinned(U, unary_table_pin.key("patches", name, kind, D, sim, rows, sampler, sg_order))


def launch_of(cf, name, sampler, reduce):
    """the recorded plan, with what every test expects of it"""
    sizes = P.patches(name)[1]
    p = cf.unary_launch()
    assert p["pmax"] == sizes.max() and p["sampler"] == sampler and p["reduce"] == reduce == cf.routes()["unary"] and not p["refused"]
    return p, sizes


# ------------------------------------------------------------------ k_unary_reduce_flat: the tail loops behind the registers
@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("name", ["A", "C", "F"])
def test_flat_reduction_tails(ctx, name, sim):
    """ray-table sampler, every patch beyond the 96 values per label that travel through registers (A: 200..253, C: 776..1012, F: 2856..2875: the
    tail loops run 13 to 348 rounds); on F k_unary_rays needs 82 KB of LDS"""
    cf = product(ctx, name, sim=sim)
    U = table(cf)
    p, sizes = launch_of(cf, name, "rays", "flat")
    assert sizes.min() > P.FLAT_REGS and p["reduce_lds"] == 16 * p["pmax"] <= P.LDS_DEFAULT and p["reduce_threads"] == 256
    assert (p["sampler_lds"] > P.LDS_DEFAULT) == (name == "F")
    check(U, name, sim=sim)


def test_flat_reduction_tails_with_weights(ctx):
    """case A with a set_dataaffintyweighting row: sW is not all ones in either half of the sums"""
    cf = product(ctx, "A", rows=1)
    U = table(cf)
    p, sizes = launch_of(cf, "A", "rays", "flat")
    assert sizes.min() > P.FLAT_REGS
    check(U, "A", rows=1)
    assert not np.allclose(U, P.oracle_table("A"), rtol=1e-3, atol=0)  # the weights matter


def test_flat_reduction_tails_many_labels(ctx):
    """case A with the sampling grid one order finer: 57 labels for the 32 label groups of a workgroup, so that the second pass reloads its 96
    register values ("not prefetched") and then walks the tail"""
    cf = product(ctx, "A", sg_order=4)
    assert 32 < cf.L <= 64
    U = table(cf)
    p, sizes = launch_of(cf, "A", "rays", "flat")
    assert sizes.min() > P.FLAT_REGS
    check(U, "A", sg_order=4)


# ------------------------------------------------------------------ k_unary_samples: label ranges, LDS passes, LDS beyond 64 KB
@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_complete_sampler(ctx, monkeypatch, name, sim):
    """the complete-search sampler on the same cases: one common reduction, so the table is bit-equal to the ray-table one.  A: 4 label ranges of 5
    labels, 1000 to 1265 samples per workgroup (two passes); B: 15 labels, where ranges of 4 and of 3 labels would need 70 and 64.4 KB, so 8 ranges of
    2 labels, 1444 to 1452 samples (two passes); C: a workgroup per label (ranges of 2 labels fit up to 816 points), 776 to 1012 samples (two passes
    from 769 points) and up to 66.8 KB of LDS (the attribute)"""
    U_ray = table(product(ctx, name, sim=sim))
    complete_search(monkeypatch)
    cf = product(ctx, name, sim=sim)
    U = table(cf)
    p, sizes = launch_of(cf, name, "samples", "flat")
    L = cf.L
    lper = -(-L // p["nsplit"])
    assert p["nsplit"] == {"A": 4, "B": 8, "C": L}[name]
    assert lper * sizes.min() > P.CHUNK  # every workgroup makes a second LDS pass
    assert p["sampler_lds"] == 8 * (5 + lper) * p["pmax"] + 72 * L + 18432 and (p["sampler_lds"] > P.LDS_DEFAULT) == (name == "C")
    assert np.array_equal(U, U_ray)
    check(U, name, sim=sim, sampler="samples")


def refused(cf, name, which="sampler"):
    """the table is refused cleanly, with the patch size in the message, before anything of it was launched; asking again changes nothing"""
    pmax = int(P.patches(name)[1].max())
    for _ in range(2):
        with pytest.raises(MsmError, match="a patch of %d points does not fit in LDS" % pmax) as e:
            cf.computeUnaryCosts()
        assert e.value.code == MSM_ERR_CAPACITY
        p = cf.unary_launch()
        assert p["refused"] == which and p["pmax"] == pmax
        assert cf.counters()["samples"] == 0 and cf.routes()["unary"] == "none" and not cf.unary_fix_counters().any()
    return p


@pytest.mark.parametrize("sim", [2, 4])
def test_complete_sampler_near_and_beyond_a_workgroups_lds(ctx, monkeypatch, sim):
    """k_unary_samples with a workgroup per label asks for 48 pmax + 72 L + 18 432 bytes.  Case F (2875 points, 15 labels): 157 512 bytes, 6 KB below
    the 160 KB of a workgroup -- the table must be right (four passes per workgroup; with DICE the fused reduction over 2875 values per label).
    Case G (4511 points): 236 040 bytes -- refused with MSM_ERR_CAPACITY on this sampler only (test_beyond_64_kb: the ray sampler takes G); then a
    case-A table on the same context is right."""
    complete_search(monkeypatch)
    cf, cg, ca = product(ctx, "F", sim=sim), product(ctx, "G", sim=sim), product(ctx, "A", sim=sim)
    U = table(cf)
    p, sizes = launch_of(cf, "F", "samples", "univariate" if sim == 4 else "flat")
    assert p["nsplit"] == cf.L and p["sampler_lds"] == 48 * p["pmax"] + 72 * cf.L + 18432 == 157512 and sizes.min() > 3 * P.CHUNK
    check(U, "F", sim=sim, sampler="samples")
    p = refused(cg, "G")
    assert p["sampler"] == "samples" and p["sampler_lds"] == 48 * p["pmax"] + 72 * cg.L + 18432 > P.LDS_WORKGROUP
    U = table(ca)
    launch_of(ca, "A", "samples", "univariate" if sim == 4 else "flat")
    check(U, "A", sim=sim, sampler="samples")


# ------------------------------------------------------------------ DICE: k_unary_reduce_univariate, and the reduction fused into k_unary_samples
@pytest.mark.parametrize("sim", [4, 5])
@pytest.mark.parametrize("name,sampler", [("A", "rays"), ("A", "samples"), ("C", "rays"), ("C", "samples"), ("F", "rays")])
def test_fused_dice(ctx, monkeypatch, name, sampler, sim):
    """DICE and generalised DICE of the univariate class.  Ray table: k_unary_reduce_univariate over all control points.  Complete sampler: the
    reduction over sT[lper * pmax] inside k_unary_samples (A: 5 labels per workgroup, C: 1), and the redo list for the control points with
    deferred samples -- which every one of the nsplit workgroups of a control point may append to."""
    if sampler == "samples":
        complete_search(monkeypatch)
    cf = product(ctx, name, sim=sim)
    U = table(cf)
    p, sizes = launch_of(cf, name, sampler, "univariate")
    assert p["reduce_lds"] == 16 * p["pmax"] and p["nsplit"] == {"A": 4, "C": cf.L, "F": cf.L}[name]
    check(U, name, sim=sim, sampler=sampler)


# ------------------------------------------------------------------ dynamic LDS beyond 64 KB in the ray sampler and the univariate reductions
@pytest.mark.parametrize("sim", [2, 1, 4])
@pytest.mark.parametrize("name", ["G", "H"])
def test_beyond_64_kb(ctx, name, sim):
    """G (4511 points): k_unary_rays 127 KB, reduction 16 pmax = 72 KB; H (5618 points): 158 KB and 90 KB.  Both kernels need their
    attribute raised; both fit a workgroup, so the table must be there and right."""
    cf = product(ctx, name, sim=sim)
    U = table(cf)
    p, sizes = launch_of(cf, name, "rays", "univariate" if sim == 4 else "flat")
    assert p["nsplit"] == cf.L and P.LDS_DEFAULT < p["sampler_lds"] == 28 * p["pmax"] + 72 * cf.L + 32 <= P.LDS_WORKGROUP
    assert P.LDS_DEFAULT < p["reduce_lds"] == 16 * p["pmax"] <= P.LDS_WORKGROUP
    check(U, name, sim=sim)


# ------------------------------------------------------------------ multivariate / patchwise reductions over 2875 points
MV = [("multivariate", 3, "features"), ("patchwise", 3, "features"), ("multivariate", 12, "mv8"), ("patchwise", 12, "pw8<4>"), ("patchwise", 40, "pw8<8>")]


@pytest.mark.parametrize("sim", [2, 1])
@pytest.mark.parametrize("kind,D,route", MV)
def test_multivariate_reductions(ctx, kind, D, route, sim):
    """case F: the reductions that walk a patch 64 or eight points at a time, over 2856 to 2875 points (359 to 360 rounds of eight, the last one
    partly filled)"""
    cf = product(ctx, "F", kind, D, sim)
    U = table(cf)
    p, sizes = launch_of(cf, "F", "rays", route)
    assert p["reduce_lds"] == 0 and p["sampler_lds"] > P.LDS_DEFAULT and (sizes % 8 != 0).any()
    check(U, "F", kind, D, sim)


@pytest.mark.parametrize("kind,route", [("multivariate", "mv8"), ("patchwise", "pw8<4>")])
def test_multivariate_reductions_with_a_weight_row_per_dimension(ctx, kind, route):
    cf = product(ctx, "F", kind, 12, 2, rows=12)
    U = table(cf)
    launch_of(cf, "F", "rays", route)
    check(U, "F", kind, 12, 2, rows=12)


# ------------------------------------------------------------------ patchwise DICE: k_unary_reduce_features with two LDS patches per wavefront
@pytest.mark.parametrize("name", ["A", "D", "F"])
def test_patchwise_dice_lds_tiers(ctx, name):
    """64 pmax bytes for four wavefronts.  A (253 points): 16 KB; D (1230 points): 77 KB, the attribute; F (2875 points): 180 KB do not fit, so one
    wavefront per control point with 16 pmax = 45 KB"""
    cf = product(ctx, name, "patchwise", 3, 4)
    U = table(cf)
    p, sizes = launch_of(cf, name, "rays", "features")
    if name == "A":
        assert (p["reduce_threads"], p["reduce_lds"]) == (256, 64 * p["pmax"]) and p["reduce_lds"] <= P.LDS_DEFAULT
    elif name == "D":
        assert (p["reduce_threads"], p["reduce_lds"]) == (256, 64 * p["pmax"]) and P.LDS_DEFAULT < p["reduce_lds"] <= P.LDS_WORKGROUP
    else:
        assert (p["reduce_threads"], p["reduce_lds"]) == (64, 16 * p["pmax"]) and 64 * p["pmax"] > P.LDS_WORKGROUP
    check(U, name, "patchwise", 3, 4)


# ------------------------------------------------------------------ beyond every kernel's LDS
def test_too_large_everywhere(ctx, monkeypatch):
    """case X: patches of 11 435 to 11 512 points.  k_unary_rays would need 323 KB, k_unary_samples 572 KB: every class is refused on the host, on
    either sampler, with the patch size in the message; nothing of the table is launched, and the context goes on to compute case A"""
    def all_refused(made):
        for cf in made:
            p = refused(cf, "X")
            assert p["sampler_lds"] > P.LDS_WORKGROUP
            ptr, _ = cf.patches()  # the cost function still answers
            assert np.diff(ptr).max() == p["pmax"]

    all_refused([product(ctx, "X", kind, 1, sim) for kind, sim in [("univariate", 2), ("univariate", 4), ("multivariate", 2), ("patchwise", 4)]])
    ca = product(ctx, "A")
    U = table(ca)
    launch_of(ca, "A", "rays", "flat")
    check(U, "A")
    complete_search(monkeypatch)
    all_refused([product(ctx, "X")])
    ca = product(ctx, "A")
    U = table(ca)
    launch_of(ca, "A", "samples", "flat")
    check(U, "A", sampler="samples")
