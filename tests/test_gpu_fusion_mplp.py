"""MPLP over the binary problem of one label step on the GPU: k_fusion_mplp -- one launch of one workgroup -- against the host literal
msm_fusion_mplp_step bit for bit in every output, with the messages in LDS and in global memory; the cost function's route (octets and unary costs
staying on the device) in each launch form of the label step; and the fusion level loop with the opt-in solve on either route."""
import functools

import numpy as np
import pytest

import fusion_mplp_cases as FC
import strain_collapse_cases as SC
import newmsm_amd as M
from newmsm_amd import api, problem, registration, synthetic
from newmsm_amd._lib import lib
from helpers import HCP
from test_fusion_mplp_cpu import CASES, _refusals, refused_with_x_untouched

pytestmark = pytest.mark.gpu

GPU_CASES = dict(CASES, **{"ico3 rough": dict(order=3, kind="rough"), "ico3 smooth": dict(order=3, kind="smooth"), "ico3 settled": dict(order=3, kind="settled")})


@functools.lru_cache(maxsize=None)
def literal(name, sweeps, polish):
    """the host literal's result, computed once per case"""
    return api.fusion_mplp_step(*FC.case(**GPU_CASES[name]), sweeps=sweeps, polish=polish)


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_one_launch_gives_the_literals_bits(ctx, name):
    case = FC.case(**GPU_CASES[name])
    for sweeps, polish in ((0, 0), (1, 0), (12, 0), (0, 3), (5, 1), (12, 8)):
        got = api.fusion_mplp_step_gpu(ctx, *case, sweeps=sweeps, polish=polish)
        FC.same(got, literal(name, sweeps, polish), (name, sweeps, polish))
        stats = api.fusion_mplp_gpu_stats(ctx)
        assert stats["launches"] == 1 and stats["sweeps_run"] == got.sweeps_run and stats["kernel_ms"] > 0.0
        assert stats["levels_per_sweep"] == len(api.mcmc_schedule(case[2], len(case[0]))[2]) - 1
    print(name, stats, "passes", got.passes_run)
    if name == "ico3 rough":
        assert got.sweeps_run == 12 and stats["levels_per_sweep"] == 28 and api.mplp_colouring(case[2], 642)[1] == 6
    if name.endswith("settled"):
        assert got.sweeps_run == 1


@pytest.mark.parametrize("where", ["lds", "global"])
@pytest.mark.parametrize("name", ["ico1 rough lone node", "ico2 rough shuffled", "ico3 rough", "ico2 settled"])
def test_both_message_placements_give_the_same_bits(ctx, monkeypatch, name, where):
    monkeypatch.setenv("MSMHIP_FUSION_MSG", where)
    case = FC.case(**GPU_CASES[name])
    for sweeps, polish in ((12, 0), (12, 8)):
        FC.same(api.fusion_mplp_step_gpu(ctx, *case, sweeps=sweeps, polish=polish), literal(name, sweeps, polish), (name, where, sweeps, polish))


def test_message_placement_variable_is_checked(ctx, monkeypatch):
    case = FC.case(0, "rough")
    monkeypatch.setenv("MSMHIP_FUSION_MSG", "registers")
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*MSMHIP_FUSION_MSG=registers \\(lds or global\\)"):
        api.fusion_mplp_step_gpu(ctx, *case)
    monkeypatch.delenv("MSMHIP_FUSION_MSG")
    FC.same(api.fusion_mplp_step_gpu(ctx, *case, sweeps=4, polish=2), api.fusion_mplp_step(*case, sweeps=4, polish=2))


def test_no_unary_costs_and_no_triplets(ctx):
    _, octets, triplets = FC.case(1, "rough")
    FC.same(api.fusion_mplp_step_gpu(ctx, None, octets, triplets, sweeps=6, polish=4, N=42), api.fusion_mplp_step(None, octets, triplets, sweeps=6, polish=4, N=42))
    lone = np.array([[1.0, 0.5], [0.25, 2.0], [3.0, 3.0]])
    FC.same(api.fusion_mplp_step_gpu(ctx, lone, None, None, sweeps=4, polish=2), api.fusion_mplp_step(lone, None, None, sweeps=4, polish=2))
    FC.same(api.fusion_mplp_step_gpu(ctx, np.zeros((42, 2)), np.zeros((80, 8)), triplets, sweeps=7, polish=3),
            api.fusion_mplp_step(np.zeros((42, 2)), np.zeros((80, 8)), triplets, sweeps=7, polish=3))


def test_node_with_more_slots_than_a_record_lists(ctx):
    """the fan of mplp_literal.py: hub 0 lies on twelve triangles, so each of its slots has eleven others -- more than the seven a slot's record
    lists, and the update walks the incidence lists instead; the rim nodes (one other slot) and node 13 (none) take the listed route"""
    import mplp_literal as ML

    triplets = ML.fan_case()[2]
    rng = np.random.default_rng(5)
    unary2, octets = rng.uniform(0.0, 1.0, (14, 2)), rng.uniform(-2.0, 2.0, (12, 8))
    for sweeps, polish in ((12, 0), (12, 8)):
        FC.same(api.fusion_mplp_step_gpu(ctx, unary2, octets, triplets, sweeps=sweeps, polish=polish),
                api.fusion_mplp_step(unary2, octets, triplets, sweeps=sweeps, polish=polish), ("fan", sweeps, polish))


def test_refusals_are_the_host_literals(ctx):
    ok, cases = _refusals()
    api.fusion_mplp_step_gpu(ctx, *ok, sweeps=4, polish=2)
    for args, kw, pattern in cases:
        refused_with_x_untouched(lambda *a: lib().msm_fusion_mplp_step_gpu(ctx.h, *a), args, kw, pattern)
    FC.same(api.fusion_mplp_step_gpu(ctx, *ok, sweeps=4, polish=2), api.fusion_mplp_step(*ok, sweeps=4, polish=2))  # and the context is as good as before


# ---------------------------------------------------------------- the cost function's route

# (form, kind, D, MSMHIP_OCTETS=copy): the packed strain move, the fused triclique move, the copied route
FORMS = [("strain", "univariate", 1, False), ("fused", "ho_univariate", 1, False), ("general", "univariate", 1, True)]


@functools.lru_cache(maxsize=None)
def inputs(D):
    return problem.pairwise_inputs(4, 2, D=D)  # data ico4 / control ico2, 19 labels


def make(ctx, kind, inp):
    cf, keep = problem.build_cost(ctx, inp, kind=kind, **HCP)
    cf.get_source_data()
    assert cf.N == 162 and cf.T == 320 and cf.L == 19
    return cf, keep


def step_tables(cf, lab, label):
    """unary2 and octets of the step, fetched: what the host literal is fed with"""
    U = cf.computeUnaryCosts()
    unary2 = np.stack([U[lab, np.arange(cf.N)], U[label]], axis=1)
    return unary2, np.array(cf.tripletOctets(lab, label))


@pytest.mark.parametrize("form,kind,D,copy", FORMS)
def test_cost_route_in_every_launch_form(ctx, monkeypatch, form, kind, D, copy):
    if copy:
        monkeypatch.setenv("MSMHIP_OCTETS", "copy")
    inp = inputs(D)
    cf, keep = make(ctx, kind, inp)
    lab = np.random.default_rng(77).integers(0, cf.L, cf.N).astype(np.int32)
    label, other = 4, 7
    unary2, octets = step_tables(cf, lab, label)
    after_plain = cf.routes(), cf.unary_fix_counters()
    assert after_plain[0]["move"].startswith("fused") if form == "fused" else after_plain[0]["move"] == "strain"
    want = api.fusion_mplp_step(unary2, octets, inp["triplets"], sweeps=10, polish=8)
    e0 = cf.counters()["triplet"]
    got = cf.fusion_mplp_step(lab, label, sweeps=10, polish=8)
    FC.same(got, want, form)
    assert cf.counters()["triplet"] - e0 == 8 * cf.T and cf.routes() == after_plain[0] and np.array_equal(cf.unary_fix_counters(), after_plain[1])
    assert api.fusion_mplp_gpu_stats(ctx)["launches"] == 1 + (cf.routes()["move_deferred"] > 0)
    print(form, cf.routes(), api.fusion_mplp_gpu_stats(ctx), "E(0)", got.energies[0], "E", got.energy, "bound", got.bound, "sweeps", got.sweeps_run)
    # a step queued ahead, for another label and for the same one: dropped, and nothing else changes
    A = ctx.host_array((cf.T, 8))
    for queued in (other, label):
        cf.prefetchTripletOctets(lab, queued, A)
        FC.same(cf.fusion_mplp_step(lab, label, sweeps=10, polish=8), want, (form, "queued", queued))
        assert cf.routes() == after_plain[0] and np.array_equal(cf.unary_fix_counters(), after_plain[1])
    # other sweep and polish counts over the same step, the message placement forced
    for where in ("lds", "global"):
        monkeypatch.setenv("MSMHIP_FUSION_MSG", where)
        FC.same(cf.fusion_mplp_step(lab, label, sweeps=3, polish=0), api.fusion_mplp_step(unary2, octets, inp["triplets"], sweeps=3, polish=0), (form, where))
    monkeypatch.delenv("MSMHIP_FUSION_MSG")
    # refusals of the arguments leave the cost function as it was
    for kw, pattern in ((dict(sweeps=1025), "1025 sweeps"), (dict(polish=-1), "-1 polish passes")):
        with pytest.raises(M.MsmError, match=pattern):
            cf.fusion_mplp_step(lab, label, **kw)
    bad = lab.copy()
    bad[7] = cf.L
    with pytest.raises(M.MsmError, match=r"labeling\[7\] out of range"):
        cf.fusion_mplp_step(bad, label)
    FC.same(cf.fusion_mplp_step(lab, label, sweeps=10, polish=8), want, (form, "after the refusals"))
    cf.close()


def test_cost_route_fills_the_unary_table_itself(ctx):
    """a cost function whose unary table has not been computed yet: the step computes it, as msm_cost_mplp_optimise does, and later steps reuse it"""
    inp = inputs(1)
    cf, keep = make(ctx, "univariate", inp)
    lab = np.random.default_rng(78).integers(0, cf.L, cf.N).astype(np.int32)
    samples = cf.counters()["samples"]
    first = cf.fusion_mplp_step(lab, 3, sweeps=6, polish=2)
    filled = cf.counters()["samples"]
    assert filled > samples
    again = cf.fusion_mplp_step(lab, 3, sweeps=6, polish=2)
    assert cf.counters()["samples"] == filled  # the table was reused
    want = api.fusion_mplp_step(*step_tables(cf, lab, 3), inp["triplets"], sweeps=6, polish=2)
    FC.same(first, want, "first")
    FC.same(again, want, "again")
    cf.close()


def test_cost_route_refuses_a_non_finite_octet(ctx):
    """the label steps of strain_collapse_cases.py that meet collapsed triangles: their octets hold NaN or infinity, the step is refused by the table's
    name with x untouched, and the cost function solves a clean step of the same labelling's centre afterwards as before"""
    cf, keep = SC.product_cost(ctx)
    triplets = SC.inputs()["triplets"]
    tab = np.array(cf.computeTripletCosts())
    clean_lab = np.zeros(cf.N, dtype=np.int32)
    clean = [label for label in range(1, cf.L) if np.isfinite(SC.octets_from_table(tab, triplets, clean_lab, label)).all()][0]
    want = api.fusion_mplp_step(*step_tables(cf, clean_lab, clean), triplets, sweeps=5, polish=2)
    FC.same(cf.fusion_mplp_step(clean_lab, clean, sweeps=5, polish=2), want, "before")
    for lab, label, n in SC.collapse_moves(tab, triplets, cf.N, keep=2):
        assert n >= 1
        with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*msm_cost_fusion_mplp_step: the octet table holds a non-finite value"):
            cf.fusion_mplp_step(lab, label, sweeps=5, polish=2)
    FC.same(cf.fusion_mplp_step(clean_lab, clean, sweeps=5, polish=2), want, "after the refusals")
    cf.close()


# ---------------------------------------------------------------- the level loop

def level(ctx, mplp_gpu, speculate):
    """two iterations of the fusion level loop at cp ico2 with the MPLP solve: (labelings, per-step traces).  labeldist 0.4: at the default 0.5 the
    sampling grid's own vertices let neighbouring control points meet, and a collapsed triangle's non-finite cost is refused (test_gpu_mplp.py)"""
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 1, 21)
    src = synthetic.features(synthetic.known_warp(xyz, seed=23, rot_deg=4.0, amp=2.5), 1, 21)
    ops = registration.ProductOps(ctx, mplp_gpu=mplp_gpu, fusion_mplp=True, fusion_sweeps=10, fusion_polish=8)
    trace = []
    out = registration.run_discrete_level(ops, xyz, tri, ref, xyz, tri, src, xyz, cp_order=2, iters=2, kind="univariate", optimiser="fusion",
                                          cost_params=dict(lambda_=0.0005), labeldist=0.4, speculate=speculate, fusion_trace=trace)
    return out[3], trace


def test_level_loop_routes_agree_and_every_step_descends(ctx):
    base, trace = level(ctx, True, True)
    assert len(base) == 2 and len(trace) > 0
    for mplp_gpu, speculate in ((True, False), (False, True), (False, False)):
        labs, tr = level(ctx, mplp_gpu, speculate)
        assert len(labs) == len(base) and all(np.array_equal(a, b) for a, b in zip(labs, base)), (mplp_gpu, speculate)
        assert len(tr) == len(trace)
        for (i0, l0, r0), (i1, l1, r1) in zip(trace, tr):
            assert (i0, l0) == (i1, l1)
            FC.same(r1, r0, (mplp_gpu, speculate, i0, l0))
    for it, label, r in trace:
        assert r.energy <= r.energies[0], (it, label, r.energy, r.energies[0])  # never worse than changing nothing
        assert r.bound <= r.energy + 1e-9 * max(1.0, abs(r.energy))
    moved = sum(int(r.x.any()) for _, _, r in trace)
    print("label steps solved", len(trace), "steps that moved a node", moved, "labels in use", [len(np.unique(l)) for l in base])
    assert moved > 0


# ---------------------------------------------------------------- the executables

# the two-level configuration of the executable tests (test_gpu_mplp_round.py) with --dopt=HOCR; --rescaleL keeps the control points apart
CONF = ("--simval=2,2\n--sigma_in=2,2\n--sigma_ref=2,2\n--lambda=0.2,0.2\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=2,3\n--SGgrid=4,5\n--datagrid=4,5\n"
        "--regoption=3\n--regexp=2\n--dopt=HOCR\n--VN\n--k_exponent=2\n--bulkmod=1.6\n--shearmod=0.4\n--rescaleL\n")


def test_both_executables(ctx, tmp_path):
    """MSMHIP_FUSION=mplp MSMHIP_FUSION_SWEEPS=6 MSMHIP_FUSION_POLISH=4: tools/register_files.py and tools/cpp/newmsm write the same bytes, which are not
    the stand-in's; unset and MSMHIP_FUSION=icm write the stand-in's bytes alike"""
    import os
    import subprocess
    import sys

    import __graft_entry__ as g
    from newmsm_amd import meshio

    exe = g.build_cpp_newmsm()
    xyz, tri = M.make_mesh_from_icosa(5)
    ref = synthetic.features(xyz, 2, 5)
    src = synthetic.features(synthetic.known_warp(xyz, seed=8, rot_deg=3.0, amp=2.0), 2, 5)
    d = str(tmp_path) + "/"
    with open(d + "conf", "w") as f:
        f.write(CONF)
    meshio.save_surface(d + "in.surf.gii", synthetic.known_warp(xyz, seed=3, rot_deg=0.0, amp=0.7) + 0.25, tri)
    meshio.save_surface(d + "ref.surf.gii", xyz, tri)
    meshio.save_metric(d + "in.func.gii", src)
    meshio.save_metric(d + "ref.func.gii", ref)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--inmesh=" + d + "in.surf.gii", "--refmesh=" + d + "ref.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "ref.func.gii", "--conf=" + d + "conf"]
    plain = {k: v for k, v in os.environ.items() if not k.startswith("MSMHIP_FUSION")}
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    runs = [("py.mplp.", [sys.executable, "tools/register_files.py"], dict(MSMHIP_FUSION="mplp", MSMHIP_FUSION_SWEEPS="6", MSMHIP_FUSION_POLISH="4")),
            ("cpp.mplp.", [exe], dict(MSMHIP_FUSION="mplp", MSMHIP_FUSION_SWEEPS="6", MSMHIP_FUSION_POLISH="4")),
            ("cpp.unset.", [exe], {}), ("cpp.icm.", [exe], dict(MSMHIP_FUSION="icm"))]
    for tag, cmd, env in runs:
        run = subprocess.run(cmd + common + ["--out=" + d + tag], cwd=root, env=dict(plain, **env), capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, (tag, run.stdout, run.stderr)

    def read(tag, n):
        with open(d + tag + n, "rb") as f:
            return f.read()

    for n in names:
        assert read("py.mplp.", n) == read("cpp.mplp.", n), "%s differs between the two executables" % n
        assert read("cpp.unset.", n) == read("cpp.icm.", n), "%s: MSMHIP_FUSION=icm is not the default" % n
    assert read("cpp.mplp.", names[0]) != read("cpp.icm.", names[0])  # the solve took part
