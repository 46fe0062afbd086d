"""MPLP and its rounding under the forbidden-entry reading on the GPU (msm_mplp_optimise_forbid_gpu, msm_mplp_round_forbid_gpu, msm_cost_set_mplp_forbid;
newmsm_amd/csrc/mplp.cpp, mplp_kernels.hip; DESIGN.md 5.19 "Forbidden entries").  Every case asks for the host literal's bits (msm_mplp_optimise_forbid,
msm_mplp_round_forbid, which tests/test_mplp_forbid_cpu.py holds against the numpy restatement) on the same arguments: labelling, sweeps_run, energies,
bounds, messages, passes_run, and the device's classification counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, config, registration, synthetic

import mplp_forbid_literal as FL
import mplp_literal as ML
import mplp_round_literal as RL
from tests import strain_collapse_cases as SC

pytestmark = pytest.mark.gpu
INF = np.inf


def _both(ctx, case, sweeps=6, polish=3, modes=(0, 1), what=""):
    """the sweeps on both sides, then the rounding of the host's messages on both sides; the sweeps' result"""
    U, tc, triplets, start = case
    hc, gc = np.full(4, -1, dtype=np.int64), np.full(4, -1, dtype=np.int64)
    want = api.mplp_optimise(*case, sweeps=sweeps, bounds=True, messages=True, forbid=True, counts=hc)
    got = api.mplp_optimise_gpu(ctx, *case, sweeps=sweeps, bounds=True, messages=True, forbid=True, counts=gc)
    ML.same(got, want, what)
    assert gc.tolist() == hc.tolist() == api.mplp_classify(U, tc).tolist(), (what, gc, hc)
    assert api.mplp_gpu_stats(ctx)["sweeps_run"] == want.sweeps_run
    ML.same(api.mplp_optimise_gpu(ctx, *case, sweeps=sweeps, bound=True, forbid=True), want, what)  # the bound alone: one pass after the last sweep
    for mode in modes:
        gc[:] = -1
        w = api.mplp_round(U, tc, triplets, want.labeling, messages=want.messages, mode=mode, polish=polish, forbid=True)
        g = api.mplp_round_gpu(ctx, U, tc, triplets, want.labeling, messages=want.messages, mode=mode, polish=polish, forbid=True, counts=gc)
        RL.same(g, w, (what, "mode", mode))
        assert gc.tolist() == hc.tolist() and api.mplp_round_gpu_stats(ctx)["passes_run"] == w.passes_run
    return got


@pytest.mark.parametrize("name", sorted(FL.CASES))
def test_the_cpu_cases(ctx, name):
    got = _both(ctx, FL.CASES[name](), what=name)
    if name == "triplet L1 forbidden":
        assert got.bound == INF and got.energy == INF and np.all(got.messages == INF)
    if name == "fan":
        assert got.messages[0, 0, 1] == INF and got.labeling[0] != 1
        assert np.isinf(got.messages[:, 0, 1]).all()  # every factor's cavity at hub label 1 holds factor 0's +inf: staged, folded and written as +inf


@pytest.mark.parametrize("name,sweeps", [("ico0 L20", 5), ("ico0 L61", 3), ("ico0 L67", 3), ("ico2 L7 shuffled", 4)])
def test_label_counts_round_the_kernels_thresholds(ctx, name, sweeps):
    """L^3 a multiple of 256 and not; 32 key copies at 61 and 67 labels, and at 67 more labels than a wavefront has lanes in the decode and the polish;
    a shuffled triplet list with many levels"""
    got = _both(ctx, FL.GPU_CASES[name](), sweeps=sweeps, polish=2, what=name)
    assert got.labeling.any()


@pytest.mark.parametrize("slots", ["1", "4"])
def test_fewer_copies_of_the_minima_in_lds(ctx, monkeypatch, slots):
    monkeypatch.setenv("MSMHIP_MPLP_SLOTS", slots)
    _both(ctx, FL.CASES["ico0 L19"](), what="slots " + slots)
    _both(ctx, FL.CASES["fan"](), what="fan, slots " + slots)


def test_a_run_longer_than_a_chunk_reaches_its_fixed_point(ctx):
    """300 sweeps are more than one chunk of 256: two triangles sharing a node reach their fixed point after 46 of them (the launches behind it return
    at once), the infeasible octahedron runs them all"""
    got = _both(ctx, FL.CASES["two triangles"](), sweeps=300, modes=(0,), what="fixed point")
    assert 3 < got.sweeps_run < 300
    _both(ctx, FL.octahedron(FL.OCTAHEDRON_SEEDS[-1]), sweeps=300, modes=(0,), what="infeasible octahedron")


@pytest.mark.parametrize("args", [(0, 19, 11), (0, 19, 13, 0.05)])
def test_equivalence_on_tables_without_forbidden_entries(ctx, args):
    case = ML.ico_case(*args)
    counts = np.full(4, -1, dtype=np.int64)
    plain = api.mplp_optimise_gpu(ctx, *case, sweeps=6, bounds=True, messages=True)
    ML.same(api.mplp_optimise_gpu(ctx, *case, sweeps=6, bounds=True, messages=True, forbid=True, counts=counts), plain)
    ML.same(api.mplp_optimise(*case, sweeps=6, bounds=True, messages=True, forbid=True), plain)
    assert counts.tolist() == [0, 0, 0, 0]
    for mode in (0, 1):
        RL.same(api.mplp_round_gpu(ctx, *case, messages=plain.messages, mode=mode, polish=4, forbid=True, counts=counts),
                api.mplp_round_gpu(ctx, *case, messages=plain.messages, mode=mode, polish=4))
        assert counts.tolist() == [0, 0, 0, 0]


def test_refusals_are_the_host_literals(ctx):
    ok, cases = FL.refusal_cases()
    _both(ctx, ok, sweeps=2)
    before = api.mplp_gpu_stats(ctx)
    for args, pattern in cases:
        lab = np.array(args[3])
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_optimise_gpu(ctx, *args, sweeps=3, forbid=True)
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_round_gpu(ctx, *args, mode=1, polish=2, forbid=True)
        assert np.array_equal(lab, args[3])
    T, L = len(ok[2]), ok[0].shape[0]
    for value, pattern in ((np.nan, "MSM_ERR_INVALID.*the messages hold a NaN"), (-INF, "MSM_ERR_INVALID.*the messages hold -infinity")):
        m = np.zeros((T, 3, L))
        m[3, 1, 2] = value
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_round_gpu(ctx, *ok, messages=m, mode=0, polish=2, forbid=True)
    m = np.zeros((T, 3, L))
    m[3, 1, 2] = INF
    RL.same(api.mplp_round_gpu(ctx, *ok, messages=m, mode=0, polish=2, forbid=True), api.mplp_round(*ok, messages=m, mode=0, polish=2, forbid=True))
    assert api.mplp_gpu_stats(ctx) == before
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*the triplet table holds a non-finite value.*--fixnan"):
        api.mplp_optimise_gpu(ctx, *ok, sweeps=3)  # the plain entry point still refuses
    _both(ctx, ok, sweeps=2)  # and the context is as good as before


def test_the_last_entry_of_the_table_is_counted(ctx):
    """+inf in the last element of the last triplet and nothing else: the end of the classification pass's walk over the table"""
    case = ML.last_entry_forbidden()
    _both(ctx, case, sweeps=3, polish=2, what="last entry")
    counts = np.full(4, -1, dtype=np.int64)
    api.mplp_optimise_gpu(ctx, *case, sweeps=3, forbid=True, counts=counts)
    assert counts.tolist() == [0, 0, 1, 0]


def test_the_rounding_keeps_the_sweeps_counts(ctx):
    """the collapsed-triangle table: after mplp_round(then_polish=True) on a cost function that has made no other call, mplp_forbidden() is what it is
    after mplp_optimise on the same tables -- the sweeps' reading reaches the rounding and the polish and comes back from them"""
    swept, keep_swept = SC.product_cost(ctx)
    rounded, keep_rounded = SC.product_cost(ctx)
    start = np.zeros(swept.N, dtype=np.int32)
    for cf in (swept, rounded):
        cf.set_mplp_forbid()
        assert cf.mplp_forbidden().tolist() == [0, 0, 0, 0]
    swept.mplp_optimise(start, sweeps=3)
    rounded.mplp_round(start, sweeps=3, polish=2, then_polish=True)
    tc = np.array(swept.computeTripletCosts())
    want = [0, int(np.isnan(tc).sum()), int((tc == INF).sum()), 0]
    assert want[1] >= 1 and want[2] >= 1
    assert swept.mplp_forbidden().tolist() == rounded.mplp_forbidden().tolist() == want
    swept.close()
    rounded.close()


def test_the_real_table(ctx):
    """the strain regulariser's own table on the regular ico1 control grid under unrescaled labels, the moving data warped so that the unary table is
    not flat: 10 sweeps and the rounding with polish 8 over the cost function's device tables, over uploaded tables and on the host -- the same bits;
    D <= the returned E^ + tol; the returned labelling uses no forbidden entry"""
    inp = dict(SC.inputs())
    inp["src_feat"] = synthetic.features(synthetic.known_warp(inp["source_orig_xyz"], seed=77, rot_deg=3.0, amp=1.2), 1, 1234)
    cf, keep = SC.product_cost(ctx, inp=inp)
    triplets = inp["triplets"]
    U, tc = np.array(cf.computeUnaryCosts()), np.array(cf.computeTripletCosts())
    assert np.isfinite(U).all() and np.ptp(U) > 0 and np.isnan(tc).sum() >= 1 and (tc == INF).sum() >= 1 and not (tc == -INF).any()
    start, on_collapsed = SC.collapsed_start(tc, triplets, cf.N)  # sits on collapsed triangles: E^ = +inf
    assert on_collapsed >= 1 and FL.energy(U, tc, triplets, start) == INF
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*the triplet table holds a non-finite value"):
        cf.mplp_optimise(start, sweeps=3)
    cf.set_mplp_forbid()
    kw = dict(sweeps=10, bounds=True, messages=True)
    want = api.mplp_optimise(U, tc, triplets, start, forbid=True, **kw)
    for _ in range(2):
        ML.same(cf.mplp_optimise(start, **kw), want, "cost function")
        assert cf.mplp_forbidden().tolist() == api.mplp_classify(U, tc).tolist() == [0, int(np.isnan(tc).sum()), int((tc == INF).sum()), 0]
    ML.same(api.mplp_optimise_gpu(ctx, U, tc, triplets, start, forbid=True, **kw), want, "uploaded")
    wr = api.mplp_round(U, tc, triplets, want.labeling, messages=want.messages, mode=0, polish=8, forbid=True)
    RL.same(api.mplp_round_gpu(ctx, U, tc, triplets, want.labeling, messages=want.messages, mode=0, polish=8, forbid=True), wr, "uploaded")
    got, sweeps_run, bound = cf.mplp_round(start, sweeps=10, polish=8)
    RL.same(got, wr, "cost function")
    assert sweeps_run == want.sweeps_run and bound == want.bound
    t = FL.tol(U, triplets, want.messages)
    print("counts", cf.mplp_forbidden(), "start", FL.energy(U, tc, triplets, start), "decodes", want.energies, "rounded", wr.energies, "bound", bound, "tol", t,
          "infinite messages", int(np.isinf(want.messages).sum()))
    assert got.energy < INF and bound <= got.energy + t and not FL.uses_forbidden(tc, triplets, got.labeling)
    then, _, _ = cf.mplp_round(start, sweeps=10, polish=8, then_polish=True)
    assert np.array_equal(then.labeling, api.mplp_round(U, tc, triplets, wr.labeling, mode=1, polish=8, forbid=True).labeling)
    wp = api.mplp_round(U, tc, triplets, start, mode=1, polish=8, forbid=True)
    RL.same(cf.mplp_polish(start, polish=8), wp, "polish")
    assert wp.energies[0] == INF
    cf.set_mplp_forbid(False)
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*the triplet table holds a non-finite value"):
        cf.mplp_polish(start, polish=2)
    cf.close()


CONF = ("--simval=2,2\n--sigma_in=2,2\n--sigma_ref=2,2\n--lambda=0.2,0.2\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=1,2\n--SGgrid=3,4\n--datagrid=3,4\n"
        "--regoption=3\n--regexp=2\n--dopt=MPLP\n--VN\n--k_exponent=2\n--bulkmod=1.6\n--shearmod=0.4\n--mciters=5,5\n")  # no --rescaleL: labeldist 0.5 as it is


def _two_level_inputs():
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 2, 5)
    src = synthetic.features(synthetic.known_warp(xyz, seed=8, rot_deg=3.0, amp=2.0), 2, 5)
    return xyz, tri, synthetic.known_warp(xyz, seed=3, rot_deg=0.0, amp=0.7) + 0.25, src, ref


def test_level_loop(ctx):
    """two levels without label rescaling: every second iteration's labels let control points meet.  Refused without mplp_forbid, complete with it,
    the device route and the fetched-table route giving the same labellings and spheres, with the rounding and without"""
    xyz, tri, ixyz, src, ref = _two_level_inputs()
    levels, run_kw, _ = config.levels_from_config(config.parse_config(CONF), 2, mplp=True)
    assert len(levels) == 2 and all(lv["optimiser"] == "mplp" and not lv.get("rescale_labels") for lv in levels)

    def run(**ops_kw):
        labs = []
        reg, regs, energies = registration.run_multiresolution(registration.ProductOps(ctx, **ops_kw), ixyz, tri, src, xyz, tri, ref, levels, labelings_out=labs, **run_kw)
        return reg, regs, energies, labs

    for gpu in (True, False):
        with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*the triplet table holds a non-finite value"):
            run(mplp_gpu=gpu)
    for round_kw in (dict(), dict(mplp_round=True, mplp_polish=4)):
        got = run(mplp_forbid=True, **round_kw)
        want = run(mplp_forbid=True, mplp_gpu=False, **round_kw)
        assert len(got[3]) == 4 and all(np.array_equal(a, b) for a, b in zip(got[3], want[3])) and any(l.any() for l in got[3])
        assert np.array_equal(got[0], want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1])) and got[2] == want[2]
        assert np.isfinite(got[0]).all()


def test_both_executables(ctx, tmp_path):
    """MSMHIP_MPLP=on MSMHIP_MPLP_FORBID=on, alone and beside MSMHIP_MPLP_ROUND=on: tools/register_files.py and tools/cpp/newmsm write the same bytes for
    the two-level configuration without --rescaleL; without MSMHIP_MPLP_FORBID the run is refused; the variable without MSMHIP_MPLP=on, or with another
    value, ends both with a message and exit status 1"""
    import __graft_entry__ as g
    from newmsm_amd import meshio

    exe = g.build_cpp_newmsm()
    xyz, tri, ixyz, src, ref = _two_level_inputs()
    d = str(tmp_path) + "/"
    with open(d + "conf", "w") as f:
        f.write(CONF)
    meshio.save_surface(d + "in.surf.gii", ixyz, tri)
    meshio.save_surface(d + "ref.surf.gii", xyz, tri)
    meshio.save_metric(d + "in.func.gii", src)
    meshio.save_metric(d + "ref.func.gii", ref)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--inmesh=" + d + "in.surf.gii", "--refmesh=" + d + "ref.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "ref.func.gii", "--conf=" + d + "conf"]
    plain = {k: v for k, v in os.environ.items() if not k.startswith("MSMHIP_MPLP")}
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    for tag, cmd in (("py.", [sys.executable, "tools/register_files.py"]), ("cpp.", [exe])):
        for env, text in ((dict(MSMHIP_MPLP_FORBID="on"), "needs MSMHIP_MPLP=on"), (dict(MSMHIP_MPLP="on", MSMHIP_MPLP_FORBID="yes"), "MSMHIP_MPLP_FORBID=yes"),
                          (dict(MSMHIP_MPLP="on"), "the triplet table holds a non-finite value")):
            off = subprocess.run(cmd + common + ["--out=" + d + "off." + tag], cwd=root, env=dict(plain, **env), capture_output=True, text=True, timeout=600)
            assert off.returncode == 1 and text in off.stdout + off.stderr, (off.returncode, off.stdout, off.stderr)
            assert not any(os.path.exists(d + "off." + tag + n) for n in names)
        for sub, env in (("", dict()), ("round.", dict(MSMHIP_MPLP_ROUND="on"))):
            run = subprocess.run(cmd + common + ["--out=" + d + sub + tag], cwd=root, env=dict(plain, MSMHIP_MPLP="on", MSMHIP_MPLP_FORBID="on", **env),
                                 capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stderr
    for sub in ("", "round."):
        for n in names:
            with open(d + sub + "py." + n, "rb") as fa, open(d + sub + "cpp." + n, "rb") as fb:
                assert fa.read() == fb.read(), "%s%s differs between the two executables" % (sub, n)
