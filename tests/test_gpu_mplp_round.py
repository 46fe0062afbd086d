"""The rounding of MPLP's messages on the GPU (msm_mplp_round_gpu, msm_cost_mplp_round, msm_cost_mplp_polish; newmsm_amd/csrc/mplp.cpp,
mplp_kernels.hip; DESIGN.md 5.19 "Rounding"): a launch per colour class, a workgroup per node in the conditioned decode and a wavefront per node in a
polish pass.  Every case asks for the host literal's bits (msm_mplp_round) on the same arguments: labelling, passes run, energies."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, problem, registration, synthetic

import mplp_literal as ML
import mplp_round_literal as RL

pytestmark = pytest.mark.gpu
HCP = dict(rmode=3, lambda_=0.01, mu=0.4, kappa=1.6, k_exp=2.0, rexp=2.0)


def _both(ctx, case, sweeps=3, polish=4, modes=(0, 1)):
    """the messages after `sweeps` host sweeps, rounded on both sides in the modes asked for; the mode-0 result"""
    U, tc, triplets, start = case
    m = api.mplp_optimise(U, tc, triplets, start, sweeps=sweeps, bound=False, messages=True).messages if sweeps else None
    first = None
    for mode in modes:
        want = api.mplp_round(U, tc, triplets, start, messages=m, mode=mode, polish=polish)
        got = api.mplp_round_gpu(ctx, U, tc, triplets, start, messages=m, mode=mode, polish=polish)
        RL.same(got, want, "mode %d" % mode)
        stats = api.mplp_round_gpu_stats(ctx)
        assert stats["passes_run"] == want.passes_run and stats["classes"] == api.mplp_colouring(triplets, U.shape[1])[1]
        first = got if first is None else first
    return first


@pytest.mark.parametrize("L", [1, 2, 3])
def test_one_triplet(ctx, L):
    """three classes of one node: neither, one and both of the others fixed, on blocks smaller than a workgroup"""
    _both(ctx, RL.CASES["triplet L%d" % L]())
    _both(ctx, RL.CASES["triplet L%d" % L](), sweeps=0)  # NULL messages


@pytest.mark.parametrize("L", [16, 19, 20, 61])
def test_ico0_faces(ctx, L):
    """L^3 a multiple of the workgroup's 256 threads (16) and not; 64 copies of every minimum up to 41 labels, 32 at 61"""
    got = _both(ctx, ML.ico_case(0, L), sweeps=2 if L == 61 else 5)
    assert got.labeling.any()


@pytest.mark.parametrize("slots", ["1", "4"])
def test_fewer_copies_of_the_minima_in_lds(ctx, monkeypatch, slots):
    monkeypatch.setenv("MSMHIP_MPLP_SLOTS", slots)
    _both(ctx, ML.ico_case(0, 19), modes=(0,))


def test_ico0_faces_70_labels(ctx):
    """the argmin runs over more than a wavefront of labels, in the decode's workgroup and in the polish's wavefront"""
    _both(ctx, ML.ico_case(0, 70), sweeps=1, polish=2)


def test_fan_round_one_hub_and_an_isolated_node(ctx):
    """the hub's twelve slots; node 13 is in no triplet and takes argmin theta"""
    U, tc, triplets, start = case = ML.fan_case()
    start = np.array(start)
    start[13] = int(np.argmax(U[:, 13]))
    got = _both(ctx, (U, tc, triplets, start))
    assert got.labeling[13] == int(np.argmin(U[:, 13]))


def test_every_slot_and_fixed_subset(ctx):
    case = RL.CASES["twelve"]()
    assert len(RL.combinations(case[2], case[0].shape[1])) == 12
    _both(ctx, case, polish=8)


@pytest.mark.parametrize("shuffled", [False, True])
def test_ico2_faces(ctx, shuffled):
    _both(ctx, ML.ico_case(2, 19, 12, 0.0, False, shuffled), sweeps=2)


def test_ico4_faces(ctx):
    """N = 2562, L = 5: classes of several hundred workgroups"""
    case = ML.ico_case(4, 5)
    colour, classes = api.mplp_colouring(case[2], case[0].shape[1])
    assert np.bincount(colour).max() > 300
    _both(ctx, case, sweeps=2, polish=6)


def test_tables_with_entries_of_1e7(ctx):
    for args in ((0, 19, 19, 0.05), (2, 7, 13, 0.05)):
        U, tc, triplets, start = case = ML.ico_case(*args)
        got = _both(ctx, case, sweeps=10, polish=8, modes=(0,))
        assert got.energies[1] < 1e7


def test_whole_number_tables_with_ties(ctx):
    """exact ties: the lowest label in the decode, the current label in the polish"""
    U, tc, triplets, start = case = RL.CASES["ties"]()
    _both(ctx, case, sweeps=5)
    ones = np.ones(U.shape[1], dtype=np.int32)
    got = _both(ctx, (U, tc, triplets, ones), modes=(1,), polish=1)
    assert not np.any(got.labeling == 2)
    flat = (np.full_like(U, 1.5), np.full_like(tc, -0.25), triplets, start)
    assert np.array_equal(_both(ctx, flat, modes=(1,), sweeps=0).labeling, start)


def test_fixed_point_before_the_polish_is_used_up(ctx):
    """the launches behind the fixed point return at once; the energies repeat the last value"""
    got = _both(ctx, ML.ico_case(2, 8), polish=64)
    assert 1 <= got.passes_run < 64 and np.all(got.energies[1 + got.passes_run:] == got.energies[-1])
    again = _both(ctx, ML.ico_case(2, 8)[:3] + (got.labeling,), modes=(1,), polish=8)
    assert again.passes_run == 1 and np.array_equal(again.labeling, got.labeling)


def test_refusals_are_the_host_literals(ctx):
    ok, cases = RL.refusal_cases()
    api.mplp_round_gpu(ctx, *ok[:4], messages=ok[4], mode=ok[5], polish=ok[6])
    before = api.mplp_round_gpu_stats(ctx)
    for args, pattern in cases:
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_round_gpu(ctx, *args[:4], messages=args[4], mode=args[5], polish=args[6])
    assert api.mplp_round_gpu_stats(ctx) == before
    _both(ctx, ok[:4])


def test_mode_1_reads_no_messages(ctx):
    """the messages mode 0 refuses change nothing in mode 1"""
    ok, _ = RL.refusal_cases()
    want = api.mplp_round(*ok[:4], mode=1, polish=2)
    for m in RL.unread_messages():
        RL.same(api.mplp_round_gpu(ctx, *ok[:4], messages=m, mode=1, polish=2), want)


@pytest.mark.parametrize("kind", ["univariate", "ho_univariate"])
def test_cost_function_tables_and_messages_stay_on_the_device(ctx, kind):
    """msm_cost_mplp_round = msm_cost_mplp_optimise(messages) + msm_mplp_round(mode 0) with that winner handed in; msm_cost_mplp_polish = mode 1"""
    inp = problem.pairwise_inputs(data_order=4, cp_order=2, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind=kind, **HCP)
    cf.get_source_data()
    start = np.zeros(cf.N, dtype=np.int32)
    U, tc = cf.computeUnaryCosts(), cf.computeTripletCosts()
    r = cf.mplp_optimise(start, sweeps=5, bound=True, messages=True)
    want = api.mplp_round(U, tc, inp["triplets"], r.labeling, messages=r.messages, mode=0, polish=6)
    for _ in range(2):
        got, sweeps_run, bound = cf.mplp_round(start, sweeps=5, polish=6)
        RL.same(got, want)
        assert sweeps_run == r.sweeps_run and bound == r.bound and got.energy <= r.energy
    print(kind, "start", want.energies[0], "rounded", want.energies[1], "polished", want.energy, "bound", bound)
    then, _, _ = cf.mplp_round(start, sweeps=5, polish=6, then_polish=True)
    assert np.array_equal(then.labeling, api.mplp_round(U, tc, inp["triplets"], want.labeling, mode=1, polish=6).labeling)
    rng = np.random.default_rng(3)
    other = rng.integers(0, cf.L, cf.N).astype(np.int32)
    RL.same(cf.mplp_polish(other, polish=6), api.mplp_round(U, tc, inp["triplets"], other, mode=1, polish=6))
    with pytest.raises(M.MsmError, match="msm_mcmc_optimise: label of node 3 out of range"):
        bad = np.array(start)
        bad[3] = cf.L
        cf.mplp_round(bad)
    with pytest.raises(M.MsmError, match="1025 polish passes"):
        cf.mplp_polish(start, polish=1025)
    cf.close()


def test_level_loop(ctx):
    """run_discrete_level(optimiser="mplp") with the rounding: the device route and the fetched-table route give the same bytes; the first iteration,
    whose tables are those of the level without the rounding, ends no higher than there"""
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 1, 21)
    src = synthetic.features(synthetic.known_warp(xyz, seed=23, rot_deg=4.0, amp=2.5), 1, 21)
    kw = dict(cp_order=2, iters=3, mciters=5, seed=5, kind="univariate", optimiser="mplp", cost_params=dict(lambda_=0.0005), labeldist=0.4)
    t_gpu = {}
    got = registration.run_discrete_level(registration.ProductOps(ctx, mplp_round=True, mplp_polish=4), xyz, tri, ref, xyz, tri, src, xyz, timings=t_gpu, **kw)
    want = registration.run_discrete_level(registration.ProductOps(ctx, mplp_gpu=False, mplp_round=True, mplp_polish=4), xyz, tri, ref, xyz, tri, src, xyz, **kw)
    plain = registration.run_discrete_level(registration.ProductOps(ctx), xyz, tri, ref, xyz, tri, src, xyz, **kw)
    assert "triplet_table" not in t_gpu and "unary_table" not in t_gpu
    assert len(got[3]) == 3 and all(np.array_equal(a, b) for a, b in zip(got[3], want[3])) and all(l.any() for l in got[3])
    assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    print("energies with the rounding", got[2], "without", plain[2])
    assert got[2][0] <= plain[2][0]  # the first iteration has the same tables: the rounding starts from the sweeps' winner


CONF = ("--simval=2,2\n--sigma_in=2,2\n--sigma_ref=2,2\n--lambda=0.2,0.2\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=2,3\n--SGgrid=4,5\n--datagrid=4,5\n"
        "--regoption=3\n--regexp=2\n--dopt=MPLP\n--VN\n--k_exponent=2\n--bulkmod=1.6\n--shearmod=0.4\n--rescaleL\n--mciters=5,5\n")


def test_both_executables(ctx, tmp_path):
    """MSMHIP_MPLP=on MSMHIP_MPLP_ROUND=on MSMHIP_MPLP_POLISH=4: tools/register_files.py and tools/cpp/newmsm write the same bytes; the variable without
    MSMHIP_MPLP=on, or a polish count out of range, ends both with a message and exit status 1"""
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
    plain = {k: v for k, v in os.environ.items() if not k.startswith("MSMHIP_MPLP")}
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    for tag, cmd in (("py.", [sys.executable, "tools/register_files.py"]), ("cpp.", [exe])):
        for env, text in ((dict(MSMHIP_MPLP_ROUND="on"), "needs MSMHIP_MPLP=on"), (dict(MSMHIP_MPLP="on", MSMHIP_MPLP_ROUND="yes"), "MSMHIP_MPLP_ROUND=yes"),
                          (dict(MSMHIP_MPLP="on", MSMHIP_MPLP_ROUND="on", MSMHIP_MPLP_POLISH="65"), "MSMHIP_MPLP_POLISH=65")):
            off = subprocess.run(cmd + common + ["--out=" + d + "off." + tag], cwd=root, env=dict(plain, **env), capture_output=True, text=True, timeout=600)
            assert off.returncode == 1 and text in off.stdout + off.stderr, (off.returncode, off.stdout, off.stderr)
            assert not any(os.path.exists(d + "off." + tag + n) for n in names)
        run = subprocess.run(cmd + common + ["--out=" + d + tag], cwd=root, env=dict(plain, MSMHIP_MPLP="on", MSMHIP_MPLP_ROUND="on", MSMHIP_MPLP_POLISH="4"),
                             capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr
    for n in names:
        with open(d + "py." + n, "rb") as fa, open(d + "cpp." + n, "rb") as fb:
            assert fa.read() == fb.read(), "%s differs between the two executables" % n
