"""MPLP over the binary problem of one label step on the host (msm_fusion_mplp_step; newmsm_amd/csrc/fusion_mplp.cpp) against the
composition it is defined as -- api.mplp_optimise, then api.mplp_round mode 0, at L = 2 --, its properties against brute force, its refusals, and how
both level loops read its configuration.  No GPU."""
import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api

import fusion_mplp_cases as FC

CASES = {
    "ico0 smooth": dict(order=0, kind="smooth"),
    "ico0 rough": dict(order=0, kind="rough"),
    "ico1 smooth": dict(order=1, kind="smooth"),
    "ico1 rough": dict(order=1, kind="rough"),
    "ico1 rough lone node": dict(order=1, kind="rough", lone_node=True),
    "ico2 smooth": dict(order=2, kind="smooth"),
    "ico2 rough": dict(order=2, kind="rough"),
    "ico2 rough shuffled": dict(order=2, kind="rough", shuffled=True),
    "ico2 settled": dict(order=2, kind="settled"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_is_the_composition_of_the_two_entry_points(name):
    unary2, octets, triplets = case = FC.case(**CASES[name])
    for sweeps, polish in ((0, 0), (1, 0), (12, 0), (0, 3), (5, 1), (12, 8)):
        got = api.fusion_mplp_step(*case, sweeps=sweeps, polish=polish)
        FC.same(got, FC.composition(*case, sweeps, polish), (name, sweeps, polish))
        assert len(got.energies) == 1 + sweeps + (1 + polish if polish else 0) and len(got.bounds) == sweeps
        assert set(np.unique(got.x)) <= {0, 1} and got.energy == FC.energy(*case, got.x) and got.energy == got.energies.min()
        assert got.energy <= got.energies[0] == FC.energy(*case, np.zeros(len(unary2), dtype=np.int32))
    print(name, "N", len(unary2), "T", len(triplets), "levels", len(api.mcmc_schedule(triplets, len(unary2))[2]) - 1, "sweeps run of 12:", got.sweeps_run,
          "passes", got.passes_run, "E(0)", got.energies[0], "E", got.energy, "bound", got.bound)


def test_the_cases_cover_what_they_are_for():
    """the rough table reaches no fixed point in 12 sweeps, the settled one does at once; the shuffled list has another level count; the lone node is kept"""
    assert api.fusion_mplp_step(*FC.case(2, "rough"), sweeps=12, polish=0).sweeps_run == 12
    assert api.fusion_mplp_step(*FC.case(3, "rough"), sweeps=12, polish=0).sweeps_run == 12
    early = api.fusion_mplp_step(*FC.case(2, "settled"), sweeps=12, polish=0)
    assert early.sweeps_run == 1 and np.all(early.energies[early.sweeps_run:] == early.energies[early.sweeps_run])
    assert np.all(early.bounds[early.sweeps_run - 1:] == early.bound)
    levels = [len(api.mcmc_schedule(FC.case(2, "rough", shuffled=s)[2], 162)[2]) - 1 for s in (False, True)]
    assert levels[0] != levels[1], levels
    unary2, octets, triplets = FC.case(1, "rough", lone_node=True)
    assert len(unary2) == 43 and triplets.max() == 41
    got = api.fusion_mplp_step(unary2, octets, triplets, sweeps=5, polish=2)
    assert got.x[42] == int(unary2[42, 1] < unary2[42, 0])


def test_no_unary_costs_is_a_table_of_zeros():
    _, octets, triplets = FC.case(1, "rough")
    for sweeps, polish in ((6, 0), (6, 4)):
        got = api.fusion_mplp_step(None, octets, triplets, sweeps=sweeps, polish=polish, N=42)
        FC.same(got, api.fusion_mplp_step(np.zeros((42, 2)), octets, triplets, sweeps=sweeps, polish=polish), "NULL against zeros")
        FC.same(got, FC.composition(None, octets, triplets, sweeps, polish, N=42), "NULL against the composition")


def test_all_zero_tables_change_nothing_and_stop_after_one_sweep():
    _, _, triplets = FC.case(1)
    got = api.fusion_mplp_step(np.zeros((42, 2)), np.zeros((80, 8)), triplets, sweeps=7, polish=3)
    assert not got.x.any() and got.sweeps_run == 1 and got.energy == 0.0 and got.bound == 0.0
    assert not got.energies.any() and not got.bounds.any()
    none = api.fusion_mplp_step(np.ones((5, 2)), None, None, sweeps=4, polish=2)  # no triplet: no sweep runs, the bound is the sum of the node minima
    assert none.sweeps_run == 0 and not none.x.any() and none.energy == 5.0 and none.bound == 5.0 and np.all(none.energies == 5.0) and np.all(none.bounds == 5.0)


@pytest.mark.parametrize("kind", ["smooth", "rough"])
def test_bound_and_energy_bracket_the_optimum_at_ico0(kind):
    """all 4 096 labellings: bound - slack <= min E <= returned energy <= E(0), the slack DESIGN.md 5.19's own"""
    case = FC.case(0, kind)
    best, slack = FC.brute_force(*case), FC.slack(*case)
    for sweeps, polish in ((1, 0), (10, 0), (10, 8), (40, 8)):
        got = api.fusion_mplp_step(*case, sweeps=sweeps, polish=polish)
        print(kind, sweeps, polish, "bound", got.bound, "optimum", best, "energy", got.energy, "E(0)", got.energies[0], "slack", slack)
        assert got.bound - slack <= best <= got.energy + slack and got.energy <= got.energies[0]
        assert np.all(got.bounds - slack <= best)


def _refusals():
    unary2, octets, triplets = (np.array(a) for a in FC.case(0, "rough"))
    nan_u, inf_u, nan_o, inf_o, twice, far = np.array(unary2), np.array(unary2), np.array(octets), np.array(octets), np.array(triplets), np.array(triplets)
    nan_u[3, 1] = np.nan
    inf_u[11, 0] = -np.inf
    nan_o[0, 0] = np.nan
    inf_o[19, 7] = np.inf
    twice[4, 2] = twice[4, 0]
    far[11, 1] = 12
    unary, octet = "MSM_ERR_INVALID.*msm_fusion_mplp_step: the unary table holds a non-finite value", "MSM_ERR_INVALID.*msm_fusion_mplp_step: the octet table holds a non-finite value"
    return (unary2, octets, triplets), [
        ((nan_u, octets, triplets), {}, unary), ((inf_u, octets, triplets), {}, unary), ((unary2, nan_o, triplets), {}, octet),
        ((unary2, inf_o, triplets), {}, octet), ((nan_u, inf_o, triplets), {}, unary),  # the unary table is named first
        ((None, nan_o, triplets), dict(N=12), octet),
        ((unary2, octets, twice), {}, "MSM_ERR_INVALID.*msm_fusion_mplp_step: triplet 4 names a node twice"),
        ((unary2, octets, far), {}, "MSM_ERR_INVALID.*triplet node out of range"),
        ((unary2, octets, triplets), dict(sweeps=-1), "MSM_ERR_INVALID.*msm_fusion_mplp_step: -1 sweeps \\(0 to 1024\\)"),
        ((unary2, octets, triplets), dict(sweeps=1025), "MSM_ERR_INVALID.*msm_fusion_mplp_step: 1025 sweeps \\(0 to 1024\\)"),
        ((unary2, octets, triplets), dict(polish=-1), "MSM_ERR_INVALID.*msm_fusion_mplp_step: -1 polish passes \\(0 to 1024\\)"),
        ((unary2, octets, triplets), dict(polish=1025), "MSM_ERR_INVALID.*msm_fusion_mplp_step: 1025 polish passes \\(0 to 1024\\)")]


def refused_with_x_untouched(call, args, kw, pattern):
    """drives the C entry point through `call(tables..., x, sweeps, polish)` with caller-owned outputs preset to sentinels"""
    import ctypes as C

    from newmsm_amd._lib import c_dp, c_ip

    unary2, octets, triplets = args
    N = kw.get("N", None if unary2 is None else len(unary2))
    sweeps, polish = kw.get("sweeps", 4), kw.get("polish", 2)
    x = np.full(N, 7, dtype=np.int32)
    energies, bounds = np.full(3000, -3.0), np.full(1100, -4.0)
    run, passes, energy, bound = C.c_int32(-5), C.c_int32(-6), C.c_double(-7.0), C.c_double(-8.0)
    u = None if unary2 is None else np.ascontiguousarray(unary2, dtype=np.float64)
    o, tr = np.ascontiguousarray(octets, dtype=np.float64), np.ascontiguousarray(triplets, dtype=np.int32)
    with pytest.raises(M.MsmError, match=pattern):
        api.check(call(C.cast(None, c_dp) if u is None else u.ctypes.data_as(c_dp), o.ctypes.data_as(c_dp), tr.ctypes.data_as(c_ip), len(tr), N, sweeps, polish,
                       x.ctypes.data_as(c_ip), C.byref(run), C.byref(passes), C.byref(energy), C.byref(bound), energies.ctypes.data_as(c_dp),
                       bounds.ctypes.data_as(c_dp)))
    assert np.all(x == 7) and np.all(energies == -3.0) and np.all(bounds == -4.0)
    assert (run.value, passes.value, energy.value, bound.value) == (-5, -6, -7.0, -8.0)


def test_every_refusal_leaves_the_outputs_untouched():
    from newmsm_amd._lib import lib

    ok, cases = _refusals()
    for args, kw, pattern in cases:
        refused_with_x_untouched(lib().msm_fusion_mplp_step, args, kw, pattern)
    assert api.fusion_mplp_step(*ok, sweeps=4, polish=2).sweeps_run >= 1


# ---------------------------------------------------------------- configuration: the level loops and the executables

def test_product_ops_configuration():
    from newmsm_amd import registration

    ops = registration.ProductOps(None)
    assert (ops.fusion_mplp, ops.fusion_sweeps, ops.fusion_polish) == (False, 10, 8)
    ops = registration.ProductOps(None, fusion_mplp=True, fusion_sweeps=3, fusion_polish=0)
    assert (ops.fusion_mplp, ops.fusion_sweeps, ops.fusion_polish) == (True, 3, 0)
    case = FC.case(1, "rough")
    FC.same(ops.fusion_mplp_step(*case), api.fusion_mplp_step(*case, sweeps=3, polish=0))
    for kw in (dict(fusion_sweeps=0), dict(fusion_sweeps=257), dict(fusion_polish=-1), dict(fusion_polish=65)):
        with pytest.raises(ValueError, match="whole number from"):
            registration.ProductOps(None, **kw)


def test_cpp_level_options_and_wrapper(built):
    """tests/cpp/fusion_mplp_client.cpp: LevelOptions' defaults and msmhip::fusion_mplp_step over the octahedron, every bit of its outputs"""
    import os
    import subprocess

    from tests.test_cpp_host import build_cpp

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "fusion_mplp_client")
    build_cpp(os.path.join(root, "tests", "cpp", "fusion_mplp_client.cpp"), exe)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = dict(line.split(" ", 1) for line in run.stdout.strip().splitlines())
    assert lines["defaults"] == "0 10 8"
    triplets = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)
    unary2 = np.array([[((7 * i + 3 * x) % 11) / 8.0 for x in range(2)] for i in range(6)])
    octets = np.array([[((5 * t + 3 * e * e) % 13 - 6) / 4.0 for e in range(8)] for t in range(8)])
    want = api.fusion_mplp_step(unary2, octets, triplets, sweeps=6, polish=3)
    assert [int(v) for v in lines["x"].split()] == want.x.tolist()
    assert lines["run"] == "%d %d" % (want.sweeps_run, want.passes_run)
    e = lines["energy"].split()
    assert float.fromhex(e[0]) == want.energy and float.fromhex(e[2]) == want.bound
    assert [float.fromhex(v) for v in lines["energies"].split()] == want.energies.tolist()
    assert [float.fromhex(v) for v in lines["bounds"].split()] == want.bounds.tolist()
    assert "1025 sweeps (0 to 1024)" in lines["refused"]


SETTINGS = [(dict(MSMHIP_FUSION="fastpd"), "MSMHIP_FUSION=fastpd: the binary solve of a label step is the stand-in (icm, or unset) or MPLP on the device (mplp)"),
            (dict(MSMHIP_FUSION_SWEEPS="5"), "MSMHIP_FUSION_SWEEPS=5 sets the sweeps of a label step's MPLP solve: it needs MSMHIP_FUSION=mplp"),
            (dict(MSMHIP_FUSION="icm", MSMHIP_FUSION_POLISH="2"), "MSMHIP_FUSION_POLISH=2 sets the polish passes of a label step's MPLP solve: it needs MSMHIP_FUSION=mplp"),
            (dict(MSMHIP_FUSION="mplp", MSMHIP_FUSION_SWEEPS="0"), "MSMHIP_FUSION_SWEEPS=0: the number of sweeps must be a whole number from 1 to 256"),
            (dict(MSMHIP_FUSION="mplp", MSMHIP_FUSION_SWEEPS="257"), "MSMHIP_FUSION_SWEEPS=257: the number of sweeps must be a whole number from 1 to 256"),
            (dict(MSMHIP_FUSION="mplp", MSMHIP_FUSION_SWEEPS="ten"), "MSMHIP_FUSION_SWEEPS=ten: the number of sweeps must be a whole number from 1 to 256"),
            (dict(MSMHIP_FUSION="mplp", MSMHIP_FUSION_POLISH="65"), "MSMHIP_FUSION_POLISH=65: the number of polish passes must be a whole number from 0 to 64"),
            (dict(MSMHIP_FUSION="mplp", MSMHIP_FUSION_POLISH="-1"), "MSMHIP_FUSION_POLISH=-1: the number of polish passes must be a whole number from 0 to 64")]


def test_both_executables_refuse_bad_settings_alike(built, tmp_path):
    """every setting outside MSMHIP_FUSION=mplp|icm, MSMHIP_FUSION_SWEEPS=1..256, MSMHIP_FUSION_POLISH=0..64 ends tools/register_files.py and
    tools/cpp/newmsm with the same message and exit status 1, before a file or a GPU is looked at; so does --groupwise with MSMHIP_FUSION=mplp"""
    import os
    import subprocess
    import sys

    import __graft_entry__ as g

    exe = g.build_cpp_newmsm()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    plain = {k: v for k, v in os.environ.items() if not k.startswith("MSMHIP_FUSION")}
    d = str(tmp_path) + "/"
    pairwise = ["--inmesh=" + d + "none.surf.gii", "--refmesh=" + d + "none.surf.gii", "--indata=" + d + "none.func.gii", "--refdata=" + d + "none.func.gii",
                "--conf=" + d + "none", "--out=" + d + "out."]
    groupwise = ["--groupwise", "--meshes=" + d + "none", "--data=" + d + "none", "--template=" + d + "none.surf.gii", "--conf=" + d + "none", "--out=" + d + "out."]
    group_text = "MSMHIP_FUSION=mplp solves label steps of triplets alone: a --groupwise run (pair factors between the subjects) keeps the stand-in; unset it"
    for cmd in ([sys.executable, "tools/register_files.py"], [exe]):
        for env, text in SETTINGS:
            run = subprocess.run(cmd + pairwise, cwd=root, env=dict(plain, **env), capture_output=True, text=True, timeout=120)
            assert run.returncode == 1 and text in run.stdout + run.stderr, (cmd, env, run.returncode, run.stdout, run.stderr)
        for env, text in SETTINGS[:1] + [(dict(MSMHIP_FUSION="mplp"), group_text), (dict(MSMHIP_FUSION="mplp", MSMHIP_FUSION_SWEEPS="20"), group_text)]:
            run = subprocess.run(cmd + groupwise, cwd=root, env=dict(plain, **env), capture_output=True, text=True, timeout=120)
            assert run.returncode == 1 and text in run.stdout + run.stderr, (cmd, env, run.returncode, run.stdout, run.stderr)
        # accepted settings get past the parsing: the run ends at the first missing file instead
        for env in (dict(MSMHIP_FUSION="icm"), dict(MSMHIP_FUSION="mplp", MSMHIP_FUSION_SWEEPS="256", MSMHIP_FUSION_POLISH="0")):
            run = subprocess.run(cmd + pairwise, cwd=root, env=dict(plain, **env), capture_output=True, text=True, timeout=120)
            assert run.returncode == 1 and "MSMHIP_FUSION" not in run.stdout + run.stderr, (cmd, env, run.returncode, run.stdout, run.stderr)
