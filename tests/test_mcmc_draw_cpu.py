"""The Monte Carlo optimiser's proposals drawn on the device, the host half (newmsm_amd/csrc/mcmc_draw.hpp; DESIGN.md 5.16 "Proposals on the device"): the
thresholds against the label function they stand for, the stream rebuilt from the hand-written pieces against the library's own stream (std::mt19937 +
std::geometric_distribution), the block bound, the context's mode, the executables' environment variable, and the pieces as a program of their own under
the sanitizers.  These tests are what notices a toolchain whose generate_canonical or log differs from the one the definition was written against.  No GPU."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(19, float(np.float32(0.8))), (3, 0.05), (1, 0.5), (7, 0.2), (200, float(np.float32(0.3))), (19, 0.95), (4, 1.0)]
IDS = ["L%d_p%g" % c for c in CASES]
SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32 + 5]
LOWEST, ONE = 0x3CA0000000000000, 0x3FF0000000000000  # the bit patterns of 2^-53 and 1.0
T, SWEEPS = 1000, 1000  # a million proposals


def _label_function(bits, p):
    """floor(log(x) / log(1 - p)) of the double with this bit pattern, as the host computes it (math.log is the host's log; log(0) is -inf there)"""
    x = float(np.array([bits], dtype=np.uint64).view(np.float64)[0])
    c = -math.inf if p == 1.0 else math.log(1.0 - p)
    return math.floor(math.log(x) / c)


@functools.lru_cache(maxsize=None)
def _library_stream(L, p, seed):
    out = api.mcmc_proposals(L, p, seed, T, SWEEPS)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _mirror_stream(L, p, seed):
    out, candidates = api.mcmc_proposals_mirror(L, p, seed, T, SWEEPS, counted=True)
    out.setflags(write=False)
    return out, candidates


@pytest.mark.parametrize("L,p", CASES, ids=IDS)
def test_thresholds_are_the_steps_of_the_label_function(L, p):
    thr = api.mcmc_draw_thresholds(L, p)
    assert thr.dtype == np.uint64 and thr.shape == (L,)
    t = [int(v) for v in thr]
    assert all(LOWEST <= v <= ONE for v in t)
    assert all(t[k] <= t[k - 1] for k in range(1, L))  # non-increasing in k
    for k in range(1, L + 1):
        for bits in range(max(t[k - 1] - 64, LOWEST), min(t[k - 1] + 64, ONE) + 1):
            assert (bits >= t[k - 1]) == (_label_function(bits, p) <= k - 1), (k, hex(bits))


def test_a_parameter_of_one_makes_every_label_zero():
    thr = api.mcmc_draw_thresholds(4, 1.0)
    assert [int(v) for v in thr] == [LOWEST] * 4  # no pattern in [2^-53, 1] is below any threshold: the count is 0
    assert not api.mcmc_proposals_mirror(4, 1.0, 3, 50, 20).any()
    assert not api.mcmc_proposals(4, 1.0, 3, 50, 20).any()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("L,p", CASES, ids=IDS)
def test_mirror_is_the_library_stream(L, p, seed):
    mirror, candidates = _mirror_stream(L, p, seed)
    assert mirror.shape == (SWEEPS, T) and mirror.dtype == np.uint16
    assert np.array_equal(mirror, _library_stream(L, p, seed))
    assert candidates >= T * SWEEPS
    assert int(mirror.max()) < L


@pytest.mark.parametrize("L,p", CASES, ids=IDS)
def test_only_the_low_32_bits_of_a_seed_count(L, p):
    assert np.array_equal(_mirror_stream(L, p, 2 ** 32 + 5)[0], api.mcmc_proposals(L, p, 5, T, SWEEPS))
    if L > 1 and p < 1.0:  # (otherwise every proposal is 0 whatever the seed)
        assert not np.array_equal(_mirror_stream(L, p, 2 ** 32 + 5)[0], _mirror_stream(L, p, 1)[0])


def test_mirror_without_the_count_is_the_same_stream():
    assert np.array_equal(api.mcmc_proposals_mirror(19, 0.8, 7, 320, 9), api.mcmc_proposals(19, 0.8, 7, 320, 9))
    assert api.mcmc_proposals_mirror(19, 0.8, 7, 0, 9).shape == (9, 0)


@pytest.mark.parametrize("L,p", CASES, ids=IDS)
def test_block_bound_covers_the_expected_and_the_actual_candidates(L, p):
    a = 1.0 if p == 1.0 else 1.0 - (1.0 - p) ** L
    for need in (1, 312, 10 ** 6):
        bound = api.mcmc_draw_block_bound(need, L, p)
        assert bound == math.ceil((need / a + 16.0 * math.sqrt(need * (1.0 - a)) / a + 624.0) / 312.0) + 1
        assert 312 * bound >= need / a
    bound = api.mcmc_draw_block_bound(T * SWEEPS, L, p)
    for seed in SEEDS:
        assert _mirror_stream(L, p, seed)[1] < 312 * bound


def test_bad_arguments_are_refused():
    for call in (lambda: api.mcmc_draw_thresholds(0, 0.5), lambda: api.mcmc_draw_thresholds(3, 0.0), lambda: api.mcmc_draw_thresholds(3, 1.5),
                 lambda: api.mcmc_proposals_mirror(70000, 0.5, 0, 4, 1), lambda: api.mcmc_proposals_mirror(3, 0.0, 0, 4, 1),
                 lambda: api.mcmc_draw_block_bound(-1, 3, 0.5), lambda: api.mcmc_draw_block_bound(5, 0, 0.5)):
        with pytest.raises(M.MsmError):
            call()


def test_context_mode_round_trip_and_refusals():
    lib = M.lib()
    import ctypes as C

    mode = C.c_int32(7)
    assert lib.msm_ctx_set_mcmc_draw(None, 1) == -1 and lib.msm_ctx_get_mcmc_draw(None, C.byref(mode)) == -1  # MSM_ERR_INVALID: no context
    assert lib.msm_abi_version() == 12  # the draw only adds symbols
    if M.device_count() < 1:  # a context needs a device; tests/test_gpu_mcmc_draw.py makes the round trip where there is one
        return
    ctx = M.Context(0)
    assert ctx.get_mcmc_draw() == 0
    ctx.set_mcmc_draw(1)
    assert ctx.get_mcmc_draw() == 1
    with pytest.raises(M.MsmError):
        ctx.set_mcmc_draw(2)
    assert ctx.get_mcmc_draw() == 1
    ctx.set_mcmc_draw("host")
    assert ctx.get_mcmc_draw() == 0
    assert lib.msm_ctx_get_mcmc_draw(ctx.h, None) == -1


@pytest.mark.parametrize("tool", ["py", "cpp"])
def test_the_executables_refuse_a_device_draw_without_device_sweeps(tool, tmp_path):
    import __graft_entry__ as g

    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_files.py")] if tool == "py" else [g.build_cpp_newmsm()]
    cmd += ["--inmesh=none.surf.gii", "--indata=none.func.gii", "--refdata=none.func.gii", "--out=" + str(tmp_path) + "/"]
    base = {k: v for k, v in os.environ.items() if k not in ("MSMHIP_MCMC", "MSMHIP_MCMC_DRAW")}
    for env in (dict(MSMHIP_MCMC_DRAW="gpu"), dict(MSMHIP_MCMC_DRAW="gpu", MSMHIP_MCMC="host"), dict(MSMHIP_MCMC_DRAW="device", MSMHIP_MCMC="gpu"),
                dict(MSMHIP_MCMC_DRAW="", MSMHIP_MCMC="gpu")):
        run = subprocess.run(cmd, cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, timeout=120)
        assert run.returncode == 1 and "MSMHIP_MCMC_DRAW" in run.stderr, (env, run.stdout, run.stderr)
        assert ("MSMHIP_MCMC=gpu" in run.stderr) == (env["MSMHIP_MCMC_DRAW"] == "gpu"), (env, run.stderr)


def test_host_pieces_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/mcmc_draw_host_check.cpp: the hand-written engine against std::mt19937 over 10 blocks, the candidate against generate_canonical, the
    thresholds' neighbourhoods, the mirror against McmcProposals -- a program of its own (no HIP, no Python), built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "mcmc_draw_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpp", "mcmc_draw_host_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
