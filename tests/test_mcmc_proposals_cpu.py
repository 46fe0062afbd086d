"""The host half of the Monte Carlo optimiser's GPU sweeps (newmsm_amd/csrc/mcmc.cpp): the proposal stream factored out of msm_mcmc_optimise and the level
schedule one workgroup walks.  No GPU."""
import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api


def _faces(order):
    xyz, tri = M.make_mesh_from_icosa(order)
    return len(xyz), np.ascontiguousarray(api.estimate_triplets(tri), dtype=np.int32)


def _replay(U, tc, triplets, labeling, stream):
    """MCMC::optimise (M/mcmc_opt.h:31-134) in plain Python over a given proposal stream (sweeps x T)"""
    lab = np.array(labeling, dtype=np.int64)
    for sweep in stream:
        for t, (a, b, c) in enumerate(triplets):
            p = int(sweep[t])
            cur = (lab[a], lab[b], lab[c])
            costs = []
            for k in range(8):
                la, lb, lc = (p if k & 4 else cur[0]), (p if k & 2 else cur[1]), (p if k & 1 else cur[2])
                costs.append(tc[t, la, lb, lc] + (U[la, a] + U[lb, b] + U[lc, c]) / 3.0)
            best = 0
            for k in range(1, 8):
                if costs[k] < costs[best]:
                    best = k
            if best & 4:
                lab[a] = p
            if best & 2:
                lab[b] = p
            if best & 1:
                lab[c] = p
    return lab.astype(np.int32)


def test_the_stream_is_what_the_host_optimiser_consumes():
    """ico1 faces, L = 5, 7 sweeps: replaying the factored-out stream in plain Python gives msm_mcmc_optimise's labelling"""
    N, triplets = _faces(1)
    L, sweeps, seed, mcparam = 5, 7, 11, 0.4
    rng = np.random.default_rng(3)
    U, tc = rng.normal(size=(L, N)), rng.normal(size=(len(triplets), L, L, L))
    start = rng.integers(0, L, N).astype(np.int32)
    stream = api.mcmc_proposals(L, mcparam, seed, len(triplets), sweeps)
    assert stream.shape == (sweeps, len(triplets)) and stream.max() < L and len(np.unique(stream)) > 1
    want = api.mcmc_optimise(U, tc, triplets, start, mcparam=mcparam, iters=sweeps, seed=seed)
    assert not np.array_equal(want, start)
    assert np.array_equal(_replay(U, tc, triplets, start, stream), want)


@pytest.mark.parametrize("chunk", [1, 3, 64])
def test_chunks_do_not_change_the_stream(chunk):
    whole = api.mcmc_proposals(19, 0.8, 5, 320, 70)
    assert np.array_equal(api.mcmc_proposals(19, 0.8, 5, 320, 70, chunk_sweeps=chunk), whole)


def test_parameter_one_proposes_label_zero_only():
    assert not api.mcmc_proposals(19, 1.0, 9, 80, 12).any()


def test_the_stream_refuses_labels_beyond_16_bits():
    with pytest.raises(M.MsmError, match="65535"):
        api.mcmc_proposals(65536, 0.5, 0, 4, 1)
    assert api.mcmc_proposals(65535, 0.5, 0, 4, 1).shape == (1, 4)


def test_host_pieces_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/mcmc_host_check.cpp: the schedule builder and the proposal stream as a program of their own (no HIP, no Python), built with
    -fsanitize=address,undefined: the schedule's properties, a level-by-level walk against the serial one, the chunked stream against the serial loop"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mcmc_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(root, "tests", "cpp", "mcmc_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def _check_schedule(triplets, N):
    triplets = np.asarray(triplets, dtype=np.int32).reshape(-1, 3)
    level, order, off = api.mcmc_schedule(triplets, N)
    T = len(triplets)
    assert sorted(order.tolist()) == list(range(T))  # every triplet once
    assert off[0] == 0 and off[-1] == T and np.all(np.diff(off) > 0)
    for l in range(len(off) - 1):
        members = order[off[l]:off[l + 1]]
        assert np.all(level[members] == l) and np.all(np.diff(members) > 0)  # by level, ascending within one
        nodes = [set(triplets[t].tolist()) for t in members]
        assert sum(len(s) for s in nodes) == len(set().union(*nodes))  # no two triplets of a level share a node
    last = {}  # node -> the highest level among the earlier triplets that touch it
    for t in range(T):
        before = [last[n] for n in triplets[t].tolist() if n in last]
        assert level[t] == (1 + max(before) if before else 0)  # above every earlier sharer, and no higher than that asks for
        for n in triplets[t].tolist():
            last[n] = level[t]
    return len(off) - 1


@pytest.mark.parametrize("order,levels", [(0, 10), (2, 28), (4, 32)])
def test_schedule_of_icosphere_faces(order, levels):
    N, triplets = _faces(order)
    assert _check_schedule(triplets, N) == levels


def test_schedule_of_lists_that_are_no_mesh():
    assert _check_schedule([[0, 0, 1], [2, 3, 4], [2, 3, 4], [1, 1, 1], [4, 0, 5]], 6) == 3  # a node named twice, two identical triplets
    assert _check_schedule(np.arange(30).reshape(10, 3), 30) == 1                             # disjoint: one level
    assert _check_schedule(np.zeros((7, 3)), 1) == 7                                           # a chain: a level each
    level, order, off = api.mcmc_schedule(np.zeros((0, 3), dtype=np.int32), 4)
    assert len(level) == 0 and off.tolist() == [0]
    with pytest.raises(M.MsmError, match="triplet node out of range"):
        api.mcmc_schedule([[0, 1, 6]], 6)
