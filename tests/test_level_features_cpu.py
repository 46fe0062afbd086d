"""The level loops' batched branch (ops.features_gpu: one level_features_batch call per level) without a GPU: over an
oracle-backed ops object whose level_features_batch IS the composition of the separate calls (registration.composed_level_features), the four option
shapes must give the bytes of the unbatched branch.  What this checks is the loops' ordering logic -- which data sets go into which call, ReferenceCache
fills and hits and their keys, the tail postponed under --IN / --INc, --INc's cut without --excl -- not a kernel."""
import numpy as np
import pytest

import histmatch_literal as HL
import trans_excl_cases as C
from newmsm_amd import group_registration, registration


class PlainOps(HL.LiteralMatchMixin, C.MaskOracleOps):
    """the oracle's ops + the literal's matching: the unbatched branch"""

    def __init__(self):
        import newmsm_amd as M

        super().__init__(M.mcmc_optimise)


class BatchedOps(PlainOps):
    """the same with the opt-in: level_features_batch is the composition of this object's own calls, and every call is recorded"""

    features_gpu = True

    def __init__(self):
        super().__init__()
        self.batches = []

    def level_features_batch(self, ico, meshes, datas, sigmas, exclude, intensity, varnorm, cutthr):
        self.batches.append((len(meshes), [float(s) for s in sigmas], bool(exclude), bool(intensity), bool(varnorm)))
        return registration.composed_level_features(self, lambda name, fn, *a: fn(*a), ico, meshes, datas, sigmas, exclude, intensity, varnorm, cutthr)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def case():
    return C.pairwise_case(order=4, D=2, cap=True)


def pair_runs(case, **kw):
    out = []
    for ops in (BatchedOps(), PlainOps()):
        lab = []
        k = dict(kw)
        if k.pop("cached", False):
            k["ref_cache"] = registration.ReferenceCache()
            C.run(ops, case, C.DISCRETE_PAIR, **k)  # fills the cache; the run compared below hits it at every level
            assert (k["ref_cache"].fills, k["ref_cache"].hits) == (2, 0)
        out.append((C.run(ops, case, C.DISCRETE_PAIR, lab, **k), lab, ops, k.get("ref_cache")))
    (got, lg, bops, cache), (want, lw, _, _) = out
    assert len(lg) == len(lw) == 4 and all(np.array_equal(a, b) for a, b in zip(lg, lw))
    assert same(got[0], want[0]) and all(same(a, b) for a, b in zip(got[1], want[1])) and got[2] == want[2]
    return bops, cache


@pytest.mark.parametrize("kw,exclude,intensity", [(dict(), False, False), (dict(excl=True, cutthr=C.CUTTHR), True, False),
                                                  (dict(intensity=True), False, True), (dict(intensity=True, cut=True, cutthr=C.CUTTHR), True, True)],
                         ids=["plain", "excl", "IN", "INc"])
def test_pairwise_loop_one_call_per_level(case, kw, exclude, intensity):
    """n = 2 per level with the level's two sigmas; --INc's cut makes the masks without --excl; the switches go into the call, nothing follows it"""
    bops, _ = pair_runs(case, **kw)
    assert bops.batches == [(2, [lv["sigma_in"], lv["sigma_ref"]], exclude, intensity, True) for lv in C.DISCRETE_PAIR]


@pytest.mark.parametrize("kw,exclude,postponed", [(dict(excl=True, cutthr=C.CUTTHR), True, False), (dict(intensity=True, cut=True, cutthr=C.CUTTHR), True, True),
                                                  (dict(intensity=True), False, True)], ids=["excl", "INc", "IN"])
def test_pairwise_loop_under_a_reference_cache(case, kw, exclude, postponed):
    """a ReferenceCache: n = 1 calls -- the input data at every level, the reference data only where the cache is filled -- without matching, with the
    variance normalisation postponed under --IN / --INc (finish_features runs over the two afterwards)"""
    bops, cache = pair_runs(case, cached=True, **kw)
    vn = not postponed
    fill = [(1, [s], exclude, False, vn) for lv in C.DISCRETE_PAIR for s in (lv["sigma_in"], lv["sigma_ref"])]
    hit = [(1, [lv["sigma_in"]], exclude, False, vn) for lv in C.DISCRETE_PAIR]
    assert bops.batches == fill + hit and (cache.fills, cache.hits) == (2, 2)
    assert len(getattr(bops, "match_calls", [])) == (4 if postponed else 0)  # two levels, two runs: the tail ran outside the batch


def test_group_loop_one_call_per_level():
    """group_case() under --INc --VN (masks from the cut, S - 1 subjects matched to subject 0, the tail inside the call): n = S per level, and the run's
    spheres, grids, energies and labelings are the unbatched run's"""
    meshes, datas, txyz, tri, levels, mask, _ = C.group_case()
    kw = dict(intensity=True, cut=True, cutthr=C.CUTTHR)
    out = []
    for ops in (BatchedOps(), PlainOps()):
        lab = []
        out.append((group_registration.run_group_multiresolution(ops, meshes, datas, txyz, tri, levels, labelings_out=lab, mask=mask, varnorm=True, fixnan=True, **kw), lab, ops))
    (got, lg, bops), (want, lw, _) = out
    assert len(lg) == len(lw) == 4 and all(np.array_equal(a, b) for a, b in zip(lg, lw))
    assert all(same(a, b) for a, b in zip(got[0], want[0])) and all(same(a, b) for a, b in zip(got[1], want[1]))
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got[2], want[2]))
    assert bops.batches == [(3, [lv["sigma_in"]] * 3, True, True, True) for lv in levels]


class Captured(Exception):
    def __init__(self, feats):
        self.feats = feats


class _StubGroup:
    """stops a level where its model has taken every subject's features"""

    def __init__(self, S):
        self.S, self.feats = S, {}

    def set_template(self, *a):
        pass

    def initialize(self, *a):
        pass

    def set_subject(self, s, mesh, feat):
        self.feats[s] = np.array(feat)
        if len(self.feats) == self.S:
            raise Captured([self.feats[k] for k in range(self.S)])


@pytest.mark.parametrize("kw,exclude,intensity", [(dict(excl=True, cutthr=C.CUTTHR), True, False), (dict(), False, False), (dict(intensity=True), False, True)],
                         ids=["excl", "plain", "IN"])
def test_group_level_features_by_option(kw, exclude, intensity):
    """the other option shapes, at the first level alone: the features the model is handed"""
    meshes, datas, txyz, tri, levels, mask, _ = C.group_case()
    feats = []
    for cls in (BatchedOps, PlainOps):
        ops = cls()
        ops.group = lambda S, *a, **k: _StubGroup(S)
        with pytest.raises(Captured) as e:
            group_registration.run_group_multiresolution(ops, meshes, datas, txyz, tri, levels, mask=mask, varnorm=True, fixnan=True, **kw)
        feats.append((e.value.feats, ops))
    (got, bops), (want, _) = feats
    assert len(got) == 3 and all(same(a, b) for a, b in zip(got, want))
    assert bops.batches == [(3, [levels[0]["sigma_in"]] * 3, exclude, intensity, True)]


def test_host_pieces_under_the_sanitizers(tmp_path):
    """tests/cpp/level_features_host_check.cpp: the variance row body and the one parallel section over the rows of all data sets as a program of their own (no
    HIP, no Python), built with -fsanitize=address,undefined: the batched section against the row body row by row, and the degenerate rows"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "level_features_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(root, "tests", "cpp", "level_features_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
