"""The reports of the direction table's host testing hooks, pinned word for word (csrc/ray_table_check.cpp; no GPU needed).

The other tests of the hooks hold a report to a bar -- no violation, a share above a bound -- so work on the hooks that is meant to leave them alone could
move a word unseen: another point, another order of the random numbers, another candidate order.  tests/golden/ray_check_reports.json holds every word
msm_ray_table_check, msm_ray_hint_check, msm_ray_depth_check and msm_ray_cert_check report, and msm_ray_table_signature, for four small meshes with 2000
samples and seeds 1 and 2, recorded from the library as it was before the hooks came to share their candidate order and their point loop.  The folded mesh
has no table: every hook returns early for it, and that is pinned too."""
import json
import os

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api
from ray_retry_cases import mesh as retry_mesh

HEX = ("r2lo_bits", "r2hi_bits", "cell_hash", "edge_hash", "more_hash", "excl_hash")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_check_reports.json")
MESHES = ["ico2", "ico3_strongly_warped", "ico4_warped", "ico4_folded"]
SEEDS = [1, 2]
NSAMPLES = 2000


def mesh(name):
    if name == "ico4_folded":  # tests/test_ray_table_signature_cpu.py's ico4_jittered: not a simple surface, no table
        xyz, tri = M.make_mesh_from_icosa(4)
        return xyz + np.random.default_rng(4).normal(scale=2.0, size=xyz.shape), tri
    return retry_mesh(name)


def reports(name):
    """every word the hooks report for the mesh, as JSON holds it"""
    xyz, tri = mesh(name)
    sig = api.ray_table_signature(xyz, tri)
    out = {"signature": {k: ("%016x" % v if k in HEX else v) for k, v in sig.items()}}
    for seed in SEEDS:
        out["seed%d" % seed] = {
            "table": api.ray_table_check(xyz, tri, nsamples=NSAMPLES, seed=seed),
            "hint": api.ray_hint_check(xyz, tri, nsamples=NSAMPLES, seed=seed),
            "depth": api.ray_depth_check(xyz, tri, nsamples=NSAMPLES, seed=seed),
            "cert": api.ray_cert_check(xyz, tri, nsamples=NSAMPLES, seed=seed),
        }
    return json.loads(json.dumps(out))


with open(GOLDEN) as f:
    RECORDED = json.load(f)


@pytest.mark.parametrize("name", MESHES)
def test_hooks_report_the_recorded_words(built, name):
    got = reports(name)
    assert got == RECORDED[name], (got, RECORDED[name])
    for seed in SEEDS:
        r = got["seed%d" % seed]
        if name == "ico4_folded":  # no table: nothing but the zeroed report (and the hint hook's sub-cell count)
            assert got["signature"]["G"] == 0 and not r["table"]["simple"]
            assert r["table"]["points"] == r["hint"]["points"] == r["depth"]["points"] == r["cert"]["points"] == 0
        else:  # the pinned words are not trivial ones
            assert r["table"]["points"] == r["hint"]["points"] == r["depth"]["points"] == NSAMPLES and r["cert"]["points"] > NSAMPLES
            assert r["table"]["violations"] == 0 and r["hint"]["cells_changed"] == 0 and r["depth"]["unlisted"] == 0
            assert r["cert"]["fp64_failures"] == 0 and r["cert"]["reference_disagrees"] == 0 and r["cert"]["certified_points"] > 0
        assert r["hint"]["subcells"] == 3


def test_the_seeds_differ(built):
    """(the two seeds draw different points: a hook that ignored its seed would still match one record)"""
    assert RECORDED["ico4_warped"]["seed1"] != RECORDED["ico4_warped"]["seed2"]
