"""The direction table, whole, pinned (csrc/ray_table.cpp: build_ray_table), through the testing hook msm_ray_table_signature (no GPU needed).

The other host tests of the table see its cell array only; the edge planes, the further candidates, the exclusion records and the radius range reach the
kernels unseen.  The hook reports the table's sizes, the bit patterns of its radius range and a 64-bit FNV-1a hash of each of its four arrays;
tests/golden/ray_table_signatures.json holds what the build gave before it was cut into passes.  Work on the build that is meant to leave the table alone
must leave every one of these words alone; work that is meant to change the table records new values, and says so."""
import json
import os

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, synthetic

HEX = ("r2lo_bits", "r2hi_bits", "cell_hash", "edge_hash", "more_hash", "excl_hash")
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_table_signatures.json")) as f:
    RECORDED = json.load(f)
MESHES = ["ico3", "ico4", "ico5", "ico6", "ico4_warped", "ico3_strongly_warped", "ico5_radial", "ico4_jittered"]


def mesh(name):
    xyz, tri = M.make_mesh_from_icosa(int(name[3]))
    if name.endswith("strongly_warped"):
        xyz = synthetic.known_warp(xyz, seed=5, rot_deg=5.0, amp=6.0)
    elif name.endswith("warped"):
        xyz = synthetic.known_warp(xyz, seed=3, rot_deg=5.0, amp=2.0)
    elif name.endswith("radial"):  # off the sphere by up to 1e-3: still one triangle per ray
        xyz = xyz * (1.0 + 1e-5 * np.random.default_rng(6).normal(size=(len(xyz), 1)))
    elif name.endswith("jittered"):  # folds: not a simple surface, no table
        xyz = xyz + np.random.default_rng(4).normal(scale=2.0, size=xyz.shape)
    return xyz, tri


def signature(name):
    s = api.ray_table_signature(*mesh(name))
    return {k: ("%016x" % v if k in HEX else v) for k, v in s.items()}


@pytest.mark.parametrize("name", MESHES)
def test_table_has_its_recorded_signature(built, name):
    got = signature(name)
    assert got == RECORDED[name], (got, RECORDED[name])
    if name == "ico4_jittered":
        assert got["G"] == 0 and not got["simple"] and got["cells"] == got["edges"] == got["more"] == got["excl"] == 0
    else:
        assert got["G"] > 0 and got["cells"] == 6 * got["G"] ** 2 and got["more"] > 0 and got["excl"] > 0  # all four arrays are non-trivial


@pytest.mark.parametrize("name", ["ico4_warped", "ico5"])
def test_signature_does_not_depend_on_the_host_threads(built, monkeypatch, name):
    for workers in ("1", "3", "8"):
        monkeypatch.setenv("MSMHIP_HOST_THREADS", workers)
        assert signature(name) == RECORDED[name], workers


def test_switch_changes_the_cell_hash_and_the_certs_field_only(built, monkeypatch):
    on = signature("ico4_warped")
    monkeypatch.setenv("MSMHIP_RAY_CERTS", "off")
    off = signature("ico4_warped")
    assert off == RECORDED["ico4_warped_certs_off"]
    assert on["certs"] == 1 and off["certs"] == 0 and on["cell_hash"] != off["cell_hash"]
    assert {k for k in on if on[k] != off[k]} == {"certs", "cell_hash"}
