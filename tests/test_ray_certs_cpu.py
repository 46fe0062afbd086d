"""The certificates of the direction table's cells (csrc/internal.hpp: kRayWBits, csrc/ray_table.cpp: build_ray_table, csrc/search_device.hpp: ray_cell_of),
on the host, through the testing hook msm_ray_cert_check (no GPU needed).

One bit per sub-cell, in the top nine bits of a cell's fourth word, says that the candidate the sub-cell's hint names passes the acceptance test for every
direction of the sub-cell and needs no vouching, so k_unary_rays and ray_find take it without loading its edge planes.  A certificate may only skip a test
that would have passed: for every sampled point of a certified sub-cell the first candidate must pass the FP64 edge-plane test at the threshold the
table's proof asks for, and must be the triangle the reference's leaf search returns.  (tests/test_host_logic.py:
test_direction_table_accepts_only_the_reference_answer runs through the same certificates with its own points.)"""
import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, synthetic

MESHES = ["ico3", "ico4", "ico4_warped", "ico3_strongly_warped"]
TOP9 = np.uint32(0xFF800000)


def mesh(name):
    xyz, tri = M.make_mesh_from_icosa(int(name[3]))
    if name.endswith("strongly_warped"):
        xyz = synthetic.known_warp(xyz, seed=5, rot_deg=5.0, amp=6.0)
    elif name.endswith("warped"):
        xyz = synthetic.known_warp(xyz, seed=3, rot_deg=5.0, amp=2.0)
    return xyz, tri


@pytest.mark.parametrize("name", MESHES)
def test_a_certified_first_candidate_is_the_answer(built, name):
    # 20 000 random directions and the placed points: borders and corners of sub-cells, cells and cube faces (within 1e-6 of a cell), mesh vertices, edge
    # midpoints displaced by 1e-9
    rep = api.ray_cert_check(*mesh(name), nsamples=20000, seed=11)
    print(name, rep)
    assert rep["points"] == 20000 + rep["placed"] and rep["placed"] >= 9000
    assert rep["certified_points"] > 0 and 0 < rep["certified_subcells"] < rep["subcells"], rep
    assert rep["fp64_failures"] == 0, rep
    assert rep["reference_disagrees"] == 0, rep


def test_certified_share_on_ico6(built):
    # regular ico6 (the benchmark's target), 200 000 random directions.  A numpy model of the table (G = 256, 3 x 3 sub-cells, margins and guard band
    # ignored) put 0.596 of the directions into a sub-cell whose four corners lie in one triangle; the bar is that, lowered for the guard band, the margins
    # and the cells whose hinted triangle sits in ray_more.  Measured: 0.5713 of the 212 000 points, 0.6073 of the sub-cells.
    rep = api.ray_cert_check(*M.make_mesh_from_icosa(6), nsamples=200000, seed=3)
    random_points = rep["points"] - rep["placed"]
    assert random_points == 200000
    assert rep["fp64_failures"] == 0 and rep["reference_disagrees"] == 0, rep
    # (the share is taken over all points: the 10 000 placed ones sit on borders, vertices and edges, are certified less often, and only lower it)
    share = rep["certified_points"] / rep["points"]
    print("ico6: certified share of points %.4f, of sub-cells %.4f" % (share, rep["certified_subcells"] / rep["subcells"]))
    assert share >= 0.50, share


def test_switch_clears_the_nine_bits_and_nothing_else(built, monkeypatch):
    xyz, tri = mesh("ico4_warped")
    on = api.ray_cert_check(xyz, tri, nsamples=0, return_cells=True)
    monkeypatch.setenv("MSMHIP_RAY_CERTS", "off")
    off = api.ray_cert_check(xyz, tri, nsamples=0, return_cells=True)
    a, b = on["cell_array"].view(np.uint32), off["cell_array"].view(np.uint32)
    assert a.shape == b.shape and a.shape[0] == on["cells"] > 0
    assert np.array_equal(a[:, :3], b[:, :3])
    assert np.array_equal(a[:, 3] & ~TOP9, b[:, 3] & ~TOP9)
    assert not (b[:, 3] & TOP9).any() and off["certified_subcells"] == 0 and off["certified_points"] == 0
    assert (a[:, 3] & TOP9).any() and on["certified_subcells"] > 0


@pytest.mark.parametrize("name", ["ico4_warped", "ico5"])
def test_cells_do_not_depend_on_the_host_threads(built, monkeypatch, name):
    # the content cache of tables (csrc/api.cpp: RayCacheEntry) compares and copies these arrays: word for word the same with 1, 3 and 8 workers
    xyz, tri = mesh(name)
    tables = []
    for workers in ("1", "3", "8"):
        monkeypatch.setenv("MSMHIP_HOST_THREADS", workers)
        rep = api.ray_cert_check(xyz, tri, nsamples=0, return_cells=True)
        tables.append(rep["cell_array"])
    assert np.array_equal(tables[0], tables[1]) and np.array_equal(tables[0], tables[2])
    assert (tables[0][:, 3].view(np.uint32) & TOP9).any(), "no cell carries a certificate"
