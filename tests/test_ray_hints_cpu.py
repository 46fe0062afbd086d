"""The first-candidate hints of the direction table's cells (csrc/internal.hpp: kRayHintK, csrc/ray_table.cpp: build_ray_table,
csrc/search_device.hpp: ray_cell_of), on the host, through the testing hook msm_ray_hint_check (no GPU needed).

A cell lists up to four candidate triangles (more in ray_more); the spare top bits of its first three words say, for each of its 3 x 3
sub-cells, which of the candidates stored in the cell itself a kernel tries first.  The hints may reorder a cell's candidates and nothing
else: the set a kernel tries stays what it was, so no result can change (at most one listed candidate passes the acceptance test; that
guarantee is tests/test_host_logic.py: test_direction_table_accepts_only_the_reference_answer, which runs through the same ray_cell_of)."""
import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, synthetic

MESHES = ["ico3", "ico4", "ico4_warped", "ico3_strongly_warped"]


def mesh(name):
    xyz, tri = M.make_mesh_from_icosa(int(name[3]))
    if name.endswith("strongly_warped"):
        xyz = synthetic.known_warp(xyz, seed=5, rot_deg=5.0, amp=6.0)
    elif name.endswith("warped"):
        xyz = synthetic.known_warp(xyz, seed=3, rot_deg=5.0, amp=2.0)
    return xyz, tri


@pytest.fixture(scope="module")
def reports(built):
    return {name: api.ray_hint_check(*mesh(name), nsamples=20000, seed=11) for name in MESHES}


@pytest.mark.parametrize("name", MESHES)
def test_hints_keep_every_cells_candidates(reports, name):
    # in every sub-cell of every cell: the hinted candidate first, the others behind it in their stored order, the ray_more reference where it
    # was, and a first candidate whenever the cell has one.  Every mesh here has cells with more than four candidates: those are the cells
    # whose fourth word is not an id and must never be hinted at.
    rep = reports[name]
    assert rep["subcells"] >= 1 and rep["cells"] > 0 and rep["points"] == 20000
    assert rep["cells_with_more"] > 0, rep
    assert rep["cells_changed"] == 0, rep


@pytest.mark.parametrize("name", MESHES)
def test_hinted_first_candidate_is_right_at_least_as_often(reports, name):
    rep = reports[name]
    print(name, {k: rep[k] for k in ("points", "hinted", "unhinted", "listed")})
    assert rep["listed"] <= rep["points"]
    assert rep["unhinted"] <= rep["listed"] and rep["hinted"] <= rep["listed"]
    assert rep["hinted"] >= rep["unhinted"], rep


def test_hit_rates_on_ico6(built):
    # 200 000 random directions on the regular ico6 sphere (the benchmark's target): the cell's best-ranked candidate is the answer three times
    # out of four (what k_unary_rays' comment says; this pins the hook to it), the hinted one at least 0.85 of the time (a model of the table
    # gave 0.87 for 2 x 2 sub-cells, 0.91 for 3 x 3 and 0.75 without hints; measured with 3 x 3: 0.9025 hinted, 0.7420 without).
    rep = api.ray_hint_check(*M.make_mesh_from_icosa(6), nsamples=200000, seed=3)
    hinted, unhinted = rep["hinted"] / rep["points"], rep["unhinted"] / rep["points"]
    print("ico6: hinted %.4f unhinted %.4f listed %.4f" % (hinted, unhinted, rep["listed"] / rep["points"]))
    assert rep["points"] == 200000 and rep["cells_changed"] == 0
    assert 0.70 <= unhinted <= 0.80, unhinted
    assert hinted >= 0.85, hinted


@pytest.mark.parametrize("name", ["ico4_warped", "ico5"])
def test_table_does_not_depend_on_the_host_threads(built, monkeypatch, name):
    # the content cache of tables (csrc/api.cpp: RayCacheEntry) compares and copies these arrays: word for word the same with 1, 3 and 8 workers
    xyz, tri = mesh(name)
    tables = []
    for workers in ("1", "3", "8"):
        monkeypatch.setenv("MSMHIP_HOST_THREADS", workers)
        rep = api.ray_hint_check(xyz, tri, nsamples=0, return_cells=True)
        assert rep["cell_array"].shape == (rep["cells"], 4) and rep["cells"] > 0
        tables.append(rep["cell_array"])
    assert np.array_equal(tables[0], tables[1]) and np.array_equal(tables[0], tables[2])
    if rep["subcells"] > 1:
        assert (tables[0][:, :3].astype(np.uint32) >> 26).any(), "no cell carries a hint"
