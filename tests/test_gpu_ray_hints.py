"""The consumers of the direction table's cells once the cells carry first-candidate hints (csrc/search_device.hpp: ray_cell_of hands a cell
out with the hinted candidate first): the unary sampling kernel, the fusion move and the plain triangle queries.

The order in which a cell's candidates are tried cannot change a result, so a table through the direction table is the table through the complete
search bit for bit (MSMHIP_DISABLE_RAYTABLE, read when a target's search structures are built, switches between the two as in
tests/test_gpu_unary.py: test_ray_table_and_general_kernel_agree), and both are the oracle's within the suite's tolerances."""
import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import problem, synthetic
from tests.helpers import oracle_cost

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sim", [2, 1], ids=["correlation", "ssd"])
@pytest.mark.parametrize("target_warp", [0.0, 2.0], ids=["regular", "warped"])
@pytest.mark.parametrize("data_order,cp_order", [(4, 2), (5, 3)])
def test_unary_table_through_hinted_cells(ctx, monkeypatch, data_order, cp_order, target_warp, sim):
    inp = problem.pairwise_inputs(data_order, cp_order, D=1, target_warp=target_warp)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate", simmeasure=sim)
    cf.get_source_data()
    U_ray = cf.computeUnaryCosts()
    monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")
    cf2, keep2 = problem.build_cost(ctx, inp, kind="univariate", simmeasure=sim)
    cf2.get_source_data()
    U_gen = cf2.computeUnaryCosts()
    monkeypatch.delenv("MSMHIP_DISABLE_RAYTABLE")
    oc = oracle_cost(inp, "univariate", simmeasure=sim)
    oc.get_source_data()
    Uo = oc.unary_table()
    assert np.isfinite(Uo).all() and U_ray.shape == Uo.shape
    assert np.array_equal(U_ray, U_gen)
    assert np.allclose(U_ray, Uo, rtol=1e-10, atol=1e-12), np.max(np.abs(U_ray - Uo))


def test_fusion_move_through_hinted_cells(ctx, monkeypatch):
    """One tripletOctets of an ho_univariate cost at ico5 / ico3 (k_ho_move is the other consumer of the reordered candidates), through the
    direction table and through the complete search.  The two searches run different kernel families for this cost, which sum a bin in different
    orders (csrc/cost_cliques.cpp: "its two kernel families sum in different orders"), so the two moves are each held to the oracle at the
    tolerance of tests/test_gpu_hot_configs.py, and to each other at that tolerance, not bit for bit."""
    rtol, atol = 1e-9, 1e-11
    hcp = dict(rmode=3, mu=0.4, kappa=1.6, k_exp=2.0, rexp=2.0, lambda_=0.025)
    inp = problem.pairwise_inputs(5, 3, D=1)
    oc = oracle_cost(inp, "ho_univariate", **hcp)
    oc.get_source_data()
    rng = np.random.default_rng(17)
    labeling, label = rng.integers(0, len(inp["labels"]), len(inp["cp_xyz"])).astype(np.int32), 7
    want = oc.triplet_octets(labeling, label, threads=8)
    got = {}
    for search in ("raytable", "complete"):
        if search == "complete":
            monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")
        cf, keep = problem.build_cost(ctx, inp, kind="ho_univariate", **hcp)
        cf.get_source_data()
        got[search] = np.array(cf.tripletOctets(labeling, label))
        assert got[search].shape == want.shape and np.isfinite(got[search]).all()
        print(search, "max |move - oracle| = %.3e" % np.abs(got[search] - want).max())
        assert np.allclose(got[search], want, rtol=rtol, atol=atol, equal_nan=True), np.abs(got[search] - want).max()
    monkeypatch.delenv("MSMHIP_DISABLE_RAYTABLE")
    assert np.allclose(got["raytable"], got["complete"], rtol=rtol, atol=atol)


@pytest.mark.parametrize("mode", [M.WEIGHTS_PROJECTED, M.WEIGHTS_RAW])
def test_queries_through_hinted_cells(ctx, mode):
    # 6 000 queries (k_query_rays answers from 4 096 on) on a warped ico4: random directions, points on and a hair off edges and vertices
    xyz, tri = M.make_mesh_from_icosa(4)
    xyz = synthetic.known_warp(xyz, seed=9, rot_deg=3.0, amp=2.0)
    rng = np.random.default_rng(8)
    q = rng.normal(size=(6000, 3))
    edge = 0.5 * (xyz[tri[:1500, 0]] + xyz[tri[:1500, 1]])
    q[:1500] = edge + rng.normal(scale=1e-9, size=edge.shape)
    q[1500:2500] = xyz[:1000] + rng.normal(scale=1e-7, size=(1000, 3))
    q = q * (100.0 / np.linalg.norm(q, axis=1, keepdims=True))
    mesh = M.Mesh(ctx, xyz, tri)
    plain = mesh.query_triangles(q, mode=mode)
    mesh.prepare_search(wait=True)
    table = mesh.query_triangles(q, mode=mode)
    assert table[0] == 0 and (np.asarray(table[1]) >= 0).all()
    for a, b in zip(plain, table):  # status, triangles, vertex ids, weights
        assert np.array_equal(a, b)
