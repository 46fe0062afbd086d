"""The consumers of the direction table's cells once the cells carry certificates (csrc/internal.hpp: kRayWBits; csrc/search_device.hpp: ray_cell_of
says whether the sub-cell of a point is certified): k_unary_rays lets a certified lane sit out the three edge-plane loads of its first candidate and
take it untested, ray_find (the plain triangle queries, the clique kernels) returns it at once.

A certificate only skips a test that would have passed, so a table with certificates is the table without them (MSMHIP_RAY_CERTS=off, read when a
table is built) and the table through the complete search (MSMHIP_DISABLE_RAYTABLE=1) bit for bit, and all are the oracle's within the suite's
tolerances.  Each table is computed twice, and the fix-up counters must be zero again afterwards."""
import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import problem, synthetic
from tests.helpers import oracle_cost

pytestmark = pytest.mark.gpu


def table(ctx, inp, kind, sim):
    """the table of a freshly built cost function whose target has its search structures ready, twice: bit-equal, every fix-up counter zero again"""
    cf, keep = problem.build_cost(ctx, inp, kind=kind, simmeasure=sim)
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)  # (the table is otherwise built in the background, and a first launch may not have it yet)
    U = cf.computeUnaryCosts().copy()
    assert not cf.unary_fix_counters().any()
    assert np.array_equal(U, cf.computeUnaryCosts())
    assert not cf.unary_fix_counters().any()
    return U


def three_tables(ctx, monkeypatch, inp, kind, sim):
    with_certs = table(ctx, inp, kind, sim)
    monkeypatch.setenv("MSMHIP_RAY_CERTS", "off")
    without = table(ctx, inp, kind, sim)
    monkeypatch.delenv("MSMHIP_RAY_CERTS")
    monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")
    complete = table(ctx, inp, kind, sim)
    monkeypatch.delenv("MSMHIP_DISABLE_RAYTABLE")
    return with_certs, without, complete


@pytest.mark.parametrize("sim", [2, 1], ids=["correlation", "ssd"])
@pytest.mark.parametrize("target_warp", [0.0, 2.0], ids=["regular", "warped"])
@pytest.mark.parametrize("data_order,cp_order", [(4, 2), (5, 3)])
def test_unary_table_through_certified_cells(ctx, monkeypatch, data_order, cp_order, target_warp, sim):
    inp = problem.pairwise_inputs(data_order, cp_order, D=1, target_warp=target_warp)
    with_certs, without, complete = three_tables(ctx, monkeypatch, inp, "univariate", sim)
    oc = oracle_cost(inp, "univariate", simmeasure=sim)
    oc.get_source_data()
    Uo = oc.unary_table()
    assert np.isfinite(Uo).all() and with_certs.shape == Uo.shape
    assert np.array_equal(with_certs, without)
    assert np.array_equal(with_certs, complete) and np.array_equal(without, complete)
    for U in (with_certs, without, complete):
        assert np.allclose(U, Uo, rtol=1e-10, atol=1e-12), np.max(np.abs(U - Uo))


def test_multivariate_table_through_certified_cells(ctx, monkeypatch):
    # D = 3 at ico4 / ico2: the sampling kernel stores (triangle, raw weights) per sample -- the stri / sw3 outputs of a certified lane -- and one
    # common kernel reduces them
    inp = problem.pairwise_inputs(4, 2, D=3)
    with_certs, without, complete = three_tables(ctx, monkeypatch, inp, "multivariate", 2)
    oc = oracle_cost(inp, "multivariate")
    oc.get_source_data()
    Uo = oc.unary_table()
    assert np.isfinite(Uo).all() and with_certs.shape == Uo.shape
    assert np.array_equal(with_certs, without) and np.array_equal(with_certs, complete)
    for U in (with_certs, without):
        assert np.allclose(U, Uo, rtol=1e-9, atol=1e-11), np.max(np.abs(U - Uo))


@pytest.mark.parametrize("mode", [M.WEIGHTS_PROJECTED, M.WEIGHTS_RAW])
def test_queries_through_certified_cells(ctx, mode):
    # ray_find returns a certified first candidate at once.  The 6 000 queries of tests/test_gpu_ray_hints.py: test_queries_through_hinted_cells
    # (k_query_rays answers from 4 096 on) on a warped ico4: random directions, points on and a hair off edges and vertices
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
    through_table = mesh.query_triangles(q, mode=mode)
    assert through_table[0] == 0 and (np.asarray(through_table[1]) >= 0).all()
    for a, b in zip(plain, through_table):  # status, triangles, vertex ids, weights
        assert np.array_equal(a, b)


def test_fusion_move_through_certified_cells(ctx, monkeypatch):
    """One tripletOctets of an ho_univariate cost at ico5 / ico3, through the direction table and through the complete search, each held to the
    oracle at the tolerance of tests/test_gpu_hot_configs.py (the two searches run kernel families that sum a bin in different orders, so they are
    held to each other at that tolerance, not bit for bit)."""
    rtol, atol = 1e-9, 1e-11
    hcp = dict(rmode=3, mu=0.4, kappa=1.6, k_exp=2.0, rexp=2.0, lambda_=0.025)
    inp = problem.pairwise_inputs(5, 3, D=1)
    oc = oracle_cost(inp, "ho_univariate", **hcp)
    oc.get_source_data()
    rng = np.random.default_rng(23)
    labeling, label = rng.integers(0, len(inp["labels"]), len(inp["cp_xyz"])).astype(np.int32), 5
    want = oc.triplet_octets(labeling, label, threads=8)
    got = {}
    for search in ("raytable", "complete"):
        if search == "complete":
            monkeypatch.setenv("MSMHIP_DISABLE_RAYTABLE", "1")
        cf, keep = problem.build_cost(ctx, inp, kind="ho_univariate", **hcp)
        cf.get_source_data()
        keep["target"].prepare_search(wait=True)
        got[search] = np.array(cf.tripletOctets(labeling, label))
        assert got[search].shape == want.shape and np.isfinite(got[search]).all()
        print(search, "max |move - oracle| = %.3e" % np.abs(got[search] - want).max())
        assert np.allclose(got[search], want, rtol=rtol, atol=atol, equal_nan=True), np.abs(got[search] - want).max()
    monkeypatch.delenv("MSMHIP_DISABLE_RAYTABLE")
    assert np.allclose(got["raytable"], got["complete"], rtol=rtol, atol=atol)
