"""The large-patch cases of tests/unary_patch_cases.py on the oracle alone, and the unary launch plan (msm_unary_launch_plan, msm_unary_fix_offsets:
the host arithmetic the launchers act on) on its own -- no GPU.  The first part makes sure that tests/test_gpu_unary_patches.py compares what it
claims: patches of the sizes each threshold needs, and oracle tables that are finite in every entry and far from constant (np.ptp > 0.1; measured
0.19 to 0.87), so the GPU test compares every entry without a NaN-for-NaN rule.  The bounds are conditions; the measured sizes are in the docstrings."""
import numpy as np
import pytest

import unary_patch_cases as P
from newmsm_amd import api

SWEEP_L = [1, 15, 19, 80, 300]
SWEEP_PMAX = [0, 1, 96, 97, 571, 572, 768, 1024, 1025, 2560, 2561, 4096, 4097, 10240, 10241, 11512]
KINDS = [("univariate", 1, 2), ("univariate", 1, 4), ("multivariate", 3, 2), ("multivariate", 12, 1), ("patchwise", 12, 2), ("patchwise", 40, 1),
         ("patchwise", 3, 4), ("multivariate", 3, 4)]


@pytest.mark.parametrize("name", list(P.CASES))
def test_patch_sizes(name):
    """A 200..253, B 722..726, C 776..1012, D 929..1230, E 2471..2478, F 2856..2875, G 4484..4511, H 5596..5618, X 11435..11512 (measured)"""
    _, _, _, N, L, lo, hi = P.CASES[name]
    ptr, sizes = P.patches(name)
    assert len(sizes) == N and len(P.inputs(name)["labels"]) == L
    assert lo <= sizes.min() and sizes.max() <= hi, (sizes.min(), sizes.max())


@pytest.mark.parametrize("name,kind,D,sim", [(n, "univariate", 1, 2) for n in P.TABLES] + [("D", "patchwise", 3, 4), ("F", "multivariate", 3, 2), ("F", "multivariate", 12, 2)])
def test_oracle_table_is_finite_and_varied(name, kind, D, sim):
    """spread of the oracle's table (np.ptp), measured: 0.19 to 0.87 over the cases"""
    U = P.oracle_table(name, kind, D, sim)
    assert U.shape == P.CASES[name][4:2:-1]
    assert np.isfinite(U).all() and np.ptp(U) > 0.1, np.ptp(U)


def check_plan(p, L, pmax):
    assert 1 <= p["nsplit"] <= max(L, 1)
    assert p["pmax"] == pmax and p["reduce_threads"] in (64, 256)
    fits = p["sampler_lds"] <= P.LDS_WORKGROUP and p["reduce_lds"] <= P.LDS_WORKGROUP
    assert fits or p["refused"], p
    if p["refused"] == "sampler":
        assert p["sampler_lds"] > P.LDS_WORKGROUP - 64  # refused for its size (static LDS variables included), not for anything else
    if p["refused"] == "reduction":
        assert p["reduce_lds"] > P.LDS_WORKGROUP - 64


def check_offsets(N, L, pmax, pptr, order, nsplit):
    off = api.unary_fix_offsets(L, pmax, pptr, order).astype(np.int64)
    assert len(off) == P.SEGMENTS + 1 and off[0] == 0
    assert (np.diff(off) >= 0).all()
    assert off[-1] == L * int(pptr[-1])  # every sample has a slot: a segment "cannot overflow" (SamplesArgs)
    used = np.zeros(P.SEGMENTS, dtype=np.int64)
    total = 0
    for seg, n in P.workgroup_shares(N, L, nsplit, pptr, order):
        used[seg] += n  # a workgroup's share starts where the shares before it in its segment end
        assert off[seg] + used[seg] <= off[seg + 1], (seg, n)
        total += n
    assert total == L * int(pptr[-1])  # the label ranges of the nsplit workgroups cover every label exactly once


@pytest.mark.parametrize("ray_table", [True, False])
@pytest.mark.parametrize("kind,D,sim", KINDS)
def test_plan_sweep(kind, D, sim, ray_table):
    for L in SWEEP_L:
        for pmax in SWEEP_PMAX:
            check_plan(api.unary_launch_plan(kind, sim, D, L, pmax, ray_table), L, pmax)


def test_plan_thresholds_at_19_labels():
    """the values the thresholds of DESIGN.md section 5.2 are quoted for"""
    plan = lambda pmax, ray=True, kind="univariate", D=1, sim=2: api.unary_launch_plan(kind, sim, D, 19, pmax, ray)
    # nsplit: min(4, ceil(19 pmax / 768)), then raised while k_unary_samples' LDS, 8 (5 pmax + 171 + lper pmax) + 18 432 bytes, exceeds 64 KB:
    # lper = 5 holds to 571, lper = 2 to 816; from 817 every label has a workgroup of its own, and from 953 that needs more than 64 KB
    assert [plan(p)["nsplit"] for p in (40, 41, 80, 81, 121, 122, 571, 572, 816, 817, 11512)] == [1, 2, 2, 3, 3, 4, 4, 5, 10, 19, 19]
    assert plan(952, ray=False)["sampler_lds"] <= P.LDS_DEFAULT < plan(953, ray=False)["sampler_lds"]
    assert not plan(3000, ray=False)["refused"] and plan(3001, ray=False)["refused"] == "sampler"  # 48 pmax + 19 800 (+ 16 static) <= 160 KB
    # k_unary_rays with one label per workgroup: 28 pmax + 1 400 bytes (+ 16 static)
    assert plan(2290)["sampler_lds"] <= P.LDS_DEFAULT < plan(2291)["sampler_lds"]
    assert not plan(5800)["refused"] and plan(5801)["refused"] == "sampler"
    # k_unary_reduce_flat / _univariate: 16 pmax
    assert plan(4096)["reduce_lds"] == 64 * P.KB and plan(4097)["reduce_lds"] > P.LDS_DEFAULT
    assert plan(5000, sim=4)["reduce"] == "univariate" and plan(5000, sim=4)["reduce_lds"] == 16 * 5000
    # k_unary_reduce_features with patchwise DICE: 64 pmax with four wavefronts, 16 pmax with one
    pw = lambda pmax: plan(pmax, kind="patchwise", D=3, sim=4)
    assert pw(1024)["reduce_lds"] == 64 * P.KB and pw(1025)["reduce_lds"] > P.LDS_DEFAULT
    assert (pw(2560)["reduce_threads"], pw(2560)["reduce_lds"]) == (256, 160 * P.KB) and (pw(2561)["reduce_threads"], pw(2561)["reduce_lds"]) == (64, 16 * 2561)
    # the reductions' own limits (16 pmax <= 160 KB: 10 240 points) lie beyond what either sampler admits even with a single label (k_unary_rays:
    # 28 pmax + 104 + 16 static): the sampler is what refuses, and no plan is left with a reduction above a workgroup's LDS
    one = lambda pmax, **kw: api.unary_launch_plan(kw.get("kind", "univariate"), kw.get("sim", 2), kw.get("D", 1), 1, pmax, True)
    assert not one(5847)["refused"] and one(5848)["refused"] == "sampler"
    for kw in (dict(), dict(sim=4), dict(kind="patchwise", D=3, sim=4)):
        assert one(10241, **kw)["refused"] and one(5847, **kw)["reduce_lds"] <= P.LDS_WORKGROUP
    assert [plan(100, kind=k, D=D, sim=s)["reduce"] for k, D, s in KINDS] == ["flat", "univariate", "features", "mv8", "pw8<4>", "pw8<8>", "features", "features"]


@pytest.mark.parametrize("name", list(P.CASES))
def test_fix_offsets_of_the_cases(name):
    """the cases' real patches in the real launch order (Morton order of the control points)"""
    _, _, _, N, L, _, _ = P.CASES[name]
    ptr, sizes = P.patches(name)
    order = api.unary_launch_order(P.inputs(name)["cp_xyz"])
    assert sorted(order) == list(range(N))
    pmax = int(sizes.max())
    p = api.unary_launch_plan("univariate", 2, 1, L, pmax, True)
    check_plan(p, L, pmax)
    check_offsets(N, L, pmax, ptr, order, p["nsplit"])


def test_fix_offsets_sweep():
    """ragged synthetic patches (sizes from 0 to pmax, control-point counts that are no multiple of 8) over the sweep of the plan"""
    rng = np.random.default_rng(5)
    for N in (1, 12, 42, 163):
        order = rng.permutation(N).astype(np.int32)
        for L in SWEEP_L:
            for pmax in SWEEP_PMAX:
                sizes = rng.integers(0, pmax + 1, N)
                sizes[rng.integers(N)] = pmax
                ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
                nsplit = api.unary_launch_plan("univariate", 2, 1, L, pmax, True)["nsplit"]
                check_offsets(N, L, pmax, ptr, order, nsplit)
