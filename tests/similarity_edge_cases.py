"""Shared by tests/test_similarity_edges_cpu.py (the oracle alone: do the cases reach the branches?) and tests/test_gpu_similarity_edges.py (the
MI355X path against the oracle): inputs that send the similarity tails down the reference's two decisions, sparsesimkernel::corr,
M/similarities.cpp:129-158 -- `if (sum > 0.0)` before the divisions by the weight sum, and `if (varA == 0.0 || varB == 0.0) return 0.0`.

Every degenerate input here makes sums that are exact in any summation order (zeros; dyadic weights 0, 0.5, 1, 2^-10), so the branch taken is a
property of the input and not of rounding: a patch, bin or feature vector that is exactly 0 has mean 0 and variance 0 whatever the order, and
wa * 0 + wb * 0 + wc * 0 is exactly 0, so the sampled target values are exact too.  Constant non-zero vectors are left out on purpose: there the
reference's own serial sum decides between "exactly 0" and "1 ulp" (rounding noise on both sides, not a contract)."""
import functools

import numpy as np

import newmsm_amd as M
from newmsm_amd import problem, synthetic
from helpers import HCP
from oracle import oracle as O

CAP_Z = 60.0   # vertices above z = 60 on the sphere of radius 100: (1 - 0.6) / 2 = 20 % of the surface
FLOOR = 0.05   # least share of degenerate entries a case must reach on the oracle (about half of what it gives: a condition, not a measurement)
LAMBDA = 0.0075  # --lambda of the ico3 level of the HCP configuration (HCP: its regulariser options, from helpers)


@functools.lru_cache(maxsize=4)
def base(data_order, cp_order, D):
    """the smooth problem the cases are cut from (read only)"""
    return problem.pairwise_inputs(data_order, cp_order, D=D)


def cap(inp):
    """every row of both feature sets exactly 0 above CAP_Z of the mesh the row lives on (the medial wall of real data)"""
    ref, src = inp["ref_feat"].copy(), inp["src_feat"].copy()
    ref[:, inp["target_xyz"][:, 2] > CAP_Z] = 0.0
    src[:, inp["source_orig_xyz"][:, 2] > CAP_Z] = 0.0
    return dict(inp, ref_feat=ref, src_feat=src)


def source_cap(inp):
    return inp["source_orig_xyz"][:, 2] > CAP_Z


def zero_weights(inp, rows=None, seed=17):
    """cost-function weights from {0.5, 1.0}; about 10 % of the source vertices 0 in every row (a vertex's D weights sum to 0: the `sum > 0`
    branch of the multivariate classes, zero-weight points of a patch for the others) and rows 3 and 7 all 0 (the weight sum is not D)"""
    rows = inp["D"] if rows is None else rows
    rng = np.random.default_rng(seed)
    n = len(inp["source_xyz"])
    w = rng.choice([0.5, 1.0], size=(rows, n))
    w[:, rng.random(n) < 0.1] = 0.0
    for r in (3, 7):
        if r < rows:
            w[r] = 0.0
    return w


def binary_row(inp, seed=19):
    """one weight row from {0, 1} with 10 % zeros (a binary cost-function mask)"""
    return (np.random.default_rng(seed).random((1, len(inp["source_xyz"]))) >= 0.1).astype(np.float64)


def pow2_sum(inp, value=1.0):
    """D = 34 rows of exactly `value`, rows 3 and 7 zero: a vertex's weights sum to 32 * value, a power of two -- div_exact's reciprocal path
    with zero-weight lanes in the group"""
    assert inp["D"] == 34
    w = np.full((34, len(inp["source_xyz"])), float(value))
    w[3] = w[7] = 0.0
    return w


def weight_cap(inp, seed=23):
    """one weight row that is 0 below z = -CAP_Z (from {0.5, 1.0} elsewhere): whole patches of weight 0, and AbsoluteWeights 0 with them"""
    w = np.random.default_rng(seed).choice([0.5, 1.0], size=(1, len(inp["source_xyz"])))
    w[0, inp["source_orig_xyz"][:, 2] < -CAP_Z] = 0.0
    return w


def nan(inp, seed=29):
    """two target vertices NaN in every row, two source vertices NaN in one row: the rim of a mask, where get_adaptive_barycentric_weights
    (R/resampler.cpp:72-140) divides 0 by 0 (the docstring of trans_excl_cases.pairwise_case).  Correlation and SSD only: DICE sorts NaN in the
    reference, which is undefined."""
    rng = np.random.default_rng(seed)
    ref, src = inp["ref_feat"].copy(), inp["src_feat"].copy()
    ref[:, rng.choice(ref.shape[1], 2, replace=False)] = np.nan
    src[int(rng.integers(0, inp["D"])), rng.choice(src.shape[1], 2, replace=False)] = np.nan
    return dict(inp, ref_feat=ref, src_feat=src)


def case_inputs(inp, case):
    """(inputs, weight matrix or None) of a named case"""
    if case == "cap":
        return cap(inp), None
    if case == "cap_zero_weights":
        return cap(inp), zero_weights(inp)
    if case == "cap_binary_row":
        return cap(inp), binary_row(inp)
    if case == "pow2_sum":
        return inp, pow2_sum(inp)
    if case == "pow2_sum_small":
        return inp, pow2_sum(inp, 2.0 ** -10)
    if case == "cap_pow2_sum":
        return cap(inp), pow2_sum(inp)
    if case == "cap_pow2_sum_small":
        return cap(inp), pow2_sum(inp, 2.0 ** -10)
    if case == "weight_cap":
        return inp, weight_cap(inp)
    if case == "nan":
        return nan(inp), None
    raise ValueError(case)


def degenerate_unary(Uo, absw, sim):
    """the entries of an oracle table that are exactly the degenerate value: 0.5 * AbsoluteWeights for the correlation (r = 0 at every
    evaluation of the entry), 0 for SSD"""
    return Uo == (0.5 * absw)[None, :] if sim == 2 else Uo == 0.0


def bins_inside(ptr, idx, inside):
    """share of the groups (patches or bins) that are not empty and have every point in `inside`"""
    n = np.diff(ptr)
    cnt = np.add.reduceat(np.concatenate([inside[idx], [False]]).astype(np.int64), ptr[:-1])
    cnt[n == 0] = 0
    return float(((cnt == n) & (n > 0)).mean())


# ---------------------------------------------------------------- gMSM: three subjects, ico4 data / ico2 control grid / ico4 template, D = 2
GROUP_MASKS = ("none", "binary", "zeros")


def group_parts(mask, S=3, cp_order=2):
    """the pieces both sides are built from: the shape of tests/test_gpu_group.py's builder, with every subject's data exactly 0 above CAP_Z of its
    data mesh; mask: none, the binary template mask x < 50, or a template mask of all zeros (every common entry has weight 0).  cp_order 1:
    patches of 200 to 300 template vertices, beyond the 80 / 128 entries k_group_pairwise keeps in registers (its scalar tail)"""
    D = 2
    dxyz, dtri = M.make_mesh_from_icosa(4)
    cxyz, ctri = M.make_mesh_from_icosa(cp_order)
    _, mvd = M.cp_spacings(cxyz, ctri)
    samples, _ = M.label_sampling_grid(cp_order + 2, 0.5 * mvd)
    mk = dict(none=None, binary=(dxyz[:, 0] < 50.0).astype(np.float64), zeros=np.zeros(len(dxyz)))[mask]
    subjects = []
    for s in range(S):
        sph = synthetic.known_warp(dxyz, seed=40 + s, rot_deg=1.0 + s, amp=0.5)   # this subject's registered sphere so far
        feat = synthetic.features(synthetic.known_warp(dxyz, seed=90 + s, rot_deg=2.0, amp=1.0), D, seed=5)
        feat[:, dxyz[:, 2] > CAP_Z] = 0.0
        subjects.append((sph, feat, synthetic.known_warp(cxyz, seed=40 + s, rot_deg=1.0 + s, amp=0.5)))
    return dict(S=S, dxyz=dxyz, dtri=dtri, cxyz=cxyz, ctri=ctri, samples=samples, mask=mk, subjects=subjects)


def oracle_group(parts, sim):
    og = O.Group(parts["S"], simmeasure=sim, lambda_=0.2)
    keep = [O.Mesh(parts["dxyz"], parts["dtri"])]
    og.set_template(keep[0], parts["mask"])
    og.set_controlgrid(O.Mesh(parts["cxyz"], parts["ctri"]))
    for s, (sph, feat, cp_s) in enumerate(parts["subjects"]):
        om = O.Mesh(parts["dxyz"], parts["dtri"])
        og.set_subject(s, om, feat)
        om.set_coords(sph)
        og.set_subject(s, om, feat)
        og.reset_cpgrid(s, cp_s)
        keep.append(om)
    og.set_labels(parts["samples"])
    og.setup()
    return og, keep


def product_group(ctx, parts, sim):
    g = M.DiscreteGroupCostFunction(ctx, parts["S"], simmeasure=sim, lambda_=0.2)
    keep = [M.Mesh(ctx, parts["dxyz"], parts["dtri"])]
    g.set_template(keep[0], parts["mask"])
    g.Initialize(parts["cxyz"], parts["ctri"])
    for s, (sph, feat, cp_s) in enumerate(parts["subjects"]):
        regular = M.Mesh(ctx, parts["dxyz"], parts["dtri"])
        g.reset_meshspace(s, regular, feat)        # first call: _ORIG_MESHES = the regular sphere
        regular.set_coords(sph)
        g.reset_meshspace(s, regular, feat)
        g.reset_CPgrid(s, cp_s)
        keep.append(regular)
    g.set_labels(parts["samples"])
    g.setupCostFunction()
    return g, keep


def group_queries(P, L, n=1500, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, P, n).astype(np.int32), rng.integers(0, L, n).astype(np.int32), rng.integers(0, L, n).astype(np.int32)]
