"""Inputs on which the strain regulariser meets collapsed triangles, the classifier of its values and the comparison with the oracle
(tests/test_strain_collapse_cpu.py pins the oracle's side, tests/test_gpu_strain_collapse.py compares the kernels).

A label combination that puts two control points of a triplet on (nearly) the same spot gives triangle_strain (M/reg_tools.cpp:551-646) a deformed
triangle without area.  That is what a level without --rescaleL evaluates every second iteration (the labels are the sampling grid's own vertices at
half the control-point spacing: neighbours meet half way, 2e-14 to 3e-9 apart after rounding) and what gMSM evaluates on a regular control grid.
There I3 = G00 G11 - G01 G10 is a cancellation residue of a few 1e-17 either side of 0: negative, J = sqrt(I3) is NaN and so is the energy; exactly 0,
J = 0, I1st = x / 0 and the energy is +inf; positive, the energy is finite and huge (up to 4e37).  Where the sliver's normal happens to point against
the current triangle's, the entry is the folding sentinel instead (computeTripletCost, M/DiscreteCostFunction.cpp:151-152).

An EXACT coincidence -- bitwise the same point twice -- is another path and does not occur on those inputs: the normal is (0, 0, 0), the dot product
0 passes the folding test (`< 0`), calculate_tri finds no tangent pair, the 2-D triangle is all zeros, F = 0, I1 = 1, J = 0, I1st = 0/0 = NaN, and
`(I1st <= 2)` is false on it: NaN.  coincident_inputs() builds it by handing two nodes of a triplet the same rotation.

Everything here is the oracle's or plain numpy; the product's objects are built by the functions that take a context."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import newmsm_amd as M
from newmsm_amd import problem, synthetic
from oracle import oracle as O
from tests.helpers import oracle_cost

RTOL, ATOL = 1e-9, 1e-11  # those of tests/test_gpu_cost_kinds.py
BASE = dict(lambda_=0.2, mu=0.4, kappa=1.6, rmode=3)
SETTINGS = {"k2_r2": dict(k_exp=2.0, rexp=2.0), "k1.5_r1": dict(k_exp=1.5, rexp=1.0), "lambda0": dict(k_exp=2.0, rexp=2.0, lambda_=0.0)}
ANAT = dict(lambda_=0.05, mu=0.4, kappa=1.6, rmode=5, k_exp=2.0, rexp=2.0)
ANAT_STEP = 4  # every fourth triplet: the oracle takes 0.6 s per triplet of the anatomical regulariser, eight of them side by side
HO_TRIPLETS = 6  # the first six triplets that hold non-finite entries
GROUP_LAMBDA, GROUP_FOLD = 0.2, 1e7  # the group's folded cost is MSM_FOLDING itself, not times lambda

# (NaN, +inf, -inf, folded, finite above the fold value) of the oracle's values
COUNTS = {
    ("cp1", "k2_r2"): (211, 248, 0, 8136, 631),
    ("cp1", "k1.5_r1"): (211, 248, 0, 8136, 227),
    ("cp1", "lambda0"): (459, 0, 0, 548261, 0),  # 0 * inf: every non-finite strain is a NaN; the fold value is 0, as is every other entry
    ("cp2", "k2_r2"): (315, 365, 0, 25916, 2566),
    ("ho", "k2_r2"): (31, 23, 0, 478, 30),       # the six triplets of HO_TRIPLETS
    ("anat", "step4"): (328, 15, 0, 477, 189),   # every fourth triplet
    ("coincident", "k2_r2"): (10937, 128, 0, 123144, 751),  # coincident_inputs(): 15 node pairs share a rotation
    ("group", False, 0): (211, 248, 0, 8136, 663),
    ("group", True, 0): (0, 248, 0, 8347, 663),  # FIX_NAN: the 211 NaN become 1e7, the infinities stay
    ("group", False, 1): (0, 0, 0, 8306, 657),
    ("group", True, 1): (0, 0, 0, 8306, 657),
}
FIRST_NONFINITE = [(0, 16, 4, 18), (0, 16, 10, 18), (0, 16, 11, 18), (0, 16, 15, 18), (0, 16, 16, 18), (2, 14, 13, 0)]
TRIPLETS_WITH_NONFINITE = 42  # of 80

CLASSES = ("nan", "+inf", "-inf", "folded")


def classes(x, fold):
    """the four masks a value can fall into before it is a number to compare: NaN, +inf, -inf, the folding sentinel"""
    x = np.asarray(x)
    return {"nan": np.isnan(x), "+inf": x == np.inf, "-inf": x == -np.inf, "folded": x == fold}


def near_collapsed(x, fold):
    """finite entries above the fold value: triangles so close to collapse that 1 / J^k dominates"""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (x > fold)


def counts(x, fold):
    c = classes(x, fold)
    return tuple(int(c[k].sum()) for k in CLASSES) + (int(near_collapsed(x, fold).sum()),)


def has_every_class(want, fold):
    """a sample worth comparing holds at least one NaN, one +inf, one folded and one nearly collapsed entry on the oracle's side"""
    n = counts(want, fold)
    return n[0] > 0 and n[1] > 0 and n[3] > 0 and n[4] > 0


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def compare(got, want, fold, what):
    """The four class masks are the oracle's exactly; every other entry, the nearly collapsed ones included, is within RTOL / ATOL.  Returns
    the worst relative difference over the nearly collapsed entries (0.0 without any) and prints it."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    cg, cw = classes(got, fold), classes(want, fold)
    for k in CLASSES:
        if not np.array_equal(cg[k], cw[k]):
            at = np.argwhere(cg[k] != cw[k])
            first = tuple(at[0])
            raise AssertionError("%s: class %s differs at %d entries, the first at %s: got %r, oracle %r" % (what, k, len(at), first, got[first], want[first]))
    rest = ~(cw["nan"] | cw["+inf"] | cw["-inf"] | cw["folded"])
    g, w = got[rest], want[rest]
    err = np.abs(g - w)
    near = w > fold
    rel = err[near] / np.abs(w[near])
    worst = float(rel.max()) if rel.size else 0.0
    print("%s: %d entries, %s (NaN, +inf, -inf, folded, nearly collapsed); worst relative difference on the nearly collapsed %.3e, worst absolute elsewhere %.3e"
          % (what, want.size, counts(want, fold), worst, float(err[~near].max()) if (~near).any() else 0.0))
    bad = err > ATOL + RTOL * np.abs(w)
    if bad.any():
        i = int(np.argmax(np.where(bad, err / np.maximum(np.abs(w), 1e-300), 0.0)))
        raise AssertionError("%s: %d entries beyond rtol %g / atol %g, the worst got %r, oracle %r" % (what, int(bad.sum()), RTOL, ATOL, g[i], w[i]))
    return worst


# ------------------------------------------------------------------------------------------------ pairwise registration
def params(setting):
    p = dict(BASE)
    p.update(SETTINGS[setting])
    return p


@functools.lru_cache(maxsize=None)
def inputs(cp_order=1, data_order=4):
    """a regular control grid under unrescaled labels: the sampling grid's own vertices at 0.5 of the spacing"""
    return problem.pairwise_inputs(data_order=data_order, cp_order=cp_order, D=1, rescale=False, warp_amp=0.0, warp_rot=0.0)


@functools.lru_cache(maxsize=None)
def oracle_table(setting="k2_r2", cp_order=1):
    """(oracle cost function, its full triplet table T x L x L x L): left unchanged by everyone who asks"""
    oc = oracle_cost(inputs(cp_order), "univariate", **params(setting))
    oc.get_source_data()
    tab = oc.triplet_table()
    tab.setflags(write=False)
    return oc, tab


@functools.lru_cache(maxsize=None)
def coincident_inputs():
    """(inputs, [(triplet, node a, node b)]): the inputs above, but node b of 15 triplets takes node a's rotation (no node in two pairs), so that equal labels
    put the two on bitwise the same point.  Not a configuration a registration produces -- both sides take the rotations as given."""
    inp = dict(inputs())
    rot = np.array(inp["rot"]).reshape(-1, 9)
    used, shared = set(), []
    for t, ids in enumerate(inp["triplets"]):
        a, b = int(ids[0]), int(ids[1])
        if a not in used and b not in used:
            used |= {a, b}
            shared.append((t, a, b))
            rot[b] = rot[a]
    inp["rot"] = rot.reshape(np.shape(inputs()["rot"]))
    return inp, shared


@functools.lru_cache(maxsize=None)
def oracle_coincident():
    oc = oracle_cost(coincident_inputs()[0], "univariate", **params("k2_r2"))
    oc.get_source_data()
    tab = oc.triplet_table()
    tab.setflags(write=False)
    return oc, tab


def nonfinite_index(tab):
    """(n, 4): (t, a, b, c) of the table's non-finite entries, in table order"""
    return np.argwhere(~np.isfinite(tab)).astype(np.int32)


def collapse_queries(tab, extra=2000, seed=0):
    """every non-finite index of the table, its neighbours that differ in exactly one label, and `extra` random queries: four int32 columns"""
    bad = nonfinite_index(tab)
    T, L = tab.shape[0], tab.shape[1]
    rows = [bad]
    for j in (1, 2, 3):
        for l in range(L):
            q = bad[bad[:, j] != l].copy()
            q[:, j] = l
            rows.append(q)
    rng = np.random.default_rng(seed)
    rows.append(np.column_stack([rng.integers(0, T, extra)] + [rng.integers(0, L, extra) for _ in range(3)]).astype(np.int32))
    q = np.concatenate(rows).astype(np.int32)
    return tuple(np.ascontiguousarray(q[:, j]) for j in range(4))


def octet_queries(triplets, labeling, label):
    """the T x 8 evaluations of one label step as batch queries, I/Fusion/Fusion.h:188-195: k = 000..111 over (A, B, C), 0 = the current label"""
    T = len(triplets)
    t = np.repeat(np.arange(T, dtype=np.int32), 8)
    k = np.tile(np.arange(8), T)
    return (t,) + tuple(np.where(k >> (2 - j) & 1, label, labeling[triplets[t, j]]).astype(np.int32) for j in range(3))


def octets_from_table(tab, triplets, labeling, label):
    t, la, lb, lc = octet_queries(triplets, labeling, label)
    return tab[t, la, lb, lc].reshape(len(triplets), 8)


def collapse_moves(tab, triplets, N, keep=3):
    """(labeling, label, non-finite octet entries) of the `keep` label steps that meet the most collapsed triangles.  Per candidate label: walk the
    non-finite index list; where an entry holds the label at one of its three places, that place becomes the moving node and the triplet's other two
    nodes take the entry's labels, unless an earlier entry fixed them otherwise.  Nodes nobody asked for stay on the centre label."""
    bad = nonfinite_index(tab)
    L = tab.shape[1]
    found = []
    for label in range(L):
        labeling = np.full(N, -1, dtype=np.int32)
        for t, *abc in bad:
            ids = triplets[t]
            for j in range(3):
                others = [k for k in range(3) if k != j]
                if abc[j] == label and all(labeling[ids[k]] in (-1, abc[k]) for k in others):
                    for k in others:
                        labeling[ids[k]] = abc[k]
                    break
        labeling[labeling < 0] = 0
        n = int((~np.isfinite(octets_from_table(tab, triplets, labeling, label))).sum())
        found.append((n, label, labeling))
    found.sort(key=lambda f: (-f[0], f[1]))
    return [(labeling, label, n) for n, label, labeling in found[:keep]]


def collapsed_start(tab, triplets, N):
    """a labelling that sits on collapsed triangles: walk the non-finite index list and give a triplet's three nodes the entry's labels unless an
    earlier entry fixed one of them otherwise; the other nodes stay on the centre label.  Returns (labeling, triplets whose current cost is not finite)"""
    labeling = np.full(N, -1, dtype=np.int32)
    for t, *abc in nonfinite_index(tab):
        ids = triplets[t]
        if all(labeling[ids[k]] in (-1, abc[k]) for k in range(3)):
            labeling[ids] = abc
    labeling[labeling < 0] = 0
    cur = tab[np.arange(len(triplets)), labeling[triplets[:, 0]], labeling[triplets[:, 1]], labeling[triplets[:, 2]]]
    return labeling, int((~np.isfinite(cur)).sum())


def in_threads(fn, items):
    """the oracle's evaluators are re-entrant (its own OpenMP loops call them side by side) and ctypes drops the GIL"""
    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(fn, items))


def ho_triplets():
    _, tab = oracle_table()
    return [int(t) for t in np.unique(nonfinite_index(tab)[:, 0])[:HO_TRIPLETS]]


@functools.lru_cache(maxsize=None)
def oracle_ho(data_order=4):
    oc = oracle_cost(inputs(1, data_order), "ho_univariate", **params("k2_r2"))
    oc.get_source_data()
    return oc


@functools.lru_cache(maxsize=None)
def oracle_ho_tables():
    """(the six triplets, their HO tables 6 x L x L x L, the strain-only tables of the same triplets): 6 x 6 859 evaluations of the likelihood"""
    oc, ts = oracle_ho(), ho_triplets()
    tab = np.stack(in_threads(lambda t: oc.triplet_table(t, t + 1)[0], ts))
    tab.setflags(write=False)
    return ts, tab, oracle_table()[1][ts]


def anat_triplets(T=80):
    return list(range(0, T, ANAT_STEP))


@functools.lru_cache(maxsize=None)
def anatomy():
    return problem.anatomical_inputs(None, inputs())  # (the context argument is not used: host entry points only)


@functools.lru_cache(maxsize=None)
def oracle_anat():
    """(oracle cost function of the anatomical regulariser, regoption 5; the tables of every ANAT_STEP-th triplet)"""
    inp, an = inputs(), anatomy()
    oc = oracle_cost(inp, "univariate", **ANAT)
    oc.get_source_data()
    sphere = O.Mesh(an["sphere_xyz"], an["sphere_tri"])
    oc.set_anatomical(sphere, O.Octree(sphere), an["atarget_xyz"], O.Mesh(an["asource_xyz"], an["sphere_tri"]), an["w_ptr"], an["w_cp"], an["w_val"],
                      an["face_ptr"], an["face_idx"])
    tab = np.stack(in_threads(lambda t: oc.triplet_table(t, t + 1)[0], anat_triplets(oc.T)))
    tab.setflags(write=False)
    return oc, tab


def product_cost(ctx, kind="univariate", setting="k2_r2", data_order=4, cp_order=1, inp=None, **over):
    p = params(setting)
    p.update(over)
    cf, keep = problem.build_cost(ctx, inputs(cp_order, data_order) if inp is None else inp, kind=kind, **p)
    cf.get_source_data()
    return cf, keep


def product_anat(ctx):
    an = anatomy()
    cf, keep = problem.build_cost(ctx, inputs(), kind="univariate", **ANAT)
    cf.get_source_data()
    keep["sphere"] = M.Mesh(ctx, an["sphere_xyz"], an["sphere_tri"])
    cf.set_anatomical(keep["sphere"], an["atarget_xyz"], an["asource_xyz"], an["sphere_tri"], an["w_ptr"], an["w_cp"], an["w_val"], an["face_ptr"], an["face_idx"])
    return cf, keep


def octets_all_ways(ctx, cf, monkeypatch):
    """tripletOctets the three ways tests/test_gpu_cost_kinds.py::check_octets_all_ways delivers it (that function asserts finite costs and stays
    as it is): through the staging block, into the caller's mapped array -- both k_triplet_octets_packed --, and MSMHIP_OCTETS=copy, k_triplet_octets"""
    def run(labeling, label):
        got = {"pageable": np.array(cf.tripletOctets(labeling, label)), "mapped": np.array(cf.tripletOctets(labeling, label, ctx.host_array((cf.T, 8))))}
        monkeypatch.setenv("MSMHIP_OCTETS", "copy")
        got["copy"] = np.array(cf.tripletOctets(labeling, label))
        monkeypatch.delenv("MSMHIP_OCTETS")
        return got

    return run


# ------------------------------------------------------------------------------------------------ groupwise
def group_geometry():
    """S = 2 on ico3 data / ico1 control grid / 19 unrescaled labels: subject 0 on the regular control grid, subject 1 on a warped one"""
    dxyz, dtri = M.make_mesh_from_icosa(3)
    cxyz, ctri = M.make_mesh_from_icosa(1)
    _, mvd = M.cp_spacings(cxyz, ctri)
    samples, _ = M.label_sampling_grid(3, 0.5 * mvd)
    subjects = []
    for s in range(2):
        sphere = synthetic.known_warp(dxyz, seed=40 + s, rot_deg=1.0 + s, amp=0.5)
        feat = synthetic.features(synthetic.known_warp(dxyz, seed=90 + s, rot_deg=2.0, amp=1.0), 1, seed=5)
        cp = cxyz if s == 0 else synthetic.known_warp(cxyz, seed=41, rot_deg=2.0, amp=0.5)
        subjects.append((sphere, feat, cp))
    return dxyz, dtri, cxyz, ctri, samples, subjects


@functools.lru_cache(maxsize=None)
def oracle_group(fixnan):
    dxyz, dtri, cxyz, ctri, samples, subjects = group_geometry()
    og = O.Group(2, simmeasure=2, lambda_=GROUP_LAMBDA, fixnan=fixnan)
    og.set_template(O.Mesh(dxyz, dtri), None)  # (the group keeps its meshes alive)
    og.set_controlgrid(O.Mesh(cxyz, ctri))
    for s, (sphere, feat, cp) in enumerate(subjects):
        om = O.Mesh(dxyz, dtri)
        og.set_subject(s, om, feat)  # first call: the original mesh is the regular sphere
        om.set_coords(sphere)
        og.set_subject(s, om, feat)
        og.reset_cpgrid(s, cp)
    og.set_labels(samples)
    og.setup()
    return og


def product_group(ctx, fixnan):
    dxyz, dtri, cxyz, ctri, samples, subjects = group_geometry()
    g = M.DiscreteGroupCostFunction(ctx, 2, simmeasure=2, lambda_=GROUP_LAMBDA, fixnan=fixnan)
    keep = [M.Mesh(ctx, dxyz, dtri)]
    g.set_template(keep[0], None)
    g.Initialize(cxyz, ctri)
    for s, (sphere, feat, cp) in enumerate(subjects):
        m = M.Mesh(ctx, dxyz, dtri)
        g.reset_meshspace(s, m, feat)
        m.set_coords(sphere)
        g.reset_meshspace(s, m, feat)
        g.reset_CPgrid(s, cp)
        keep.append(m)
    g.set_labels(samples)
    g.setupCostFunction()
    return g, keep


def subject_queries(s, Tc, L):
    """the subject's whole table as batch queries, in table order"""
    q = np.arange(Tc * L ** 3)
    return (q // L ** 3 + s * Tc).astype(np.int32), (q // L ** 2 % L).astype(np.int32), (q // L % L).astype(np.int32), (q % L).astype(np.int32)


@functools.lru_cache(maxsize=None)
def oracle_group_table(fixnan, s):
    og = oracle_group(fixnan)
    Tc = og.T // 2
    tab = og.triplet_batch(*subject_queries(s, Tc, og.L), threads=8).reshape(Tc, og.L, og.L, og.L)
    tab.setflags(write=False)
    return tab
