"""gMSM with the Monte Carlo optimiser, subject by subject, on the GPU: the conditional unary table and the triplet table of a subject
against the batch evaluators (bit for bit: the same kernels through the same launchers), a block against the host optimiser on the downloaded tables, a
pass against the Python composition of the calls, repeatability, the refusals, and end-to-end runs through the level loop and both executables.

Shapes: data and template ico3 (642 vertices), control grid ico1 (42 nodes, 80 triplets), the level's own label set (19 labels), D = 2; S = 2 (some nodes
of the second subject have no incident pair), 3 and 4; correlation everywhere, one SSD case with a template mask and fixnan, one DICE case."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, config, group_registration, meshio, synthetic
from tests import group_mcmc_literal as lit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, TC, MCPARAM, SWEEPS = 42, 80, 0.5, 40
CASES = {"S2": dict(S=2, crowd=(3, 11, 20)), "S3": dict(S=3), "S4": dict(S=4), "ssd_mask_fixnan": dict(S=3, sim=1, mask=True, fixnan=True), "dice": dict(S=3, sim=4)}
_groups = {}


def make(ctx, S=3, sim=2, mask=False, fixnan=False, setup=True, crowd=()):
    """crowd: these control points of subject 0 are moved most of the way to a neighbour, whose twin in the other subjects is then the closest node of
    both: the moved points' own twins are nobody's closest node"""
    dxyz, dtri = M.make_mesh_from_icosa(3)
    cxyz, ctri = M.make_mesh_from_icosa(1)
    _, mvd = M.cp_spacings(cxyz, ctri)
    samples, _ = M.label_sampling_grid(3, 0.5 * mvd)
    g = M.DiscreteGroupCostFunction(ctx, S, simmeasure=sim, lambda_=0.2, fixnan=fixnan)
    tm = M.Mesh(ctx, dxyz, dtri)
    g.set_template(tm, np.cos(dxyz[:, 0] / 30.0) if mask else None)
    g.Initialize(cxyz, ctri)
    keep = [tm]
    for s in range(S):
        feat = synthetic.features(synthetic.known_warp(dxyz, seed=90 + s, rot_deg=2.0, amp=1.0), 2, seed=5)
        mesh = M.Mesh(ctx, dxyz, dtri)
        g.reset_meshspace(s, mesh, feat)
        mesh.set_coords(synthetic.known_warp(dxyz, seed=40 + s, rot_deg=1.0 + s, amp=0.5))
        g.reset_meshspace(s, mesh, feat)
        cp = synthetic.known_warp(cxyz, seed=40 + s, rot_deg=1.0 + s, amp=0.5)
        for v in (crowd if s == 0 else ()):
            face = ctri[np.argmax(np.any(ctri == v, axis=1))]  # a triangle of v: its first other corner is a neighbour
            nb = int(face[face != v][0])
            q = 0.2 * cp[v] + 0.8 * cp[nb]
            cp[v] = q / np.linalg.norm(q) * 100.0
        g.reset_CPgrid(s, cp)
        keep.append(mesh)
    g.set_labels(samples)
    if setup:
        g.setupCostFunction()
    g._keep_meshes = keep
    return g


class Case:
    """a group with everything the tests share computed once: the pair list, its literal incidence, a labelling, every subject's tables from the batch
    evaluators' values"""

    def __init__(self, ctx, name):
        self.g = g = make(ctx, **CASES[name])
        self.S, self.L = g.S, g.L
        self.pairs = g.getPairs()
        self.ptr, self.idx = lit.incidence(self.pairs, g.S * N)
        self.lab = np.random.default_rng(17).integers(0, g.L, g.S * N).astype(np.int32)
        self._tables = {}

    def tables(self, s, lab=None):
        """(U_s, tc_s, local triplets) as the library returns them"""
        key = (s, None if lab is None else lab.tobytes())
        if key not in self._tables:
            self._tables[key] = (self.g.conditional_unary(s, self.lab if lab is None else lab), self.g.subject_triplet_table(s), self.g.subject_triplets(s))
        return self._tables[key]


@pytest.fixture
def case(ctx):
    def get(name):
        if name not in _groups:
            _groups[name] = Case(ctx, name)
        return _groups[name]

    return get


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def total_energy(c, lab):
    """the group energy from the batch evaluators: the pairs in order, then the triplets"""
    tri = c.g.getTriplets()
    pw = c.g.computePairwiseCost(np.arange(len(c.pairs)), lab[c.pairs[:, 0]], lab[c.pairs[:, 1]])
    tc = c.g.computeTripletCost(np.arange(len(tri)), lab[tri[:, 0]], lab[tri[:, 1]], lab[tri[:, 2]])
    return float(np.sum(pw) + np.sum(tc))


@pytest.mark.parametrize("name", list(CASES))
def test_conditional_unary_is_the_batch_evaluators_values_added_in_pair_order(case, name):
    c = case(name)
    assert (c.L, c.g.N, c.g.Tc) == (19, N, TC)
    if name == "S2":  # only subject 0's nodes start pairs: the nodes of subject 1 nobody is closest to have none
        assert np.any(np.diff(c.ptr)[N:] == 0)
    for s in range(c.S):
        qp, qa, qb, seg = lit.conditional_queries(c.pairs, c.ptr, c.idx, c.lab, s, N, c.L)
        want = lit.segment_sums(c.g.computePairwiseCost(qp, qa, qb), seg, N, c.L)
        got = c.tables(s)[0]
        assert same_bits(got, want), (name, s, np.nanmax(np.abs(got - want)))
        empty = np.diff(c.ptr)[s * N:(s + 1) * N] == 0
        assert np.all(got[:, empty] == 0.0) and not np.any(np.signbit(got[:, empty]))
    if name == "ssd_mask_fixnan":
        assert not np.any(np.isnan(c.tables(0)[0]))


@pytest.mark.parametrize("name", ["S3", "ssd_mask_fixnan"])
def test_subject_triplet_table_is_the_batch_evaluators(case, name):
    c = case(name)
    a, b, d = [x.ravel().astype(np.int32) for x in np.meshgrid(np.arange(c.L), np.arange(c.L), np.arange(c.L), indexing="ij")]
    for s in (0, c.S - 1):
        got = c.tables(s)[1]
        for t in (0, 37, TC - 1):
            want = c.g.computeTripletCost(np.full(len(a), s * TC + t, dtype=np.int32), a, b, d)
            assert same_bits(got[t].ravel(), want), (s, t)
    t_all = np.repeat(np.arange(TC, dtype=np.int32), 8)  # and every triplet on a few label triples
    rng = np.random.default_rng(1)
    la, lb, lc = (rng.integers(0, c.L, len(t_all)).astype(np.int32) for _ in range(3))
    assert same_bits(c.tables(1)[1][t_all, la, lb, lc], c.g.computeTripletCost(TC + t_all, la, lb, lc))
    tri = c.g.subject_triplets(1)
    assert tri.min() == 0 and tri.max() == N - 1 and np.array_equal(tri + N, c.g.getTriplets()[TC:2 * TC])


def check_block(c, s, seeds, iters=SWEEPS):
    U, tc, tri = c.tables(s)
    start = c.lab[s * N:(s + 1) * N]
    want, _, E, best = api.mcmc_optimise_chains(U, tc, tri, start, seeds, mcparam=MCPARAM, iters=iters)
    e0 = api.mcmc_energy(U, tc, tri, start)
    take = api.group_mcmc_accept(e0, E[best])
    lab, (got0, got1), acc = c.g.mcmc_subject(s, c.lab, seeds, mcparam=MCPARAM, iters=iters)
    assert acc is take
    assert same_bits([got0, got1], [e0, E[best] if take else e0])
    expect = c.lab.copy()
    if take:
        expect[s * N:(s + 1) * N] = want
    assert np.array_equal(lab, expect)
    return acc


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("draw", ["host", "device"])
@pytest.mark.parametrize("name", ["S2", "S3"])
def test_a_block_is_the_host_optimiser_on_the_downloaded_tables(ctx, case, name, draw, K):
    c = case(name)
    ctx.set_mcmc_draw(1 if draw == "device" else 0)
    try:
        accepted = [check_block(c, s, api.group_mcmc_seeds(3, 1, K, c.S, s)) for s in range(c.S)]
    finally:
        ctx.set_mcmc_draw(0)
    assert any(accepted)  # a random labelling is far from a minimum: the sweeps lower some block's energy


@pytest.mark.parametrize("name", ["S4", "ssd_mask_fixnan", "dice"])
def test_a_block_in_chunks_of_one_sweep(case, name, monkeypatch):
    monkeypatch.setenv("MSMHIP_MCMC_CHUNK_SWEEPS", "1")
    c = case(name)
    check_block(c, 1, api.group_mcmc_seeds(3, 0, 5, c.S, 1), iters=7)


@pytest.mark.parametrize("name", ["S2", "dice"])
def test_no_sweeps_accept_nothing(case, name):
    c = case(name)
    for s in range(c.S):
        assert check_block(c, s, api.group_mcmc_seeds(0, 0, 3, c.S, s), iters=0) is False
    lab, rec = c.g.mcmc_pass(c.lab, mcparam=MCPARAM, iters=0, seed=0, it=0, chains=3, passes=2)
    assert np.array_equal(lab, c.lab) and not rec[:, :, 2].any() and same_bits(rec[:, :, 0], rec[:, :, 1])


def composed_pass(c, lab, seed, it, K, passes, iters):
    """msm_group_mcmc_pass out of the three calls: the tables of every block from the library, the block on the host"""
    def tables(s, cur):
        return c.g.conditional_unary(s, cur), c.tables(s)[1], c.tables(s)[2]

    def chains(U, tc, tri, start, seeds, mcparam, n):
        return api.mcmc_optimise_chains(U, tc, tri, start, seeds, mcparam=mcparam, iters=n)

    return lit.run_pass(chains, api.mcmc_energy, tables, lab, c.S, N, MCPARAM, iters, seed, it, K, passes)


@pytest.mark.parametrize("name,K,passes", [("S2", 1, 1), ("S3", 3, 2), ("S4", 2, 1), ("ssd_mask_fixnan", 2, 2), ("dice", 2, 1)])
def test_a_pass_is_the_composition_of_its_blocks(case, name, K, passes):
    c = case(name)
    want_lab, want = composed_pass(c, c.lab, 11, 2, K, passes, SWEEPS)
    lab, rec = c.g.mcmc_pass(c.lab, mcparam=MCPARAM, iters=SWEEPS, seed=11, it=2, chains=K, passes=passes)
    assert np.array_equal(lab, want_lab)
    rec = rec.reshape(passes * c.S, 8)
    assert same_bits(rec[:, 0], [r[0] for r in want]) and same_bits(rec[:, 1], [r[1] for r in want])
    assert np.array_equal(rec[:, 2], [float(r[2]) for r in want]) and np.array_equal(rec[:, 3], [float(r[3]) for r in want])
    assert np.all(rec[:, 1] <= rec[:, 0]) and rec[:, 2].any() and np.all(rec[:, 4:] >= 0.0)
    # the group energy from the batch evaluators moves by the accepted blocks' changes: every incident pair appears once in a block's table
    before, after = total_energy(c, c.lab), total_energy(c, lab)
    change = float(np.sum(rec[:, 1] - rec[:, 0]))
    print("%s: total %.10g -> %.10g, blocks' changes %.10g" % (name, before, after, change))
    assert after < before and np.isclose(after - before, change, rtol=1e-9, atol=0.0)
    # twice the same bits
    lab2, rec2 = c.g.mcmc_pass(c.lab, mcparam=MCPARAM, iters=SWEEPS, seed=11, it=2, chains=K, passes=passes)
    assert np.array_equal(lab2, lab) and same_bits(rec2[:, :, :4], rec.reshape(passes, c.S, 8)[:, :, :4])
    assert same_bits(c.g.conditional_unary(0, lab), c.g.conditional_unary(0, lab))


def raises(code, text, fn, *a, **kw):
    with pytest.raises(M.MsmError) as e:
        fn(*a, **kw)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_refusals(ctx, case):
    c = case("S2")
    g, lab = c.g, c.lab
    seeds = api.group_mcmc_seeds(0, 0, 2, 2, 0)
    raises(-1, "subject 2 out of range", g.conditional_unary, 2, lab)
    raises(-1, "subject -1 out of range", g.subject_triplet_table, -1)
    raises(-1, "subject 2 out of range", g.mcmc_subject, 2, lab, seeds)
    bad = lab.copy()
    bad[N + 3] = g.L
    raises(-1, "msm_mcmc_optimise: label of node %d out of range" % (N + 3), g.conditional_unary, 0, bad)
    raises(-1, "label of node %d out of range" % (N + 3), g.mcmc_subject, 0, bad, seeds)
    raises(-1, "label of node %d out of range" % (N + 3), g.mcmc_pass, bad)
    raises(-1, "0 chains (1 to 256)", g.mcmc_pass, lab, chains=0)
    raises(-1, "257 chains (1 to 256)", g.mcmc_pass, lab, chains=257)
    raises(-1, "257 chains (1 to 256)", g.mcmc_subject, 0, lab, np.zeros(257, dtype=np.uint64))
    raises(-1, "the geometric distribution parameter must be in (0, 1]", g.mcmc_pass, lab, mcparam=0.0)
    raises(-1, "the geometric distribution parameter must be in (0, 1]", g.mcmc_subject, 0, lab, seeds, mcparam=1.5)
    raises(-1, "0 passes", g.mcmc_pass, lab, passes=0)
    assert np.array_equal(lab, c.lab)
    fresh = make(ctx, S=2, setup=False)  # never set up
    fresh.S, fresh.N, fresh.L, fresh.Tc = 2, N, 19, TC
    raises(-6, "msm_group_finalize() must be called first", fresh.mcmc_pass, lab)
    raises(-6, "msm_group_finalize() must be called first", fresh.conditional_unary, 0, lab)
    raises(-6, "msm_group_finalize() must be called first", fresh.subject_triplet_table, 0)
    # a rank of a sharded run: subject 1 comes from elsewhere
    fresh.setup_subjects([0])
    fresh.import_subject(1, *g.export_subject(1))
    fresh.finalize()
    raises(-6, "one rank only", fresh.mcmc_pass, lab)
    raises(-6, "one rank only", fresh.mcmc_subject, 0, lab, seeds)
    raises(-6, "one rank only", fresh.conditional_unary, 0, lab)


def test_two_level_run_through_the_level_loop(ctx):
    """run_group_discrete_opt(optimiser="mcmc") under run_group_multiresolution: every block's kept energy at most its start's, some accepted, the same
    run twice the same bits; the device draw gives the same labellings"""
    S = 3
    xyz, tri = M.make_mesh_from_icosa(3)
    meshes = [(synthetic.known_warp(xyz, seed=40 + s, rot_deg=0.0, amp=1.0), tri) for s in range(S)]
    # every subject's features rotated by 12 degrees about an axis of its own: a misalignment of the size of the label steps, so blocks are accepted
    datas = [synthetic.features(synthetic.known_warp(meshes[s][0], seed=90 + s, rot_deg=12.0, amp=4.0), 2, seed=5) for s in range(S)]
    level = dict(data_order=3, cp_order=1, sg_order=3, simmeasure=2, optimiser="mcmc", mciters=30, mcparam=MCPARAM, cost_params=dict(lambda_=0.001))
    levels = [dict(level, iters=2, sigma_in=2.0), dict(level, iters=1, sigma_in=0.0)]
    assert group_registration.run_group_discrete_opt is group_registration.run_group_level

    def run(draw):
        labs, blocks = [], []
        ops = group_registration.ProductGroupOps(ctx, mcmc_draw_gpu=draw)
        try:
            regs, _, energies = group_registration.run_group_multiresolution(ops, meshes, datas, xyz, tri, levels, fixnan=True, varnorm=True, labelings_out=labs, mcmc_chains=2,
                                                                             mcmc_passes=2, blocks_out=blocks)
        finally:
            ctx.set_mcmc_draw(0)
        return regs, energies, labs, blocks

    regs, energies, labs, blocks = run(False)
    assert len(labs) == 3 and len(blocks) == 3 and all(b.shape == (2, S, 8) for b in blocks)
    for b in blocks:
        assert np.all(b[:, :, 1] <= b[:, :, 0])
    assert any(b[:, :, 2].any() for b in blocks) and any(np.any(l != 0) for l in labs) and np.all(np.isfinite(np.concatenate(energies)))
    regs2, energies2, labs2, _ = run(True)
    assert all(np.array_equal(a, b) for a, b in zip(labs, labs2)) and energies == energies2
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(regs, regs2))
    with pytest.raises(ValueError):
        group_registration.run_group_level(group_registration.ProductGroupOps(ctx), xyz, tri, xyz, tri, np.stack(datas), [xyz] * S, 1, optimiser="fastpd")


def test_both_executables_write_the_same_files(ctx, tmp_path):
    """--groupwise with --dopt=MCMC: with MSMHIP_GROUP_MCMC=on both executables run and write byte-identical files (two chains, two passes, the device draw);
    without the variable they end with the reference's message and exit status 1"""
    import __graft_entry__ as g

    exe = g.build_cpp_newmsm()
    S = 3
    xyz, tri = M.make_mesh_from_icosa(3)
    d = str(tmp_path) + "/"
    text = "--simval=2,2\n--sigma_in=2,0\n--lambda=0.1,0.1\n--it=2,1\n--opt=DISCRETE,DISCRETE\n--CPgrid=1,1\n--SGgrid=3,3\n--datagrid=3,3\n--dopt=MCMC\n--mciters=30,30\n--mcparam=0.5\n--VN\n--fixnan\n"
    with open(d + "conf", "w") as f:
        f.write(text)
    meshio.save_surface(d + "template.surf.gii", xyz, tri)
    for s in range(S):
        sph = synthetic.known_warp(xyz, seed=40 + s, rot_deg=0.0, amp=1.0)
        meshio.save_surface(d + "sphere%d.surf.gii" % s, sph, tri)
        meshio.save_metric(d + "data%d.func.gii" % s, synthetic.features(synthetic.known_warp(sph, seed=90 + s, rot_deg=12.0, amp=4.0), 2, seed=5))
    with open(d + "meshes.txt", "w") as f:
        f.write("".join(d + "sphere%d.surf.gii\n" % s for s in range(S)))
    with open(d + "data.txt", "w") as f:
        f.write("".join(d + "data%d.func.gii\n" % s for s in range(S)))
    common = ["--groupwise", "--meshes=" + d + "meshes.txt", "--data=" + d + "data.txt", "--template=" + d + "template.surf.gii", "--conf=" + d + "conf", "--verbose"]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MSMHIP_GROUP_MCMC") and k not in ("MSMHIP_MCMC_CHAINS", "MSMHIP_MCMC_DRAW")}
    on = dict(clean, MSMHIP_GROUP_MCMC="on", MSMHIP_MCMC_CHAINS="2", MSMHIP_GROUP_MCMC_PASSES="2", MSMHIP_MCMC_DRAW="gpu")
    tools = {"py": [sys.executable, "tools/register_files.py"], "cpp": [exe]}
    for tool, cmd in tools.items():
        run = subprocess.run(cmd + common + ["--out=" + d + tool + "."], cwd=ROOT, env=on, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr
        assert "Groupwise MCMC, subject by subject: 2 chains per block, 2 passes per iteration, proposals drawn on the GPU." in run.stdout
        off = subprocess.run(cmd + common + ["--out=" + d + "off."], cwd=ROOT, env=clean, capture_output=True, text=True, timeout=600)
        assert off.returncode == 1 and "Groupwise mode is only supported in the HOCR version of MSM." in off.stderr
    moved = 0.0
    for s in range(S):
        for name in ("sphere-%d.reg.surf.gii" % s, "sphere-%d.LR.reg.surf.gii" % s, "transformed_and_reprojected-%d.func.gii" % s):
            a, b = open(d + "py." + name, "rb").read(), open(d + "cpp." + name, "rb").read()
            assert a == b and len(a) > 0, name
        moved = max(moved, float(np.max(np.abs(meshio.load_surface(d + "py.sphere-%d.LR.reg.surf.gii" % s)[0] - xyz))))
    assert moved > 1e-3  # the registration moved something
    cfg = config.parse_config(text)
    assert config.levels_from_config(cfg, 2, groupwise=True)[0][0]["optimiser"] == "mcmc"
