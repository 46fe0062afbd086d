"""A subject's patch lists reach a group by four routes -- a set-up on this GPU, msm_group_import_subject (host arrays), msm_group_import_subject_dev (one
subject in device memory) and msm_group_import_subjects_dev (a batch in strided device buffers) -- and msm_group_finalize decides the pair kernel's
lanes and LDS from what the route recorded of them.  Here: the three import routes give the same group, each refuses corrupted lists without adopting
anything, and the record is that of the lists that arrived last.  Device buffers are torch tensors, so every test runs in a child process (as
test_gpu_group.py's exchange test does)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_worker(tmp_path, body, **consts):
    script = tmp_path / "worker.py"
    script.write_text("ROOT = %r\n" % ROOT + "".join("%s = %r\n" % kv for kv in consts.items()) + body)
    env = {k: v for k, v in os.environ.items() if k != "MSMHIP_GROUP_PAIR_LANES"}
    pr = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-3000:]
    return json.loads(pr.stdout.strip().splitlines()[-1])


CRAFTED = '''
import os, sys, json
import numpy as np
import torch
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import newmsm_amd as M
import group_pair_cases as C

ctx = M.Context(0)
D, SIM, INVALID, CAPACITY = 2, 2, -1, -7
PPTR, PIDX = C.csr(CASE)
F = [np.ascontiguousarray(f) for f in C.features(D)]
ROWLEN, PER = C.N * C.L + 1, C.L * D * C.VT
rng = np.random.default_rng(31)
QUERY = tuple(rng.integers(0, hi, 400).astype(np.int32) for hi in (C.P, C.L, C.L))   # one fixed sample for every group of this process

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

def by_host(g, pptr=PPTR, pidx=PIDX):
    for s in range(C.S):
        g.import_subject(s, F[s], pptr[s], pidx[s])

def by_dev(g, pptr=PPTR, pidx=PIDX):
    for s in range(C.S):
        f, pp, pi = dev(F[s]), dev(pptr[s]), dev(pidx[s])
        torch.cuda.synchronize()   # torch's copies are complete before the library reads the tensors from its own (non-blocking) streams
        g.import_subject_dev(s, f.data_ptr(), pp.data_ptr(), pi.data_ptr(), len(pidx[s]))

def batch_buffers(pptr=PPTR, pidx=PIDX):
    """both subjects in strided buffers whose strides are longer than the arrays: (F, pptr, pidx tensors, their strides, the index counts)"""
    imax = max(len(i) for i in pidx) + 5
    f = torch.zeros((C.S, PER + 8), dtype=torch.float64, device="cuda:0")
    pp = torch.full((C.S, ROWLEN + 3), -3, dtype=torch.int32, device="cuda:0")
    pi = torch.full((C.S, imax), -1, dtype=torch.int32, device="cuda:0")
    for s in range(C.S):
        f[s, :PER] = dev(F[s].ravel()); pp[s, :ROWLEN] = dev(pptr[s]); pi[s, :len(pidx[s])] = dev(pidx[s])
    torch.cuda.synchronize()
    return f, pp, pi, (PER + 8, ROWLEN + 3, imax), [len(i) for i in pidx]

def by_batch(g, pptr=PPTR, pidx=PIDX):
    f, pp, pi, (sf, spp, spi), counts = batch_buffers(pptr, pidx)
    g.import_subjects_dev(list(range(C.S)), f.data_ptr(), sf, pp.data_ptr(), spp, pi.data_ptr(), spi, counts)

ROUTES = {"host": by_host, "dev": by_dev, "batch": by_batch}

def code_of(call):
    try:
        call()
    except M.MsmError as e:
        return e.code
    return 0

def finalized(g):
    """what finalize() decided, whether export_subject returns what went in, and the costs of the fixed sample"""
    g.finalize()
    back = [g.export_subject(s) for s in range(C.S)]
    same = all(np.array_equal(f, F[s]) and np.array_equal(pp, PPTR[s]) and np.array_equal(pi, PIDX[s]) for s, (f, pp, pi) in enumerate(back))
    launch = g.pair_launch()
    return [launch[k] for k in ("lanes", "patch_max", "npatch", "nsmall")], bool(same), g.computePairwiseCost(*QUERY)
'''

AGREE = CRAFTED + '''
sizes = C.CASES[CASE]()
nsmall = int((sizes <= 80).sum())
want = [16 if 10 * nsmall >= 9 * C.ROWS else 32, int(sizes.max()), C.ROWS, nsmall]
out, costs = {"want": want}, {}
for name, route in ROUTES.items():
    g, keep = C.empty_group(ctx, D, SIM)
    route(g)
    stats, same, costs[name] = finalized(g)
    out[name] = {"stats": stats, "export": same}
out["finite"] = int(np.isfinite(costs["host"]).sum())
out["bit_equal"] = bool(all(c.tobytes() == costs["host"].tobytes() for c in costs.values()))
print(json.dumps(out))
'''


@pytest.mark.parametrize("case", ["thresholds", "lanes16", "lanes32"])
def test_the_three_import_routes_agree(tmp_path, case):
    """The same rows and maps through import_subject, import_subject_dev (a subject at a time) and import_subjects_dev (both subjects in one call, padded
    strides): after finalize() the lanes, the largest patch, the patch count and the count of patches of at most 80 entries are those numpy gives from the
    row sizes, export_subject returns exactly what went in, and 400 pair costs are bit-equal across the routes."""
    o = run_worker(tmp_path, AGREE, CASE=case)
    for route in ("host", "dev", "batch"):
        assert o[route] == {"stats": o["want"], "export": True}, (route, o)
    assert o["bit_equal"] and o["finite"] > 300, o


REFUSE = CRAFTED + '''
M_ = C.N * C.L
def corrupted(what):
    """subject 1's lists with one fault; subject 0's as they are"""
    pp, pi = PPTR[1].copy(), PIDX[1].copy()
    if what == "end":
        pp[M_] += 1                    # pptr[M] != npidx
    elif what == "decreasing":
        pp[100] = pp[101] + 3          # row 100 has a negative length
    elif what == "id_vt":
        pi[len(pi) // 2] = C.VT
    elif what == "id_negative":
        pi[5] = -1
    return [PPTR[0], pp], [PIDX[0], pi]

g0, keep0 = C.empty_group(ctx, D, SIM)
by_host(g0)
_, _, reference = finalized(g0)
out = {}
for name, route in ROUTES.items():
    g, keep = C.empty_group(ctx, D, SIM)
    codes = [code_of(lambda: route(g, *corrupted(what))) for what in ("end", "decreasing", "id_vt", "id_negative")]
    if name == "batch":  # an index count beyond its slot, and slots too short for the row offsets: the import says INVALID, the export CAPACITY
        f, pp, pi, (sf, spp, spi), counts = batch_buffers()
        both = list(range(C.S))
        codes.append(code_of(lambda: g.import_subjects_dev(both, f.data_ptr(), sf, pp.data_ptr(), spp, pi.data_ptr(), min(counts) - 1, counts)))
        codes.append(code_of(lambda: g.import_subjects_dev(both, f.data_ptr(), sf, pp.data_ptr(), ROWLEN - 1, pi.data_ptr(), spi, counts)))
    route(g)  # nothing of the refused lists was adopted: the good ones give the costs of a group that never saw them
    stats, same, costs = finalized(g)
    again = [code_of(lambda: route(g, *corrupted(what))) for what in ("end", "decreasing", "id_vt", "id_negative")]  # ... nor over the good ones
    _, same2, costs2 = finalized(g)
    exports = []
    if name == "batch":
        exports.append(code_of(lambda: g.export_subjects_dev(both, f.data_ptr(), sf, pp.data_ptr(), spp, pi.data_ptr(), min(counts) - 1)))
        exports.append(code_of(lambda: g.export_subjects_dev(both, f.data_ptr(), sf, pp.data_ptr(), ROWLEN - 1, pi.data_ptr(), spi)))
    out[name] = {"codes": codes, "again": again, "exports": exports, "export": bool(same and same2),
                 "costs": bool(costs.tobytes() == reference.tobytes() and costs2.tobytes() == reference.tobytes())}
out["INVALID"], out["CAPACITY"], out["finite"] = INVALID, CAPACITY, int(np.isfinite(reference).sum())
print(json.dumps(out))
'''


def test_every_import_route_refuses_corrupted_lists(tmp_path):
    """pptr[M] != npidx, a decreasing row, a vertex id of Vt and one of -1: MSM_ERR_INVALID on every route, on a fresh group and over good lists, and the
    good lists give the costs of a group that never saw the bad ones.  The batched route also refuses an index count beyond its slot and slots
    too short for the row offsets (the export of such slots: MSM_ERR_CAPACITY)."""
    o = run_worker(tmp_path, REFUSE, CASE="thresholds")
    for route in ("host", "dev", "batch"):
        r = o[route]
        assert r["codes"] == [o["INVALID"]] * (6 if route == "batch" else 4) and r["again"] == [o["INVALID"]] * 4, (route, o)
        assert r["export"] and r["costs"], (route, o)
    assert o["batch"]["exports"] == [o["CAPACITY"]] * 2 and o["finite"] > 300, o


LATEST = '''
import os, sys, json
import numpy as np
import torch
sys.path.insert(0, ROOT)
import newmsm_amd as M
from newmsm_amd import synthetic

ctx = M.Context(0)
S, Dm = 4, 2
dxyz, dtri = M.make_mesh_from_icosa(3)
cxyz, ctri = M.make_mesh_from_icosa(1)
_, mvd = M.cp_spacings(cxyz, ctri)
samples, _ = M.label_sampling_grid(3, 0.5 * mvd)
def make(warp):
    """test_gpu_group.py's exchange group; warp: the seed of the subjects' spheres (the control grids are the same for every warp)"""
    g = M.DiscreteGroupCostFunction(ctx, S, lambda_=0.2)
    tm = M.Mesh(ctx, dxyz, dtri); g.set_template(tm); g.Initialize(cxyz, ctri); keep = [tm]
    for s in range(S):
        m = M.Mesh(ctx, dxyz, dtri)
        feat = synthetic.features(synthetic.known_warp(dxyz, seed=90 + s, rot_deg=2.0, amp=1.0), Dm, seed=5)
        g.reset_meshspace(s, m, feat)
        m.set_coords(synthetic.known_warp(dxyz, seed=warp + s, rot_deg=1.0 + s, amp=0.5)); g.reset_meshspace(s, m, feat)
        g.reset_CPgrid(s, synthetic.known_warp(cxyz, seed=40 + s, rot_deg=1.0 + s + (warp - 40) / 4.0, amp=0.5)); keep.append(m)
    g.set_labels(samples)
    return g, keep

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

def outcome(g):
    """pair_launch()'s statistics against those of the lists export_subject returns, the lists themselves, and a label step"""
    g.finalize()
    lists = [g.export_subject(s) for s in range(S)]
    sizes = np.concatenate([np.diff(pp) for _, pp, _ in lists])
    nsmall = int((sizes <= 80).sum())
    want = [16 if 10 * nsmall >= 9 * len(sizes) else 32, int(sizes.max()), len(sizes), nsmall]
    launch = g.pair_launch()
    lab = np.random.default_rng(3).integers(0, g.L, g.num_nodes).astype(np.int32)
    return [launch[k] for k in ("lanes", "patch_max", "npatch", "nsmall")] == want, lists, g.fusionMove(lab, 5), want

def direct(lists, warp):
    """a group that is handed these lists and nothing else"""
    g, keep = make(warp)
    g.setup_subjects([])
    for s, (f, pp, pi) in enumerate(lists):
        g.import_subject(s, f, pp, pi)
    return outcome(g) + (keep,)

def same_step(a, b):
    return bool(np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1]))

other, keep_other = make(47)   # the same subjects under other warps: other lists, of other lengths
other.setupCostFunction()
theirs = [other.export_subject(s) for s in range(S)]
out = {}

# (a) subject 3 set up here, then lists from the other group imported over it
g, keep = make(40)
g.setup_subjects([0, 1, 2, 3])
before = g.export_subject(3)[1]
f, pp, pi = (dev(a) for a in theirs[3])
torch.cuda.synchronize()
g.import_subject_dev(3, f.data_ptr(), pp.data_ptr(), pi.data_ptr(), len(theirs[3][2]))
ok, lists, step, want = outcome(g)
ok_d, lists_d, step_d, _, keep_d = direct(lists, 40)
out["a"] = {"stats": ok, "direct_stats": ok_d, "arrived": bool(np.array_equal(lists[3][1], theirs[3][1]) and np.array_equal(lists[3][2], theirs[3][2])),
            "differs": bool(not np.array_equal(before, theirs[3][1])), "step": same_step(step, step_d), "finite": int(np.isfinite(step[0]).sum()), "want": want}

# (b) subjects 2 and 3 imported in a batch, then subject 3 set up here over what was imported
g, keep = make(40)
g.setup_subjects([0, 1])
rows, imax = len(theirs[2][1]), max(len(theirs[2][2]), len(theirs[3][2])) + 5
fb = torch.stack([dev(theirs[s][0]) for s in (2, 3)])
ppb = torch.stack([dev(theirs[s][1]) for s in (2, 3)])
pib = torch.full((2, imax), -1, dtype=torch.int32, device="cuda:0")
for k, s in enumerate((2, 3)):
    pib[k, :len(theirs[s][2])] = dev(theirs[s][2])
torch.cuda.synchronize()
g.import_subjects_dev([2, 3], fb.data_ptr(), fb[0].numel(), ppb.data_ptr(), rows, pib.data_ptr(), imax, [len(theirs[s][2]) for s in (2, 3)])
g.setup_more_subjects([3])
ok, lists, step, want = outcome(g)
ok_d, lists_d, step_d, _, keep_d = direct(lists, 40)
out["b"] = {"stats": ok, "direct_stats": ok_d, "arrived": bool(np.array_equal(lists[2][1], theirs[2][1]) and np.array_equal(lists[3][1], before)),
            "differs": bool(not np.array_equal(before, theirs[3][1])), "step": same_step(step, step_d), "finite": int(np.isfinite(step[0]).sum()), "want": want}
print(json.dumps(out))
'''


def test_the_latest_arrival_of_a_subjects_lists_counts(tmp_path):
    """A real set-up (S = 4, ico3 data, ico1 control grid).  (a) subject 3 is set up here, then lists from a differently warped group are imported over
    it; (b) subjects 2 and 3 are imported in a batch, then subject 3 is set up here over the import.  After finalize() the lanes, the largest patch
    and the two patch counts are those of the lists export_subject returns for the four subjects, and a label step equals that of a group which
    was handed those lists directly -- a record left behind by the earlier arrival would show in either."""
    o = run_worker(tmp_path, LATEST)
    for k in ("a", "b"):
        r = o[k]
        assert r["stats"] and r["direct_stats"] and r["arrived"] and r["differs"] and r["step"], (k, o)
        assert r["finite"] > 500, (k, o)  # of the 252 pairs' 1 008 costs: the steps that were compared hold numbers
