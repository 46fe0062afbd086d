"""Times the dedrift stage of a groupwise run on the GPU, stage by stage and in total, and -- with --baseline, in the same run, alternating with it --
the same pipeline composed from the entry points that existed before the stage was built (barycentric_coords_resample, sphere_project_warp on a mesh
handle, metric_resample, numpy for the sums, the distortion arithmetic, numpy.corrcoef and numpy.percentile for the pairs).

    python tools/time_dedrift.py [--subjects 64] [--order 6] [--rows 2] [--runs 10] [--warmup 3] [--baseline] [--out profiles/dedrift_time.json]
    python tools/time_dedrift.py --once        one pass of the new path only (for `rocprofv3 --kernel-trace --stats -- python tools/time_dedrift.py --once`)

Every timed call ends in a synchronisation of the context's stream (the library's host-array entry points are complete on return), so the host clock
around a stage measures the stage.  Mesh handles are created inside the timed window of both paths (a finished run hands over files, not handles).
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import dedrift  # noqa: E402


def inputs(S, order, D):
    """S smooth synthetic warps of the icosphere (the generator of the tests' invariance case) and data that share one smooth field"""
    xyz, tri = M.make_mesh_from_icosa(order)
    u = xyz / 100.0
    regs, datas = [], []
    field = np.random.default_rng(999).standard_normal((D, 4, 3))
    for s in range(S):
        rng = np.random.default_rng(s)
        Cm, a = rng.standard_normal((3, 3)), rng.standard_normal(3)
        y = xyz + 1.5 * (u @ Cm.T) * np.sin(2.0 * (u @ a))[:, None]
        reg = y / np.linalg.norm(y, axis=1, keepdims=True) * 100.0
        v = reg / 100.0
        noise = np.random.default_rng(2000 + s)
        rows = [np.sin(3.0 * (v @ A[0])) + 0.7 * np.cos(2.0 * (v @ A[1])) + 0.5 * np.sin(5.0 * (v @ A[2]) + 1.0) * np.cos(v @ A[3])
                + 0.05 * noise.standard_normal(len(v)) for A in field]
        regs.append(reg)
        datas.append(np.array(rows))
    return xyz, tri, regs, datas


class Clock:
    def __init__(self):
        self.t = {}

    def __call__(self, name, fn, *a, **kw):
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        self.t[name] = self.t.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
        return out


def new_path(ctx, tmpl, xyz, tri, regs, datas, percentile):
    clk = Clock()
    S = len(regs)
    d = clk("create", dedrift.Dedrift, ctx, tmpl, S)
    meshes = [clk("meshes", M.Mesh, ctx, regs[s], tri) for s in range(S)]
    for s in range(S):
        clk("accumulate", d.accumulate, meshes[s], xyz)
    W, _ = clk("finish", d.finish)
    out = [clk("correct", d.correct, s, meshes[s], xyz, datas[s]) for s in range(S)]
    stats = clk("group_stats", d.group_stats, percentile)
    summ = clk("summary", dedrift.distortion_summary, [o[2] for o in out])
    means = clk("pair_means", lambda: (dedrift.pair_means(stats[2]), dedrift.pair_means(stats[3])))
    for m in meshes:
        m.close()
    d.close()
    return clk.t, dict(W=W, out=out, stats=stats, summary=summ, means=means)


def numpy_distortion(orig, corrected, tri, tid_ptr, tid):
    """the distortion rows in numpy: the J / R arithmetic of triangle_strain per triangle, then the per-vertex means (what a user without the stage
    would write; regular meshes: every vertex has five or six triangles)"""
    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], b[:, 0] * a[:, 2] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1)

    def unit(a):
        return a / np.sqrt((a * a).sum(axis=1))[:, None]

    def frame(P):
        n = unit(cross(P[:, 2] - P[:, 0], P[:, 1] - P[:, 0]))
        b = np.zeros_like(n)
        b[:, 0] = 1.0
        c = cross(n, b)
        bad = (c * c).sum(axis=1) == 0.0
        if bad.any():
            b[bad] = [0.0, 1.0, 0.0]
            c[bad] = cross(n[bad], b[bad])
        return unit(c), unit(cross(n, c)), n

    o, f = orig[tri], corrected[tri]
    e1, e2, n = frame(o)
    t1, t2, _ = frame(f)
    neg = np.einsum("ij,ij->i", cross(e1, e2), n) < 0  # det [e1 e2 n] < 0: swap the first two columns
    c1, c2 = np.where(neg[:, None], e2, e1), np.where(neg[:, None], e1, e2)
    A = np.stack([np.einsum("tvj,tj->tv", o, c1), np.einsum("tvj,tj->tv", o, c2)], axis=2)
    B = np.stack([np.einsum("tvj,tj->tv", f, t1), np.einsum("tvj,tj->tv", f, t2)], axis=2)
    c0, c1_, c4, c5 = A[:, 1, 0] - A[:, 0, 0], A[:, 1, 1] - A[:, 0, 1], A[:, 2, 0] - A[:, 0, 0], A[:, 2, 1] - A[:, 0, 1]
    b0, b1, b4, b5 = B[:, 1, 0] - B[:, 0, 0], B[:, 1, 1] - B[:, 0, 1], B[:, 2, 0] - B[:, 0, 0], B[:, 2, 1] - B[:, 0, 1]
    det = c0 * c5 - c4 * c1_
    i00, i01, i10, i11 = c5 / det, -c4 / det, -c1_ / det, c0 / det
    F00, F01, F10, F11 = b0 * i00 + b4 * i10, b0 * i01 + b4 * i11, b1 * i00 + b5 * i10, b1 * i01 + b5 * i11
    G00, G01, G11 = F00 * F00 + F10 * F10, F00 * F01 + F10 * F11, F01 * F01 + F11 * F11
    J = np.sqrt(G00 * G11 - G01 * G01)
    I = (G00 + G11) / J
    R = np.where(I <= 2, 1.0, 0.5 * (I + np.sqrt(np.maximum(I * I - 4, 0.0))))
    lj, lr = np.log2(J), np.log2(R)
    cnt = np.diff(tid_ptr)
    return np.stack([np.add.reduceat(lj[tid], tid_ptr[:-1]) / cnt, np.add.reduceat(lr[tid], tid_ptr[:-1]) / cnt])


def baseline_path(ctx, tmpl, xyz, tri, regs, datas, percentile, adjacency):
    clk = Clock()
    S, D = len(regs), datas[0].shape[0]
    meshes = [clk("meshes", M.Mesh, ctx, regs[s], tri) for s in range(S)]
    total = np.zeros_like(xyz)
    for s in range(S):
        inv = clk("accumulate", M.barycentric_coords_resample, meshes[s], xyz, xyz)
        total = clk("accumulate", np.add, total, inv)

    def finish():
        drift = total / S
        p = drift - (drift.min(axis=0) + drift.max(axis=0)) / 2
        return p / np.sqrt((p * p).sum(axis=1))[:, None] * 100.0

    W = clk("finish", finish)
    out = []
    for s in range(S):
        clk("correct", M.sphere_project_warp_mesh, meshes[s], tmpl, W)
        corrected = clk("correct", meshes[s].get_coords)
        res = clk("correct", M.metric_resample, meshes[s], datas[s], tmpl)
        dist = clk("correct", numpy_distortion, xyz, corrected, tri, adjacency[0], adjacency[1])
        out.append((corrected, res, dist))

    def stats():
        maps = np.array([o[1] for o in out])  # S x D x V
        mean = maps.mean(axis=0)
        sd = maps.std(axis=0)
        cc = np.array([np.corrcoef(maps[:, d, :]) for d in range(D)])
        masks = maps > np.percentile(maps, percentile, axis=2)[:, :, None]
        dice = np.zeros((D, S, S))
        for d in range(D):
            m = masks[:, d, :].astype(np.float32)
            both = m @ m.T
            n = m.sum(axis=1)
            dice[d] = 2 * both / (n[:, None] + n[None, :])
        return mean, sd, cc, dice

    st = clk("group_stats", stats)
    summ = clk("summary", dedrift.distortion_summary, [o[2] for o in out])
    means = clk("pair_means", lambda: (dedrift.pair_means(st[2]), dedrift.pair_means(st[3])))
    for m in meshes:
        m.close()
    return clk.t, dict(W=W, out=out, stats=st, summary=summ, means=means)


def median_stages(runs):
    keys = runs[0].keys()
    med = {k: float(np.median([r[k] for r in runs])) for k in keys}
    totals = [sum(r.values()) for r in runs]
    return med, float(np.median(totals)), float(np.min(totals)), float(np.max(totals))


def main(argv):
    ap = argparse.ArgumentParser(prog="time_dedrift.py")
    ap.add_argument("--subjects", type=int, default=64)
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--percentile", type=float, default=75.0)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if M.device_count() < 1:
        raise SystemExit("time_dedrift.py: no GPU visible; nothing is measured without one")
    xyz, tri, regs, datas = inputs(a.subjects, a.order, a.rows)
    ctx = M.Context(0)
    tmpl = M.Mesh(ctx, xyz, tri)
    if a.once:
        new_path(ctx, tmpl, xyz, tri, regs, datas, a.percentile)
        new_path(ctx, tmpl, xyz, tri, regs, datas, a.percentile)
        print(json.dumps(dict(tool="time_dedrift", once=True)))
        return 0
    _, _, tid_ptr, tid = M.mesh_adjacency(tri, len(xyz))
    new_runs, base_runs, agree = [], [], None
    for k in range(a.warmup + a.runs):
        t_new, r_new = new_path(ctx, tmpl, xyz, tri, regs, datas, a.percentile)
        if a.baseline:
            t_base, r_base = baseline_path(ctx, tmpl, xyz, tri, regs, datas, a.percentile, (tid_ptr, tid))
            if agree is None:  # faster and different is not faster: the two paths compute the same things
                agree = dict(W=float(np.abs(r_new["W"] - r_base["W"]).max()),
                             resampled=float(max(np.abs(x[1] - y[1]).max() for x, y in zip(r_new["out"], r_base["out"]))),
                             distortion=float(max(np.abs(x[2] - y[2]).max() for x, y in zip(r_new["out"], r_base["out"]))),
                             cc=float(np.abs(r_new["stats"][2] - r_base["stats"][2]).max()), dice=float(np.abs(r_new["stats"][3] - r_base["stats"][3]).max()))
        if k >= a.warmup:
            new_runs.append(t_new)
            if a.baseline:
                base_runs.append(t_base)
    med, total, lo, hi = median_stages(new_runs)
    line = dict(tool="time_dedrift", subjects=a.subjects, order=a.order, rows=a.rows, vertices=len(xyz), runs=a.runs, warmup=a.warmup,
                new=dict(stages_ms=med, total_ms=total, total_min_ms=lo, total_max_ms=hi))
    if a.baseline:
        bmed, btotal, blo, bhi = median_stages(base_runs)
        line["baseline"] = dict(stages_ms=bmed, total_ms=btotal, total_min_ms=blo, total_max_ms=bhi)
        line["max_abs_difference"] = agree
        line["new_not_above_baseline"] = bool(total <= btotal)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
