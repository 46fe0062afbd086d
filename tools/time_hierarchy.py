"""Times the hierarchy stage on the GPU: msm_dedrift_group_stats and msm_dedrift_group_stats_select over the whole set (one path: the select uploads
a list, group_stats does not) in the same run, the select under a mask and over a part of the resident set, and one hierarchy.merge_groups stage by stage.

    python tools/time_hierarchy.py [--order 6] [--rows 2] [--sizes 64,256] [--runs 10] [--warmup 3] [--out profiles/hierarchy_time.json]
    python tools/time_hierarchy.py --once      one group_stats and one select at S = 256 only (for `rocprofv3 --kernel-trace --stats -- python ... --once`)

(a) for every S of --sizes, S synthetic maps through set_map: group_stats, the select with every subject listed and no mask, and group_stats a second
    time (the same call twice: what the machine's noise does to a ratio), taking turns within every round.  The two entry points are compared before a
    time is reported: every array bit-equal.
(b) at S = 256, when it is among the sizes: the select under a mask that keeps about 90 % of the vertices, and with a 32-subject list.
(c) one merge_groups of 2 x 32 subjects, the time of every call of its ops object summed per kind.
Every timed call is complete on return (host arrays), so the host clock around it measures it.  Reported: the median of --runs after --warmup, with the
fastest and the slowest run; for (a) also the median and the quartiles of the ratios select / group_stats and group_stats again / group_stats, round by
round.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import dedrift, hierarchy  # noqa: E402


def synthetic_maps(xyz, S, D):
    """S maps that share one smooth field and carry white noise of their own (continuous values: no ties with a percentile threshold)"""
    u = xyz / 100.0
    A = np.random.default_rng(999).standard_normal((D, 3, 3))
    field = np.array([np.sin(3.0 * (u @ A[d, 0])) + 0.7 * np.cos(2.0 * (u @ A[d, 1])) + 0.5 * np.sin(5.0 * (u @ A[d, 2]) + 1.0) for d in range(D)])
    return [field + 0.3 * np.random.default_rng(3000 + s).standard_normal(field.shape) for s in range(S)]


def smooth_warp(xyz, seed, amp):
    rng = np.random.default_rng(seed)
    Cm, a = rng.standard_normal((3, 3)), rng.standard_normal(3)
    u = xyz / 100.0
    y = xyz + amp * (u @ Cm.T) * np.sin(2.0 * (u @ a))[:, None]
    return y / np.linalg.norm(y, axis=1, keepdims=True) * 100.0


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def alternating(fns, runs, warmup):
    """{name: [ms]}: the functions take turns within every round, so that a drift of the machine meets all of them alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    t = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return t


def figure(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def spread(num, den):
    """the ratio of two legs round by round: its median and quartiles"""
    q1, med, q3 = np.percentile([x / y for x, y in zip(num, den)], [25, 50, 75])
    return dict(median=float(med), q1=float(q1), q3=float(q3))


def resident(ctx, tmpl, maps):
    d = dedrift.Dedrift(ctx, tmpl, len(maps))
    for s, m in enumerate(maps):
        d.set_map(s, m)
    return d


def assert_agreement(d, S):
    mean, stdev, cc, dice = d.group_stats(75.0)
    got = d.group_stats_select(list(range(S)), None, 75.0)
    assert np.array_equal(got[0], mean) and np.array_equal(got[1], stdev), "mean / stdev differ"
    assert np.array_equal(got[2], cc), "cc differs by %g" % float(np.abs(got[2] - cc).max())
    assert np.array_equal(got[3], dice), "dice differs"
    assert np.allclose(got[4], dedrift.pair_means(cc), rtol=0, atol=1e-9) and np.allclose(got[5], dedrift.pair_means(dice), rtol=1e-12, atol=0)


class ClockedOps(dedrift.ProductOps):
    """ProductOps with the host time of every call summed per kind"""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.ms = {}
        for name in ("begin", "accumulate", "finish", "correct", "set_warp", "group_stats_select", "distortion_summary", "end"):
            setattr(self, name, self.clocked(name, getattr(self, name)))

    def clocked(self, name, fn):
        def call(*a, **kw):
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        return call


def merge_inputs(xyz, tri, per_child, D):
    children = []
    for g in range(2):
        subjects, data = [], []
        for s in range(per_child):
            corrected = smooth_warp(xyz, 100 * g + s, 1.5)
            subjects.append((xyz, corrected, tri))
            data.append(synthetic_maps(corrected, 1, D)[0] + 0.05 * np.random.default_rng(5000 + 100 * g + s).standard_normal((D, len(xyz))))
        children.append(dict(reg=smooth_warp(xyz, 900 + g, 1.0), mean=synthetic_maps(xyz, 1, D)[0], subjects=subjects, data=data))
    return children


def main(argv):
    ap = argparse.ArgumentParser(prog="time_hierarchy.py")
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--sizes", default="64,256", help="the numbers of subjects of leg (a)")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    ctx = M.Context(a.device)
    xyz, tri = M.make_mesh_from_icosa(a.order)
    tmpl = M.Mesh(ctx, xyz, tri)
    V, D = len(xyz), a.rows
    if a.once:
        d = resident(ctx, tmpl, synthetic_maps(xyz, 256, D))
        d.group_stats(75.0)
        d.group_stats_select(list(range(256)), None, 75.0)
        d.close()
        return 0
    result = dict(order=a.order, vertices=V, rows=D, runs=a.runs, warmup=a.warmup, whole_set={}, part={}, merge={})
    for S in [int(x) for x in a.sizes.split(",")]:
        d = resident(ctx, tmpl, synthetic_maps(xyz, S, D))
        assert_agreement(d, S)
        everyone = list(range(S))
        t = alternating(dict(group_stats=lambda: d.group_stats(75.0), select=lambda: d.group_stats_select(everyone, None, 75.0),
                             group_stats_again=lambda: d.group_stats(75.0)), a.runs, a.warmup)
        result["whole_set"][str(S)] = dict(group_stats=figure(t["group_stats"]), select=figure(t["select"]), group_stats_again=figure(t["group_stats_again"]),
                                           select_over_group_stats=spread(t["select"], t["group_stats"]),
                                           again_over_group_stats=spread(t["group_stats_again"], t["group_stats"]))
        if S == 256:
            mask = (np.random.default_rng(1).uniform(size=V) < 0.9).astype(np.float64)
            some = [int(s) for s in np.random.default_rng(2).choice(S, 32, replace=False)]
            result["part"]["mask_kept"] = int(mask.sum())
            result["part"]["masked_256"] = figure(timed(lambda: d.group_stats_select(everyone, mask, 75.0), a.runs, a.warmup))
            result["part"]["list_32_of_256"] = figure(timed(lambda: d.group_stats_select(some, None, 75.0), a.runs, a.warmup))
        d.close()
    children = merge_inputs(xyz, tri, 32, D)
    stages = []
    for _ in range(a.warmup + a.runs):
        ops = ClockedOps(ctx)
        t0 = time.perf_counter()
        hierarchy.merge_groups(ops, (xyz, tri), children)
        ops.ms["total"] = (time.perf_counter() - t0) * 1e3
        stages.append(ops.ms)
    for k in stages[0]:
        result["merge"][k] = figure([s[k] for s in stages[a.warmup:]])
    result["merge"]["subjects"] = 64
    tmpl.close()
    ctx.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
