"""Times msm_histogram_match (--IN / --INc) warm, beside the same definition in numpy on the host, at three shapes on ico6
(40 962 vertices): the groupwise level (S = 64 subjects: 63 sources of D = 2 rows against subject 0), D = 1 and D = 32 (one source each).

    python tools/time_histmatch.py [--runs 10] [--warmup 3] [--order 6] [--kernel-stats stats.csv] [--out profiles/histmatch_time.json]
    python tools/time_histmatch.py --once     two calls per shape only (for `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_histmatch.py --once`)

The entry point is complete on return (it ends in a synchronisation of the context's stream), so the host clock around a call measures the call: uploads,
four kernels, download.  The host side is the definition vectorised per row (numpy.bincount, cumsum, searchsorted): the same arithmetic, and the tool checks
that the two results are equal bit for bit before it reports a time.  --kernel-stats: the *_kernel_stats.csv of a separate profiler run of --once; the
k_hist_* rows are copied into the result (a profiled run's wall clock is not reported).  Prints one JSON line; --out also writes it to a file."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import newmsm_amd as M  # noqa: E402

B = 256
SHAPES = [("groupwise_S64_D2", 63, 2), ("pairwise_D1", 1, 1), ("pairwise_D32", 1, 32)]


def host_row(x, mx, y, my):
    """one row by the definition, vectorised"""
    fx, fy = np.isfinite(x), np.isfinite(y)
    cx, cy = (fx & (mx > 0)) if mx is not None else fx, (fy & (my > 0)) if my is not None else fy
    if not cx.any() or not cy.any():
        return x.copy()
    lo_x, hi_x, lo_y, hi_y = x[fx].min(), x[fx].max(), y[fy].min(), y[fy].max()
    if hi_x == lo_x or hi_y == lo_y:
        return x.copy()
    w_x, w_y = (hi_x - lo_x) / B, (hi_y - lo_y) / B
    bx = np.minimum(np.maximum(((x[cx] - lo_x) / w_x).astype(np.int64) + 1, 1), B)
    by = np.minimum(np.maximum(((y[cy] - lo_y) / w_y).astype(np.int64) + 1, 1), B)
    hx, hy = np.bincount(bx, minlength=B + 1)[1:], np.bincount(by, minlength=B + 1)[1:]
    cdf_x, cdf_y = np.cumsum(hx) / float(hx.sum()), np.cumsum(hy) / float(hy.sum())
    j = np.searchsorted(cdf_y, cdf_x, side="left")  # newbin - 1: the smallest j with CDF_y[j] >= c
    j[B - 1] = B - 1
    below = cdf_y[np.maximum(j - 1, 0)]
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.where(j > 0, (cdf_x - below) / (cdf_y[j] - below), 0.0)
    dist[B - 1] = 0.0
    t = np.minimum(np.maximum(lo_y + j * w_y + dist * w_y, lo_y), hi_y)
    out = x.copy()
    out[cx] = t[bx - 1]
    return out


def host_match(src, ref, src_excl, ref_excl):
    out = np.empty_like(src)
    for s in range(src.shape[0]):
        for d in range(src.shape[1]):
            out[s, d] = host_row(src[s, d], None if src_excl is None else src_excl[s, 0], ref[d], None if ref_excl is None else ref_excl[0])
    return out


def inputs(n_src, D, V, seed):
    """smooth-ish data of different scales per matrix, a zero-valued cap of a tenth of the vertices (the medial wall) with its one-row mask"""
    rng = np.random.default_rng(seed)
    src = rng.normal(size=(n_src, D, V)) * rng.uniform(0.5, 3.0, size=(n_src, D, 1)) + rng.uniform(-1.0, 1.0, size=(n_src, D, 1))
    ref = rng.gamma(2.0, 2.0, size=(D, V)) - 1.5
    cap = V // 10
    src[:, :, :cap] = 0.0
    ref[:, :cap] = 0.0
    src_excl, ref_excl = np.ones((n_src, 1, V)), np.ones((1, V))
    src_excl[:, :, :cap] = 0.0
    ref_excl[:, :cap] = 0.0
    return src, ref, src_excl, ref_excl


def timed(fn, runs, warmup):
    ms = []
    for k in range(warmup + runs):
        t0 = time.perf_counter()
        out = fn()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def kernel_rows(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "k_hist_" in r["Name"]:
                name = r["Name"][r["Name"].index("k_hist_"):].split("(")[0]
                rows[name] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


def main(argv):
    ap = argparse.ArgumentParser(prog="time_histmatch.py")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if M.device_count() < 1:
        raise SystemExit("time_histmatch.py: no GPU visible; nothing is measured without one")
    V = M.icosphere_counts(a.order)[0]
    ctx = M.Context(0)
    line = dict(tool="time_histmatch", order=a.order, vertices=V, runs=a.runs, warmup=a.warmup, shapes={})
    for k, (name, n_src, D) in enumerate(SHAPES):
        src, ref, se, re_ = inputs(n_src, D, V, 50 + k)
        if a.once:
            M.histogram_match(ctx, src, ref, se, re_)
            M.histogram_match(ctx, src, ref, se, re_)
            continue
        got, gpu = timed(lambda: M.histogram_match(ctx, src, ref, se, re_), a.runs, a.warmup)
        want, host = timed(lambda: host_match(src, ref, se, re_), max(1, a.runs // 3), 1)
        equal = bool(np.array_equal(got, want))
        if not equal:  # faster and different is not faster
            raise SystemExit("time_histmatch.py: %s: the GPU result differs from the host's in %d values" % (name, int((got != want).sum())))
        line["shapes"][name] = dict(sources=n_src, rows=D, values=int(src.size), megabytes_up_and_down=round((2 * src.nbytes + ref.nbytes + se.nbytes + re_.nbytes) / 1e6, 1),
                                    gpu_call=gpu, host_numpy=host, equal_bits=equal, gpu_not_slower=bool(gpu["median_ms"] <= host["median_ms"]))
    if a.kernel_stats:
        line["kernels"] = kernel_rows(a.kernel_stats)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
