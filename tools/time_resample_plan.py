"""Times a resampling plan (msm_resample_plan_*) beside the way the same job was done before it, on the GPU only.

    python tools/time_resample_plan.py [--repeats 3] [--maps 1200] [--kernel-stats stats.csv] [--out profiles/resample_plan_time.json]
    python tools/time_resample_plan.py --once     one apply_dev per shape and dtype (for `rocprofv3 --kernel-trace --stats --output-format csv -- python ... --once`)

Shapes: a warped ico7 sphere (163 842 vertices) resampled to ico6 (40 962), and a warped ico6 sphere to ico6; --maps float32 maps (a resting-state run)
and 4 float64 maps (what a registration level resamples).  Reported per shape:
    create_ms        msm_resample_plan_create (two searches, the list surgery, the copy out of the context's scratch), host clock, complete on return
    plan_apply_ms    ResamplePlan.apply with host arrays: slabs through the pinned staging blocks, host clock around a call that ends synchronised
    baseline_ms      the same maps through metric_resample in chunks of 32 rows widened to float64, as that entry point requires -- it rebuilds trees and
                     weights per chunk and moves twice the bytes.  Alternated with the plan call, --repeats times each; `apart` says whether the slower
                     plan call is still faster than the fastest baseline call (the difference exceeds the spread of either)
    apply_dev_ms     ResamplePlan.apply_dev on device tensors, by device events on the context's stream
    algorithmic bytes of an apply (tile_bytes below), over apply_dev_ms and over the summed kernel time of a separate profiler run (--kernel-stats),
    as a share of the HBM peak (8.0 TB/s, MI355X_MICROARCH.md): the apply is bandwidth-bound, its FP64 work is two operations per 12 to 16 bytes read.
The float64 results of the two ways are compared bit for bit, and the float32 result with the baseline's rounded once: a time is only printed when they
are equal.  Fails without a device: nothing here is measured on a CPU."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import synthetic  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X_MICROARCH.md
SHAPES = [("ico7_to_ico6", 7, 6), ("ico6_to_ico6", 6, 6)]
BASELINE_CHUNK = 32


def tile_bytes(V_in, V_out, nnz, nd, es):
    """Bytes one tile of nd <= PLAN_TILE maps of es-byte elements has to move at the least (csrc/resample_plan_kernels.hip): the maps in (read) and the
    vertex-major tile (written); the tile read once by the row kernel -- a vertex' line is used by several rows, every further use is expected from the
    L2 --, one pass over the rows (4-byte columns, 8-byte weights, row offsets) and the vertex-major result (written); the result read and written
    map-major.  Lines of a ragged tile are counted at the width that is used."""
    maps_in, maps_out = V_in * nd * es, V_out * nd * es
    return (maps_in + maps_in) + (maps_in + 12 * nnz + 4 * (V_out + 1) + maps_out) + (maps_out + maps_out)


def apply_bytes(V_in, V_out, nnz, D, es):
    full, rest = divmod(D, M.PLAN_TILE)
    return full * tile_bytes(V_in, V_out, nnz, M.PLAN_TILE, es) + (tile_bytes(V_in, V_out, nnz, rest, es) if rest else 0)


def baseline(min_, mnew, data):
    """the parent commit's way: metric_resample per chunk of rows, in float64"""
    out = np.empty((data.shape[0], mnew.V))
    for d0 in range(0, data.shape[0], BASELINE_CHUNK):
        M.metric_resample(min_, data[d0:d0 + BASELINE_CHUNK].astype(np.float64), mnew, out=out[d0:d0 + BASELINE_CHUNK])
    return out


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def dev_apply_ms(ctx, plan, host, repeats):
    """(milliseconds by device events per repeat, the result as a host array)"""
    import torch

    stream = torch.cuda.ExternalStream(ctx.stream)
    t = torch.from_numpy(host).to("cuda")
    out = torch.empty((host.shape[0], plan.V_out), dtype=t.dtype, device="cuda")
    torch.cuda.synchronize()
    ms = []
    for k in range(repeats + 1):  # the first call warms up (scratch of the tiles)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        plan.apply_dev(t, out)
        e1.record(stream)
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_time(e1))
    return ms, out.cpu().numpy()


def kernel_rows(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "k_plan_" in r["Name"]:
                name = r["Name"][r["Name"].index("k_plan_"):].split("(")[0]
                rows[name] = dict(calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) / 1e6, average_us=float(r["AverageNs"]) / 1e3)
    return rows


def main(argv):
    ap = argparse.ArgumentParser(prog="time_resample_plan.py")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--maps", type=int, default=1200)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import torch  # noqa: F401  before the library is loaded: it then shares torch's HIP runtime (the other way round torch finds no device)

    if M.device_count() < 1:
        raise SystemExit("time_resample_plan.py: no GPU visible; nothing is measured without one")
    if a.repeats < 3:
        raise SystemExit("time_resample_plan.py: at least three repeats")
    ctx = M.Context(0)
    rng = np.random.default_rng(77)
    line = dict(tool="time_resample_plan", repeats=a.repeats, tile=M.PLAN_TILE, hbm_peak_bytes_per_s=HBM_PEAK, shapes={})
    for name, oin, onew in SHAPES:
        xin, tin = M.make_mesh_from_icosa(oin)
        xnew, tnew = M.make_mesh_from_icosa(onew)
        min_, mnew = M.Mesh(ctx, synthetic.known_warp(xin, seed=21, rot_deg=5.0, amp=1.0), tin), M.Mesh(ctx, xnew, tnew)
        d32 = rng.standard_normal((a.maps, len(xin)), dtype=np.float32)
        d64 = rng.standard_normal((4, len(xin)))
        M.ResamplePlan(min_, mnew).close()  # warm: trees, scratch
        created = []
        for k in range(a.repeats):
            t0 = time.perf_counter()
            plan = M.ResamplePlan(min_, mnew)
            created.append((time.perf_counter() - t0) * 1e3)
            if k + 1 < a.repeats:
                plan.close()
        V_in, V_out, nnz, longest = plan.sizes()
        if a.once:
            for host in (d32, d64):
                dev_apply_ms(ctx, plan, host, 1)
            continue
        entry = dict(V_in=V_in, V_out=V_out, nnz=nnz, longest_row=longest, create_ms=stats(created), cases={})
        for case, host in (("float32_D%d" % a.maps, d32), ("float64_D4", d64)):
            plan.apply(host[:min(len(host), 2 * M.PLAN_TILE)])  # warm both ways at this dtype
            baseline(min_, mnew, host[:min(len(host), BASELINE_CHUNK)])
            tp, tb = [], []
            for _ in range(a.repeats):  # alternated: other people's work shares the host
                t0 = time.perf_counter()
                got = plan.apply(host)
                tp.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                want = baseline(min_, mnew, host)
                tb.append((time.perf_counter() - t0) * 1e3)
            if not np.array_equal(got, want.astype(host.dtype)):  # faster and different is not faster
                raise SystemExit("time_resample_plan.py: %s %s: the plan's result differs from the baseline's in %d values" % (name, case, int((got != want.astype(host.dtype)).sum())))
            dev_ms, dev_out = dev_apply_ms(ctx, plan, host, a.repeats)
            if not np.array_equal(dev_out, got):
                raise SystemExit("time_resample_plan.py: %s %s: apply_dev differs from apply" % (name, case))
            nbytes = apply_bytes(V_in, V_out, nnz, host.shape[0], host.dtype.itemsize)
            dev = stats(dev_ms)
            entry["cases"][case] = dict(maps=int(host.shape[0]), host_megabytes_in_and_out=round((host.nbytes + got.nbytes) / 1e6, 1), plan_apply_ms=stats(tp),
                                        baseline_ms=stats(tb), apart=bool(max(tp) < min(tb)), speedup_of_medians=float(np.median(tb) / np.median(tp)),
                                        equal_bits=True, apply_dev_ms=dev, algorithmic_megabytes=round(nbytes / 1e6, 1),
                                        apply_dev_share_of_hbm_peak=float(nbytes / (dev["median_ms"] * 1e-3) / HBM_PEAK), bound="HBM bandwidth")
        line["shapes"][name] = entry
        plan.close()
    if a.kernel_stats and not a.once:
        line["kernels_of_once_run"] = kernel_rows(a.kernel_stats)
        # the --once run: one warm-up and one timed apply_dev per shape and dtype, i.e. every apply's tiles twice
        total_s = sum(r["total_ms"] for r in line["kernels_of_once_run"].values()) * 1e-3
        nbytes = 2 * sum(apply_bytes(e["V_in"], e["V_out"], e["nnz"], D, es) for e in line["shapes"].values() for D, es in ((a.maps, 4), (4, 8)))
        line["kernels_share_of_hbm_peak"] = float(nbytes / total_s / HBM_PEAK) if total_s > 0 else None
    text = json.dumps(line)
    print(text)
    if a.out and not a.once:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
