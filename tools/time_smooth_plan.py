"""Times a smoothing plan (msm_resample_plan_create_smooth) beside the way the same job was done before it, on the GPU only.

    python tools/time_smooth_plan.py [--repeats 3] [--maps 1200] [--baseline-lib PARENT/libmsmhip.so] [--out profiles/smooth_plan_time.json]

Shapes: a warped ico6 sphere (40 962 vertices) smoothed with sigma 2 (rows of 13 to 19 entries) and sigma 4 (55 to 73); --maps float32 maps (a
resting-state run) and 4 float64 maps.  Reported per shape:
    create_ms        msm_resample_plan_create_smooth (the closest-vertex search, two sweeps over the neighbourhoods, the scan), host clock, complete on return
    plan_apply_ms    ResamplePlan.apply with host arrays: slabs through the pinned staging blocks, host clock around a call that ends synchronised
    baseline_ms      the same maps through msm_smooth_data in chunks of 64 rows widened to float64 -- the entry point takes FP64 only, redoes the sweep
                     per call and keeps up to 64 maps in registers -- by a worker process that loads --baseline-lib through MSM_LIB_PATH (the parent
                     commit's build; without the option this build's own msm_smooth_data, whose code is the same).  The worker runs one call when it is
                     told to: the two ways alternate, --repeats times each; `apart` says whether the slowest plan call is still faster than the
                     fastest baseline call
    apply_dev_ms     ResamplePlan.apply_dev on device tensors, by device events on the context's stream
    algorithmic bytes of an apply (tile_bytes of tools/time_resample_plan.py plus the rows' divisors) over apply_dev_ms as a share of the HBM peak
A time is only printed when the results agree: the float64 results bit for bit, the float32 result with the baseline's rounded once (compared by digest:
the worker keeps its arrays).  Fails without a device: nothing here is measured on a CPU."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import _lib, synthetic  # noqa: E402
from time_resample_plan import HBM_PEAK, apply_bytes, dev_apply_ms, stats  # noqa: E402

ORDER = 6
SIGMAS = (2.0, 4.0)
BASELINE_CHUNK = 64  # msm_smooth_data keeps up to 64 maps in registers (k_smooth); beyond that it accumulates in global memory


def inputs(maps):
    """the sphere and the two sets of maps: the same in the timing process and in the worker"""
    xyz, tri = M.make_mesh_from_icosa(ORDER)
    xyz = synthetic.known_warp(xyz, seed=21, rot_deg=5.0, amp=1.0)
    rng = np.random.default_rng(77)
    return xyz, tri, {"float32_D%d" % maps: rng.standard_normal((maps, len(xyz)), dtype=np.float32), "float64_D4": rng.standard_normal((4, len(xyz)))}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def baseline(mesh, data, sigma):
    out = np.empty((data.shape[0], mesh.V))
    for d0 in range(0, data.shape[0], BASELINE_CHUNK):
        out[d0:d0 + BASELINE_CHUNK] = M.smooth_data(mesh, data[d0:d0 + BASELINE_CHUNK].astype(np.float64), mesh, sigma)
    return out


def worker(maps):
    """the baseline's process: for every line `sigma case` on stdin one baseline call, answered with `milliseconds digest` (of the result in the case's dtype)"""
    ctx = M.Context(0)
    xyz, tri, cases = inputs(maps)
    mesh = M.Mesh(ctx, xyz, tri)
    print("ready %s" % _lib.LIB_PATH, flush=True)
    for line in sys.stdin:
        sigma, case = line.split()
        host = cases[case]
        t0 = time.perf_counter()
        got = baseline(mesh, host, float(sigma))
        ms = (time.perf_counter() - t0) * 1e3
        print("%r %s" % (ms, digest(got.astype(host.dtype))), flush=True)
    ctx.close()
    return 0


def main(argv):
    ap = argparse.ArgumentParser(prog="time_smooth_plan.py")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--maps", type=int, default=1200)
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import torch  # noqa: F401  before the library is loaded: it then shares torch's HIP runtime (the other way round torch finds no device)

    if a.worker:
        for name in ("msm_resample_plan_create_smooth", "msm_resample_plan_divisors"):
            _lib.SIGNATURES.pop(name, None)  # the parent commit's library does not have them, and the worker calls msm_smooth_data only
    if M.device_count() < 1:
        raise SystemExit("time_smooth_plan.py: no GPU visible; nothing is measured without one")
    if a.worker:
        return worker(a.maps)
    if a.repeats < 3:
        raise SystemExit("time_smooth_plan.py: at least three repeats")
    env = dict(os.environ)
    if a.baseline_lib:
        env["MSM_LIB_PATH"] = os.path.abspath(a.baseline_lib)
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--maps", str(a.maps)], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(sigma, case):
        child.stdin.write("%r %s\n" % (sigma, case))
        child.stdin.flush()
        answer = child.stdout.readline().split()
        if len(answer) != 2:
            raise SystemExit("time_smooth_plan.py: the baseline's process ended (status %s)" % child.poll())
        return float(answer[0]), answer[1]

    try:
        ready = child.stdout.readline().split()
        if len(ready) != 2 or ready[0] != "ready":
            raise SystemExit("time_smooth_plan.py: the baseline's process did not start (status %s)" % child.poll())
        ctx = M.Context(0)
        xyz, tri, cases = inputs(a.maps)
        mesh = M.Mesh(ctx, xyz, tri)
        line = dict(tool="time_smooth_plan", repeats=a.repeats, tile=M.PLAN_TILE, hbm_peak_bytes_per_s=HBM_PEAK, baseline_chunk=BASELINE_CHUNK,
                    baseline_lib="parent build (MSM_LIB_PATH)" if a.baseline_lib else "this build", shapes={})
        for sigma in SIGMAS:
            M.ResamplePlan.smoothing(mesh, mesh, sigma).close()  # warm: tree, scratch
            created = []
            for k in range(a.repeats):
                t0 = time.perf_counter()
                plan = M.ResamplePlan.smoothing(mesh, mesh, sigma)
                created.append((time.perf_counter() - t0) * 1e3)
                if k + 1 < a.repeats:
                    plan.close()
            V_in, V_out, nnz, longest = plan.sizes()
            entry = dict(V_in=V_in, V_out=V_out, nnz=nnz, longest_row=longest, shortest_row=int(np.diff(plan.weights()[0]).min()), create_ms=stats(created), cases={})
            for case, host in cases.items():
                plan.apply(host[:min(len(host), 2 * M.PLAN_TILE)])  # warm both ways at this dtype
                ask(sigma, "float64_D4")
                tp, tb = [], []
                for _ in range(a.repeats):  # alternated: other people's work shares the host
                    t0 = time.perf_counter()
                    got = plan.apply(host)
                    tp.append((time.perf_counter() - t0) * 1e3)
                    ms, want = ask(sigma, case)
                    tb.append(ms)
                if digest(got) != want:  # faster and different is not faster
                    raise SystemExit("time_smooth_plan.py: sigma %g %s: the plan's result differs from the baseline's" % (sigma, case))
                dev_ms, dev_out = dev_apply_ms(ctx, plan, host, a.repeats)
                if not np.array_equal(dev_out, got):
                    raise SystemExit("time_smooth_plan.py: sigma %g %s: apply_dev differs from apply" % (sigma, case))
                tiles = -(-host.shape[0] // M.PLAN_TILE)
                nbytes = apply_bytes(V_in, V_out, nnz, host.shape[0], host.dtype.itemsize) + 8 * V_out * tiles  # the divisors: once per tile
                dev = stats(dev_ms)
                entry["cases"][case] = dict(maps=int(host.shape[0]), host_megabytes_in_and_out=round((host.nbytes + got.nbytes) / 1e6, 1), plan_apply_ms=stats(tp),
                                            baseline_ms=stats(tb), apart=bool(max(tp) < min(tb)), speedup_of_medians=float(np.median(tb) / np.median(tp)),
                                            equal_bits=True, apply_dev_ms=dev, algorithmic_megabytes=round(nbytes / 1e6, 1),
                                            apply_dev_share_of_hbm_peak=float(nbytes / (dev["median_ms"] * 1e-3) / HBM_PEAK), bound="HBM bandwidth")
            line["shapes"]["ico%d_sigma%g" % (ORDER, sigma)] = entry
            plan.close()
        ctx.close()
    finally:
        child.stdin.close()
        try:
            child.wait(timeout=60)
        except subprocess.TimeoutExpired:
            child.kill()
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
