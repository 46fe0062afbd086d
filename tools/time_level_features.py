"""Times msm_level_features (a level's featurespace::initialise for all data sets in one call) warm, beside the composition of the
existing entry points -- msm_create_exclusion, msm_metric_resample, msm_smooth_data, msm_histogram_match, msm_variance_normalise, call after call as
registration.level_features / finish_features make them -- of another build of the library.

    python tools/time_level_features.py [--baseline-lib PARENT/libmsmhip.so] [--runs 10] [--warmup 3] [--shapes pairwise,group] [--subjects 64]
                                        [--out profiles/level_features_time.json]

--baseline-lib: the parent commit's build; without it this build's own entry points, whose routes are the same.  Both libraries are loaded into this one
process, each with a context and mesh handles of its own, and the two sides take turns call by call: `warmup` unrecorded rounds, then `runs` recorded ones;
median and min - max of the host clock around each call (both end in a synchronisation of their stream).  A time is printed only when the two results are
equal byte for byte.  Shapes, each with and without a zero-valued cap of a tenth of the sphere (the cut range of --excl): pairwise ico6 natives onto ico6
with D = 1 and D = 32 (sigma 2, --VN); groupwise S subjects with D = 2 on irregular ico6 natives onto ico6 and onto ico4 (sigma 2), with --VN and with
--IN --VN.  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import _lib, synthetic  # noqa: E402

c_dp, c_ip = _lib.c_dp, _lib.c_ip
CUTTHR = (0.0, 0.0001)
CAP_Z = 80.0
NEEDED = ["msm_last_error", "msm_ctx_create", "msm_ctx_destroy", "msm_mesh_create", "msm_mesh_destroy", "msm_create_exclusion", "msm_metric_resample", "msm_smooth_data",
          "msm_histogram_match", "msm_variance_normalise"]


def load(path):
    L = C.CDLL(path)
    for name in NEEDED:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return L


def dp(a):
    return a.ctypes.data_as(c_dp)


class Side:
    """one library with a context and the mesh handles of a shape"""

    def __init__(self, L):
        self.L = L
        self.ctx = L.msm_ctx_create(0)
        if not self.ctx:
            raise SystemExit("time_level_features.py: no context: %s" % L.msm_last_error().decode())
        self.meshes = []

    def ok(self, status):
        if status != 0:
            raise SystemExit("time_level_features.py: %s" % self.L.msm_last_error().decode())

    def mesh(self, xyz, tri):
        x = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).T)
        t = np.ascontiguousarray(np.asarray(tri, dtype=np.int32).T)
        h = self.L.msm_mesh_create(self.ctx, dp(x), x.shape[1], t.ctypes.data_as(c_ip), t.shape[1])
        if not h:
            raise SystemExit("time_level_features.py: %s" % self.L.msm_last_error().decode())
        self.meshes.append(h)
        return h

    def drop_meshes(self):
        for h in self.meshes:
            self.L.msm_mesh_destroy(h)
        self.meshes = []

    def close(self):
        self.drop_meshes()
        self.L.msm_ctx_destroy(self.ctx)


def composition(side, grid, Vg, handles, sizes, datas, D, sigmas, exclude, intensity, varnorm):
    """the chain of entry points, as registration.level_features + finish_features call them (fresh result arrays per call, as there)"""
    L = side.L
    n = len(handles)
    feat, mask = np.zeros((n, D, Vg)), (np.zeros((n, Vg)) if exclude else None)
    for i in range(n):
        f = np.zeros((D, Vg))
        if exclude:
            e = np.zeros(sizes[i])
            side.ok(L.msm_create_exclusion(dp(datas[i]), D, sizes[i], CUTTHR[0], CUTTHR[1], dp(e)))
            eo = np.zeros(Vg)
            side.ok(L.msm_metric_resample(handles[i], dp(datas[i]), D, grid, dp(e), dp(f), dp(eo)))
            if sigmas[i] > 0:
                f2, eo2 = np.zeros((D, Vg)), np.zeros(Vg)
                side.ok(L.msm_smooth_data(grid, dp(f), D, grid, float(sigmas[i]), dp(eo), dp(f2), dp(eo2)))
                f, eo = f2, eo2
            mask[i] = eo
        else:
            side.ok(L.msm_metric_resample(handles[i], dp(datas[i]), D, grid, None, dp(f), None))
            if sigmas[i] > 0:
                f2 = np.zeros((D, Vg))
                side.ok(L.msm_smooth_data(grid, dp(f), D, grid, float(sigmas[i]), None, dp(f2), None))
                f = f2
        feat[i] = f
    if intensity and n > 1:
        src = np.ascontiguousarray(feat[1:])
        out = np.empty_like(src)
        se = np.ascontiguousarray(mask[1:]) if exclude else None
        side.ok(L.msm_histogram_match(side.ctx, n - 1, D, Vg, dp(src), dp(se) if exclude else None, 1 if exclude else 0, Vg, dp(feat[0]),
                                      dp(mask[0]) if exclude else None, 1 if exclude else 0, dp(out)))
        feat[1:] = out
    if varnorm:
        for i in range(n):
            row = np.array(feat[i])
            side.ok(L.msm_variance_normalise(dp(row), D, Vg, dp(mask[i]) if exclude else None))
            feat[i] = row
    return feat, mask


def one_call(L, side, grid, Vg, handles, datas, D, sigmas, exclude, intensity, varnorm):
    n = len(handles)
    hs = (C.c_void_p * n)(*handles)
    rows = (c_dp * n)(*[dp(d) for d in datas])
    sg = np.asarray(sigmas, dtype=np.float64)
    p = _lib.LevelFeaturesParams(int(exclude), int(intensity), int(varnorm), 0, CUTTHR[0], CUTTHR[1])
    feat, mask = np.zeros((n, D, Vg)), (np.zeros((n, Vg)) if exclude else None)
    side.ok(L.msm_level_features(grid, n, hs, rows, D, dp(sg), C.byref(p), dp(feat), dp(mask) if exclude else None))
    return feat, mask


def stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), max_ms=round(float(np.max(ms)), 3))


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def natives(n, order, D, cap, seed):
    xyz0, tri = M.make_mesh_from_icosa(order)
    out = []
    for i in range(n):
        xyz = synthetic.known_warp(xyz0, seed=seed + i, rot_deg=0.0, amp=0.7)
        data = synthetic.features(synthetic.known_warp(xyz, seed=seed + 500 + i, rot_deg=3.0, amp=2.0), D, seed + i) * (1.0 + 0.1 * i) + 0.05 * i
        if cap:
            data[:, xyz[:, 2] > CAP_Z] = 0.0
        out.append((xyz, tri, np.ascontiguousarray(data)))
    return out


def main(argv):
    ap = argparse.ArgumentParser(prog="time_level_features.py")
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="pairwise,group")
    ap.add_argument("--subjects", type=int, default=64)
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if M.device_count() < 1:
        raise SystemExit("time_level_features.py: no GPU visible; nothing is measured without one")
    if a.runs < 10 or a.warmup < 3:
        raise SystemExit("time_level_features.py: at least 10 recorded calls after 3 warm-ups")
    here = M.lib()
    new, base = Side(here), Side(load(a.baseline_lib) if a.baseline_lib else here)
    shapes = []
    if "pairwise" in a.shapes:
        shapes += [("pairwise_D1", 2, 1, a.order, False, True), ("pairwise_D32", 2, 32, a.order, False, True)]
    if "group" in a.shapes:
        for g in (a.order, a.order - 2):
            shapes += [("group_S%d_D2_ico%d_VN" % (a.subjects, g), a.subjects, 2, g, False, True), ("group_S%d_D2_ico%d_IN_VN" % (a.subjects, g), a.subjects, 2, g, True, True)]
    line = dict(tool="time_level_features", baseline=("another build: " + os.path.basename(os.path.dirname(os.path.abspath(a.baseline_lib)))) if a.baseline_lib else "this build",
                native_order=a.order, runs=a.runs, warmup=a.warmup, sigma=2.0, shapes={})
    cache = {}
    for name, n, D, gorder, intensity, varnorm in shapes:
        gxyz, gtri = M.make_mesh_from_icosa(gorder)
        for cap in (False, True):
            key = (n, D, cap)
            if key not in cache:
                cache.clear()
                cache[key] = natives(n, a.order, D, cap, 100)
            nats = cache[key]
            datas, sizes, sigmas = [d for _, _, d in nats], [len(x) for x, _, _ in nats], [2.0] * n
            sides = []
            for side in (new, base):
                side.drop_meshes()
                sides.append((side, side.mesh(gxyz, gtri), [side.mesh(x, t) for x, t, _ in nats]))
            (sn, gn, hn), (sb, gb, hb) = sides
            t_new, t_base = [], []
            for k in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                got = one_call(here, sn, gn, len(gxyz), hn, datas, D, sigmas, cap, intensity, varnorm)
                t1 = time.perf_counter()
                want = composition(sb, gb, len(gxyz), hb, sizes, datas, D, sigmas, cap, intensity, varnorm)
                t2 = time.perf_counter()
                if k >= a.warmup:
                    t_new.append((t1 - t0) * 1e3)
                    t_base.append((t2 - t1) * 1e3)
            if not (same(got[0], want[0]) and same(got[1], want[1])):  # faster and different is not faster
                raise SystemExit("time_level_features.py: %s (cap %s): the one call and the composition differ" % (name, cap))
            one, comp = stats(t_new), stats(t_base)
            spread = comp["max_ms"] - comp["min_ms"]
            line["shapes"][name + ("_cap" if cap else "")] = dict(
                data_sets=n, rows=D, grid_order=gorder, masks=cap, intensity=intensity, varnorm=varnorm, one_call=one, composition=comp, equal_bytes=True,
                ranges_apart=bool(one["max_ms"] < comp["min_ms"] or comp["max_ms"] < one["min_ms"]),
                one_call_within_bar=bool(one["median_ms"] <= comp["median_ms"] + spread))
            print("%s%s: one call %.2f ms (%.2f - %.2f), composition %.2f ms (%.2f - %.2f)" % (name, "_cap" if cap else "", one["median_ms"], one["min_ms"], one["max_ms"],
                                                                                            comp["median_ms"], comp["min_ms"], comp["max_ms"]), file=sys.stderr, flush=True)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    new.close()
    if base is not new:
        base.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
