"""The reference's five resampler programs (libraries/msm-newresampler/demo) behind one entry point, from files to files, on the MI355X path:

    python tools/resample_files.py metric-resample  --metric_in=F --current_sphere=S --ico=N --output=BASE   -> BASE-resampled_data.func.gii
    python tools/resample_files.py NN-resample      --metric_in=F --current_sphere=S --ico=N --output=BASE   -> BASE-resampled_data.func.gii, BASE-sphere.surf.gii
    python tools/resample_files.py surface-resample --surface_in=A --current_sphere=S --ico=N --output=BASE  -> BASE-anat.surf.gii, BASE-sphere.surf.gii
    python tools/resample_files.py smoothing        --metric_in=F --current_sphere=S --sigma=X --output=BASE -> BASE-smoothed_data.func.gii
    python tools/resample_files.py applywarp        --to_be_deformed=S --warp=W --output=BASE                -> BASEwarped.surf.gii

under the programs' own option names, output names (the suffix rule is Mesh::save_gifti's, R/mesh.cpp:582-631), sentences for a missing option
("metric_in was not set, but required.", exit status 1) and --ico ranges (metric-resample 2..6, NN-resample 3..6).  Spheres are rescaled to radius
100 with true_rescale, as the programs do.

ADDITIONS to the programs (the three resampling subcommands):
    --new_sphere=FILE     in place of --ico: any target sphere, e.g. the reference mesh of a registration
    --metric_in=FILE      may be given several times: all files go through ONE plan (weights built once), and each output gets -<stem of its input>
                          before -resampled_data
    --label_in=FILE       a .label.gii through the same plan by the largest-summed-weight vote -> BASE-resampled_data.label.gii, label table kept
    --method=adap_bary|barycentric|nearest   the plan's rows (default: the program's own)
    --excl_thr=lo,hi      create_exclusion (R/mesh.cpp:1257-1273) on the first input masks the resampling, as save_transformed_data does
                          (M/mesh_registration.cpp:371-383)
and to `smoothing`: --metric_in may be repeated as well -- all files go through ONE smoothing plan (the neighbourhood sweep runs once; each output gets
-<stem of its input> before -smoothed_data) -- and --excl_thr masks the smoothing by the first input (smooth_data's EXCL argument).  The files' float32
values are smoothed with FP64 sums and rounded once, which is what one input without a mask has always given.

After a registration, everything else the subject has follows its sphere.reg in one call:
    python tools/resample_files.py metric-resample --current_sphere=PREFIX.sphere.reg.surf.gii --new_sphere=ref.sphere.surf.gii \\
        --metric_in=myelin.func.gii --metric_in=rest.func.gii --label_in=parc.label.gii --output=OUT
"""
import argparse
import os
import sys

import numpy as np

RAD = 100.0
PROGRAMS = {
    # name: (required options in the program's order of complaint, --ico range or None, the program's rows)
    "metric-resample": (("metric_in", "current_sphere", "ico", "output"), (2, 6), "adap_bary"),
    "NN-resample": (("metric_in", "current_sphere", "ico", "output"), (3, 6), "nearest"),
    "surface-resample": (("surface_in", "current_sphere", "ico", "output"), None, "barycentric"),
    "smoothing": (("metric_in", "current_sphere", "sigma", "output"), None, None),
    "applywarp": (("to_be_deformed", "warp", "output"), None, None),
}
METHODS = ("adap_bary", "barycentric", "nearest")


class Refused(Exception):
    """what a program prints before it returns 1"""


def parser(program):
    required, _, rows = PROGRAMS[program]
    ap = argparse.ArgumentParser(prog="resample_files.py " + program, allow_abbrev=False, description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name in required:
        if name == "metric_in":
            ap.add_argument("--metric_in", action="append", help="metric file to resample (addition: may be repeated)")
        elif name == "ico":
            ap.add_argument("--ico", type=int, help="the order of the generated regular icosahedron to resample to")
        elif name == "sigma":
            ap.add_argument("--sigma", type=float, help="sigma parameter of smoothing (e.g. 0.5)")
        else:
            ap.add_argument("--" + name)
    if program == "smoothing":
        ap.add_argument("--excl_thr", help="addition: lo,hi -- create_exclusion on the first input masks the smoothing")
    if rows:
        ap.add_argument("--new_sphere", help="addition: a target sphere file in place of --ico")
        ap.add_argument("--method", choices=METHODS, default=rows, help="addition: the rows of the plan")
        ap.add_argument("--excl_thr", help="addition: lo,hi -- create_exclusion on the first input masks the resampling")
    if rows and "metric_in" in required:
        ap.add_argument("--label_in", help="addition: a .label.gii resampled through the same plan")
    return ap


def parse(argv):
    """-> (program, options); raises Refused with the program's own sentence.  Touches no file and no device."""
    if not argv or argv[0] in ("-h", "--help"):
        raise Refused(__doc__)
    program = argv[0]
    if program not in PROGRAMS:
        raise Refused("unknown program %r (one of %s)" % (program, ", ".join(PROGRAMS)))
    required, ico_range, rows = PROGRAMS[program]
    ap = parser(program)

    def refuse(message):
        raise Refused(message)

    ap.error = refuse
    opt = ap.parse_args(argv[1:])
    for name in required:
        if getattr(opt, name) is not None:
            if name == "ico":
                if getattr(opt, "new_sphere", None) is not None:
                    raise Refused("ico and new_sphere were both set: the target is one or the other.")
                if ico_range and not ico_range[0] <= opt.ico <= ico_range[1]:
                    raise Refused("Invalid ico dimension")
            continue
        if name == "ico" and getattr(opt, "new_sphere", None) is not None:
            continue
        if name == "metric_in" and getattr(opt, "label_in", None) is not None:
            continue
        raise Refused("%s was not set, but required." % name)
    if getattr(opt, "excl_thr", None) is not None:
        try:
            lo, hi = (float(x) for x in opt.excl_thr.split(","))
        except ValueError:
            raise Refused("excl_thr takes two numbers: lo,hi")
        opt.excl_thr = (lo, hi)
    return program, opt


def gifti_name(name):
    """Mesh::save_gifti's file name, R/mesh.cpp:582-594"""
    return name if name.endswith("gii") or name.endswith(".gz") else name + ".gii"


def true_rescale(xyz, rad=RAD):
    """R/mesh.cpp:1210-1219 with Point::normalize (R/point.cpp:26-34): the same operations in the same order"""
    x, y, z = (np.ascontiguousarray(xyz[:, k], dtype=np.float64) for k in range(3))
    n = np.sqrt(x * x + y * y + z * z)
    n = np.where(n > 1.0e-8, n, 1.0)
    return np.stack([x / n * rad, y / n * rad, z / n * rad], axis=1)


def stem(path):
    base = os.path.basename(path)
    for ext in (".func.gii", ".shape.gii", ".label.gii", ".gii", ".asc", ".dpv", ".txt"):
        if base.endswith(ext):
            return base[:-len(ext)]
    return base


def run(program, opt):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import newmsm_amd as M
    from newmsm_amd import meshio

    written = []
    ctx = M.Context(0)
    if program == "applywarp":
        xyz, tri = meshio.load_surface(opt.to_be_deformed)
        warp, _ = meshio.load_surface(opt.warp)
        xyz, warp = true_rescale(xyz), true_rescale(warp)
        if len(warp) != len(xyz):
            raise Refused("the warp has %d vertices, the mesh to be deformed %d" % (len(warp), len(xyz)))
        moved = M.sphere_project_warp(xyz, M.Mesh(ctx, xyz, tri), warp)  # sphere_project_warp(to_be_deformed, to_be_deformed, warp)
        written.append(gifti_name(opt.output + "warped.surf"))
        meshio.save_surface(written[-1], moved, tri)
        return written
    sxyz, stri = meshio.load_surface(opt.current_sphere)
    sxyz = true_rescale(sxyz)
    source = M.Mesh(ctx, sxyz, stri)
    if program == "smoothing":
        excl = None
        if opt.excl_thr is not None:
            excl = M.create_exclusion(meshio.load_metric(opt.metric_in[0], nvertices=len(sxyz)), opt.excl_thr[0], opt.excl_thr[1])
        plan = M.ResamplePlan.smoothing(source, source, opt.sigma, excl)  # ONE sweep for every input
        for path in opt.metric_in:
            data = meshio.load_metric(path, nvertices=len(sxyz), dtype=np.float32)  # the file's own floats; the sums run in FP64 and are rounded once
            tag = "-" + stem(path) if len(opt.metric_in) > 1 else ""
            written.append(gifti_name(opt.output + tag + "-smoothed_data.func"))
            out = plan.apply(data)
            meshio.save_metric(written[-1], out[0] if excl is not None else out)
        plan.close()
        return written
    if opt.new_sphere is not None:
        txyz, ttri = meshio.load_surface(opt.new_sphere)
        txyz = true_rescale(txyz)
    else:
        txyz, ttri = M.make_mesh_from_icosa(opt.ico, RAD)
    target = M.Mesh(ctx, txyz, ttri)
    metrics = list(getattr(opt, "metric_in", None) or [])
    label_in = getattr(opt, "label_in", None)
    excl = None
    if opt.excl_thr is not None:
        if program == "surface-resample":
            first = meshio.load_surface(opt.surface_in)[0].T
        elif metrics:
            first = meshio.load_metric(metrics[0], nvertices=len(sxyz))
        else:
            first = meshio.load_label(label_in)[0].astype(np.float64)
        excl = M.create_exclusion(first, opt.excl_thr[0], opt.excl_thr[1])
    plan = M.ResamplePlan(source, target, opt.method, excl)  # ONE plan for every input
    take = (lambda r: r[0]) if excl is not None else (lambda r: r)
    if program == "surface-resample":
        anat, _ = meshio.load_surface(opt.surface_in)
        if len(anat) != len(sxyz):
            raise Refused("the surface has %d vertices, its sphere %d" % (len(anat), len(sxyz)))
        moved = take(plan.apply(np.ascontiguousarray(anat.T)))
        written.append(gifti_name(opt.output + "-anat.surf"))
        meshio.save_surface(written[-1], moved.T, ttri)
    for path in metrics:
        data = meshio.load_metric(path, nvertices=len(sxyz), dtype=np.float32)  # the file's own floats; the sums run in FP64 and are rounded once
        tag = "-" + stem(path) if len(metrics) > 1 else ""
        written.append(gifti_name(opt.output + tag + "-resampled_data.func"))
        meshio.save_metric(written[-1], take(plan.apply(data)))
    if label_in is not None:
        keys, table = meshio.load_label(label_in)
        if keys.shape[1] != len(sxyz):
            raise Refused(" mismatch between data and surface dimensions")
        written.append(opt.output + "-resampled_data.label.gii")
        meshio.save_label(written[-1], plan.apply_labels(keys), table)
    if program in ("NN-resample", "surface-resample"):
        written.append(gifti_name(opt.output + "-sphere.surf"))
        meshio.save_surface(written[-1], txyz, ttri)
    plan.close()
    return written


def main(argv=None):
    try:
        program, opt = parse(sys.argv[1:] if argv is None else argv)
        for path in run(program, opt):
            print(path)
    except (Refused, ValueError, RuntimeError) as e:  # the programs print what() of any exception and return 1
        print(e)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
