"""A cohort registered to one template, from files to files, in one process on the MI355X path -- what the reference's *_to_template pipelines do with one
newmsm process per subject, wb_command and nibabel (gMSM_scripts/newMSM_HCP_to_template_v2.sh, run_HCP_to_template_v2.sh, gMSM_tutorial/typical_MSM.sh,
get_group_stats.sh / .py, and the second line of every block compare_stats.py prints):

    python tools/cohort_files.py --meshes=LIST --data=LIST --refmesh=R --refdata=RD --conf=CONF --out=PREFIX. [--trans=LIST] [-f GIFTI|ASCII|ASCII_MAT]
                                 [--percentile=75] [--workers=N]

--meshes / --data / --trans: text files with one path per line (read_ascii_list); subject i is line i of each.  A --meshes list of ONE line serves every
subject (the scripts' common sunet.ico-6.sphere).  Inputs are prepared as tools/register_files.py prepares them (every sphere recentred and rescaled to
radius 100, --trans taken as it is), the configuration goes through the same grammar, and MSMHIP_RIGID / MSMHIP_HISTMATCH mean what they mean there.

Written per subject i, under the names the groupwise mode and tools/dedrift_files.py use:
    <out>sphere-<i>.reg<surf>                     the input sphere moved through the final warp
    <out>sphere-<i>.LR.reg<surf>                  the last level's data grid at its registered position
    <out>transformed_and_reprojected-<i><data>    the subject's data resampled from its registered sphere onto the reference
    <out>sphere-<i>.distortion<data>              two rows: areal (log2 J) and shape (log2 R) distortion of sphere-<i>.reg as written against the input sphere
the first three byte for byte what tools/register_files.py writes for that subject alone; and for the cohort:
    <out>mean<data>, <out>stdev<data>             over the subjects' transformed_and_reprojected files as written
    <out>group_stats.txt                          mean pairwise correlation and Dice overlap per data row of those files, and the distortion summary (mean, max,
                                                  95 %, 98 % of areal; mean and max of shape), in compare_stats.py's wording
The distortion maps come from msm_surface_distortion: subjects that share the input mesh file go in one batched call, the others in a call each.  The
summary comes from msm_abs_summary.  Agreement with wb_command's own arithmetic is unpinned.

Out of scope, and refused when asked for: cost-function weightings and aMSM surfaces per subject (--inweight / --refweight / --inanat / --refanat), a
weight mask for the statistics (--mask), per-group statistics from a clustering file (--clusters).  There is no C++ executable twin of this tool; a
target mesh or its direction table is not shared between the workers' contexts; the cost kernels are not batched across subjects.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import cohort, config, dedrift, meshio  # noqa: E402
import dedrift_files  # noqa: E402
import register_files  # noqa: E402

DEFAULT_WORKERS = 2  # the setting that measured fastest (tools/time_cohort.py)
OUT_OF_SCOPE = {
    "inweight": "cost-function weightings per subject are out of scope",
    "refweight": "cost-function weightings per subject are out of scope",
    "inanat": "aMSM surfaces per subject are out of scope",
    "refanat": "aMSM surfaces per subject are out of scope",
    "mask": "a weight mask for the statistics is out of scope",
    "clusters": "per-group statistics from a clustering file are out of scope",
}


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="cohort_files.py", description="a cohort registered to one template in a single run on the MI355X path, with its statistics. "
                                 "Out of scope: cost-function weightings and aMSM surfaces per subject, a weight mask for the statistics, per-group statistics from "
                                 "a clustering file, a C++ executable twin of this tool, sharing a target mesh or its direction table between contexts, any "
                                 "batching of the cost kernels across subjects.")
    ap.add_argument("-m", "--meshes", required=True, help="list of paths to the subjects' input spheres; one line serves every subject")
    ap.add_argument("--data", required=True, help="list of paths of the subjects' data files")
    ap.add_argument("-R", "--refmesh", required=True, help="reference (template) sphere")
    ap.add_argument("-I", "--refdata", required=True, help="reference (template) data")
    ap.add_argument("-t", "--trans", default="", help="list of paths of the subjects' sphere.reg files of an earlier run: every first level starts from its subject's")
    ap.add_argument("-c", "--conf", default="", help="configuration file")
    ap.add_argument("-o", "--out", required=True, help="output basename")
    ap.add_argument("-f", "--format", default="GIFTI", help="format of output files: GIFTI, ASCII or ASCII_MAT")
    ap.add_argument("--percentile", type=float, default=75.0, help="threshold of the Dice overlap (compare_stats.py: 75)")
    ap.add_argument("--workers", type=int, default=DEFAULT_WORKERS, help="subjects registered side by side, each on a context of its own (default %d)" % DEFAULT_WORKERS)
    for flag, why in OUT_OF_SCOPE.items():
        ap.add_argument("--" + flag, default="", help="refused: " + why)
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def subject_lists(mesh_files, data_files, trans_files=None):
    """per subject (mesh path, data path, trans path or None).  One mesh line serves every subject; any other difference in the counts is an error that
    names both."""
    S = len(data_files)
    if S == 0:
        raise SystemExit("cohort_files.py: --data lists no subject")
    if len(mesh_files) == 1:
        mesh_files = list(mesh_files) * S
    if len(mesh_files) != S:
        raise SystemExit("cohort_files.py: %d meshes, %d data files (one mesh for all subjects, or one per subject)" % (len(mesh_files), S))
    if trans_files is not None and len(trans_files) != S:
        raise SystemExit("cohort_files.py: %d transformed meshes (--trans), %d data files" % (len(trans_files), S))
    return [(mesh_files[s], data_files[s], trans_files[s] if trans_files is not None else None) for s in range(S)]


def cohort_levels(cfg, D):
    levels, run_kw, skipped = config.levels_from_config(cfg, D, rigid=register_files.rigid_enabled(),
                                                        **(dict(histmatch=True) if register_files.histmatch_enabled() else {}))
    for index, method in skipped:
        print("cohort_files.py: level %d (--opt=%s) is outside the path (the affine stage stays on the CPU in newmsm): skipped" % (index + 1, method), file=sys.stderr)
    if not levels:
        raise SystemExit("cohort_files.py: the configuration holds no DISCRETE level")
    return levels, run_kw


def distortion_maps(ctx, entries, origs, finals):
    """per subject its 2 x V distortion map: the subjects that share an input mesh file in ONE msm_surface_distortion call, the others in a call each"""
    groups = {}
    for s, (mesh_path, _, _) in enumerate(entries):
        groups.setdefault(mesh_path, []).append(s)
    out = [None] * len(entries)
    for members in groups.values():
        xyz, tri = origs[members[0]]
        maps = M.surface_distortion(ctx, xyz, tri, np.stack([finals[s] for s in members]))
        for k, s in enumerate(members):
            out[s] = maps[k]
    return out


def distortion_summary(ctx, distortions):
    """dedrift.distortion_summary's figures through msm_abs_summary"""
    areal = np.concatenate([d[0].ravel() for d in distortions])
    shape = np.concatenate([d[1].ravel() for d in distortions])
    a_mean, a_max, a_p = M.abs_summary(ctx, areal, (95.0, 98.0))
    s_mean, s_max, _ = M.abs_summary(ctx, shape)
    return dict(areal_mean=a_mean, areal_max=a_max, areal_95=float(a_p[0]), areal_98=float(a_p[1]), shape_mean=s_mean, shape_max=s_max)


def main(argv):
    a = parse_args(argv)
    for flag, why in OUT_OF_SCOPE.items():
        if getattr(a, flag):
            raise SystemExit("cohort_files.py: --%s: %s" % (flag, why))
    surf_ext, data_ext = dedrift_files.output_formats(a.format)
    if a.workers < 1:
        raise SystemExit("cohort_files.py: --workers must be at least 1")
    entries = subject_lists(register_files.read_ascii_list(a.meshes), register_files.read_ascii_list(a.data),
                            register_files.read_ascii_list(a.trans) if a.trans else None)
    S = len(entries)
    rxyz, rtri = meshio.load_surface(a.refmesh)
    rxyz = register_files.on_sphere(rxyz)
    rdata = meshio.load_data(a.refdata, len(rxyz))
    loaded, subjects, origs = {}, [], []
    for s, (mesh_path, data_path, trans_path) in enumerate(entries):
        if mesh_path not in loaded:
            xyz, tri = meshio.load_surface(mesh_path)
            loaded[mesh_path] = (register_files.on_sphere(xyz), tri)
        xyz, tri = loaded[mesh_path]
        if a.verbose:
            print("Mesh #%d is %s, data %s" % (s, mesh_path, data_path))
        data = meshio.load_data(data_path, len(xyz))
        if data.shape[0] != rdata.shape[0]:
            raise SystemExit("Mesh_registration: input and reference data have different numbers of feature rows (%d, %d)" % (data.shape[0], rdata.shape[0]))
        subject = dict(xyz=xyz, tri=tri, data=data)
        if trans_path:  # set_transformed: as loaded
            subject["trans"] = meshio.load_surface(trans_path)[0]
        subjects.append(subject)
        origs.append((xyz, tri))
    cfg = config.parse_config(register_files.read_conf(a.conf))
    levels, run_kw = cohort_levels(cfg, rdata.shape[0])
    if a.verbose:
        print("This is newMSM's DISCRETE path on an MI355X (msm-mi355x): %d subjects to one template, %d at a time.\nStarting multiresolution with %d levels."
              % (S, min(a.workers, S), len(levels)))
    results = cohort.run_cohort(cohort.product_ops(a.device), subjects, rxyz, rtri, rdata, levels, workers=a.workers, **run_kw, **config.run_options(cfg))
    last_tri = M.make_mesh_from_icosa(levels[-1]["data_order"])[1]
    finals, maps = [], []
    for s, r in enumerate(results):
        reg_path = a.out + "sphere-%d.reg" % s + surf_ext
        map_path = a.out + "transformed_and_reprojected-%d" % s + data_ext
        meshio.save_surface(reg_path, r["sphere_reg"], subjects[s]["tri"])                                  # transform
        meshio.save_surface(a.out + "sphere-%d.LR.reg" % s + surf_ext, r["level_regs"][-1], last_tri)       # saveSPH_reg
        register_files.save_data(map_path, rxyz, r["transformed"])                                          # save_transformed_data
        finals.append(meshio.load_surface(reg_path)[0])  # what a later tool reads: the sphere as written
        maps.append(meshio.load_data(map_path, len(rxyz)))
    ctx = M.Context(a.device)
    distortions = distortion_maps(ctx, entries, origs, finals)
    for s in range(S):
        dedrift_files.save_data(a.out + "sphere-%d.distortion" % s + data_ext, origs[s][0], distortions[s])
    stats = dedrift.pairwise_stats(ctx, (rxyz, rtri), maps, a.percentile)
    dedrift_files.save_data(a.out + "mean" + data_ext, rxyz, stats["mean"])
    dedrift_files.save_data(a.out + "stdev" + data_ext, rxyz, stats["stdev"])
    text = dedrift.format_stats("typical MSM", dedrift_files.row_names(maps[0].shape[0]), stats["cc_mean"], stats["dice_mean"], distortion_summary(ctx, distortions))
    with open(a.out + "group_stats.txt", "w") as f:
        f.write(text)
    print(text, end="")
    ctx.close()
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main(sys.argv[1:]))
    except (config.ConfigError, ValueError) as e:  # MeshregException: the message, exit status 1 (CLI/newmsm.cpp:62-65)
        raise SystemExit(str(e))
    except (cohort.CohortError, M.MsmError) as e:  # a subject failed, or the library reported an error: the message, a non-zero exit status
        raise SystemExit("cohort_files.py: %s" % e)
