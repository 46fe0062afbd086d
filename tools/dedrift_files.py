"""Dedrifts a finished groupwise run, from files to files, on the MI355X path -- what the reference's tutorial pipeline does with wb_command and nibabel
once gMSM has written its spheres (gMSM_scripts/gMSM_tutorial/gw_MSM.sh:65-128, compare_stats.py):

    python tools/dedrift_files.py --meshes=LIST --data=LIST --template=T --regs=PREFIX. --out=PREFIX. [-f GIFTI|ASCII|ASCII_MAT] [--percentile=75] [--before]

--meshes / --data / --template are the inputs of the groupwise run (the same list files, prepared the same way: every sphere recentred and rescaled to
radius 100), --regs the output basename of that run: <regs>sphere-<i>.reg<surf> are read.  Written under --out:
    <out>dedriftwarp<surf>                             the dedrift warp W on the template's triangles (gw_MSM.sh:82-92)
    <out>sphere-<i>.reg.corrected<surf>                every registered sphere pushed through W (:94-101)
    <out>transformed_and_reprojected.dedrift-<i><data> the subject's data resampled from its corrected sphere onto the template (:103-112)
    <out>sphere-<i>.distortion<data>                   two rows: areal (log2 J) and shape (log2 R) distortion of the corrected sphere against the input sphere (:122)
    <out>mean<data>, <out>stdev<data>                  over the subjects (:125-130)
    <out>group_stats.txt                               mean pairwise correlation and Dice overlap per data row, and the distortion summary, in
                                                       compare_stats.py's wording
--before also prints (and writes into group_stats.txt, first) the pairwise figures of the run's own <regs>transformed_and_reprojected-<i><data> files, so
that both are seen side by side.

The inverse of a registration is taken onto the subject's own input sphere (newmsm_amd/dedrift.py); the tutorial script passes the template there, which is
the same thing exactly when every input sphere is the template.  Agreement with wb_command's arithmetic is unpinned.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import dedrift, meshio  # noqa: E402

RAD = 100.0
SURF_EXTS = (".surf.gii", ".asc")
DATA_EXTS = (".func.gii", ".dpv", ".txt")


def on_sphere(xyz, rad=RAD):
    """recentre + true_rescale (R/mesh.cpp:1198-1255), as the groupwise run prepared its inputs (tools/register_files.py)"""
    xyz = xyz - xyz.mean(axis=0)
    return xyz * (rad / np.linalg.norm(xyz, axis=1, keepdims=True))


def output_formats(fmt):
    """Mesh_registration::set_output_format, M/mesh_registration.cpp:827-842"""
    if fmt == "GIFTI":
        return ".surf.gii", ".func.gii"
    if fmt in ("ASCII", "ASCII_MAT"):
        return ".asc", (".dpv" if fmt == "ASCII" else ".txt")
    raise SystemExit("dedrift_files.py: -f must be GIFTI, ASCII or ASCII_MAT")


def save_data(path, mesh_xyz, data):
    """the values as floats in every format; the text formats with the nine digits that give a float back exactly (.dpv: the first row only, as
    Mesh::save_dpv writes it)"""
    if path.endswith(".dpv"):
        meshio.save_dpv(path, mesh_xyz, data, digits=9)
    elif path.endswith(".txt"):
        meshio.save_matrix(path, data, digits=9)
    else:
        meshio.save_metric(path, data)


def existing(stem, exts):
    for e in exts:
        if os.path.exists(stem + e):
            return stem + e
    raise SystemExit("dedrift_files.py: none of %s exists" % ", ".join(stem + e for e in exts))


def read_ascii_list(path):
    with open(path) as f:
        return f.read().split()


def row_names(D):
    return ["Sulc", "Curv"][:D] if D <= 2 else ["Row %d" % (d + 1) for d in range(D)]


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="dedrift_files.py", description="dedrifting and group statistics of a finished groupwise run on the MI355X path")
    ap.add_argument("-m", "--meshes", required=True, help="list of paths to the run's input meshes")
    ap.add_argument("--data", required=True, help="list of paths of the run's data files")
    ap.add_argument("--template", required=True, help="the run's template sphere")
    ap.add_argument("--regs", required=True, help="output basename of the groupwise run (its sphere-<i>.reg files are read)")
    ap.add_argument("-o", "--out", required=True, help="output basename")
    ap.add_argument("-f", "--format", default="GIFTI", help="format of output files: GIFTI, ASCII or ASCII_MAT")
    ap.add_argument("--percentile", type=float, default=75.0, help="threshold of the Dice overlap (compare_stats.py: 75)")
    ap.add_argument("--before", action="store_true", help="also report the pairwise figures of the run's un-dedrifted transformed_and_reprojected-<i> files")
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def main(argv):
    a = parse_args(argv)
    surf_ext, data_ext = output_formats(a.format)
    mesh_files, data_files = read_ascii_list(a.meshes), read_ascii_list(a.data)
    if len(mesh_files) != len(data_files):
        raise SystemExit("dedrift_files.py: %d meshes, %d data files" % (len(mesh_files), len(data_files)))
    S = len(mesh_files)
    txyz, ttri = meshio.load_surface(a.template)
    txyz = on_sphere(txyz)
    subjects, datas = [], []
    for s in range(S):
        xyz, tri = meshio.load_surface(mesh_files[s])
        reg_path = existing(a.regs + "sphere-%d.reg" % s, SURF_EXTS)
        reg, rtri = meshio.load_surface(reg_path)
        if len(reg) != len(xyz) or not np.array_equal(rtri, tri):
            raise SystemExit("dedrift_files.py: %s is not a registration of %s (different mesh)" % (reg_path, mesh_files[s]))
        if a.verbose:
            print("Mesh #%d is %s, registered as %s" % (s, mesh_files[s], reg_path))
        subjects.append((on_sphere(xyz), reg, tri))
        datas.append(meshio.load_data(data_files[s], len(xyz)))
    ctx = M.Context(a.device)
    blocks = []
    if a.before:
        maps = [meshio.load_data(existing(a.regs + "transformed_and_reprojected-%d" % s, DATA_EXTS), len(txyz)) for s in range(S)]
        b = dedrift.pairwise_stats(ctx, (txyz, ttri), maps, a.percentile)
        blocks.append(dedrift.format_stats("before dedrifting", row_names(maps[0].shape[0]), b["cc_mean"], b["dice_mean"]))
    r = dedrift.dedrift_group(ctx, (txyz, ttri), subjects, datas, percentile=a.percentile)
    meshio.save_surface(a.out + "dedriftwarp" + surf_ext, r["W"], ttri)
    for s in range(S):
        meshio.save_surface(a.out + "sphere-%d.reg.corrected" % s + surf_ext, r["corrected"][s], subjects[s][2])
        save_data(a.out + "transformed_and_reprojected.dedrift-%d" % s + data_ext, txyz, r["resampled"][s])
        save_data(a.out + "sphere-%d.distortion" % s + data_ext, subjects[s][0], r["distortion"][s])
    save_data(a.out + "mean" + data_ext, txyz, r["mean"])
    save_data(a.out + "stdev" + data_ext, txyz, r["stdev"])
    blocks.append(dedrift.format_stats("after dedrifting", row_names(r["mean"].shape[0]), r["cc_mean"], r["dice_mean"], r["summary"]))
    text = "\n".join(blocks)
    with open(a.out + "group_stats.txt", "w") as f:
        f.write(text)
    print(text, end="")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
