"""Merges registered groups up a hierarchy, from files to files, on the MI355X path -- clustered groupwise registration (cgMSM), which the reference runs
as shell scripts over newmsm, wb_command and nibabel (gMSM_scripts/run_cgMSM_ver_gw_iter.sh:16-218, run_cgMSM_ver_gw.sh, cross_register.sh:51-112,
extract_info.py):

    python tools/hierarchy_files.py --clusters=CLUSTERS.csv --path=PATH.csv --subjects=NAMES --meshes=LIST --data=LIST --template=T --conf=GMSM_CONF
                                    --dir=PREFIX [--mask=MASK] [--percentile=75] [-f GIFTI|ASCII|ASCII_MAT]

--clusters   rows line,subject,group without a header (the reference's frontal_subject_clusters_*.csv): `line` is the subject's index within its group
--path       rows left,right,root (frontal_hierarchical_path_study.csv), processed in file order: the groups left and right are merged into root
--subjects   one name per line, aligned with the lines of --meshes and --data (the subjects' input spheres and native data); a --meshes list of ONE line
             serves every subject.  Inputs are prepared as tools/dedrift_files.py prepares them (every sphere recentred and rescaled to radius 100)
--conf       the configuration of the groupwise registration of the children's mean maps (the grammar of tools/register_files.py --groupwise)
--mask       a map on the template: only its vertices with a value > 0 enter the correlations, the percentile thresholds and the overlaps (the medial wall
             kept out of them).  It is not a cost-function mask of the registration

A leaf group X (a group of --clusters) must have been registered and dedrifted already with the existing tools under --out=<dir><X>.; read are
    <dir><X>.sphere-<line>.reg.corrected<surf>   and   <dir><X>.mean<data>
Per path row the children's mean maps are registered to each other on the template mesh (register_files.py --groupwise's loop with the template as every
mesh), hierarchy.merge_groups runs, and under <dir><root>. the names of a leaf are written, so that a later row reads a root exactly like a leaf:
    child-<g>.reg<surf>                                child g's sphere from the registration of the mean maps (the merge is computed from it as written)
    dedriftwarp<surf>                                  the dedrift warp of the children's registrations
    sphere-<i>.reg.corrected<surf>                     subject i's sphere in the root's frame (its corrected sphere pushed through its child's warp)
    transformed_and_reprojected.dedrift-<i><data>      its native data resampled from there onto the template
    sphere-<i>.distortion<data>                        areal and shape distortion of that sphere against the subject's input sphere
    mean<data>, stdev<data>                            over all subjects of the root
    group_stats.txt                                    a block for the root and one per child (the child's subjects in the root's frame), in
                                                       compare_stats.py's wording
    clusters.csv                                       rows i,subject,root: the left child's subjects first
Out of scope: the clustering itself, the registration of a leaf group, weighted masks, more than one GPU, a C++ twin of this tool.  Agreement with
wb_command's arithmetic is unpinned (DESIGN.md sections 5.10 and 5.13).
"""
import argparse
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import config, dedrift, group_registration, hierarchy, meshio  # noqa: E402
import dedrift_files  # noqa: E402
import register_files  # noqa: E402


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="hierarchy_files.py", description="registered groups merged pairwise up a hierarchy on the MI355X path, with the "
                                 "statistics of every merged group and of its children")
    ap.add_argument("--clusters", required=True, help="CSV rows line,subject,group")
    ap.add_argument("--path", required=True, help="CSV rows left,right,root, processed in file order")
    ap.add_argument("--subjects", required=True, help="one subject name per line, aligned with --meshes and --data")
    ap.add_argument("-m", "--meshes", required=True, help="list of paths to the subjects' input spheres; one line serves every subject")
    ap.add_argument("--data", required=True, help="list of paths of the subjects' native data files")
    ap.add_argument("--template", required=True, help="the template sphere")
    ap.add_argument("-c", "--conf", default="", help="configuration of the groupwise registration of the children's mean maps")
    ap.add_argument("--dir", required=True, help="prefix of every group's files: <dir><group>.")
    ap.add_argument("--mask", default="", help="a map on the template; vertices with a value > 0 enter the pairwise statistics")
    ap.add_argument("--percentile", type=float, default=75.0, help="threshold of the Dice overlap (compare_stats.py: 75)")
    ap.add_argument("-f", "--format", default="GIFTI", help="format of output files: GIFTI, ASCII or ASCII_MAT")
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def read_clusters(path):
    """{group: [subject names in `line` order]} of rows line,subject,group"""
    groups = {}
    with open(path, newline="") as f:
        for n, row in enumerate(csv.reader(f)):
            if not row or not "".join(row).strip():
                continue
            if len(row) != 3:
                raise SystemExit("hierarchy_files.py: %s, row %d: expected line,subject,group, found %r" % (path, n + 1, ",".join(row)))
            try:
                line = int(row[0])
            except ValueError:
                raise SystemExit("hierarchy_files.py: %s, row %d: the line number %r is not an integer" % (path, n + 1, row[0]))
            groups.setdefault(row[2].strip(), []).append((line, row[1].strip()))
    out = {}
    for g, members in groups.items():
        members.sort()
        if [ln for ln, _ in members] != list(range(len(members))):
            raise SystemExit("hierarchy_files.py: %s: the lines of group %s are %s, expected 0 .. %d" % (path, g, [ln for ln, _ in members], len(members) - 1))
        out[g] = [name for _, name in members]
    return out


def read_path(path):
    """[(left, right, root)] in file order"""
    rows = []
    with open(path, newline="") as f:
        for n, row in enumerate(csv.reader(f)):
            if not row or not "".join(row).strip():
                continue
            if len(row) != 3:
                raise SystemExit("hierarchy_files.py: %s, row %d: expected left,right,root, found %r" % (path, n + 1, ",".join(row)))
            rows.append(tuple(x.strip() for x in row))
    return rows


def subject_table(names, mesh_files, data_files):
    """{name: (mesh path, data path)}; one mesh line serves every subject"""
    if len(mesh_files) == 1:
        mesh_files = list(mesh_files) * len(names)
    if not (len(names) == len(mesh_files) == len(data_files)):
        raise SystemExit("hierarchy_files.py: %d subject names, %d meshes, %d data files (one mesh for all subjects, or one per subject)"
                         % (len(names), len(mesh_files), len(data_files)))
    if len(set(names)) != len(names):
        raise SystemExit("hierarchy_files.py: --subjects names a subject twice")
    return {name: (mesh_files[k], data_files[k]) for k, name in enumerate(names)}


def find(stem, exts):
    for e in exts:
        if os.path.exists(stem + e):
            return stem + e
    return None


def missing_leaf_message(prefix, group, missing, a):
    """what to run first: the two commands that make a leaf group's files"""
    return ("hierarchy_files.py: leaf group %s: %s does not exist.  A leaf group must have been registered and dedrifted first, with lists of its subjects' "
            "files in `line` order:\n"
            "    python tools/register_files.py --groupwise --meshes=MESHES_%s --data=DATA_%s --template=%s --conf=%s --out=%sgw.\n"
            "    python tools/dedrift_files.py --meshes=MESHES_%s --data=DATA_%s --template=%s --regs=%sgw. --out=%s\n"
            % (group, missing, group, group, a.template, a.conf or "CONF", prefix, group, group, a.template, prefix, prefix))


def group_members(name, row_index, clusters, roots):
    """the subject names of child `name` of path row row_index: the root of an earlier row, or a leaf of the clustering file"""
    if name in roots:
        return roots[name]
    if name in clusters:
        return clusters[name]
    raise SystemExit("hierarchy_files.py: path row %d: child %s is neither a group of the clustering file nor the root of an earlier row" % (row_index + 1, name))


def child_files(a, name, members, is_leaf):
    """(path of the mean map, paths of the members' spheres) under <dir><name>., or the error that says what is missing"""
    prefix = a.dir + name + "."
    mean_path = find(prefix + "mean", dedrift_files.DATA_EXTS)
    sphere_paths = [find(prefix + "sphere-%d.reg.corrected" % i, dedrift_files.SURF_EXTS) for i in range(len(members))]
    for stem, found in [(prefix + "mean", mean_path)] + [(prefix + "sphere-%d.reg.corrected" % i, p) for i, p in enumerate(sphere_paths)]:
        if found is None:
            missing = " / ".join(stem + e for e in (dedrift_files.DATA_EXTS if stem.endswith("mean") else dedrift_files.SURF_EXTS))
            raise SystemExit(missing_leaf_message(prefix, name, missing, a) if is_leaf else "hierarchy_files.py: group %s: %s does not exist" % (name, missing))
    return mean_path, sphere_paths


def load_child(a, name, members, table, inputs, nvt, is_leaf):
    """merge_groups' child record but for `reg`, from the files under <dir><name>."""
    mean_path, sphere_paths = child_files(a, name, members, is_leaf)
    subjects, datas = [], []
    for i, subject in enumerate(members):
        if subject not in table:
            raise SystemExit("hierarchy_files.py: group %s: subject %s is not listed in --subjects" % (name, subject))
        mesh_path, data_path = table[subject]
        if mesh_path not in inputs:
            xyz, tri = meshio.load_surface(mesh_path)
            inputs[mesh_path] = (dedrift_files.on_sphere(xyz), tri)
        xyz, tri = inputs[mesh_path]
        corrected, ctri = meshio.load_surface(sphere_paths[i])
        if len(corrected) != len(xyz) or not np.array_equal(ctri, tri):
            raise SystemExit("hierarchy_files.py: %s is not a sphere of %s (different mesh)" % (sphere_paths[i], mesh_path))
        subjects.append((xyz, corrected, tri))
        datas.append(meshio.load_data(data_path, len(xyz)))
    return dict(mean=meshio.load_data(mean_path, nvt), subjects=subjects, data=datas)


def register_means(ctx, cfg, template, means):
    """the groupwise registration of the children's mean maps on the template mesh: register_files.main_groupwise's loop with the template as every mesh"""
    txyz, ttri = template
    if any(m in ("RIGID", "AFFINE") for m in cfg["opt"]):
        raise SystemExit("AFFINE/RIGID registration is not supported in groupwise mode.")
    if cfg["dopt"] != "HOCR":
        raise SystemExit("Groupwise mode is only supported in the HOCR version of MSM.")
    levels, run_kw = register_files.discrete_levels(cfg, means[0].shape[0], groupwise=True)
    regs, _, _ = group_registration.run_group_multiresolution(group_registration.ProductGroupOps(ctx), [(txyz, ttri)] * len(means), means, txyz, ttri, levels,
                                                              fixnan=cfg["fixnan"], **run_kw, **config.run_options(cfg))
    return [np.asarray(r) for r in regs]


def main(argv):
    a = parse_args(argv)
    surf_ext, data_ext = dedrift_files.output_formats(a.format)
    clusters = read_clusters(a.clusters)
    rows = read_path(a.path)
    table = subject_table(dedrift_files.read_ascii_list(a.subjects), dedrift_files.read_ascii_list(a.meshes), dedrift_files.read_ascii_list(a.data))
    roots, made = {}, set()
    for k, (left, right, root) in enumerate(rows):  # the whole path is checked before the first registration
        for child in (left, right):
            members = group_members(child, k, clusters, roots)
            if child not in made:  # its files have to be there already
                child_files(a, child, members, child in clusters)
        if left == right or root in clusters or root in made:
            raise SystemExit("hierarchy_files.py: path row %d: %s,%s,%s merges a group with itself or names a root that exists" % (k + 1, left, right, root))
        made.add(root)
        roots[root] = group_members(left, k, clusters, roots) + group_members(right, k, clusters, roots)
    txyz, ttri = meshio.load_surface(a.template)
    txyz = dedrift_files.on_sphere(txyz)
    mask = meshio.load_data(a.mask, len(txyz))[0] if a.mask else None
    cfg = config.parse_config(register_files.read_conf(a.conf))
    ctx = M.Context(a.device)
    inputs = {}
    for left, right, root in rows:
        names = (left, right)
        children = [load_child(a, c, clusters[c] if c in clusters else roots[c], table, inputs, len(txyz), c in clusters) for c in names]
        if a.verbose:
            print("Merging %s (%d subjects) and %s (%d subjects) into %s" % (left, len(children[0]["data"]), right, len(children[1]["data"]), root))
        out = a.dir + root + "."
        regs = register_means(ctx, cfg, (txyz, ttri), [c["mean"] for c in children])
        for g, c in enumerate(children):
            reg_path = out + "child-%d.reg" % g + surf_ext
            meshio.save_surface(reg_path, regs[g], ttri)
            c["reg"] = meshio.load_surface(reg_path)[0]  # what a later reader has: the sphere as written
        r = hierarchy.merge_groups(dedrift.ProductOps(ctx), (txyz, ttri), children, percentile=a.percentile, mask=mask)
        meshio.save_surface(out + "dedriftwarp" + surf_ext, r["W"], ttri)
        for i, (g, s) in enumerate(r["order"]):
            orig, _, tri = children[g]["subjects"][s]
            meshio.save_surface(out + "sphere-%d.reg.corrected" % i + surf_ext, r["composed"][i], tri)
            dedrift_files.save_data(out + "transformed_and_reprojected.dedrift-%d" % i + data_ext, txyz, r["resampled"][i])
            dedrift_files.save_data(out + "sphere-%d.distortion" % i + data_ext, orig, r["distortion"][i])
        dedrift_files.save_data(out + "mean" + data_ext, txyz, r["mean"])
        dedrift_files.save_data(out + "stdev" + data_ext, txyz, r["stdev"])
        rn = dedrift_files.row_names(r["mean"].shape[0])
        blocks = [dedrift.format_stats(root, rn, r["cc_mean"], r["dice_mean"], r["summary"])]
        for g, c in enumerate(names):
            blocks.append(dedrift.format_stats("%s within %s" % (c, root), rn, r["children_stats"][g]["cc_mean"], r["children_stats"][g]["dice_mean"]))
        text = "\n".join(blocks)
        with open(out + "group_stats.txt", "w") as f:
            f.write(text)
        with open(out + "clusters.csv", "w", newline="") as f:
            csv.writer(f, lineterminator="\n").writerows([i, name, root] for i, name in enumerate(roots[root]))
        print(text, end="")
    ctx.close()
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main(sys.argv[1:]))
    except (config.ConfigError, ValueError) as e:
        raise SystemExit(str(e))
    except M.MsmError as e:
        raise SystemExit("hierarchy_files.py: %s" % e)
