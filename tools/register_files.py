"""`newmsm` for DISCRETE levels, from files to files under newmsm's own flag names (CLI/msmOptions.h:59-157), over the MI355X path:

    python tools/register_files.py --inmesh=in.sphere.surf.gii --refmesh=ref.sphere.surf.gii --indata=in.func.gii --refdata=ref.func.gii \\
                                   --conf=config/basic_configs/config_standard_MSM_strain --out=/path/prefix. [-f GIFTI|ASCII|ASCII_MAT] [--verbose]

What CLI/newmsm.cpp:29-58 does for a pairwise run: set_input / set_reference (load, recentre, true_rescale to RAD = 100:
M/mesh_registration.cpp:416-438), the configuration file through the reference's grammar (newmsm_amd/config.py = parse_reg_options :459-784),
run_multiresolutions (:30-50: per DISCRETE level featurespace + project_CPgrid + run_discrete_opt with the optimiser --dopt names), then the three
outputs of :47-49:
    <out>sphere.reg<surf>                     transform (:352-356): the input sphere moved through the final warp
    <out>sphere.LR.reg<surf>                  saveSPH_reg (M/mesh_registration.h:170): the last level's data grid at its registered position
    <out>transformed_and_reprojected<data>    save_transformed_data (:358-408): the input data resampled from the registered sphere onto the reference
with <surf> / <data> = .surf.gii / .func.gii (GIFTI), .asc / .dpv (ASCII), .asc / .txt (ASCII_MAT) as set_output_format (:827-842) names them.

With --inanat / --refanat (both or none, CLI/newmsm.cpp:40-45) and --regoption=5 in the configuration the run is an aMSM one: the anatomical
surfaces are loaded as they are (set_anatomical, M/mesh_registration.cpp:434-438: no recentre, no rescale).  Given both, save_transformed_data
(:397-407) writes two more files, always GIFTI (Mesh::save of a name without an extension):
    <out>anat.reg.surf.gii                    project_anatomical_mesh: the input sphere's topology, each registered vertex placed on the reference anatomy
    <out>STRAINS.func.gii                     calculate_strains(2, in_anat, anat.reg): per vertex of the input anatomy the maximum and minimum principal
                                              stretch and 0.5 (lambda^2 - 1) of each (four rows)

With -t / --trans=<sphere.reg of an earlier run> (set_transformed, :440-443: loaded as it is, no recentre, no rescale) the first level starts from that
registration (project_CPgrid, :136-145) and sphere.reg is the composition: the two-stage workflow of the reference's guide (folding first, then
myelin or multimodal features).  It needs the input mesh's vertex count; with the input mesh's coordinates the reference's warning is printed and
the run goes on without it.  --excl (with --cutthr) in the configuration keeps the cut (every feature inside the thresholds: the zero-valued medial
wall) out of every level's resampling, smoothing and variance normalisation and out of the final resampling of save_transformed_data (:371-383).

Groupwise mode (CLI/newmsm.cpp:13-27, -g / --groupwise):

    python tools/register_files.py --groupwise --meshes=mesh_list.txt --data=data_list.txt --template=template.sphere.surf.gii [--mask=mask.func.gii] \
                                   --conf=gMSM_config.txt --out=/path/prefix.

--meshes / --data: text files with one path per line (read_ascii_list, M/mesh_registration.cpp:871-884), subject i = line i of both; every mesh
and the template recentred and rescaled to RAD (M/group_mesh_registration.h:46-57,72-77).  Outputs, per subject i (M/group_mesh_registration.cpp:
120-133, .h:79-82): <out>sphere-<i>.reg<surf>, <out>sphere-<i>.LR.reg<surf>, <out>transformed_and_reprojected-<i><data> (the subject's data
resampled from its registered sphere onto the TEMPLATE: without a mask, M/group_mesh_registration.cpp:127-133).  --trans is ignored there with a note
on stderr (CLI/newmsm.cpp never hands it to a groupwise run).

Outside the path and reported instead of silently dropped: AFFINE / RIGID levels (skipped with a note on stderr unless MSMHIP_RIGID=on, which runs
them), --IN / --INc (refused unless MSMHIP_HISTMATCH=on, which runs the histogram matching of DESIGN.md section 5.11 on the GPU: in every level's feature
preparation and, pairwise, before the final resampling), --excl together with both weightings; the
binary solve of --dopt=HOCR / FastPD is a stand-in (iterated conditional modes: FastPD and ELC are licence-restricted and FSL-bound), so a run
exercises the path exactly as newmsm would but its labelings are not HOCR's.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import config, group_registration, meshio, registration  # noqa: E402

RAD = 100.0
STRAIN_FIT_RADIUS = 2.0  # calculate_strains(2, in_anat, ANAT_TRANS), M/mesh_registration.cpp:405


def on_sphere(xyz, rad=RAD):
    """recentre + true_rescale (R/mesh.cpp:1198-1255), as Mesh_registration::set_input / set_reference apply them"""
    xyz = xyz - xyz.mean(axis=0)
    return xyz * (rad / np.linalg.norm(xyz, axis=1, keepdims=True))


def output_formats(fmt):
    """Mesh_registration::set_output_format, M/mesh_registration.cpp:827-842"""
    if fmt == "GIFTI":
        return ".surf.gii", ".func.gii"
    if fmt in ("ASCII", "ASCII_MAT"):
        return ".asc", (".dpv" if fmt == "ASCII" else ".txt")
    return ".vtk", ".txt"


def save_data(path, mesh_xyz, data):
    if path.endswith(".dpv"):
        meshio.save_dpv(path, mesh_xyz, data)
    elif path.endswith(".txt"):
        meshio.save_matrix(path, data)
    else:
        meshio.save_metric(path, data)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="register_files.py", description="newmsm's pairwise mode over the MI355X path (DISCRETE levels)")
    ap.add_argument("-M", "--inmesh", default="", help="input mesh (GIFTI or FreeSurfer ASCII); needs to be a sphere")
    ap.add_argument("-R", "--refmesh", default="", help="reference mesh; the input mesh when not given")
    ap.add_argument("-i", "--indata", default="", help="scalar or multivariate data for input (.func.gii / .shape.gii / .asc / .dpv / .txt)")
    ap.add_argument("-I", "--refdata", default="", help="scalar or multivariate data for reference")
    ap.add_argument("-w", "--inweight", default="", help="cost function weighting for input")
    ap.add_argument("-W", "--refweight", default="", help="cost function weighting for reference")
    ap.add_argument("-t", "--trans", default="", help="transformed source mesh (output of a previous registration, i.e. sphere.reg.surf.gii): the first level starts from it")
    ap.add_argument("-a", "--inanat", default="", help="input anatomical mesh (the input sphere's vertices on the anatomical surface; --regoption=5)")
    ap.add_argument("-A", "--refanat", default="", help="reference anatomical mesh")
    ap.add_argument("-g", "--groupwise", action="store_true", help="run newMSM in groupwise mode")
    ap.add_argument("-m", "--meshes", default="", help="groupwise mode only; list of paths to input meshes. Needs to be a sphere")
    ap.add_argument("--template", default="", help="groupwise mode only; templates sphere for resampling. Needs to be a sphere")
    ap.add_argument("--data", default="", help="groupwise mode only; list of paths of the data files")
    ap.add_argument("--mask", default="", help="groupwise mode only; mask file path")
    ap.add_argument("-o", "--out", required=True, help="output basename")
    ap.add_argument("-f", "--format", default="GIFTI", help="format of output files: GIFTI, ASCII or ASCII_MAT")
    ap.add_argument("-c", "--conf", default="", help="configuration file")
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def read_ascii_list(path):
    """Mesh_registration::read_ascii_list, M/mesh_registration.cpp:871-884: the whitespace-separated entries of a text file"""
    with open(path) as f:
        return f.read().split()


def read_conf(path):
    if not path:
        return None
    with open(path) as f:
        return f.read()


def rigid_enabled():
    """MSMHIP_RIGID=on: AFFINE / RIGID levels run (Rigid_cost_function on the GPU) instead of being skipped"""
    return os.environ.get("MSMHIP_RIGID", "") == "on"


def histmatch_enabled():
    """MSMHIP_HISTMATCH=on: --IN / --INc run (histogram matching on the GPU) instead of ending the run with an error"""
    return os.environ.get("MSMHIP_HISTMATCH", "") == "on"


def mplp_enabled():
    """MSMHIP_MPLP=on: --dopt=MPLP (an extension, not newMSM's: max-product linear programming over the MCMC optimiser's tables, --mciters sweeps per
    iteration) runs instead of ending the run with the reference's message (Unrecognized optimiser)"""
    return os.environ.get("MSMHIP_MPLP", "") == "on"


def mplp_forbid_setting():
    """MSMHIP_MPLP_FORBID=on (beside MSMHIP_MPLP=on): a --dopt=MPLP level reads the NaN and +infinity entries of its triplet table as forbidden label
    combinations instead of refusing the table ("Forbidden entries").  Anything else, or the variable without MSMHIP_MPLP=on,
    ends the run with a message and exit status 1."""
    text = os.environ.get("MSMHIP_MPLP_FORBID")
    if text is not None and text != "on":
        raise SystemExit("MSMHIP_MPLP_FORBID=%s: the forbidden-entry reading of MPLP's triplet table is switched on with MSMHIP_MPLP_FORBID=on (unset: off)" % text)
    if text is not None and not mplp_enabled():
        raise SystemExit("MSMHIP_MPLP_FORBID=on changes how --dopt=MPLP reads its triplet table: it needs MSMHIP_MPLP=on")
    return text == "on"


def mplp_pairs_setting():
    """MSMHIP_MPLP_PAIRS=on (beside MSMHIP_MPLP=on): --dopt=MPLP with --regoption=1 runs, as MPLP over the unary and pair tables of the pairwise model
    with both tables on the device, instead of ending the run with the FastPD-only message.  Anything else, or the variable
    without MSMHIP_MPLP=on, ends the run with a message and exit status 1."""
    text = os.environ.get("MSMHIP_MPLP_PAIRS")
    if text is not None and text != "on":
        raise SystemExit("MSMHIP_MPLP_PAIRS=%s: MPLP over the pair tables of --regoption=1 is switched on with MSMHIP_MPLP_PAIRS=on (unset: off)" % text)
    if text is not None and not mplp_enabled():
        raise SystemExit("MSMHIP_MPLP_PAIRS=on lets --dopt=MPLP run a --regoption=1 level: it needs MSMHIP_MPLP=on")
    return text == "on"


def mplp_round_setting():
    """MSMHIP_MPLP_ROUND=on (beside MSMHIP_MPLP=on): every iteration of a --dopt=MPLP level rounds the final messages to a labelling after its sweeps
    ("Rounding"), with MSMHIP_MPLP_POLISH=n (0 ... 64, default 8) polish passes.  Returns (on, polish); anything else, or either
    variable without MSMHIP_MPLP=on, ends the run with a message and exit status 1."""
    text, passes = os.environ.get("MSMHIP_MPLP_ROUND"), os.environ.get("MSMHIP_MPLP_POLISH")
    if text is not None and text != "on":
        raise SystemExit("MSMHIP_MPLP_ROUND=%s: the rounding of MPLP's messages is switched on with MSMHIP_MPLP_ROUND=on (unset: off)" % text)
    if text is not None and not mplp_enabled():
        raise SystemExit("MSMHIP_MPLP_ROUND=on rounds the messages of --dopt=MPLP: it needs MSMHIP_MPLP=on")
    n = 8
    if passes is not None:
        if text is None:
            raise SystemExit("MSMHIP_MPLP_POLISH=%s sets the polish passes of the rounding: it needs MSMHIP_MPLP_ROUND=on" % passes)
        try:
            n = int(passes)
        except ValueError:
            n = -1
        if not 0 <= n <= 64:
            raise SystemExit("MSMHIP_MPLP_POLISH=%s: the number of polish passes must be a whole number from 0 to 64" % passes)
    return text == "on", n


def fusion_mplp_setting():
    """MSMHIP_FUSION=mplp: the binary problem of every label step of a --dopt=HOCR level is solved by MPLP on the device (an extension: DESIGN.md section
    5.21) instead of the stand-in; icm or unset: the stand-in, today's bytes.  MSMHIP_FUSION_SWEEPS=n (1 ... 256, default 10) and MSMHIP_FUSION_POLISH=n
    (0 ... 64, default 8) set its sweeps and polish passes and need MSMHIP_FUSION=mplp.  Returns (on, sweeps, polish); anything else ends the run with a
    message and exit status 1."""
    text = os.environ.get("MSMHIP_FUSION")
    if text is not None and text not in ("mplp", "icm"):
        raise SystemExit("MSMHIP_FUSION=%s: the binary solve of a label step is the stand-in (icm, or unset) or MPLP on the device (mplp)" % text)
    on = text == "mplp"
    values = []
    for name, what, lo, hi, default in (("MSMHIP_FUSION_SWEEPS", "sweeps", 1, 256, 10), ("MSMHIP_FUSION_POLISH", "polish passes", 0, 64, 8)):
        t, n = os.environ.get(name), default
        if t is not None:
            if not on:
                raise SystemExit("%s=%s sets the %s of a label step's MPLP solve: it needs MSMHIP_FUSION=mplp" % (name, t, what))
            try:
                n = int(t)
            except ValueError:
                n = lo - 1
            if not lo <= n <= hi:
                raise SystemExit("%s=%s: the number of %s must be a whole number from %d to %d" % (name, t, what, lo, hi))
        values.append(n)
    return on, values[0], values[1]


def mcmc_gpu_enabled():
    """MSMHIP_MCMC=gpu: the --dopt=MCMC levels keep both cost tables on the device and run the optimiser's sweeps there (the same labelings)"""
    return os.environ.get("MSMHIP_MCMC", "") == "gpu"


def mcmc_chains_setting():
    """MSMHIP_MCMC_CHAINS=n (1 ... 256): every iteration of a --dopt=MCMC level runs n chains from n seeds and keeps the labelling with the lowest energy
    (DESIGN.md section 5.16); unset or 1: the single run.  Anything else ends the run with a message and exit status 1."""
    text = os.environ.get("MSMHIP_MCMC_CHAINS")
    if text is None:
        return 1
    try:
        n = int(text)
    except ValueError:
        n = 0
    if not 1 <= n <= 256:
        raise SystemExit("MSMHIP_MCMC_CHAINS=%s: the number of Monte Carlo chains must be a whole number from 1 to 256" % text)
    return n


def mcmc_draw_gpu_setting():
    """MSMHIP_MCMC_DRAW=gpu (with MSMHIP_MCMC=gpu): the GPU sweeps take their proposals from the draw kernel instead of the host's stream (DESIGN.md
    section 5.16, "Proposals on the device"; the same bytes); unset or host: the host's stream.  Anything else, or gpu without MSMHIP_MCMC=gpu, ends the
    run with a message and exit status 1."""
    text = os.environ.get("MSMHIP_MCMC_DRAW")
    if text is None or text == "host":
        return False
    if text != "gpu":
        raise SystemExit("MSMHIP_MCMC_DRAW=%s: the proposals are drawn on the host (host, or unset) or on the device (gpu)" % text)
    if not mcmc_gpu_enabled():
        raise SystemExit("MSMHIP_MCMC_DRAW=gpu draws the proposals of the GPU sweeps: it needs MSMHIP_MCMC=gpu")
    return True


def group_mcmc_setting():
    """MSMHIP_GROUP_MCMC=on: a --groupwise configuration with --dopt=MCMC runs, block-coordinate descent over the subjects with the Monte Carlo optimiser
    on every block (an extension); unset: it ends with the reference's message (M/group_mesh_registration.cpp:87).  Anything else
    ends the run with a message and exit status 1."""
    text = os.environ.get("MSMHIP_GROUP_MCMC")
    if text is None:
        return False
    if text != "on":
        raise SystemExit("MSMHIP_GROUP_MCMC=%s: the groupwise Monte Carlo optimiser is switched on with MSMHIP_GROUP_MCMC=on (unset: off)" % text)
    return True


def group_mcmc_passes_setting():
    """MSMHIP_GROUP_MCMC_PASSES=n (1 ... 64): passes over the subjects per iteration of a groupwise --dopt=MCMC level; unset: 1"""
    text = os.environ.get("MSMHIP_GROUP_MCMC_PASSES")
    if text is None:
        return 1
    try:
        n = int(text)
    except ValueError:
        n = 0
    if not 1 <= n <= 64:
        raise SystemExit("MSMHIP_GROUP_MCMC_PASSES=%s: the number of passes over the subjects must be a whole number from 1 to 64" % text)
    return n


def group_mcmc_draw_setting():
    """MSMHIP_MCMC_DRAW for a groupwise --dopt=MCMC run, whose blocks always sweep on the device: gpu, host or unset"""
    text = os.environ.get("MSMHIP_MCMC_DRAW")
    if text is None or text == "host":
        return False
    if text != "gpu":
        raise SystemExit("MSMHIP_MCMC_DRAW=%s: the proposals are drawn on the host (host, or unset) or on the device (gpu)" % text)
    return True


def discrete_levels(cfg, D, anat=False, groupwise=False):
    levels, run_kw, skipped = config.levels_from_config(cfg, D, anat=anat, groupwise=groupwise, rigid=rigid_enabled() and not groupwise,
                                                        **(dict(histmatch=True) if histmatch_enabled() else {}),
                                                        **(dict(mplp=True) if mplp_enabled() else {}),
                                                        **(dict(mplp_pairs=True) if not groupwise and mplp_pairs_setting() else {}))
    for index, method in skipped:
        print("register_files.py: level %d (--opt=%s) is outside the path (the affine stage stays on the CPU in newmsm): skipped" % (index + 1, method), file=sys.stderr)
    if not levels:
        raise SystemExit("register_files.py: the configuration holds no DISCRETE level")
    return levels, run_kw


def features_gpu_enabled():
    """MSMHIP_FEATURES=gpu: every level's features are prepared through one msm_level_features call; the same files are written"""
    return os.environ.get("MSMHIP_FEATURES", "") == "gpu"


def main_groupwise(a, surf_ext, data_ext, group_mcmc=False, chains=1, draw_gpu=False):
    """CLI/newmsm.cpp:13-27 + Group_Mesh_registration (M/group_mesh_registration.h:46-82, .cpp:26-133).  group_mcmc (MSMHIP_GROUP_MCMC=on): --dopt=MCMC runs
    instead of being refused, with `chains` chains per block and the proposals drawn where draw_gpu says"""
    passes = group_mcmc_passes_setting() if group_mcmc else 1
    for flag in ("meshes", "template", "data"):
        if not getattr(a, flag):
            raise SystemExit("register_files.py: --groupwise needs --%s" % flag)
    mesh_files, data_files = read_ascii_list(a.meshes), read_ascii_list(a.data)
    if len(mesh_files) != len(data_files):
        raise SystemExit("featurespace::Initialize do not have the same number of datasets and surface meshes")  # M/featurespace.cpp:43-44
    if a.trans:
        print("register_files.py: --trans is not used in groupwise mode: ignored", file=sys.stderr)
    cfg = config.parse_config(read_conf(a.conf))
    if any(m in ("RIGID", "AFFINE") for m in cfg["opt"]):
        raise SystemExit("AFFINE/RIGID registration is not supported in groupwise mode.")  # M/group_mesh_registration.cpp:29-30
    if cfg["dopt"] != "HOCR" and not (group_mcmc and cfg["dopt"] == "MCMC"):
        raise SystemExit("Groupwise mode is only supported in the HOCR version of MSM.")  # :87
    meshes = []
    for k, path in enumerate(mesh_files):
        if a.verbose:
            print("Mesh #%d is %s" % (k, path))
        xyz, tri = meshio.load_surface(path)
        meshes.append((on_sphere(xyz), tri))
    if a.verbose:
        print("Template is " + a.template)
    txyz, ttri = meshio.load_surface(a.template)
    txyz = on_sphere(txyz)
    datas = [meshio.load_data(path, len(meshes[k][0])) for k, path in enumerate(data_files)]
    mask = meshio.load_data(a.mask, len(txyz))[0] if a.mask else None
    levels, run_kw = discrete_levels(cfg, datas[0].shape[0], groupwise=True)
    ctx = M.Context(a.device)
    if a.verbose:
        print("This is newMSM's groupwise DISCRETE path on an MI355X (msm-mi355x).\nStarting multiresolution with %d levels." % len(levels))
        if features_gpu_enabled():
            print("Level features in one call on the GPU.")
        if cfg["dopt"] == "MCMC":
            print("Groupwise MCMC, subject by subject: %d chains per block, %d passes per iteration, proposals drawn on the %s." % (chains, passes, "GPU" if draw_gpu else "host"))
    mc_kw = dict(mcmc_chains=chains, mcmc_passes=passes) if cfg["dopt"] == "MCMC" else {}
    ops = group_registration.ProductGroupOps(ctx, features_gpu=features_gpu_enabled(), mcmc_draw_gpu=draw_gpu and cfg["dopt"] == "MCMC")
    regs, level_regs, energies = group_registration.run_group_multiresolution(ops, meshes, datas, txyz, ttri, levels, mask=mask,
                                                                              fixnan=cfg["fixnan"], **run_kw, **config.run_options(cfg), **mc_kw)
    last_tri = M.make_mesh_from_icosa(levels[-1]["data_order"])[1]
    target = M.Mesh(ctx, txyz, ttri)
    for s in range(len(meshes)):
        meshio.save_surface(a.out + "sphere-%d.reg" % s + surf_ext, regs[s], meshes[s][1])            # transform
        meshio.save_surface(a.out + "sphere-%d.LR.reg" % s + surf_ext, level_regs[-1][s], last_tri)   # saveSPH_reg
        moved = M.Mesh(ctx, regs[s], meshes[s][1])
        save_data(a.out + "transformed_and_reprojected-%d" % s + data_ext, txyz, M.metric_resample(moved, datas[s], target))  # save_transformed_data
    if a.verbose:
        for k, e in enumerate(energies):
            print("level %d: energies per iteration %s" % (k + 1, [round(v, 4) for v in e]))
    ctx.close()


def main(argv):
    a = parse_args(argv)
    chains = mcmc_chains_setting()  # (the groupwise loops run no MCMC unless MSMHIP_GROUP_MCMC=on: checked, then unused there)
    group_mcmc = a.groupwise and group_mcmc_setting()
    draw_gpu = group_mcmc_draw_setting() if group_mcmc else mcmc_draw_gpu_setting()
    surf_ext, data_ext = output_formats(a.format)
    if surf_ext == ".vtk":
        raise SystemExit("register_files.py: VTK output is not written here (GIFTI, ASCII, ASCII_MAT)")
    fusion_mplp, fusion_sweeps, fusion_polish = fusion_mplp_setting()
    if a.groupwise:
        if fusion_mplp:
            raise SystemExit("MSMHIP_FUSION=mplp solves label steps of triplets alone: a --groupwise run (pair factors between the subjects) keeps the stand-in; unset it")
        return main_groupwise(a, surf_ext, data_ext, group_mcmc, chains, draw_gpu)
    mplp_round, mplp_polish = mplp_round_setting()
    mplp_forbid = mplp_forbid_setting()
    mplp_pairs = mplp_pairs_setting()
    for flag in ("inmesh", "indata", "refdata"):
        if not getattr(a, flag):
            raise SystemExit("register_files.py: --%s is required" % flag)
    if bool(a.inanat) != bool(a.refanat):
        raise SystemExit("Error: must supply both anatomical meshes or none")  # CLI/newmsm.cpp:41-43
    ixyz, itri = meshio.load_surface(a.inmesh)
    rxyz, rtri = meshio.load_surface(a.refmesh or a.inmesh)
    ixyz, rxyz = on_sphere(ixyz), on_sphere(rxyz)
    idata, rdata = meshio.load_data(a.indata, len(ixyz)), meshio.load_data(a.refdata, len(rxyz))
    if idata.shape[0] != rdata.shape[0]:
        raise SystemExit("Mesh_registration: input and reference data have different numbers of feature rows (%d, %d)" % (idata.shape[0], rdata.shape[0]))
    cfg = config.parse_config(read_conf(a.conf))
    levels, run_kw = discrete_levels(cfg, idata.shape[0], anat=bool(a.inanat))
    excl = config.run_options(cfg)
    cfw = dict(excl)
    if chains > 1:
        cfw.update(mcmc_chains=chains)
    if a.trans:  # set_transformed: as loaded
        cfw.update(trans_xyz=meshio.load_surface(a.trans)[0])
    if a.inanat:  # set_anatomical: loaded as they are (in_anat keeps its triangles: its normals serve the strain map)
        in_anat, in_anat_tri = meshio.load_surface(a.inanat)
        cfw.update(in_anat=in_anat, ref_anat=meshio.load_surface(a.refanat)[0])
    if a.inweight and a.refweight:
        cfw.update(in_cfweight=meshio.load_data(a.inweight, len(ixyz)), ref_cfweight=meshio.load_data(a.refweight, len(rxyz)))
    ctx = M.Context(a.device)
    if a.verbose:
        print("This is newMSM's DISCRETE path on an MI355X (msm-mi355x).\nStarting multiresolution with %d levels." % len(levels))
        if mcmc_gpu_enabled():
            print("MCMC sweeps on the GPU.")
        if draw_gpu:
            print("MCMC proposals drawn on the GPU.")
        if chains > 1:
            print("MCMC with %d chains per iteration." % chains)
        if features_gpu_enabled():
            print("Level features in one call on the GPU.")
    reg, level_regs, energies = registration.run_multiresolution(registration.ProductOps(ctx, mcmc_gpu=mcmc_gpu_enabled(), features_gpu=features_gpu_enabled(), mcmc_draw_gpu=draw_gpu, mplp_round=mplp_round, mplp_polish=mplp_polish, mplp_forbid=mplp_forbid, mplp_pairs=mplp_pairs, fusion_mplp=fusion_mplp, fusion_sweeps=fusion_sweeps, fusion_polish=fusion_polish), ixyz, itri, idata, rxyz, rtri, rdata, levels, **run_kw, **cfw)
    out = a.out
    meshio.save_surface(out + "sphere.reg" + surf_ext, reg, itri)                                   # transform
    last_xyz, last_tri = M.make_mesh_from_icosa(levels[-1]["data_order"])
    meshio.save_surface(out + "sphere.LR.reg" + surf_ext, level_regs[-1], last_tri)                 # saveSPH_reg
    moved, target = M.Mesh(ctx, reg, itri), M.Mesh(ctx, rxyz, rtri)
    # save_transformed_data (:371-383): with --excl a fresh mask from the native input data keeps the cut out of the resampling; with --IN / --INc the
    # native input data is matched to the native reference data first
    if run_kw.get("intensity") and a.verbose:
        print("Intensity normalise.")
    resampled = registration.transformed_data(registration.ProductOps(ctx), moved, idata, target, rdata, intensity=run_kw.get("intensity", False), **excl)
    save_data(out + "transformed_and_reprojected" + data_ext, rxyz, resampled)
    if a.inanat:  # save_transformed_data's aMSM outputs (:397-407), GIFTI whatever -f says
        anat_reg = M.project_anatomical_mesh(moved, target, cfw["ref_anat"])
        meshio.save_surface(out + "anat.reg.surf.gii", anat_reg, itri)
        if a.verbose:
            print("Calculate strains.")
        meshio.save_metric(out + "STRAINS.func.gii", M.calculate_strains(M.Mesh(ctx, in_anat, in_anat_tri), anat_reg, STRAIN_FIT_RADIUS))
    if a.verbose:
        for k, e in enumerate(energies):
            print("level %d: energies per iteration %s" % (k + 1, [round(v, 4) for v in e]))
    ctx.close()


if __name__ == "__main__":
    try:
        main(sys.argv[1:])
    except (config.ConfigError, ValueError) as e:  # MeshregException: the message, exit status 1 (CLI/newmsm.cpp:62-65)
        raise SystemExit(str(e))
