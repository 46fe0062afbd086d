"""tools/time_rigid.py [--repeats N] -- the rigid level of the HCP MSMSulc schedule on the MI355X (GPU only): --opt=AFFINE at --datagrid=6, D = 1,
--simval=3 (-> 2), --it=50, --sigma_in/ref=0, --VN, default --stepsize / --gradsampling, on newmsm_amd/synthetic.py data (an ico6 subject whose
sulc-like feature is the reference's seen through a ~4 degree warp).  Prints one JSON line: evaluations, launches, kernel milliseconds per launch and
per evaluation, and the level's wall time (set-up: featurespace + initialise; run)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MSMSULC = os.path.join(ROOT, "tests", "golden", "MSMSulcStrainFinalconf")

import numpy as np  # noqa: E402

import newmsm_amd as M  # noqa: E402
from newmsm_amd import config, registration, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    with open(MSMSULC) as f:  # config/HCP_multimodal_alignment/MSMSulcStrainFinalconf
        lv = config.levels_from_config(config.parse_config(f.read()), 1, rigid=True)[0][0]
    assert lv["method"] == "RIGID" and lv["data_order"] == 6 and lv["simmeasure"] == 2 and lv["iters"] == 50
    ctx = M.Context(0)
    ops = registration.ProductOps(ctx)
    in_xyz, in_tri = M.make_mesh_from_icosa(6)
    ref = synthetic.features(in_xyz, 1, 7)
    src = synthetic.features(synthetic.known_warp(in_xyz, seed=9, rot_deg=4.0, amp=1.0), 1, 7)
    runs = []
    for rep in range(a.repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        in_mesh, ref_mesh = ops.mesh(in_xyz, in_tri), ops.mesh(in_xyz, in_tri)
        ico_xyz, ico_tri = ops.icosphere(lv["data_order"])
        ico = ops.mesh(ico_xyz, ico_tri)
        feats = [ops.variance_normalise(ops.metric_resample(m, d, ico)) for m, d in ((in_mesh, src), (ref_mesh, ref))]  # featurespace::initialise
        ops.unfold(ico)  # project_CPgrid at level 1
        rcf = M.RigidCostFunction(ctx, ico, ico, feats[0], feats[1], simmeasure=lv["simmeasure"]).initialise()
        rcf.update_source(ops.coords(ico))
        t1 = time.perf_counter()
        _, trace, summary = rcf.run(lv["iters"], lv["stepsize"], lv["gradsampling"])
        t2 = time.perf_counter()
        kms, launches = rcf.kernel_ms()
        rcf.close()
        runs.append(dict(setup_ms=(t1 - t0) * 1e3, run_ms=(t2 - t1) * 1e3, kernel_ms=kms, launches=launches, evaluations=summary["evaluations"],
                         iterations=len(trace), accepted=int(trace[:, 5].sum()), RECinit=summary["RECinit"], RECfinal=summary["RECfinal"]))
    last = runs[-1]
    out = dict(level="HCP_MSMSulc level 1 (AFFINE, ico6, D=1, simval 2, it 50)", V=len(in_xyz), evaluations=last["evaluations"], iterations=last["iterations"],
               accepted=last["accepted"], launches=last["launches"], kernel_ms_total=last["kernel_ms"], kernel_ms_per_launch=last["kernel_ms"] / last["launches"],
               kernel_ms_per_evaluation=last["kernel_ms"] / last["evaluations"], run_wall_ms=last["run_ms"], setup_wall_ms=last["setup_ms"],
               level_wall_ms=last["setup_ms"] + last["run_ms"], first_level_wall_ms=runs[0]["setup_ms"] + runs[0]["run_ms"],
               run_wall_ms_all=[round(r["run_ms"], 3) for r in runs], RECinit=last["RECinit"], RECfinal=last["RECfinal"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
