"""One merge of the hierarchy of clustered groupwise registration (cgMSM): registered, dedrifted groups are merged pairwise, and every subject of
both groups is carried into the merged group's frame (gMSM_scripts/run_cgMSM_ver_gw_iter.sh:16-218, run_cgMSM_ver_gw.sh, cross_register.sh:51-112,
extract_info.py).  The reference does this with gMSM on the groups' mean maps, wb_command and nibabel; here everything after that registration runs on
the GPU over the msm_dedrift_* entry points, and the subjects' maps stay resident until the statistics of the merged group and of each child have
been taken from them.

merge_groups is written over an `ops` object, like dedrift.dedrift_group: dedrift.ProductOps answers from the library, the tests answer the same
calls from a literal numpy restatement (tests/hierarchy_literal.py).

Definitions.  T the template; per child group g: R_g its sphere from the groupwise registration of the children's mean maps
(on T's triangles), mean_g its mean map; per subject s of g: M_s its input sphere, corrected_s its corrected sphere in g's frame, F_s its native data.
  inverse_g    the template's vertices located on R_g, their weights applied to T (the template is every child's input sphere), added in child order
  W            dedrift.dedrift_group's warp of those inverses
  C_g          sphere_project_warp(R_g, T, W); with it the child mean resampled from C_g onto T, and the distortion of C_g against T
  composed_s   sphere_project_warp(corrected_s, T, C_g), children in order, their subjects in order: the merged group's slots
  resampled_s  metric_resample of F_s from composed_s onto T.  The script resamples the maps it had resampled in the child's frame a second time; here
               the native data go through the composed sphere once -- the general form, as section 5.10 chose for the inverse
  distortion_s M_s against composed_s
  statistics   mean, stdev, cc, dice and the pair means of cc and dice over all slots under the mask, and the same over each child's slots: a group
               before and after the merge, in one frame
"""
import numpy as np

from . import dedrift


def merge_groups(ops, template, children, percentile=75, mask=None, details=False):
    """Merges registered child groups into their parent.

    ops        a Context (the library answers) or an ops object (dedrift.ProductOps, or the tests' literal restatement)
    template   (xyz (V(T), 3), tri) of the template sphere
    children   per child a dict: reg (R_g, V(T) x 3), mean (D x V(T)), subjects (list of (M_s, corrected_s, tri)), data (list of F_s, D x V_s)
    mask       V(T) values, a vertex enters cc, dice and the percentile iff mask > 0 (None: all)
    Returns a dict: W, child_corrected (C_g), child_mean, child_distortion (per child); composed, resampled, distortion (per slot); mean, stdev, cc, dice,
    cc_mean, dice_mean (the parent, over all slots); children_stats (per child a dict of the same six over its slots); summary (the distortion summary of
    all slots); order (the (child, subject) pair of every slot) and, with details, searches: dict(children=[...], subjects=[...]) as dedrift_group gives them.
    """
    if not hasattr(ops, "accumulate"):
        ops = dedrift.ProductOps(ops)
    txyz = np.asarray(template[0], dtype=np.float64)
    ttri = np.asarray(template[1], dtype=np.int32)
    G = len(children)
    assert G >= 1 and all(len(c["subjects"]) == len(c["data"]) and len(c["subjects"]) >= 1 for c in children)
    order = [(g, s) for g, c in enumerate(children) for s in range(len(c["subjects"]))]
    N = len(order)
    # 1. the children's registrations dedrifted: one handle of G subjects, the template as every input sphere
    st = ops.begin(txyz, ttri, G)
    try:
        child_searches = [dict(accumulate=ops.accumulate(st, g, c["reg"], ttri, txyz, details)) for g, c in enumerate(children)]  # child order
        W, _ = ops.finish(st)
        child_corrected, child_mean, child_distortion = [], [], []
        for g, c in enumerate(children):
            got = ops.correct(st, g, c["reg"], ttri, txyz, c["mean"], details)
            child_corrected.append(got[0])
            child_mean.append(got[1])
            child_distortion.append(got[2])
            if details:
                child_searches[g]["correct"] = got[3]
    finally:
        ops.end(st)
    # 2. every subject through its child's C_g, into its slot of a handle sized for all of them; 3. the statistics from the resident maps
    st = ops.begin(txyz, ttri, N)
    try:
        composed, resampled, distortion, subject_searches = [], [], [], []
        for slot, (g, s) in enumerate(order):
            if s == 0:
                ops.set_warp(st, child_corrected[g])
            orig, corrected, tri = children[g]["subjects"][s]
            got = ops.correct(st, slot, corrected, tri, orig, children[g]["data"][s], details)
            composed.append(got[0])
            resampled.append(got[1])
            distortion.append(got[2])
            if details:
                subject_searches.append(dict(correct=got[3]))
        keys = ("mean", "stdev", "cc", "dice", "cc_mean", "dice_mean")
        parent = dict(zip(keys, ops.group_stats_select(st, list(range(N)), mask, float(percentile))))
        children_stats = [dict(zip(keys, ops.group_stats_select(st, [slot for slot, (h, _) in enumerate(order) if h == g], mask, float(percentile))))
                          for g in range(G)]
    finally:
        ops.end(st)
    out = dict(W=W, child_corrected=child_corrected, child_mean=child_mean, child_distortion=child_distortion, composed=composed, resampled=resampled,
               distortion=distortion, children_stats=children_stats, summary=ops.distortion_summary(distortion), order=order, **parent)
    if details:
        out["searches"] = dict(children=child_searches, subjects=subject_searches)
    return out
