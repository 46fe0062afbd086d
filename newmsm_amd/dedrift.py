"""Dedrifting and group statistics of a finished groupwise run, over the msm_dedrift_* entry points of the C ABI.

The reference's tutorial pipeline does this with wb_command and nibabel once gMSM has written its spheres
(gMSM_scripts/gMSM_tutorial/gw_MSM.sh:65-128, compare_stats.py); here every stage runs on the GPU and the subjects' resampled maps
stay there until the statistics have been computed.

dedrift_group is written over an `ops` object, like the level loops of registration.py: ProductOps answers its calls from the library,
the tests answer the same calls from a literal numpy restatement (tests/dedrift_literal.py) and compare.

Definitions.  Per subject s: M_s its input sphere as the run used it, R_s its registered sphere (same
triangles), F_s its data; T the template.
  inverse_s    for every vertex of T its closest triangle of R_s and the barycentric weights there, applied to M_s (not normalised).  The
               tutorial script hands the template to wb_command as the sphere to unproject to: the same thing exactly when M_s is the
               template, which is its situation; M_s is the general form.
  drift        sum of inverse_s over s = 0 .. S - 1, in that order, divided by S
  W            drift minus the midpoint of its bounding box, every vertex scaled to length 100 (the dedrift warp)
  corrected_s  sphere_project_warp(R_s, T, W)
  resampled_s  metric_resample of F_s from corrected_s onto T (adaptive barycentric)
  distortion_s row 0 / row 1: per vertex the mean over its triangles of log2 J / log2 R of triangle_strain, M_s against corrected_s
  mean, stdev  over the subjects, population form; cc, dice: pairwise Pearson correlation / overlap of the masks above a percentile
"""
import ctypes as C

import numpy as np

from . import api
from ._lib import MsmError, c_dp, c_ip, check, lib


class Dedrift:
    """msm_dedrift: the handle of one group on one template (api.Mesh)."""

    def __init__(self, ctx, template, num_subjects):
        self.ctx, self.template, self.S = ctx, template, int(num_subjects)
        self.Vt = template.V
        self.D = 0
        self.h = lib().msm_dedrift_create(ctx.h, template.h, self.S)
        if not self.h:
            raise MsmError(-1, lib().msm_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            lib().msm_dedrift_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def reset(self):
        check(lib().msm_dedrift_reset(self.h))
        self.D = 0

    def accumulate(self, reg_mesh, orig_xyz, details=False):
        """one subject's inverse added to the running sum; with details: dict(tri, w, inverse) of the search and the inverse itself"""
        x, px = api._soa(orig_xyz)
        if not details:
            check(lib().msm_dedrift_accumulate(self.h, reg_mesh.h, px, x.shape[1], None, None, None))
            return None
        tri = np.zeros(self.Vt, dtype=np.int32)
        w, inv = np.zeros((3, self.Vt)), np.zeros((3, self.Vt))
        check(lib().msm_dedrift_accumulate(self.h, reg_mesh.h, px, x.shape[1], tri.ctypes.data_as(c_ip), w.ctypes.data_as(c_dp), inv.ctypes.data_as(c_dp)))
        return dict(tri=tri, w=np.ascontiguousarray(w.T), inverse=np.ascontiguousarray(inv.T))

    def finish(self):
        """(W, drift), each (V(T), 3)"""
        W, drift = np.zeros((3, self.Vt)), np.zeros((3, self.Vt))
        check(lib().msm_dedrift_finish(self.h, W.ctypes.data_as(c_dp), drift.ctypes.data_as(c_dp)))
        return np.ascontiguousarray(W.T), np.ascontiguousarray(drift.T)

    def correct(self, subject, reg_mesh, orig_xyz, data, details=False):
        """(corrected (V, 3), resampled (D, V(T)), distortion (2, V)) and, with details, dict(tri, w) of the search of R_s on T; reg_mesh holds
        corrected_s afterwards"""
        x, px = api._soa(orig_xyz)
        f, pf = api._d(np.atleast_2d(data))
        V, D = x.shape[1], f.shape[0]
        assert f.shape[1] == V
        corrected, resampled, distortion = np.zeros((3, V)), np.zeros((D, self.Vt)), np.zeros((2, V))
        tri, w = (np.zeros(V, dtype=np.int32), np.zeros((3, V))) if details else (None, None)
        check(lib().msm_dedrift_correct(self.h, int(subject), reg_mesh.h, px, V, pf, D, corrected.ctypes.data_as(c_dp), resampled.ctypes.data_as(c_dp),
                                        distortion.ctypes.data_as(c_dp), tri.ctypes.data_as(c_ip) if details else None,
                                        w.ctypes.data_as(c_dp) if details else None))
        self.D = D
        out = (np.ascontiguousarray(corrected.T), resampled, distortion)
        return out + (dict(tri=tri, w=np.ascontiguousarray(w.T)),) if details else out

    def set_map(self, subject, data):
        f, pf = api._d(np.atleast_2d(data))
        assert f.shape[1] == self.Vt
        check(lib().msm_dedrift_set_map(self.h, int(subject), pf, f.shape[0]))
        self.D = f.shape[0]

    def group_stats(self, percentile=75.0):
        """(mean, stdev (D, V(T)), cc, dice (D, S, S))"""
        D, S = self.D, self.S
        mean, stdev = np.zeros((D, self.Vt)), np.zeros((D, self.Vt))
        cc, dice = np.zeros((D, S, S)), np.zeros((D, S, S))
        check(lib().msm_dedrift_group_stats(self.h, C.c_double(float(percentile)), mean.ctypes.data_as(c_dp), stdev.ctypes.data_as(c_dp),
                                            cc.ctypes.data_as(c_dp), dice.ctypes.data_as(c_dp)))
        return mean, stdev, cc, dice

    def set_warp(self, W):
        """msm_dedrift_set_warp: W (V(T), 3), a deformation of the template's vertices, replaces the handle's warp as it is; correct may follow"""
        w, pw = api._soa(W)
        assert w.shape[1] == self.Vt
        check(lib().msm_dedrift_set_warp(self.h, pw))

    def group_stats_select(self, subjects, mask=None, percentile=75.0):
        """msm_dedrift_group_stats_select: (mean, stdev (D, V(T)), cc, dice (D, n, n), cc_mean, dice_mean (D)) over the listed resident subjects, in the
        list's order, and the vertices with mask > 0 (None: all)"""
        idx = np.ascontiguousarray(np.asarray(subjects, dtype=np.int32).ravel())
        D, n = self.D, len(idx)
        pm = None
        if mask is not None:
            m, pm = api._d(np.asarray(mask, dtype=np.float64).ravel())
            assert m.size == self.Vt
        mean, stdev = np.zeros((D, self.Vt)), np.zeros((D, self.Vt))
        cc, dice = np.zeros((D, n, n)), np.zeros((D, n, n))
        cc_mean, dice_mean = np.zeros(D), np.zeros(D)
        check(lib().msm_dedrift_group_stats_select(self.h, idx.ctypes.data_as(c_ip), n, pm, C.c_double(float(percentile)), mean.ctypes.data_as(c_dp),
                                                   stdev.ctypes.data_as(c_dp), cc.ctypes.data_as(c_dp), dice.ctypes.data_as(c_dp),
                                                   cc_mean.ctypes.data_as(c_dp), dice_mean.ctypes.data_as(c_dp)))
        return mean, stdev, cc, dice, cc_mean, dice_mean


class ProductOps:
    """The calls of dedrift_group answered by libmsmhip.  The subjects' registered spheres are kept as mesh handles from accumulate to correct."""

    def __init__(self, ctx, prepare_search=False):
        self.ctx, self.prepare_search = ctx, prepare_search

    def begin(self, template_xyz, template_tri, num_subjects):
        tmpl = api.Mesh(self.ctx, template_xyz, template_tri)
        return dict(tmpl=tmpl, d=Dedrift(self.ctx, tmpl, num_subjects), reg={})

    def accumulate(self, st, s, reg_xyz, tri, orig_xyz, details):
        m = api.Mesh(self.ctx, reg_xyz, tri)
        if self.prepare_search:
            m.prepare_search(wait=True)  # the direction table: pays from many searches per target on, results are the same either way
        st["reg"][s] = m
        return st["d"].accumulate(m, orig_xyz, details)

    def finish(self, st):
        return st["d"].finish()

    def correct(self, st, s, reg_xyz, tri, orig_xyz, data, details):
        m = st["reg"].pop(s, None) or api.Mesh(self.ctx, reg_xyz, tri)
        try:
            return st["d"].correct(s, m, orig_xyz, data, details)
        finally:
            m.close()

    def set_map(self, st, s, data):
        st["d"].set_map(s, data)

    def group_stats(self, st, percentile):
        return st["d"].group_stats(percentile)

    def set_warp(self, st, W):
        st["d"].set_warp(W)

    def group_stats_select(self, st, subjects, mask, percentile):
        return st["d"].group_stats_select(subjects, mask, percentile)

    def distortion_summary(self, distortions):
        """distortion_summary's figures through msm_abs_summary"""
        areal = np.concatenate([np.asarray(d)[0].ravel() for d in distortions])
        shape = np.concatenate([np.asarray(d)[1].ravel() for d in distortions])
        a_mean, a_max, a_p = api.abs_summary(self.ctx, areal, (95.0, 98.0))
        s_mean, s_max, _ = api.abs_summary(self.ctx, shape)
        return dict(areal_mean=a_mean, areal_max=a_max, areal_95=float(a_p[0]), areal_98=float(a_p[1]), shape_mean=s_mean, shape_max=s_max)

    def end(self, st):
        st["d"].close()
        st["tmpl"].close()


def pair_means(mat):
    """the mean over the S (S - 1) / 2 pairs i < j of every (S, S) matrix of mat (D, S, S), summed in the order of compare_stats.py's loops"""
    mat = np.asarray(mat)
    D, S = mat.shape[0], mat.shape[1]
    out = np.zeros(D)
    for d in range(D):
        acc = 0.0
        for i in range(S):
            for j in range(i + 1, S):
                acc += float(mat[d, i, j])
        out[d] = acc / (S * (S - 1) / 2) if S > 1 else float("nan")
    return out


def distortion_summary(distortions):
    """compare_stats.py:71-105 over |values| of all subjects' distortion maps: areal mean, max, 95th and 98th percentile; shape mean and max"""
    areal = np.abs(np.concatenate([np.asarray(d)[0].ravel() for d in distortions]))
    shape = np.abs(np.concatenate([np.asarray(d)[1].ravel() for d in distortions]))
    return dict(areal_mean=float(np.mean(areal)), areal_max=float(np.max(areal)), areal_95=float(np.percentile(areal, 95)),
                areal_98=float(np.percentile(areal, 98)), shape_mean=float(np.mean(shape)), shape_max=float(np.max(shape)))


def format_stats(title, names, cc_mean, dice_mean, summary=None):
    """one block in compare_stats.py's wording (:107-119)"""
    lines = ["\tStats for group " + title]
    for d, name in enumerate(names):
        lines.append("\t" + name)
        lines.append("\t\tCC similarity: {:.4}; Dice overlap: {:.4}".format(float(cc_mean[d]), float(dice_mean[d])))
    if summary is not None:
        lines.append("\tDistortion")
        lines.append("\t\tAreal mean: {:.4}; Areal Max: {:.4}; Areal 95%: {:.4}; Areal 98%: {:.4}; Shape mean: {:.4}; Shape Max: {:.4}".format(
            summary["areal_mean"], summary["areal_max"], summary["areal_95"], summary["areal_98"], summary["shape_mean"], summary["shape_max"]))
    return "\n".join(lines) + "\n"


def dedrift_group(ops, template, subjects, data, percentile=75, details=False):
    """Dedrifts a finished groupwise run and computes its group statistics.

    ops        a Context (the library answers) or an ops object (ProductOps, or the tests' literal restatement)
    template   (xyz (V(T), 3), tri) of the template sphere
    subjects   per subject (orig_xyz, reg_xyz, tri): its input sphere as the run used it, its registered sphere, their triangles
    data       per subject its D x V_s data
    Returns a dict: W, drift, corrected / resampled / distortion (lists over the subjects), mean, stdev, cc, dice, cc_mean, dice_mean (per feature,
    over the pairs i < j), summary (distortion_summary) and, with details, searches: per subject dict(accumulate=dict(tri, w, inverse), correct=dict(tri, w)),
    the decisions of both searches and the subject's inverse.
    """
    if not hasattr(ops, "accumulate"):
        ops = ProductOps(ops)
    txyz, ttri = template
    S = len(subjects)
    assert S == len(data) and S >= 1
    st = ops.begin(np.asarray(txyz, dtype=np.float64), np.asarray(ttri, dtype=np.int32), S)
    try:
        searches = []
        for s, (orig, reg, tri) in enumerate(subjects):  # subject order: the order of the additions
            searches.append(dict(accumulate=ops.accumulate(st, s, reg, tri, orig, details)))
        W, drift = ops.finish(st)
        corrected, resampled, distortion = [], [], []
        for s, (orig, reg, tri) in enumerate(subjects):
            got = ops.correct(st, s, reg, tri, orig, data[s], details)
            corrected.append(got[0])
            resampled.append(got[1])
            distortion.append(got[2])
            if details:
                searches[s]["correct"] = got[3]
        mean, stdev, cc, dice = ops.group_stats(st, float(percentile))
    finally:
        ops.end(st)
    out = dict(W=W, drift=drift, corrected=corrected, resampled=resampled, distortion=distortion, mean=mean, stdev=stdev, cc=cc, dice=dice,
               cc_mean=pair_means(cc), dice_mean=pair_means(dice), summary=distortion_summary(distortion))
    if details:
        out["searches"] = searches
    return out


def pairwise_stats(ops, template, maps, percentile=75):
    """cc / dice (and their pair means) of maps that are on the template already (per subject D x V(T)): the `before` figures of a run"""
    if not hasattr(ops, "accumulate"):
        ops = ProductOps(ops)
    txyz, ttri = template
    st = ops.begin(np.asarray(txyz, dtype=np.float64), np.asarray(ttri, dtype=np.int32), len(maps))
    try:
        for s, m in enumerate(maps):
            ops.set_map(st, s, m)
        mean, stdev, cc, dice = ops.group_stats(st, float(percentile))
    finally:
        ops.end(st)
    return dict(mean=mean, stdev=stdev, cc=cc, dice=dice, cc_mean=pair_means(cc), dice_mean=pair_means(dice))
