"""The histogram matching of --IN / --INc restated in plain numpy, statement by statement after the five steps of DESIGN.md section 5.11 (the
definition; multivariate_histogram_normalization, M/reg_tools.cpp:745-802, hands the matching itself to FSL's MISCMATHS::Histogram, which is not in
the reference tree: this restates generate / generateCDF / match from their documented behaviour, and agreement with FSL is unpinned).  Uses nothing
from the oracle.  Shared by tests/test_histmatch_cpu.py and tests/test_gpu_histmatch.py; LiteralMatchMixin adds the call the level loops make to any
ops object."""
import numpy as np

B = 256  # numbins, M/reg_tools.cpp:756


def mask_row(mask, d, n):
    """row d of the mask when it has that many rows, else row 0 (:764-767); all ones without a mask"""
    if mask is None:
        return np.ones(n)
    m = np.atleast_2d(np.asarray(mask, dtype=np.float64))
    return m[d] if m.shape[0] >= d + 1 else m[0]


def bins_of(v, lo, w):
    """step 2 for an array of finite values"""
    return np.minimum(np.maximum(((v - lo) / w).astype(np.int64) + 1, 1), B)


def match_row(x, mx, y, my):
    """one feature row: returns (the matched copy of x, the table t[1..B] or None when the row is left unchanged)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = x.copy()
    fx, fy = np.isfinite(x), np.isfinite(y)
    with np.errstate(invalid="ignore"):
        cx, cy = fx & (mx > 0), fy & (my > 0)  # counted: finite and mask > 0
    # 1. range: over all finite values, masked or not
    if not cx.any() or not cy.any():
        return out, None
    lo_x, hi_x = x[fx].min(), x[fx].max()
    lo_y, hi_y = y[fy].min(), y[fy].max()
    if hi_x == lo_x or hi_y == lo_y:
        return out, None
    # 2. bins
    w_x = (hi_x - lo_x) / B
    w_y = (hi_y - lo_y) / B
    bin_x = bins_of(x[cx], lo_x, w_x)
    bin_y = bins_of(y[cy], lo_y, w_y)
    # 3. counts and CDFs: an exact integer sum, one division
    h_x = np.bincount(bin_x, minlength=B + 1)[1:]
    h_y = np.bincount(bin_y, minlength=B + 1)[1:]
    n_x, n_y = int(h_x.sum()), int(h_y.sum())
    cdf_x = np.cumsum(h_x).astype(np.float64) / float(n_x)
    cdf_y = np.cumsum(h_y).astype(np.float64) / float(n_y)
    # 4. table
    t = np.zeros(B)
    for b in range(1, B + 1):
        c = cdf_x[b - 1]
        if b == B:
            newbin, dist = B, 0.0
        else:
            newbin = 1
            while not cdf_y[newbin - 1] >= c:  # the smallest j with CDF_y[j] >= c
                newbin += 1
            if newbin > 1:
                dist = (c - cdf_y[newbin - 2]) / (cdf_y[newbin - 1] - cdf_y[newbin - 2])
            else:
                dist = 0.0
        v = lo_y + (newbin - 1) * w_y + dist * w_y
        t[b - 1] = min(max(v, lo_y), hi_y)
    # 5. application
    out[cx] = t[bin_x - 1]
    return out, t


def histogram_match(src, ref, src_excl=None, ref_excl=None):
    """src D x Vs matched to ref D x Vt row by row; masks: rows x V or V or None"""
    src, ref = np.atleast_2d(np.asarray(src, dtype=np.float64)), np.atleast_2d(np.asarray(ref, dtype=np.float64))
    out = np.empty_like(src)
    for d in range(src.shape[0]):
        out[d] = match_row(src[d], mask_row(src_excl, d, src.shape[1]), ref[d], mask_row(ref_excl, d, ref.shape[1]))[0]
    return out


class LiteralMatchMixin:
    """ops.histogram_match as the level loops call it, from the literal; records every call (sources, target, masks as given) in self.match_calls"""

    def histogram_match(self, srcs, ref, src_excls=None, ref_excl=None):
        if not hasattr(self, "match_calls"):
            self.match_calls = []
        self.match_calls.append(([np.array(s) for s in srcs], np.array(ref), None if src_excls is None else [np.array(m) for m in src_excls],
                                 None if ref_excl is None else np.array(ref_excl)))
        return [histogram_match(s, ref, None if src_excls is None else src_excls[k], ref_excl) for k, s in enumerate(srcs)]
