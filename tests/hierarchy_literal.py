"""The literal restatement of the hierarchy stage's additions to the dedrift handle (msm_dedrift_set_warp, msm_dedrift_group_stats_select;
newmsm_amd/hierarchy.py) in numpy over the oracle: dedrift_literal.LiteralOps plus the calls hierarchy.merge_groups makes besides dedrift_group's.  The
yardstick of tests/test_hierarchy_cpu.py and tests/test_gpu_hierarchy.py.

TEST INFRASTRUCTURE: nothing here is imported by the product."""
import numpy as np

from tests import dedrift_literal as L


def select_stats(maps, mask, perc):
    """(mean, stdev, cc, dice, cc_mean, dice_mean) of the listed maps (each D x V): moments over all vertices in list order; cc and dice literally
    numpy.corrcoef and compare_stats.py's dice_overlap on x[mask > 0]; the means over the pairs a < b in the order of compare_stats.py's loops"""
    from newmsm_amd import dedrift

    mean, sd = L.moments(maps)
    keep = np.ones(maps[0].shape[1], dtype=bool) if mask is None else np.asarray(mask) > 0
    assert keep.any()
    cc, dice = L.pair_matrices([m[:, keep] for m in maps], perc)
    return mean, sd, cc, dice, dedrift.pair_means(cc), dedrift.pair_means(dice)


def threshold_gaps(maps, mask=None, perc=75):
    """dedrift_literal.threshold_gaps of the listed maps at the kept vertices (0: a tie, the masks may not be compared).  Where the percentile's
    virtual index (K - 1) perc / 100 is whole the threshold is an order statistic itself, taken without arithmetic by numpy.percentile and by the
    library alike: that value equals its threshold exactly on both sides, which is no tie in the sense meant here, and the gap is infinite."""
    keep = np.ones(np.atleast_2d(maps[0]).shape[1], dtype=bool) if mask is None else np.asarray(mask) > 0
    vidx = (int(keep.sum()) - 1) * (perc / 100.0)
    if vidx == np.floor(vidx):
        return np.inf
    return L.threshold_gaps([np.atleast_2d(m)[:, keep] for m in maps], perc)


class LiteralOps(L.LiteralOps):
    """hierarchy.merge_groups' calls answered by the restatement"""

    def set_warp(self, st, W):
        st["W"] = np.array(W, dtype=np.float64)  # taken as it is

    def group_stats_select(self, st, subjects, mask, percentile):
        return select_stats([st["maps"][s] for s in subjects], mask, percentile)

    def distortion_summary(self, distortions):
        from newmsm_amd import dedrift

        return dedrift.distortion_summary(distortions)
