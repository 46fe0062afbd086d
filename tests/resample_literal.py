"""The definitions behind msm_resample_plan_apply / _apply_labels (include/msmhip.h), restated in plain Python over CSR rows.

apply_rows     for row k and map d: acc = 0.0; for the row's entries in stored order, skipping col < 0 and, with a mask, excl[col] == 0:
               acc += float64(data[d][col]) * val (product and sum rounded separately: Python floats are IEEE doubles and never fused); the result is
               stored in the data's dtype (float32: one rounding to nearest even).  A row without kept entries gives 0.
label_vote     for row k, for every distinct key among the kept entries: the sum of val over the entries holding that key, in stored order from 0.0.
               The largest sum wins, an exact tie goes to the smallest key, a row without kept entries gets `unassigned`.  The reference has only
               nearest-vertex for labels; this is the vote `wb_command -label-resample ADAP_BARY_AREA` stands for in the pipelines.
"""
import numpy as np


def _kept(col, excl):
    return col >= 0 and (excl is None or excl[col] != 0)


def apply_rows(rp, col, val, data, excl=None):
    data = np.atleast_2d(np.asarray(data))
    out = np.zeros((data.shape[0], len(rp) - 1), dtype=data.dtype)
    for d in range(data.shape[0]):
        row = [float(x) for x in data[d]]
        for k in range(len(rp) - 1):
            acc = 0.0
            for e in range(rp[k], rp[k + 1]):
                if _kept(col[e], excl):
                    acc += row[col[e]] * float(val[e])
            out[d, k] = acc
    return out


def label_vote(rp, col, val, labels, unassigned=0, excl=None):
    """-> (D x N int32, rows whose winner was decided by the tie rule: two or more keys with exactly the largest sum)"""
    labels = np.atleast_2d(np.asarray(labels))
    out = np.zeros((labels.shape[0], len(rp) - 1), dtype=np.int32)
    tied = 0
    for d in range(labels.shape[0]):
        lab = labels[d]
        for k in range(len(rp) - 1):
            sums = {}
            for e in range(rp[k], rp[k + 1]):
                if _kept(col[e], excl):
                    key = int(lab[col[e]])
                    sums[key] = sums.get(key, 0.0) + float(val[e])
            if not sums:
                out[d, k] = unassigned
                continue
            top = max(sums.values())
            winners = sorted(key for key, s in sums.items() if s == top)
            tied += len(winners) > 1
            out[d, k] = winners[0]
    return out, tied
