"""The rows of a smoothing plan (msm_resample_plan_create_smooth, include/msmhip.h) and their apply, written out plainly: the definition the GPU tests
compare with.  smooth_data, R/resampler.cpp:168-230, as a sparse row operator.

Row i, with c = cv[i] the centre's id on sphLow: the vertices n with (unit[n] | unit[c]) >= cos(4 asin(sigma / 2R)), ascending n; the stored weight is
gain * exp(-g^2 / (2 sigma^2)), g = 2R asin(|unit[c] - unit[n]| / 2R), gain = 1 / sqrt(2 pi sigma^2), times excl[n] with a mask.  div = the sum of the
stored weights, excl_out = div / (the sum of the unmasked weights), both in stored order from 0.0.  A centre with excl[c] <= 0 has an empty row.

asin, exp, sqrt and cos are math's (the C library's, which the oracle calls too); the membership test is evaluated for all n at once with numpy, whose
elementwise products and sums are the same IEEE operations in the same order."""
import math

import numpy as np

RAD = 100.0


def unit_vectors(xyz):
    """Point::normalize, R/point.cpp:26-34"""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    n = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    n = np.where(n > 1e-8, n, 1.0)
    return x / n[:, None]


def rows(xyz_low, sigma, cv, excl=None):
    """-> (row_ptr int32 N + 1, col int32, val, div N, excl_out N or None)"""
    u = unit_vectors(xyz_low)
    N = len(u)
    cosang = math.cos(4 * math.asin(sigma / (2 * RAD)))
    gain = 1 / math.sqrt(2 * math.pi * sigma * sigma)
    row_ptr, col, val = np.zeros(N + 1, dtype=np.int32), [], []
    div, excl_out = np.zeros(N), (np.zeros(N) if excl is not None else None)
    for i in range(N):
        c = int(cv[i])
        assert 0 <= c < N
        if excl is None or excl[c] > 0:
            ref = u[c]
            members = np.nonzero(u[:, 0] * ref[0] + u[:, 1] * ref[1] + u[:, 2] * ref[2] >= cosang)[0]
            SUM, excl_sum = 0.0, 0.0
            for n in members:
                dx, dy, dz = float(ref[0] - u[n, 0]), float(ref[1] - u[n, 1]), float(ref[2] - u[n, 2])
                chord = math.sqrt(dx * dx + dy * dy + dz * dz)
                g = 2 * RAD * math.asin(chord / (2 * RAD))
                w = gain * math.exp(-(g * g) / (2 * sigma * sigma))
                excl_sum += w
                if excl is not None:
                    w = float(excl[n]) * w
                SUM += w
                col.append(int(n))
                val.append(w)
            div[i] = SUM
            if excl is not None and excl_sum != 0.0:
                excl_out[i] = SUM / excl_sum
        row_ptr[i + 1] = len(col)
    return row_ptr, np.array(col, dtype=np.int32), np.array(val, dtype=np.float64), div, excl_out


def apply(row_ptr, col, val, div, data):
    """D x V_in -> D x V_out of data's dtype: acc = 0.0; acc += (double)data[d][col] * val in stored order; acc / div where div != 0.0; one rounding.
    All rows advance together, entry by entry: each row's own sum keeps its stored order."""
    d = np.atleast_2d(np.asarray(data))
    wide = d.astype(np.float64)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    length = np.diff(row_ptr)
    acc = np.zeros((d.shape[0], len(length)))
    for j in range(int(length.max()) if len(length) else 0):
        k = np.nonzero(length > j)[0]
        e = row_ptr[k] + j
        acc[:, k] += wide[:, col[e]] * val[e]
    k = np.nonzero(np.asarray(div) != 0.0)[0]
    acc[:, k] = acc[:, k] / np.asarray(div)[k]
    return acc.astype(d.dtype)
