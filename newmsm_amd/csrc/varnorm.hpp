// varnorm.hpp -- the row body of variance_normalise (M/reg_tools.cpp:804-843), shared by msm_variance_normalise (regtools.cpp: a section per matrix)
// and msm_level_features (features.cpp: one section over the rows of all data sets).  Host only; no handle, no device.
#pragma once

#include <cmath>
#include <cstddef>

#include "host_parallel.hpp"

namespace msm {

// one feature row of V values in place; excl (V values, > 0 keeps the vertex) or nullptr.  The running mean / variance recurrence is serial:
// a division per value (:820-825).
inline void variance_normalise_row(double *row, int V, const double *excl) {
    double mean = 0.0, var = 0.0;
    size_t n = 0;
    for (int i = 0; i < V; ++i) {
        if (excl && !(excl[i] > 0.0)) continue;
        const double delta = row[i] - mean;
        mean += delta / (double)(n + 1);
        var += delta * (row[i] - mean);
        ++n;
    }
    var /= (double)(n - 1);  // unsigned, as _data[i].size() - 1 at :829
    const double sd = std::sqrt(var);
    for (int i = 0; i < V; ++i) {
        if (excl && !(excl[i] > 0.0)) continue;
        row[i] -= mean;
        if (var > 0.0) row[i] /= sd;
    }
}

// variance_normalise of every row of n matrices (D x V each, one after another) in ONE parallel section over the n x D rows; mask: n x V (matrix i
// under row i) or nullptr.  Fewer than four rows run on the calling thread, as a matrix of fewer than four rows does in msm_variance_normalise.
inline void variance_normalise_rows(double *feat, int n, int D, int V, const double *mask) {
    const int rows = n * D;
    parallel_chunks(rows, rows >= 4 ? host_workers() : 1, [&](int, int r_begin, int r_end) {
        for (int r = r_begin; r < r_end; ++r) variance_normalise_row(feat + (size_t)r * V, V, mask ? mask + (size_t)(r / D) * V : nullptr);
    });
}

}  // namespace msm
