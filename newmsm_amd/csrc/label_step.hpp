// label_step.hpp -- what the rest of the cost function's host side sees of the label step (label_step.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

struct msm_cost;

namespace msm {
// Where a step's costs land, in the order of preference: the caller's own array when it is mapped pinned memory of the context (direct), the context's
// mapped io block behind the padded labeling (pin + in_pad; the host copies them out after the kernel), or d_clique_out and a copy command into that
// block (staged_copy).  Kept with a step that is queued ahead.
struct StepDelivery {
    double *out_dev = nullptr;  // what the kernel writes
    void *pin = nullptr;        // the context's pinned io block, where the step takes it
    size_t in_pad = 0, out_bytes = 0;
    bool direct = false, staged_copy = false;
};
// the triplet part of evaluateTotalCostSum by the fused move in its single form (vals: T values); *done: false (vals untouched) where it does not apply
int fused_single_costs(msm_cost *c, const int32_t *labeling, double *vals, bool *done);
}  // namespace msm
