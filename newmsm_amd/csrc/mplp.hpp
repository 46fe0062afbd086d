// mplp.hpp -- the MPLP optimiser's sweeps on the GPU: the kernels' arguments and the host loop around them (mplp.cpp,
// mplp_kernels.hip).  The definition, the incidence lists and the serial literal are plain host code: mplp_host.hpp.
#pragma once

#include "internal.hpp"
#include "mcmc.hpp"
#include "mplp_host.hpp"

namespace msm {

constexpr int kMplpThreads = 256;  // the workgroup of a factor (update, bound term)

struct MplpArgs {
    const double *U;          // L x N
    const double *tc;         // T x L^3
    const int4 *sched;        // T records in schedule order: {triplet, node A, node B, node C} (McmcArgs::sched)
    const int32_t *inc_ptr;   // N + 1
    const int32_t *inc_slot;  // 3 T slots (3 t + s), a node's ascending
    double *m;                // T x 3 x L messages
    int32_t *changed;         // a word per sweep: raised to 1 by a message whose bits the sweep changed
    int N, L, T;
    int *status;
};

// one level of sweep `sweep`: a workgroup per factor sched[begin .. begin + count).  The whole launch returns at once when the sweep before left every
// message as it was (changed[sweep - 1] == 0): a run past its fixed point costs launches and nothing else.
// forbid (here and below): the instantiation that reads NaN / +inf table entries as forbidden combinations (DESIGN.md 5.19 "Forbidden entries")
int launch_mplp_update(msm_ctx *ctx, const MplpArgs &a, int begin, int count, int sweep, bool forbid = false);
// beliefs and decode, a wavefront per node: label[i] (may be null) and node_terms[i] = min_x b_i(x)
int launch_mplp_decode(msm_ctx *ctx, const MplpArgs &a, int32_t *label, double *node_terms);
// the factor terms of the bound after sweep `sweep`, a workgroup per factor, factor_terms[t]; returns at once where the update of that sweep did (the
// host repeats the previous sweep's bound).  sweep < 0: unconditional.
int launch_mplp_factor_terms(msm_ctx *ctx, const MplpArgs &a, double *factor_terms, int sweep, bool forbid = false);
// flags[0] / flags[1] raised to 1 by a non-finite entry of the unary / triplet table
int launch_mplp_finite(msm_ctx *ctx, const double *U, size_t nU, const double *tc, size_t ntc, int32_t *flags);
// adds to counts[0] the non-finite entries of U and to counts[1..3] the NaN / +inf / -inf entries of tc (either may be null with n = 0)
int launch_mplp_classify(msm_ctx *ctx, const double *U, size_t nU, const double *tc, size_t ntc, unsigned long long *counts);

// The rounding (DESIGN.md 5.19 "Rounding"; the literal: mplp_round_host).
struct MplpRoundArgs {
    const double *U;           // L x N
    const double *tc;          // T x L^3
    const double *m;           // T x 3 x L messages, or null: all zero
    const int4 *tri;           // T records in list order: {triplet, node A, node B, node C}
    const int32_t *inc_ptr;    // N + 1
    const int32_t *inc_slot;   // 3 T
    const int32_t *colour;     // N (MplpColouring::colour)
    const int32_t *cls_node;   // N nodes class by class (MplpColouring::node)
    int32_t *lab;              // N: the labelling being walked
    int32_t *changed;          // a word per polish pass: raised to 1 by a label the pass changed
    int N, L, T;
    int *status;
};
// the conditioned decode of the class cls_node[begin .. begin + count) at `frontier`: a workgroup per node
int launch_mplp_round(msm_ctx *ctx, const MplpRoundArgs &a, int begin, int count, int frontier, bool forbid = false);
// polish pass `pass` over that class, a wavefront per node; the whole launch returns at once when pass - 1 changed no label
int launch_mplp_polish(msm_ctx *ctx, const MplpRoundArgs &a, int begin, int count, int pass, bool forbid = false);
int mplp_update_slots(int L);

// the checks of msm_mplp_round besides mplp_check_arguments: the mode, the polish count, the label count
int mplp_round_check(const char *what, int L, int mode, int polish);
// The rounding over tables that lie on the device, arguments checked by the caller.  d_m: the device messages of mode 0 (null: all zero; use_scratch_m:
// the messages the context's last mplp_run_device left).  check_tables: look for non-finite table entries first (the messages of mode 0 always are).
// Complete on return; the outputs are written only when the call succeeds.  forbid: the forbidden-entry reading (DESIGN.md 5.19 "Forbidden entries") --
// the tables and the messages are classified instead, and counts[4] (may be null) receives the tables' counts; with check_tables false counts hands in
// what the caller's mplp_run_device counted over these tables.
int mplp_round_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_tc, const double *d_m, bool use_scratch_m, bool check_tables,
                      const int32_t *triplets, int N, int L, int T, int mode, int polish, const MplpRoundOutputs &o,
                      bool forbid = false, int64_t *counts = nullptr);

// the host optimiser's checks, with its messages (what: the entry point's name for the MPLP-specific refusals); the tables are not looked at
int mplp_check_arguments(const char *what, const int32_t *triplets, int N, int L, int T, int sweeps, const int32_t *labeling);
// MPLP over tables that lie on the device (d_U: L x N, d_tc: T x L^3), arguments checked by the caller: the finiteness pass first, then the sweeps.
// Complete on return; the outputs are written only when the call succeeds.  forbid: k_mplp_classify instead of the finiteness pass, its four counts to
// counts (may be null), and the forbidden-aware kernels where the triplet table holds a NaN or +inf.
int mplp_run_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_tc, const int32_t *triplets, int N, int L, int T, int sweeps,
                    const MplpOutputs &o, bool forbid = false, int64_t *counts = nullptr);

}  // namespace msm
