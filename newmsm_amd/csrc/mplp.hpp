// mplp.hpp -- the MPLP optimiser's sweeps on the GPU: the kernels' arguments, the reading of the tables that every route judges the same
// way (MplpReading, mplp_judge) and the host loops around the kernels (mplp.cpp, mplp_kernels.hip).  The definition, the incidence lists and the serial
// literal are plain host code: mplp_host.hpp.
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
// How the tables are read and what an inspection of them found: handed from the sweeps to the rounding that follows them over the same tables, so that
// the tables are inspected once.  forbid: the forbidden-entry reading (DESIGN.md 5.19 "Forbidden entries"), the plain one otherwise.
struct MplpReading {
    bool forbid;
    bool inspected = false;             // counts and F hold what a pass over the tables found, and the reading does not refuse them
    int64_t counts[4] = {0, 0, 0, 0};   // mplp_classify's
    bool F = false;                     // the tables call for the forbidden-aware code (never under the plain reading)
    const char *table = "triplet";      // what the plain reading's refusal calls the factor table ("pair": mplp_pairs.cpp)
    explicit MplpReading(bool forbid_) : forbid(forbid_) {}
};
// The one judgement of counted tables, and of the counted messages of mode 0 (mc; null: none), under either reading: a refusal, or MSM_OK with
// r.inspected and r.F set and *F = whether the tables or the messages call for the forbidden-aware code.
int mplp_judge(const char *what, MplpReading &r, const int64_t *mc, bool *F);

// the device messages the context's last mplp_run_device left (T x 3 x L; null before the first run)
const double *mplp_last_messages(msm_ctx *ctx);
// The rounding over tables that lie on the device, arguments checked by the caller.  d_m: the device messages of mode 0 (null: all zero; mode 1 reads
// none).  r: the reading; where a run has inspected these tables already no pass over them is launched, and nothing at all where there are no messages
// to inspect either; otherwise the inspection fills r.  Complete on return; the outputs are written only when the call succeeds.
int mplp_round_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_tc, const double *d_m, const int32_t *triplets, int N, int L, int T,
                      int mode, int polish, const MplpRoundOutputs &o, MplpReading &r);

// the host optimiser's checks, with its messages (what: the entry point's name for the MPLP-specific refusals); the tables are not looked at
int mplp_check_arguments(const char *what, const int32_t *triplets, int N, int L, int T, int sweeps, const int32_t *labeling);
// MPLP over tables that lie on the device (d_U: L x N, d_tc: T x L^3), arguments checked by the caller: the inspection first (k_mplp_classify, judged
// under r.forbid; r leaves with the counts), then the sweeps, with the forbidden-aware kernels where r.F.  Complete on return; the outputs are written
// only when the call succeeds.
int mplp_run_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_tc, const int32_t *triplets, int N, int L, int T, int sweeps,
                    const MplpOutputs &o, MplpReading &r);

}  // namespace msm
