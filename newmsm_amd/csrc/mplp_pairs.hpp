// mplp_pairs.hpp -- MPLP over the pair tables on the GPU: the kernels' arguments (mplp_pairs_kernels.hip) and the host loops around
// them (mplp_pairs.cpp).  The definition, the colourings and the serial literal are plain host code: mplp_pairs_host.hpp.
#pragma once

#include "mplp.hpp"
#include "mplp_pairs_host.hpp"

namespace msm {

constexpr int kMplpPairWaveLabels = 64;  // up to here a wavefront updates a pair, lane a holding column a; above, a workgroup of four wavefronts does

struct MplpPairArgs {
    const double *U;          // L x N
    const double *pc;         // P x L x L, theta_p(a, b) at (p L + b) L + a
    const int32_t *pairs;     // 2 P nodes in list order
    const int32_t *sched;     // the P pairs class by class (MplpColouring::node of mplp_pairs_colour_pairs)
    const int32_t *inc_ptr;   // N + 1
    const int32_t *inc_slot;  // 2 P slots (2 p + s), a node's ascending
    double *m;                // P x 2 x L messages
    int32_t *changed;         // a word per sweep: raised to 1 by a message whose bits the sweep changed
    int N, L, P;
    int *status;
};

// one pair class of sweep `sweep`: the pairs sched[begin .. begin + count).  The whole launch returns at once when the sweep before left every
// message as it was (changed[sweep - 1] == 0).
int launch_mplp_pair_update(msm_ctx *ctx, const MplpPairArgs &a, int begin, int count, int sweep);
// beliefs and decode, a wavefront per node: label[i] (may be null) and node_terms[i] = min_x b_i(x)
int launch_mplp_pair_decode(msm_ctx *ctx, const MplpPairArgs &a, int32_t *label, double *node_terms);
// the pair terms of the bound after sweep `sweep` (sweep < 0: unconditional), factor_terms[p]
int launch_mplp_pair_factor_terms(msm_ctx *ctx, const MplpPairArgs &a, double *factor_terms, int sweep);
// the N + P energy terms of `labeling`, a thread per term
int launch_mplp_pair_energy_terms(msm_ctx *ctx, const MplpPairArgs &a, const int32_t *labeling, double *terms);

struct MplpPairPolishArgs {
    const double *U, *pc;
    const int32_t *pairs, *inc_ptr, *inc_slot;
    const int32_t *cls_node;  // N nodes class by class (mplp_pairs_colour_nodes)
    int32_t *lab;             // N: the labelling being walked
    int32_t *changed;         // a word per pass: raised to 1 by a label the pass changed
    int N, L, P;
    int *status;
};
// polish pass `pass` over the node class cls_node[begin .. begin + count), a wavefront per node; returns at once when pass - 1 changed no label
int launch_mplp_pair_polish(msm_ctx *ctx, const MplpPairPolishArgs &a, int begin, int count, int pass);

// the checks every route shares, tables not looked at (what: the entry point's name in the MPLP-specific refusals)
int mplp_pairs_check_arguments(const char *what, const int32_t *pairs, int N, int L, int P, int sweeps, const int32_t *labeling);
// The sweeps over tables that lie on the device (d_U: L x N, d_pc: P x L x L), arguments checked by the caller: the finiteness refusal first
// (k_mplp_classify; *inspected says the tables have passed it already and is set), then the sweeps.  Complete on return; the outputs are written only
// when the call succeeds.
int mplp_pairs_run_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_pc, const int32_t *pairs, int N, int L, int P, int sweeps,
                          const MplpOutputs &o, bool *inspected);
// the polish over such tables (o.energies: 1 + polish values)
int mplp_pairs_polish_device(msm_ctx *ctx, const char *what, const double *d_U, const double *d_pc, const int32_t *pairs, int N, int L, int P, int polish,
                             const MplpRoundOutputs &o, bool *inspected);

}  // namespace msm
