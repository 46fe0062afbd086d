// fusion_mplp.hpp -- MPLP over the binary problem of one label step: the definitions of 5.19 at L = 2, the sweeps, their decodes,
// the rounding and the polish of a whole step in one launch of one workgroup (fusion_mplp_kernels.hip), the host side around it (fusion_mplp.cpp).
// What depends on the triplet list alone -- schedule, incidence, colouring -- is a plan, built once and kept on the device.
#pragma once

#include "internal.hpp"
#include "mplp_host.hpp"

namespace msm {

constexpr int kFusionThreads = 512;        // the one workgroup of k_fusion_mplp
constexpr int kFusionMaxSweeps = 1024;     // msm_fusion_mplp_step: sweeps 0 .. 1024, polish 0 .. kMplpMaxPolish
constexpr int kFusionNbr = 7;              // a slot's record lists up to this many other slots of its node (an icosphere's nodes have at most five)
constexpr size_t kFusionLdsBudget = 152 * 1024;  // what the messages may take of the 160 KB beside the kernel's static words

// what a triplet list fixes, host counts and device arrays
struct FusionMplpPlan {
    int N = 0, T = 0, levels = 0, classes = 0;
    DevBuf<int4> sched;          // T records in schedule order: {triplet, node A, node B, node C}
    // 6 T: per schedule position and slot s two words {count, q0, q1, q2} {q3 .. q6} -- the other slots of the slot's node in incidence order, what
    // the cavity of the update adds up; count -1: the node has more than kFusionNbr others and the kernel walks the incidence lists
    DevBuf<int4> nbr;
    DevBuf<int32_t> level_off;   // levels + 1
    DevBuf<int32_t> inc_ptr, inc_slot;   // N + 1, 3 T (MplpIncidence)
    DevBuf<int32_t> triplets;    // T x 3, list order
    DevBuf<int32_t> colour, cls_node, class_off;  // N, N, classes + 1 (MplpColouring)
};
// builds and uploads on the context's stream (the host vectors are consumed on return)
int fusion_mplp_build_plan(msm_ctx *ctx, const int32_t *triplets, int N, int T, FusionMplpPlan &plan);

// Candidate slots: 0 the start x = 0, 1 .. S the decode after each sweep, S + 1 the conditioned decode, S + 2 .. S + 1 + P the polish passes.
// The kernel's one output block, downloaded in one copy:
//   doubles  usum[C], tsum[C]  the two partial sums of a candidate's energy, each from 0.0 in ascending order (the energy is usum + 0.0 + tsum)
//            bsum[max(S, 1)]   the bound after each sweep (without a sweep: of the zero messages): the N node terms, then the T factor terms, from 0.0 in ascending order
//   int32    head[8]           sweeps run, passes run, then 1 where a value is not finite: [2] a message, [3] the unary table, [4] the octets
//   bytes    cand[C][N]        the candidate labellings
struct FusionMplpArgs {
    const double *u2;       // N x 2 (theta_i(x) = u2[2 i + x]); not read where U is given
    const double *octets;   // T x 8
    const int4 *sched, *nbr;
    const int32_t *level_off, *inc_ptr, *inc_slot, *triplets, *colour, *cls_node, *class_off;
    double *m;              // 6 T messages in global memory, or null: they live in LDS
    double *eterms;         // (N + T) x C energy terms: term j of candidate c at fusion_term_index(j, C, c)
    double *bterms;         // (N + T) x max(S, 1) bound terms, likewise
    double *sums;           // the output block's doubles (2 C + max(S, 1))
    int32_t *head;          // its eight words
    uint8_t *cand;          // its C x N bytes
    // gather of u2 from a cost function's unary table (L x N): non-null U takes the place of u2 -- theta_i(0) = U[labeling[i] N + i], theta_i(1) = U[label N + i]
    const double *U;
    const int32_t *labeling;
    double *u2w;            // N x 2: where the gathered theta is kept
    int label, L;
    int N, T, S, P, levels, classes;
    int *status;
};
inline size_t fusion_slots(int S, int P) { return (size_t)S + (size_t)P + 2; }
// Term arrays: blocks of eight terms, a block holding its eight terms column by column -- the threads that write a candidate's terms write whole
// lines, and the thread that sums column c reads one line per eight terms
__host__ __device__ inline size_t fusion_term_index(size_t j, size_t C, size_t c) { return ((j >> 3) * C + c) * 8 + (j & 7); }
inline size_t fusion_term_count(size_t nterms, size_t C) { return ((nterms + 7) >> 3) * C * 8; }
int launch_fusion_mplp(msm_ctx *ctx, const FusionMplpArgs &a, bool lds);

// msm_fusion_mplp_step's checks but for the tables' values (what: the entry point's name)
int fusion_mplp_check(const char *what, const int32_t *triplets, int N, int T, int sweeps, int polish);

// what a step hands back (any but x may be null)
struct FusionMplpOutputs {
    int32_t *x, *sweeps_run, *passes_run;
    double *energy, *bound, *energies, *bounds;
};

// One solve over tables that lie on the device.  fusion_mplp_queue: the launch and, behind it, the copy of its output block, on the context's stream;
// the tables are d_u2 (N x 2), or d_U (L x N) + d_labeling + label for the gather, and d_octets.  The caller synchronises the stream once; then
// fusion_mplp_collect judges what the kernel found in the tables (non-finite values are refused, the unary table first, before anything is written),
// picks the winners by the literal's rule and writes o.  again: the launch repeats the step's solve (stats count it).
int fusion_mplp_queue(msm_ctx *ctx, const char *what, const FusionMplpPlan &plan, const double *d_u2, const double *d_U, const int32_t *d_labeling, int label, int L,
                      const double *d_octets, int sweeps, int polish, bool again);
int fusion_mplp_collect(msm_ctx *ctx, const char *what, const FusionMplpOutputs &o);

}  // namespace msm
