// mplp_pairs_host.hpp -- MPLP over the unary table and the pair table of a --regoption=1 level, the part that is plain host C++ (no
// HIP header): the incidence lists over pair slots, the colouring of the pairs a sweep walks and of the nodes a polish pass walks, the serial literal
// msm_mplp_pairs_optimise runs and the GPU entry points reproduce bit for bit, and the polish.  The factors are edges, so the dual is the standard
// pairwise LP relaxation's and the update the published one for factors of two variables (Globerson & Jaakkola, NIPS 2007).  What 5.19
// defines for any factor size -- node sums over an incidence, the decode, the winner, the stop -- is taken from mplp_host.hpp as it is.
#pragma once

#include "mplp_host.hpp"

namespace msm {

// Slot s of pair p is number 2 p + s.  The incidence of node i: the slots that lie on it, ascending (MplpIncidence, with 2 P slots).
inline void mplp_pairs_build_incidence(const int32_t *pairs, int N, int P, MplpIncidence &inc) {
    inc.ptr.assign((size_t)N + 1, 0);
    inc.slot.assign(2 * (size_t)P, 0);
    for (size_t q = 0; q < 2 * (size_t)P; ++q) ++inc.ptr[(size_t)pairs[q] + 1];
    for (int i = 0; i < N; ++i) inc.ptr[(size_t)i + 1] += inc.ptr[(size_t)i];
    std::vector<int32_t> fill(inc.ptr.begin(), inc.ptr.end() - 1);
    for (size_t q = 0; q < 2 * (size_t)P; ++q) inc.slot[(size_t)fill[(size_t)pairs[q]]++] = (int32_t)q;  // ascending (p, s)
}

// the first pair that names one node twice, or -1
inline int mplp_pairs_first_loop(const int32_t *pairs, int P) {
    for (int p = 0; p < P; ++p)
        if (pairs[2 * (size_t)p] == pairs[2 * (size_t)p + 1]) return p;
    return -1;
}

// colours into classes: item lists the members class by class, ascending within a class (MplpColouring's layout, over pairs or nodes)
inline void mplp_pairs_fill_classes(MplpColouring &col, int n, int classes) {
    col.class_off.assign((size_t)classes + 1, 0);
    col.node.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) ++col.class_off[(size_t)col.colour[(size_t)i] + 1];
    for (int k = 0; k < classes; ++k) col.class_off[(size_t)k + 1] += col.class_off[(size_t)k];
    std::vector<int32_t> fill(col.class_off.begin(), col.class_off.end() - 1);
    for (int i = 0; i < n; ++i) col.node[(size_t)fill[(size_t)col.colour[(size_t)i]]++] = i;
}

// The sweep's schedule.  colour[p]: the smallest colour no pair q < p that shares a node with p holds, so pairs of one colour share no node;
// col.node lists the pairs class by class.  No pairs: no classes.
inline void mplp_pairs_colour_pairs(const int32_t *pairs, int P, const MplpIncidence &inc, MplpColouring &col) {
    col.colour.assign((size_t)P, 0);
    std::vector<int32_t> taken;  // taken[c] == p + 1: colour c is held by a lower pair on one of p's nodes
    int classes = 0;
    for (int p = 0; p < P; ++p) {
        for (int s = 0; s < 2; ++s) {
            const int32_t i = pairs[2 * (size_t)p + s];
            for (int32_t k = inc.ptr[(size_t)i]; k < inc.ptr[(size_t)i + 1]; ++k) {
                const int32_t q = inc.slot[(size_t)k] / 2;
                if (q >= p) break;  // (the list ascends)
                const size_t c = (size_t)col.colour[(size_t)q];
                if (taken.size() <= c) taken.resize(c + 1, 0);
                taken[c] = p + 1;
            }
        }
        int32_t c = 0;
        while ((size_t)c < taken.size() && taken[(size_t)c] == p + 1) ++c;
        col.colour[(size_t)p] = c;
        classes = std::max(classes, c + 1);
    }
    mplp_pairs_fill_classes(col, P, classes);
}

// The polish's schedule.  colour[i]: the smallest colour no lower-index node that shares a pair with i holds (a node in no pair: 0), so nodes of one
// colour share no pair.
inline void mplp_pairs_colour_nodes(const int32_t *pairs, int N, const MplpIncidence &inc, MplpColouring &col) {
    col.colour.assign((size_t)N, 0);
    std::vector<int32_t> taken;
    int classes = N > 0 ? 1 : 0;
    for (int i = 0; i < N; ++i) {
        for (int32_t k = inc.ptr[(size_t)i]; k < inc.ptr[(size_t)i + 1]; ++k) {
            const int32_t j = pairs[(size_t)(inc.slot[(size_t)k] ^ 1)];  // the pair's other node
            if (j >= i) continue;
            const size_t c = (size_t)col.colour[(size_t)j];
            if (taken.size() <= c) taken.resize(c + 1, 0);
            taken[c] = i + 1;
        }
        int32_t c = 0;
        while ((size_t)c < taken.size() && taken[(size_t)c] == i + 1) ++c;
        col.colour[(size_t)i] = c;
        classes = std::max(classes, c + 1);
    }
    mplp_pairs_fill_classes(col, N, classes);
}

// The update of pair p: theta_p(a, b) = paircosts[(p L + b) L + a]; the two cavities, the two minima of the summed table, the new messages.  A
// minimum of finite values is order-free but for the sign of a zero, which `+ 0.0` removes (5.19), so any reduction shape gives these bits.
inline void mplp_pairs_update(const double *unary, const double *paircosts, const int32_t *pairs, const MplpIncidence &inc, int N, int L, int p, double *m,
                              double *scratch /* 4 L */) {
    double *d0 = scratch, *d1 = d0 + L, *M0 = d1 + L, *M1 = M0 + L;
    mplp_node_sum(unary, m, inc, N, L, pairs[2 * (size_t)p], 2 * p, d0);
    mplp_node_sum(unary, m, inc, N, L, pairs[2 * (size_t)p + 1], 2 * p + 1, d1);
    for (int x = 0; x < 2 * L; ++x) M0[x] = std::numeric_limits<double>::infinity();
    const double *th = paircosts + (size_t)p * L * L;
    for (int b = 0; b < L; ++b)
        for (int a = 0; a < L; ++a) {
            const double v = (th[(size_t)b * L + a] + d0[a]) + d1[b];
            if (v < M0[a]) M0[a] = v;
            if (v < M1[b]) M1[b] = v;
        }
    double *out = m + (size_t)2 * p * L;
    for (int x = 0; x < L; ++x) out[x] = (M0[x] + 0.0) / 2.0 - d0[x];
    for (int x = 0; x < L; ++x) out[(size_t)L + x] = (M1[x] + 0.0) / 2.0 - d1[x];
}

// the last P terms of the bound: min over (a, b) of (theta_p(a, b) - m[p][0][a]) - m[p][1][b]
inline void mplp_pairs_factor_terms(const double *paircosts, const double *m, int L, int P, double *factor_terms) {
    for (int p = 0; p < P; ++p) {
        const double *th = paircosts + (size_t)p * L * L, *m0 = m + (size_t)2 * p * L, *m1 = m0 + L;
        double lo = std::numeric_limits<double>::infinity();
        for (int b = 0; b < L; ++b)
            for (int a = 0; a < L; ++a) {
                const double v = (th[(size_t)b * L + a] - m0[a]) - m1[b];
                if (v < lo) lo = v;
            }
        factor_terms[p] = lo;
    }
}

// the N + P terms of a labelling's energy; summed by mcmc_energy_of_terms(terms, N, P): the unary terms from 0.0, `+ 0.0`, the pair terms from 0.0
inline void mplp_pairs_energy_terms(const double *unary, const double *paircosts, const int32_t *pairs, int N, int L, int P, const int32_t *labeling,
                                    double *terms) {
    for (int i = 0; i < N; ++i) terms[i] = unary[(size_t)labeling[i] * N + i];
    for (int p = 0; p < P; ++p)
        terms[(size_t)N + p] = paircosts[((size_t)p * L + (size_t)labeling[pairs[2 * (size_t)p + 1]]) * L + (size_t)labeling[pairs[2 * (size_t)p]]];
}

// the serial literal over checked arguments: MplpOutputs and the stop are 5.19's, the sweep walks the pair classes
inline void mplp_pairs_run_host(const double *unary, const double *paircosts, const int32_t *pairs, int N, int L, int P, int sweeps, const MplpOutputs &o) {
    MplpIncidence inc;
    mplp_pairs_build_incidence(pairs, N, P, inc);
    MplpColouring col;
    mplp_pairs_colour_pairs(pairs, P, inc, col);
    const size_t nm = 2 * (size_t)P * L, nterms = (size_t)N + P;
    std::vector<double> m(nm, 0.0), before(nm), scratch(4 * (size_t)L), terms(nterms), bterms(nterms);
    std::vector<int32_t> cand((size_t)N);
    mplp_pairs_energy_terms(unary, paircosts, pairs, N, L, P, o.labeling, terms.data());
    MplpWinner win(o.labeling, N, mcmc_energy_of_terms(terms.data(), N, P));
    int run = 0;
    double e_last = 0.0, b_last = 0.0;
    for (int k = 0; k < sweeps && P > 0; ++k) {
        before = m;
        for (int32_t j = 0; j < P; ++j) mplp_pairs_update(unary, paircosts, pairs, inc, N, L, col.node[(size_t)j], m.data(), scratch.data());
        run = k + 1;
        mplp_decode(unary, m.data(), inc, N, L, cand.data(), bterms.data(), scratch.data());
        mplp_pairs_energy_terms(unary, paircosts, pairs, N, L, P, cand.data(), terms.data());
        e_last = mcmc_energy_of_terms(terms.data(), N, P);
        win.offer(cand.data(), N, e_last);
        if (o.energies) o.energies[k] = e_last;
        if (o.bounds) {
            mplp_pairs_factor_terms(paircosts, m.data(), L, P, bterms.data() + N);
            o.bounds[k] = b_last = mplp_bound_of_terms(bterms.data(), N, P);
        }
        if (std::memcmp(before.data(), m.data(), sizeof(double) * nm) == 0) break;  // a fixed point
    }
    for (int k = run; k < sweeps && run > 0; ++k) {
        if (o.energies) o.energies[k] = e_last;
        if (o.bounds) o.bounds[k] = b_last;
    }
    if (o.bound) {
        if (o.bounds && run > 0)
            *o.bound = b_last;
        else {
            mplp_decode(unary, m.data(), inc, N, L, nullptr, bterms.data(), scratch.data());
            mplp_pairs_factor_terms(paircosts, m.data(), L, P, bterms.data() + N);
            *o.bound = mplp_bound_of_terms(bterms.data(), N, P);
        }
    }
    std::copy(win.lab.begin(), win.lab.end(), o.labeling);
    if (o.sweeps_run) *o.sweeps_run = run;
    if (o.energy) *o.energy = win.energy;
    if (o.messages) std::copy(m.begin(), m.end(), o.messages);
}

// s(x) of node i with every other node held at its label: theta_i(x), then one table entry per incident slot in list order
inline void mplp_pairs_polish_scores(const double *unary, const double *paircosts, const int32_t *pairs, const MplpIncidence &inc, const int32_t *lab, int N,
                                     int L, int i, double *score) {
    for (int x = 0; x < L; ++x) score[x] = unary[(size_t)x * N + i];
    for (int32_t k = inc.ptr[(size_t)i]; k < inc.ptr[(size_t)i + 1]; ++k) {
        const int32_t q = inc.slot[(size_t)k], p = q / 2;
        const size_t other = (size_t)lab[(size_t)pairs[(size_t)(q ^ 1)]];
        const double *th = paircosts + (size_t)p * L * L;
        if ((q & 1) == 0)
            for (int x = 0; x < L; ++x) score[x] += th[other * L + (size_t)x];  // theta_p(x, x_B)
        else
            for (int x = 0; x < L; ++x) score[x] += th[(size_t)x * L + other];  // theta_p(x_A, x)
    }
}

// one pass over the node classes; a node keeps its label unless the first argmin's score is strictly lower.  Returns whether a label changed.
inline bool mplp_pairs_polish_pass(const double *unary, const double *paircosts, const int32_t *pairs, const MplpIncidence &inc, const MplpColouring &col,
                                   int32_t *lab, int N, int L, double *score /* L */) {
    bool changed = false;
    for (int32_t j = 0; j < N; ++j) {
        const int32_t i = col.node[(size_t)j];
        mplp_pairs_polish_scores(unary, paircosts, pairs, inc, lab, N, L, i, score);
        int best = 0;
        for (int x = 1; x < L; ++x)
            if (score[x] < score[best]) best = x;
        if (!(score[best] < score[lab[(size_t)i]])) best = lab[(size_t)i];
        changed |= best != lab[(size_t)i];
        lab[(size_t)i] = best;
    }
    return changed;
}

// the serial literal of the polish over checked arguments (MplpRoundOutputs with 1 + polish energies)
inline void mplp_pairs_polish_host(const double *unary, const double *paircosts, const int32_t *pairs, int N, int L, int P, int polish,
                                   const MplpRoundOutputs &o) {
    MplpIncidence inc;
    mplp_pairs_build_incidence(pairs, N, P, inc);
    MplpColouring col;
    mplp_pairs_colour_nodes(pairs, N, inc, col);
    std::vector<double> terms((size_t)N + P), score((size_t)L);
    std::vector<int32_t> cur(o.labeling, o.labeling + N);
    auto energy_of = [&](const int32_t *lab) {
        mplp_pairs_energy_terms(unary, paircosts, pairs, N, L, P, lab, terms.data());
        return mcmc_energy_of_terms(terms.data(), N, P);
    };
    double e_last = energy_of(cur.data());
    MplpWinner win(cur.data(), N, e_last);
    int run = 0;
    if (o.energies) o.energies[0] = e_last;
    for (int k = 0; k < polish; ++k) {
        const bool changed = mplp_pairs_polish_pass(unary, paircosts, pairs, inc, col, cur.data(), N, L, score.data());
        run = k + 1;
        e_last = energy_of(cur.data());
        win.offer(cur.data(), N, e_last);
        if (o.energies) o.energies[1 + k] = e_last;
        if (!changed) break;  // a fixed point
    }
    for (int k = run; k < polish; ++k)
        if (o.energies) o.energies[1 + k] = e_last;
    std::copy(win.lab.begin(), win.lab.end(), o.labeling);
    if (o.passes_run) *o.passes_run = run;
    if (o.energy) *o.energy = win.energy;
}

}  // namespace msm
