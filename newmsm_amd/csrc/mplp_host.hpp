// mplp_host.hpp -- max-product linear programming (MPLP) over the Monte Carlo optimiser's two tables, the part that is plain host C++ (no HIP header): the
// incidence lists, the serial literal of DESIGN.md 5.19 that msm_mplp_optimise runs and the GPU entry points reproduce bit for bit, the sums both
// sides form on the host, and the rounding of the messages to a labelling (the colouring and the literal msm_mplp_round runs).  Block-coordinate
// ascent on the dual of the labelling LP, written from the published update rule for factors of three variables (Globerson & Jaakkola, NIPS 2007;
// Sontag, Globerson & Jaakkola 2011, Fig. 1.4).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "mcmc_host.hpp"

namespace msm {

constexpr int kMplpMaxLabels = 1024;  // a factor's 6 L doubles of cavities and results live in LDS (mplp_kernels.hip)

// Slot s of factor t is number 3 t + s.  The incidence of node i: the slots that lie on it, ascending -- slot[ptr[i]] .. slot[ptr[i + 1] - 1].
struct MplpIncidence {
    std::vector<int32_t> ptr, slot;
};

inline void mplp_build_incidence(const int32_t *triplets, int N, int T, MplpIncidence &inc) {
    inc.ptr.assign((size_t)N + 1, 0);
    inc.slot.assign(3 * (size_t)T, 0);
    for (size_t q = 0; q < 3 * (size_t)T; ++q) ++inc.ptr[(size_t)triplets[q] + 1];
    for (int i = 0; i < N; ++i) inc.ptr[(size_t)i + 1] += inc.ptr[(size_t)i];
    std::vector<int32_t> fill(inc.ptr.begin(), inc.ptr.end() - 1);
    for (size_t q = 0; q < 3 * (size_t)T; ++q) inc.slot[(size_t)fill[(size_t)triplets[q]]++] = (int32_t)q;  // ascending (t, s)
}

// the first triplet that names a node twice, or -1
inline int mplp_first_repeated_node(const int32_t *triplets, int T) {
    for (int t = 0; t < T; ++t) {
        const int32_t a = triplets[3 * (size_t)t], b = triplets[3 * (size_t)t + 1], c = triplets[3 * (size_t)t + 2];
        if (a == b || a == c || b == c) return t;
    }
    return -1;
}

// Forbidden entries: under `forbid` a table entry or an energy term that is NaN or +inf reads as +inf, a forbidden label combination.
// The test is v < +inf, false for both; without forbid the value passes as it is.
inline double mplp_hat(double v, bool forbid) { return !forbid || v < std::numeric_limits<double>::infinity() ? v : std::numeric_limits<double>::infinity(); }

// counts[0]: non-finite unary entries; counts[1..3]: NaN, +inf, -inf triplet entries (either table may be null with n = 0)
inline void mplp_classify(const double *unary, size_t nu, const double *tcosts, size_t nt, int64_t counts[4]) {
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (size_t i = 0; i < nu; ++i) counts[0] += !(unary[i] - unary[i] == 0.0);
    for (size_t i = 0; i < nt; ++i) {
        const double v = tcosts[i];
        if (v - v == 0.0) continue;
        ++counts[v != v ? 1 : v > 0.0 ? 2 : 3];
    }
}

// Ehat: mcmc_energy_of_terms over the terms passed through mplp_hat -- finite or +inf, never NaN, where the tables passed the forbid route's checks
inline double mplp_energy_of_terms(const double *terms, int N, int T, bool forbid) {
    if (!forbid) return mcmc_energy_of_terms(terms, N, T);
    double u = 0.0, pw = 0.0, tc = 0.0;
    for (int i = 0; i < N; ++i) u += mplp_hat(terms[i], true);
    for (int t = 0; t < T; ++t) tc += mplp_hat(terms[(size_t)N + t], true);
    return u + pw + tc;
}

// d(x) = unary[x * N + i] plus the messages over the incidence of i in order, but for slot `skip` (-1: none skipped -- the belief)
inline void mplp_node_sum(const double *unary, const double *m, const MplpIncidence &inc, int N, int L, int i, int32_t skip, double *d) {
    for (int x = 0; x < L; ++x) {
        double v = unary[(size_t)x * N + i];
        for (int32_t k = inc.ptr[(size_t)i]; k < inc.ptr[(size_t)i + 1]; ++k) {
            const int32_t q = inc.slot[(size_t)k];
            if (q != skip) v += m[(size_t)q * L + x];
        }
        d[x] = v;
    }
}

// The update of factor t: the three cavities, the three minima of the summed table, the new messages.  A minimum of finite values is order-free but for
// the sign of a zero; `+ 0.0` turns a -0.0 minimum into +0.0 and changes nothing else, so any reduction shape gives these bits.
inline void mplp_update_factor(const double *unary, const double *tcosts, const int32_t *triplets, const MplpIncidence &inc, int N, int L, int t, double *m,
                               double *scratch /* 6 L */, bool forbid = false) {
    const size_t L1 = (size_t)L, L2 = L1 * L1, L3 = L2 * L1;
    double *d0 = scratch, *d1 = d0 + L, *d2 = d1 + L, *M0 = d2 + L, *M1 = M0 + L, *M2 = M1 + L;
    double *d[3] = {d0, d1, d2}, *M[3] = {M0, M1, M2};
    for (int s = 0; s < 3; ++s) mplp_node_sum(unary, m, inc, N, L, triplets[3 * (size_t)t + s], 3 * t + s, d[s]);
    for (int x = 0; x < 3 * L; ++x) M0[x] = std::numeric_limits<double>::infinity();
    const double *th = tcosts + (size_t)t * L3;
    for (int a = 0; a < L; ++a)
        for (int b = 0; b < L; ++b) {
            const double *row = th + (size_t)a * L2 + (size_t)b * L1;
            for (int c = 0; c < L; ++c) {
                const double v = ((mplp_hat(row[c], forbid) + d0[a]) + d1[b]) + d2[c];
                if (v < M0[a]) M0[a] = v;
                if (v < M1[b]) M1[b] = v;
                if (v < M2[c]) M2[c] = v;
            }
        }
    for (int s = 0; s < 3; ++s)
        for (int x = 0; x < L; ++x) {
            double nv = (M[s][x] + 0.0) / 3.0 - d[s][x];
            if (forbid && !(M[s][x] < std::numeric_limits<double>::infinity())) nv = std::numeric_limits<double>::infinity();  // label x is proved infeasible
            m[((size_t)3 * t + s) * L + x] = nv;
        }
}

// beliefs and decode: label[i] = argmin_x b_i(x), lowest label on ties; node_terms[i] = that minimum (the first N terms of the bound); either may be null
inline void mplp_decode(const double *unary, const double *m, const MplpIncidence &inc, int N, int L, int32_t *label, double *node_terms, double *scratch /* L */) {
    for (int i = 0; i < N; ++i) {
        mplp_node_sum(unary, m, inc, N, L, i, -1, scratch);
        int best = 0;
        for (int x = 1; x < L; ++x)
            if (scratch[x] < scratch[best]) best = x;
        if (label) label[i] = best;
        if (node_terms) node_terms[i] = scratch[best];
    }
}

// the last T terms of the bound: min over (a, b, c) of ((theta_t(a, b, c) - m[t][0][a]) - m[t][1][b]) - m[t][2][c]; under forbid over the combinations
// whose entry and three messages are all below +inf, +inf where there is none
inline void mplp_factor_terms(const double *tcosts, const double *m, int L, int T, double *factor_terms, bool forbid = false) {
    const size_t L1 = (size_t)L, L2 = L1 * L1, L3 = L2 * L1;
    for (int t = 0; t < T; ++t) {
        const double *th = tcosts + (size_t)t * L3, *m0 = m + (size_t)3 * t * L, *m1 = m0 + L, *m2 = m1 + L;
        const double inf = std::numeric_limits<double>::infinity();
        double lo = inf;
        for (int a = 0; a < L; ++a)
            for (int b = 0; b < L; ++b)
                for (int c = 0; c < L; ++c) {
                    const double e = th[(size_t)a * L2 + (size_t)b * L1 + c];
                    if (forbid && !(e < inf && m0[a] < inf && m1[b] < inf && m2[c] < inf)) continue;
                    const double v = ((e - m0[a]) - m1[b]) - m2[c];
                    if (v < lo) lo = v;
                }
        factor_terms[t] = lo;
    }
}

// D: from 0.0, the N node terms ascending, then the T factor terms ascending
inline double mplp_bound_of_terms(const double *terms, int N, int T) {
    double D = 0.0;
    for (size_t j = 0; j < (size_t)N + T; ++j) D += terms[j];
    return D;
}

// What a run reports, on either side.  Candidate 0 is the start, candidate k the decode after sweep k; the winner is the first lowest energy
// (mcmc_best_chain's rule).  A sweep that leaves every message's bits as they were ends the run; the sweeps it spares would repeat its decode, energy
// and bound, and energies / bounds are filled with them.
struct MplpOutputs {
    int32_t *labeling;    // N: the start in, the winner out
    int32_t *sweeps_run;  // the rest may be null
    double *energy, *bound, *energies, *bounds, *messages;
};

// tracks the winner over the candidates as they arrive
struct MplpWinner {
    std::vector<int32_t> lab;
    double energy;
    MplpWinner(const int32_t *start, int N, double e) : lab(start, start + N), energy(e) {}
    void offer(const int32_t *cand, int N, double e) {
        if (e < energy) {
            energy = e;
            std::copy(cand, cand + N, lab.begin());
        }
    }
};

// the serial literal over checked arguments
inline void mplp_run_host(const double *unary, const double *tcosts, const int32_t *triplets, int N, int L, int T, int sweeps, const MplpOutputs &o,
                          bool forbid = false) {
    MplpIncidence inc;
    mplp_build_incidence(triplets, N, T, inc);
    const size_t nm = 3 * (size_t)T * L, nterms = (size_t)N + T;
    std::vector<double> m(nm, 0.0), before(nm), scratch(6 * (size_t)L), terms(nterms), bterms(nterms);
    std::vector<int32_t> cand((size_t)N);
    mcmc_energy_terms(unary, tcosts, triplets, N, L, T, o.labeling, terms.data());
    MplpWinner win(o.labeling, N, mplp_energy_of_terms(terms.data(), N, T, forbid));
    int run = 0;
    double e_last = 0.0, b_last = 0.0;
    for (int k = 0; k < sweeps && T > 0; ++k) {
        before = m;
        for (int t = 0; t < T; ++t) mplp_update_factor(unary, tcosts, triplets, inc, N, L, t, m.data(), scratch.data(), forbid);
        run = k + 1;
        mplp_decode(unary, m.data(), inc, N, L, cand.data(), bterms.data(), scratch.data());
        mcmc_energy_terms(unary, tcosts, triplets, N, L, T, cand.data(), terms.data());
        e_last = mplp_energy_of_terms(terms.data(), N, T, forbid);
        win.offer(cand.data(), N, e_last);
        if (o.energies) o.energies[k] = e_last;
        if (o.bounds) {
            mplp_factor_terms(tcosts, m.data(), L, T, bterms.data() + N, forbid);
            o.bounds[k] = b_last = mplp_bound_of_terms(bterms.data(), N, T);
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
            mplp_factor_terms(tcosts, m.data(), L, T, bterms.data() + N, forbid);
            *o.bound = mplp_bound_of_terms(bterms.data(), N, T);
        }
    }
    std::copy(win.lab.begin(), win.lab.end(), o.labeling);
    if (o.sweeps_run) *o.sweeps_run = run;
    if (o.energy) *o.energy = win.energy;
    if (o.messages) std::copy(m.begin(), m.end(), o.messages);
}

// ---------------------------------------------------------------- rounding (DESIGN.md 5.19 "Rounding")

constexpr int kMplpMaxPolish = 1024;

// colour[i]: the smallest colour no lower-index node that shares a triplet with i holds (a node in no triplet: 0), so nodes of one colour share no
// triplet.  node lists the nodes class by class, ascending within a class: class k is node[class_off[k]] .. node[class_off[k + 1] - 1].
struct MplpColouring {
    std::vector<int32_t> colour, node, class_off;
    int classes() const { return (int)class_off.size() - 1; }
};

inline void mplp_build_colouring(const int32_t *triplets, int N, const MplpIncidence &inc, MplpColouring &col) {
    col.colour.assign((size_t)N, 0);
    std::vector<int32_t> taken;  // taken[c] == i + 1: colour c is held by a lower neighbour of node i
    int classes = N > 0 ? 1 : 0;
    for (int i = 0; i < N; ++i) {
        for (int32_t k = inc.ptr[(size_t)i]; k < inc.ptr[(size_t)i + 1]; ++k) {
            const int32_t t = inc.slot[(size_t)k] / 3;
            for (int s = 0; s < 3; ++s) {
                const int32_t j = triplets[3 * (size_t)t + s];
                if (j >= i) continue;
                const size_t c = (size_t)col.colour[(size_t)j];
                if (taken.size() <= c) taken.resize(c + 1, 0);
                taken[c] = i + 1;
            }
        }
        int32_t c = 0;
        while ((size_t)c < taken.size() && taken[(size_t)c] == i + 1) ++c;
        col.colour[(size_t)i] = c;
        classes = std::max(classes, c + 1);
    }
    col.class_off.assign((size_t)classes + 1, 0);
    col.node.assign((size_t)N, 0);
    for (int i = 0; i < N; ++i) ++col.class_off[(size_t)col.colour[(size_t)i] + 1];
    for (int k = 0; k < classes; ++k) col.class_off[(size_t)k + 1] += col.class_off[(size_t)k];
    std::vector<int32_t> fill(col.class_off.begin(), col.class_off.end() - 1);
    for (int i = 0; i < N; ++i) col.node[(size_t)fill[(size_t)col.colour[(size_t)i]]++] = i;  // ascending within a class
}

// the other two slots of slot s, ascending
inline void mplp_other_slots(int s, int &s1, int &s2) { s1 = s == 0 ? 1 : 0, s2 = s == 2 ? 1 : 2; }

// score(x) of node i at frontier f (node j is fixed when colour[j] < f): theta_i(x), then g_{t,s}(x) over the incidence of i in list order.  m null:
// all messages zero.  frontier INT_MAX reads no message.
inline void mplp_round_scores(const double *unary, const double *tcosts, const int32_t *triplets, const double *m, const MplpIncidence &inc,
                              const int32_t *colour, int frontier, const int32_t *lab, int N, int L, int i, double *score,
                              bool forbid = false) {
    const double inf = std::numeric_limits<double>::infinity();
    const size_t L1 = (size_t)L, L2 = L1 * L1, L3 = L2 * L1;
    const size_t stride[3] = {L2, L1, 1};
    for (int x = 0; x < L; ++x) score[x] = unary[(size_t)x * N + i];
    for (int32_t k = inc.ptr[(size_t)i]; k < inc.ptr[(size_t)i + 1]; ++k) {
        const int32_t q = inc.slot[(size_t)k], t = q / 3;
        const int s = q - 3 * t;
        int s1, s2;
        mplp_other_slots(s, s1, s2);
        const int32_t j1 = triplets[3 * (size_t)t + s1], j2 = triplets[3 * (size_t)t + s2];
        const bool f1 = colour[(size_t)j1] < frontier, f2 = colour[(size_t)j2] < frontier;
        const double *th = tcosts + (size_t)t * L3;
        const double *m1 = m ? m + ((size_t)3 * t + s1) * L : nullptr, *m2 = m ? m + ((size_t)3 * t + s2) * L : nullptr;
        for (int x = 0; x < L; ++x) {
            const double *row = th + (size_t)x * stride[s];
            double g;
            if (f1 && f2)
                g = mplp_hat(row[(size_t)lab[(size_t)j1] * stride[s1] + (size_t)lab[(size_t)j2] * stride[s2]], forbid);
            else {
                g = std::numeric_limits<double>::infinity();
                const int a0 = f1 ? lab[(size_t)j1] : 0, a1 = f1 ? a0 + 1 : L, b0 = f2 ? lab[(size_t)j2] : 0, b1 = f2 ? b0 + 1 : L;
                for (int y1 = a0; y1 < a1; ++y1)
                    for (int y2 = b0; y2 < b1; ++y2) {
                        double v = row[(size_t)y1 * stride[s1] + (size_t)y2 * stride[s2]];
                        // a forbidden entry, or a message of +inf it would subtract: the combination is +inf and lowers nothing
                        if (forbid && !(v < inf && (f1 || !m1 || m1[y1] < inf) && (f2 || !m2 || m2[y2] < inf))) continue;
                        if (!f1) v = v - (m1 ? m1[y1] : 0.0);
                        if (!f2) v = v - (m2 ? m2[y2] : 0.0);
                        if (v < g) g = v;
                    }
                g = g + 0.0;
            }
            score[x] += g;
        }
    }
}

// one walk over the classes: frontier k for class k in the conditioned decode (polish false), INT_MAX in a polish pass, where a node keeps its label
// unless another one's score is strictly lower.  Returns whether a label changed.
inline bool mplp_round_pass(const double *unary, const double *tcosts, const int32_t *triplets, const double *m, const MplpIncidence &inc,
                            const MplpColouring &col, bool polish, int32_t *lab, int N, int L, double *score /* L */,
                            bool forbid = false) {
    bool changed = false;
    for (int k = 0; k < col.classes(); ++k)
        for (int32_t p = col.class_off[(size_t)k]; p < col.class_off[(size_t)k + 1]; ++p) {
            const int32_t i = col.node[(size_t)p];
            mplp_round_scores(unary, tcosts, triplets, m, inc, col.colour.data(), polish ? std::numeric_limits<int>::max() : k, lab, N, L, i, score, forbid);
            int best = 0;
            for (int x = 1; x < L; ++x)
                if (score[x] < score[best]) best = x;
            if (polish && !(score[best] < score[lab[(size_t)i]])) best = lab[(size_t)i];
            changed |= best != lab[(size_t)i];
            lab[(size_t)i] = best;
        }
    return changed;
}

struct MplpRoundOutputs {
    int32_t *labeling;    // N: candidate 0 in, the winner out
    int32_t *passes_run;  // the rest may be null
    double *energy, *energies;  // energies: 2 + polish values in mode 0, 1 + polish in mode 1
};

// the serial literal of the rounding over checked arguments; messages may be null (all zero) and are not read in mode 1
inline void mplp_round_host(const double *unary, const double *tcosts, const int32_t *triplets, int N, int L, int T, const double *messages, int mode,
                            int polish, const MplpRoundOutputs &o, bool forbid = false) {
    MplpIncidence inc;
    mplp_build_incidence(triplets, N, T, inc);
    MplpColouring col;
    mplp_build_colouring(triplets, N, inc, col);
    std::vector<double> terms((size_t)N + T), score((size_t)L);
    std::vector<int32_t> cur(o.labeling, o.labeling + N);
    auto energy_of = [&](const int32_t *lab) {
        mcmc_energy_terms(unary, tcosts, triplets, N, L, T, lab, terms.data());
        return mplp_energy_of_terms(terms.data(), N, T, forbid);
    };
    double e_last = energy_of(cur.data());
    MplpWinner win(cur.data(), N, e_last);
    int n = 0, run = 0;
    if (o.energies) o.energies[n] = e_last;
    ++n;
    if (mode == 0) {
        mplp_round_pass(unary, tcosts, triplets, messages, inc, col, false, cur.data(), N, L, score.data(), forbid);
        e_last = energy_of(cur.data());
        win.offer(cur.data(), N, e_last);
        if (o.energies) o.energies[n] = e_last;
        ++n;
    }
    for (int p = 0; p < polish; ++p) {
        const bool changed = mplp_round_pass(unary, tcosts, triplets, nullptr, inc, col, true, cur.data(), N, L, score.data(), forbid);
        run = p + 1;
        e_last = energy_of(cur.data());
        win.offer(cur.data(), N, e_last);
        if (o.energies) o.energies[n + p] = e_last;
        if (!changed) break;  // a fixed point
    }
    for (int p = run; p < polish; ++p)
        if (o.energies) o.energies[n + p] = e_last;
    std::copy(win.lab.begin(), win.lab.end(), o.labeling);
    if (o.passes_run) *o.passes_run = run;
    if (o.energy) *o.energy = win.energy;
}

}  // namespace msm
