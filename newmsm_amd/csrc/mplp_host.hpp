// mplp_host.hpp -- max-product linear programming (MPLP) over the Monte Carlo optimiser's two tables, the part that is plain host C++ (no HIP header): the
// incidence lists, the serial literal of DESIGN.md 5.19 that msm_mplp_optimise runs and the GPU entry points reproduce bit for bit, and the sums both
// sides form on the host.  Block-coordinate ascent on the dual of the labelling LP, written from the published update rule for factors of three
// variables (Globerson & Jaakkola, NIPS 2007; Sontag, Globerson & Jaakkola 2011, Fig. 1.4).
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

inline bool mplp_all_finite(const double *v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!(v[i] - v[i] == 0.0)) return false;  // a NaN or an infinity
    return true;
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
                               double *scratch /* 6 L */) {
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
                const double v = ((row[c] + d0[a]) + d1[b]) + d2[c];
                if (v < M0[a]) M0[a] = v;
                if (v < M1[b]) M1[b] = v;
                if (v < M2[c]) M2[c] = v;
            }
        }
    for (int s = 0; s < 3; ++s)
        for (int x = 0; x < L; ++x) m[((size_t)3 * t + s) * L + x] = (M[s][x] + 0.0) / 3.0 - d[s][x];
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

// the last T terms of the bound: min over (a, b, c) of ((theta_t(a, b, c) - m[t][0][a]) - m[t][1][b]) - m[t][2][c]
inline void mplp_factor_terms(const double *tcosts, const double *m, int L, int T, double *factor_terms) {
    const size_t L1 = (size_t)L, L2 = L1 * L1, L3 = L2 * L1;
    for (int t = 0; t < T; ++t) {
        const double *th = tcosts + (size_t)t * L3, *m0 = m + (size_t)3 * t * L, *m1 = m0 + L, *m2 = m1 + L;
        double lo = std::numeric_limits<double>::infinity();
        for (int a = 0; a < L; ++a)
            for (int b = 0; b < L; ++b)
                for (int c = 0; c < L; ++c) {
                    const double v = ((th[(size_t)a * L2 + (size_t)b * L1 + c] - m0[a]) - m1[b]) - m2[c];
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
inline void mplp_run_host(const double *unary, const double *tcosts, const int32_t *triplets, int N, int L, int T, int sweeps, const MplpOutputs &o) {
    MplpIncidence inc;
    mplp_build_incidence(triplets, N, T, inc);
    const size_t nm = 3 * (size_t)T * L, nterms = (size_t)N + T;
    std::vector<double> m(nm, 0.0), before(nm), scratch(6 * (size_t)L), terms(nterms), bterms(nterms);
    std::vector<int32_t> cand((size_t)N);
    mcmc_energy_terms(unary, tcosts, triplets, N, L, T, o.labeling, terms.data());
    MplpWinner win(o.labeling, N, mcmc_energy_of_terms(terms.data(), N, T));
    int run = 0;
    double e_last = 0.0, b_last = 0.0;
    for (int k = 0; k < sweeps && T > 0; ++k) {
        before = m;
        for (int t = 0; t < T; ++t) mplp_update_factor(unary, tcosts, triplets, inc, N, L, t, m.data(), scratch.data());
        run = k + 1;
        mplp_decode(unary, m.data(), inc, N, L, cand.data(), bterms.data(), scratch.data());
        mcmc_energy_terms(unary, tcosts, triplets, N, L, T, cand.data(), terms.data());
        e_last = mcmc_energy_of_terms(terms.data(), N, T);
        win.offer(cand.data(), N, e_last);
        if (o.energies) o.energies[k] = e_last;
        if (o.bounds) {
            mplp_factor_terms(tcosts, m.data(), L, T, bterms.data() + N);
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
            mplp_factor_terms(tcosts, m.data(), L, T, bterms.data() + N);
            *o.bound = mplp_bound_of_terms(bterms.data(), N, T);
        }
    }
    std::copy(win.lab.begin(), win.lab.end(), o.labeling);
    if (o.sweeps_run) *o.sweeps_run = run;
    if (o.energy) *o.energy = win.energy;
    if (o.messages) std::copy(m.begin(), m.end(), o.messages);
}

}  // namespace msm
