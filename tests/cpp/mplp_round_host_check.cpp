// mplp_round_host_check.cpp -- the rounding of MPLP's messages (newmsm_amd/csrc/mplp_host.hpp: mplp_build_colouring, mplp_round_host) as a program of
// its own: no HIP, no Python, built by tests/test_mplp_round_cpu.py with -fsanitize=address,undefined.  A fan of triangles round a hub with an isolated
// node, both modes, messages from the sweeps and none, one label, no triplets, no polish.  Prints "ok".
#include <cstdio>
#include <random>

#include "../../newmsm_amd/csrc/mplp_host.hpp"

using namespace msm;

static int fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

static double energy_of(const std::vector<double> &U, const std::vector<double> &tc, const std::vector<int32_t> &tri, int N, int L, int T,
                        const std::vector<int32_t> &lab) {
    std::vector<double> terms((size_t)N + T);
    mcmc_energy_terms(U.data(), tc.data(), tri.data(), N, L, T, lab.data(), terms.data());
    return mcmc_energy_of_terms(terms.data(), N, T);
}

int main() {
    std::mt19937 gen(9);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    {  // twelve triangles round node 0, node 13 in none of them
        const int N = 14, L = 5, T = 12, polish = 6;
        std::vector<int32_t> tri;
        for (int k = 0; k < T; ++k) tri.insert(tri.end(), {1 + k, 0, 1 + (k + 1) % 12});
        MplpIncidence inc;
        mplp_build_incidence(tri.data(), N, T, inc);
        MplpColouring col;
        mplp_build_colouring(tri.data(), N, inc, col);
        if (col.colour[0] != 0 || col.colour[13] != 0 || col.classes() < 3 || col.class_off[(size_t)col.classes()] != N) return fail("colouring sizes");
        for (int t = 0; t < T; ++t) {
            const int a = col.colour[(size_t)tri[3 * (size_t)t]], b = col.colour[(size_t)tri[3 * (size_t)t + 1]], c = col.colour[(size_t)tri[3 * (size_t)t + 2]];
            if (a == b || a == c || b == c) return fail("two nodes of a triplet share a colour");
        }
        for (int k = 0; k < col.classes(); ++k)
            for (int p = col.class_off[(size_t)k]; p < col.class_off[(size_t)k + 1]; ++p) {
                if (col.colour[(size_t)col.node[(size_t)p]] != k) return fail("class lists");
                if (p > col.class_off[(size_t)k] && col.node[(size_t)p - 1] >= col.node[(size_t)p]) return fail("class order");
            }
        std::vector<double> U((size_t)L * N), tc((size_t)T * L * L * L), m((size_t)3 * T * L);
        for (double &v : U) v = u(gen);
        for (double &v : tc) v = u(gen);
        std::vector<int32_t> start(N, 4), won = start;
        mplp_run_host(U.data(), tc.data(), tri.data(), N, L, T, 5, MplpOutputs{won.data(), nullptr, nullptr, nullptr, nullptr, nullptr, m.data()});
        const double e0 = energy_of(U, tc, tri, N, L, T, won);
        for (int mode = 0; mode < 2; ++mode) {
            std::vector<int32_t> lab = won;
            std::vector<double> energies((size_t)(mode == 0 ? 2 : 1) + polish, -1.0);
            int32_t run = -1;
            double energy = 0;
            mplp_round_host(U.data(), tc.data(), tri.data(), N, L, T, m.data(), mode, polish, MplpRoundOutputs{lab.data(), &run, &energy, energies.data()});
            if (energies[0] != e0 || energy > e0 || energy != energy_of(U, tc, tri, N, L, T, lab)) return fail("the returned energy");
            if (run < 1 || run > polish) return fail("passes run");
            for (double e : energies)
                if (e < energy) return fail("an energy below the winner's");
            std::vector<int32_t> lab2 = won, lab3 = won;
            mplp_round_host(U.data(), tc.data(), tri.data(), N, L, T, m.data(), mode, polish, MplpRoundOutputs{lab2.data(), nullptr, nullptr, nullptr});
            if (lab2 != lab) return fail("the labelling depends on the optional outputs");
            mplp_round_host(U.data(), tc.data(), tri.data(), N, L, T, nullptr, mode, 0, MplpRoundOutputs{lab3.data(), &run, &energy, energies.data()});
            if (run != 0 || energy > e0) return fail("no messages, no polish");
        }
    }
    {  // one triangle with one label; then no triplets at all: every node takes the argmin of its unary cost
        const int32_t tri[3] = {2, 0, 1};
        const double U1[3] = {0.5, 0.25, 0.125}, tc1[1] = {2.0};
        int32_t lab[3] = {0, 0, 0}, run = -1;
        double energy = 0, energies[4];
        mplp_round_host(U1, tc1, tri, 3, 1, 1, nullptr, 0, 2, MplpRoundOutputs{lab, &run, &energy, energies});
        if (run != 1 || energy != 2.875 || lab[0] || lab[1] || lab[2]) return fail("one label");
        const double U2[6] = {0.5, 0.1, 0.3, 0.2, 0.4, 0.3};  // L = 2, N = 3
        int32_t lab2[3] = {0, 0, 0};
        mplp_round_host(U2, nullptr, nullptr, 3, 2, 0, nullptr, 0, 2, MplpRoundOutputs{lab2, &run, &energy, energies});
        if (lab2[0] != 1 || lab2[1] != 0 || lab2[2] != 0 || run != 1) return fail("no triplets");
    }
    std::printf("ok\n");
    return 0;
}
