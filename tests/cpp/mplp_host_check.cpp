// mplp_host_check.cpp -- the MPLP optimiser's host literal (newmsm_amd/csrc/mplp_host.hpp) as a program of its own: no HIP, no Python, built by
// tests/test_mplp_cpu.py with -fsanitize=address,undefined.  A fan of triangles round a hub with an isolated node, a single triangle against brute force,
// a run without triplets and one without sweeps; every optional output asked for and none.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <random>

#include "../../newmsm_amd/csrc/mplp_host.hpp"

using namespace msm;

static int fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

int main() {
    std::mt19937 gen(7);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    {  // twelve triangles round node 0, node 13 in none of them
        const int N = 14, L = 5, T = 12, sweeps = 9;
        std::vector<int32_t> tri;
        for (int k = 0; k < T; ++k) tri.insert(tri.end(), {0, 1 + k, 1 + (k + 1) % 12});
        if (mplp_first_repeated_node(tri.data(), T) != -1) return fail("a repeated node where there is none");
        MplpIncidence inc;
        mplp_build_incidence(tri.data(), N, T, inc);
        if (inc.ptr[1] - inc.ptr[0] != 12 || inc.ptr[14] - inc.ptr[13] != 0 || inc.ptr[N] != 3 * T) return fail("incidence sizes");
        for (int i = 0; i < N; ++i)
            for (int k = inc.ptr[i] + 1; k < inc.ptr[i + 1]; ++k)
                if (inc.slot[k - 1] >= inc.slot[k]) return fail("incidence order");
        std::vector<double> U((size_t)L * N), tc((size_t)T * L * L * L);
        for (double &v : U) v = u(gen);
        for (double &v : tc) v = u(gen);
        int64_t counts[4];
        mplp_classify(U.data(), U.size(), tc.data(), tc.size(), counts);
        if (counts[0] || counts[1] || counts[2] || counts[3]) return fail("finite tables called non-finite");
        std::vector<int32_t> lab(N, 4), start = lab;
        std::vector<double> energies(sweeps), bounds(sweeps), m((size_t)3 * T * L), terms((size_t)N + T);
        int32_t run = -1;
        double energy = 0, bound = 0;
        mplp_run_host(U.data(), tc.data(), tri.data(), N, L, T, sweeps, MplpOutputs{lab.data(), &run, &energy, &bound, energies.data(), bounds.data(), m.data()});
        mcmc_energy_terms(U.data(), tc.data(), tri.data(), N, L, T, start.data(), terms.data());
        const double e0 = mcmc_energy_of_terms(terms.data(), N, T);
        mcmc_energy_terms(U.data(), tc.data(), tri.data(), N, L, T, lab.data(), terms.data());
        if (mcmc_energy_of_terms(terms.data(), N, T) != energy || energy > e0) return fail("the returned energy");
        if (run < 1 || run > sweeps || bound > energy + 1e-12) return fail("sweeps run or bound");
        for (int k = 1; k < sweeps; ++k)
            if (bounds[k] < bounds[k - 1] - 1e-12) return fail("the bound fell");
        std::vector<int32_t> lab2 = start;
        mplp_run_host(U.data(), tc.data(), tri.data(), N, L, T, sweeps, MplpOutputs{lab2.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
        if (lab2 != lab) return fail("the labelling depends on the optional outputs");
        tc[17] = std::nan("");
        mplp_classify(U.data(), U.size(), tc.data(), tc.size(), counts);
        if (counts[0] != 0 || counts[1] != 1 || counts[2] != 0 || counts[3] != 0) return fail("a NaN not counted as one NaN");
        tri[5] = tri[3];
        if (mplp_first_repeated_node(tri.data(), T) != 1) return fail("the repeated node not found");
    }
    {  // one triangle, three labels: the optimum and a tight bound
        const int N = 3, L = 3, T = 1;
        const int32_t tri[3] = {0, 1, 2};
        std::vector<double> U((size_t)L * N), tc((size_t)L * L * L);
        for (double &v : U) v = u(gen);
        for (double &v : tc) v = u(gen);
        double best = 1e300;
        for (int a = 0; a < L; ++a)
            for (int b = 0; b < L; ++b)
                for (int c = 0; c < L; ++c) best = std::min(best, U[(size_t)a * N] + U[(size_t)b * N + 1] + U[(size_t)c * N + 2] + tc[(size_t)(a * L + b) * L + c]);
        int32_t lab[3] = {2, 2, 2}, run = 0;
        double energy = 0, bound = 0;
        mplp_run_host(U.data(), tc.data(), tri, N, L, T, 10, MplpOutputs{lab, &run, &energy, &bound, nullptr, nullptr, nullptr});
        if (run > 3 || std::fabs(energy - best) > 1e-13 || std::fabs(bound - best) > 1e-13) return fail("single triangle");
        int32_t keep[3] = {1, 0, 2};
        mplp_run_host(U.data(), tc.data(), tri, N, L, 0, 5, MplpOutputs{keep, &run, &energy, &bound, nullptr, nullptr, nullptr});  // no triplets
        if (run != 0 || keep[0] != 1 || keep[1] != 0 || keep[2] != 2) return fail("a run without triplets");
        mplp_run_host(U.data(), tc.data(), tri, N, L, T, 0, MplpOutputs{keep, &run, &energy, &bound, nullptr, nullptr, nullptr});  // no sweeps
        if (run != 0 || keep[0] != 1 || keep[1] != 0 || keep[2] != 2 || bound > energy) return fail("a run without sweeps");
    }
    std::printf("ok\n");
    return 0;
}
