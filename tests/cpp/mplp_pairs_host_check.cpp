// mplp_pairs_host_check.cpp -- the host literal of MPLP over the pair tables (newmsm_amd/csrc/mplp_pairs_host.hpp) as a program of its own: no HIP, no
// Python, built by tests/test_mplp_pairs_cpu.py with -fsanitize=address,undefined.  A star with an isolated node and reversed pairs (both colourings,
// the incidence, a run, a polish), a chain against brute force, a run without pairs and one without sweeps; every optional output asked for and none.
// Prints "ok".
#include <cmath>
#include <cstdio>
#include <random>

#include "../../newmsm_amd/csrc/mplp_pairs_host.hpp"

using namespace msm;

static int fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

static double energy_of(const std::vector<double> &U, const std::vector<double> &pc, const std::vector<int32_t> &pairs, int N, int L, const int32_t *lab) {
    const int P = (int)(pairs.size() / 2);
    std::vector<double> terms((size_t)N + P);
    mplp_pairs_energy_terms(U.data(), pc.data(), pairs.data(), N, L, P, lab, terms.data());
    return mcmc_energy_of_terms(terms.data(), N, P);
}

int main() {
    std::mt19937 gen(7);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    {  // hub 0 with 20 leaves, every second pair written leaf first; node 21 in no pair
        const int N = 22, L = 5, P = 20, sweeps = 9, polish = 6;
        std::vector<int32_t> pairs;
        for (int k = 0; k < P; ++k) pairs.insert(pairs.end(), {k % 2 ? 1 + k : 0, k % 2 ? 0 : 1 + k});
        if (mplp_pairs_first_loop(pairs.data(), P) != -1) return fail("a loop where there is none");
        MplpIncidence inc;
        mplp_pairs_build_incidence(pairs.data(), N, P, inc);
        if (inc.ptr[1] - inc.ptr[0] != P || inc.ptr[N] - inc.ptr[N - 1] != 0 || inc.ptr[N] != 2 * P) return fail("incidence sizes");
        for (int i = 0; i < N; ++i)
            for (int k = inc.ptr[i] + 1; k < inc.ptr[i + 1]; ++k)
                if (inc.slot[k - 1] >= inc.slot[k]) return fail("incidence order");
        MplpColouring pc_col, n_col;
        mplp_pairs_colour_pairs(pairs.data(), P, inc, pc_col);
        mplp_pairs_colour_nodes(pairs.data(), N, inc, n_col);
        if (pc_col.classes() != P) return fail("the pairs of a star do not take a colour each");
        for (int p = 0; p < P; ++p)
            if (pc_col.colour[p] != p || pc_col.node[p] != p) return fail("pair colours of a star");
        if (n_col.classes() != 2 || n_col.colour[0] != 0 || n_col.colour[N - 1] != 0) return fail("node colours of a star");
        for (int i = 1; i <= P; ++i)
            if (n_col.colour[i] != 1) return fail("a leaf's colour");
        std::vector<double> U((size_t)L * N), pc((size_t)P * L * L);
        for (double &v : U) v = u(gen);
        for (double &v : pc) v = u(gen);
        std::vector<int32_t> lab(N, 4), start = lab;
        std::vector<double> energies(sweeps), bounds(sweeps), m((size_t)2 * P * L);
        int32_t run = -1;
        double energy = 0, bound = 0;
        mplp_pairs_run_host(U.data(), pc.data(), pairs.data(), N, L, P, sweeps, MplpOutputs{lab.data(), &run, &energy, &bound, energies.data(), bounds.data(), m.data()});
        if (energy_of(U, pc, pairs, N, L, lab.data()) != energy || energy > energy_of(U, pc, pairs, N, L, start.data())) return fail("the returned energy");
        if (run < 1 || run > sweeps || bound > energy + 1e-12) return fail("sweeps run or bound");
        for (int k = 1; k < sweeps; ++k)
            if (bounds[k] < bounds[k - 1] - 1e-12) return fail("the bound fell");
        std::vector<int32_t> lab2 = start;
        mplp_pairs_run_host(U.data(), pc.data(), pairs.data(), N, L, P, sweeps, MplpOutputs{lab2.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
        if (lab2 != lab) return fail("the labelling depends on the optional outputs");
        // the polish from the start: never worse, and at its fixed point no single node improves
        std::vector<int32_t> pol = start;
        std::vector<double> pe(1 + polish);
        int32_t passes = -1;
        double penergy = 0;
        mplp_pairs_polish_host(U.data(), pc.data(), pairs.data(), N, L, P, polish, MplpRoundOutputs{pol.data(), &passes, &penergy, pe.data()});
        if (passes < 1 || passes > polish || penergy > pe[0] || pe[0] != energy_of(U, pc, pairs, N, L, start.data())) return fail("the polish's energies");
        if (penergy != energy_of(U, pc, pairs, N, L, pol.data())) return fail("the polish's energy is not its labelling's");
        if (passes < polish)
            for (int i = 0; i < N; ++i)
                for (int x = 0; x < L; ++x) {
                    std::vector<int32_t> t = pol;
                    t[i] = x;
                    if (energy_of(U, pc, pairs, N, L, t.data()) < penergy - 1e-12) return fail("a single node improves the polished labelling");
                }
        std::vector<int32_t> pol2 = start;
        mplp_pairs_polish_host(U.data(), pc.data(), pairs.data(), N, L, P, polish, MplpRoundOutputs{pol2.data(), nullptr, nullptr, nullptr});
        if (pol2 != pol) return fail("the polish depends on the optional outputs");
        pairs[7] = pairs[6];
        if (mplp_pairs_first_loop(pairs.data(), P) != 3) return fail("the loop not found");
    }
    {  // a chain of four nodes, three labels: a tree, so the optimum and a tight bound
        const int N = 4, L = 3, P = 3;
        const std::vector<int32_t> pairs = {0, 1, 2, 1, 2, 3};
        std::vector<double> U((size_t)L * N), pc((size_t)P * L * L);
        for (double &v : U) v = u(gen);
        for (double &v : pc) v = u(gen);
        double best = 1e300;
        int32_t t[4];
        for (t[0] = 0; t[0] < L; ++t[0])
            for (t[1] = 0; t[1] < L; ++t[1])
                for (t[2] = 0; t[2] < L; ++t[2])
                    for (t[3] = 0; t[3] < L; ++t[3]) best = std::min(best, energy_of(U, pc, pairs, N, L, t));
        int32_t lab[4] = {2, 2, 2, 2}, run = 0;
        double energy = 0, bound = 0;
        mplp_pairs_run_host(U.data(), pc.data(), pairs.data(), N, L, P, 200, MplpOutputs{lab, &run, &energy, &bound, nullptr, nullptr, nullptr});
        if (std::fabs(energy - best) > 1e-13 || std::fabs(bound - best) > 1e-12) return fail("a chain is not solved exactly");
        int32_t keep[4] = {1, 0, 2, 1};
        mplp_pairs_run_host(U.data(), pc.data(), pairs.data(), N, L, 0, 5, MplpOutputs{keep, &run, &energy, &bound, nullptr, nullptr, nullptr});  // no pairs
        if (run != 0 || keep[0] != 1 || keep[1] != 0 || keep[2] != 2 || keep[3] != 1) return fail("a run without pairs");
        mplp_pairs_run_host(U.data(), pc.data(), pairs.data(), N, L, P, 0, MplpOutputs{keep, &run, &energy, &bound, nullptr, nullptr, nullptr});  // no sweeps
        if (run != 0 || keep[0] != 1 || keep[1] != 0 || keep[2] != 2 || keep[3] != 1 || bound > energy) return fail("a run without sweeps");
        mplp_pairs_polish_host(U.data(), pc.data(), pairs.data(), N, L, P, 0, MplpRoundOutputs{keep, &run, &energy, nullptr});  // no passes
        if (run != 0 || keep[0] != 1 || keep[3] != 1) return fail("a polish without passes");
    }
    std::printf("ok\n");
    return 0;
}
