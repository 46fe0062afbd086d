// mplp_forbid_host_check.cpp -- MPLP and its rounding under the forbidden-entry reading (newmsm_amd/csrc/mplp_host.hpp with forbid = true; DESIGN.md 5.19
// "Forbidden entries") as a program of its own: no HIP, no Python, built by tests/test_mplp_forbid_cpu.py with -fsanitize=address,undefined.  A fan of
// triangles round a hub, one factor forbidding a whole hub label (NaN) and one a whole rim label (+infinity), random forbidden entries besides; one
// triplet with its single entry forbidden; a finite table, where forbid changes no bit.  Prints "ok".
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
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::mt19937 gen(9);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    {
        const int N = 14, L = 4, T = 12, sweeps = 6, polish = 4;
        std::vector<int32_t> tri;
        for (int k = 0; k < T; ++k) tri.insert(tri.end(), {0, 1 + k, 1 + (k + 1) % 12});
        std::vector<double> U((size_t)L * N), tc((size_t)T * L * L * L), m((size_t)3 * T * L), energies(sweeps), bounds(sweeps);
        for (double &v : U) v = u(gen);
        for (double &v : tc) v = u(gen);
        std::vector<double> finite = tc;
        for (double &v : tc) {
            const double r = u(gen);
            if (r < 0.04) v = r < 0.02 ? nan : inf;
        }
        for (int b = 0; b < L; ++b)
            for (int c = 0; c < L; ++c) tc[(size_t)1 * L * L + (size_t)b * L + c] = nan;                        // factor 0, hub label 1
        for (int a = 0; a < L; ++a)
            for (int c = 0; c < L; ++c) tc[(size_t)5 * L * L * L + (size_t)a * L * L + (size_t)2 * L + c] = inf;  // factor 5, first rim node's label 2
        U[(size_t)1 * N + 0] = -5.0;  // the forbidden hub label tempts
        int64_t counts[4];
        mplp_classify(U.data(), U.size(), tc.data(), tc.size(), counts);
        if (counts[0] || counts[1] < 16 || counts[2] < 16 || counts[3]) return fail("classification");
        std::vector<int32_t> start(N, 1), won = start;  // the start sits on factor 0's forbidden entries
        int32_t run = -1;
        double energy = 0, bound = 0;
        mplp_run_host(U.data(), tc.data(), tri.data(), N, L, T, sweeps, MplpOutputs{won.data(), &run, &energy, &bound, energies.data(), bounds.data(), m.data()}, true);
        if (run < 1) return fail("sweeps run");
        if (!(m[1] == inf)) return fail("the hub's forbidden label has no infinite message");
        for (double v : m)
            if (v != v || v == -inf) return fail("a message is NaN or -infinity");
        if (won[0] == 1 || !(energy < inf)) return fail("the winner uses the forbidden hub label");
        for (int k = 0; k < sweeps; ++k)
            if (energies[k] != energies[k] || bounds[k] != bounds[k] || bounds[k] > energy + 1e-11  /* 26 terms of magnitude <= 5: far below */) return fail("energies and bounds");
        for (int mode = 0; mode < 2; ++mode) {
            std::vector<int32_t> lab = mode == 0 ? won : start;
            std::vector<double> re((size_t)(mode == 0 ? 2 : 1) + polish, -1.0);
            double e = 0;
            mplp_round_host(U.data(), tc.data(), tri.data(), N, L, T, m.data(), mode, polish, MplpRoundOutputs{lab.data(), &run, &e, re.data()}, true);
            for (double v : re)
                if (v != v || v < e) return fail("a rounding energy is NaN or below the winner's");
            if (mode == 0 && e > energy) return fail("the rounding is worse than what it was handed");
            if (mode == 1 && !(re[0] == inf)) return fail("the start's energy is not +infinity");
        }
        // a finite table: forbid changes no bit
        std::vector<int32_t> a = start, b = start;
        std::vector<double> ma(m.size()), mb(m.size()), ea(sweeps), eb(sweeps), ba(sweeps), bb(sweeps);
        mplp_run_host(U.data(), finite.data(), tri.data(), N, L, T, sweeps, MplpOutputs{a.data(), nullptr, nullptr, nullptr, ea.data(), ba.data(), ma.data()}, false);
        mplp_run_host(U.data(), finite.data(), tri.data(), N, L, T, sweeps, MplpOutputs{b.data(), nullptr, nullptr, nullptr, eb.data(), bb.data(), mb.data()}, true);
        if (a != b || std::memcmp(ma.data(), mb.data(), sizeof(double) * ma.size()) || std::memcmp(ea.data(), eb.data(), sizeof(double) * sweeps) ||
            std::memcmp(ba.data(), bb.data(), sizeof(double) * sweeps))
            return fail("forbid changes a finite table's outputs");
    }
    {  // one triplet, one label, its single entry forbidden: the labelling stays, energy and bound are +infinity
        const int32_t tri[3] = {0, 1, 2};
        const double U1[3] = {0.5, 0.25, 0.125}, tc1[1] = {nan};
        int32_t lab[3] = {0, 0, 0}, run = -1;
        double energy = 0, bound = 0, m[3], e2[3];
        mplp_run_host(U1, tc1, tri, 3, 1, 1, 3, MplpOutputs{lab, &run, &energy, &bound, nullptr, nullptr, m}, true);
        if (!(energy == inf) || !(bound == inf) || lab[0] || lab[1] || lab[2] || !(m[0] == inf && m[1] == inf && m[2] == inf)) return fail("one forbidden entry");
        mplp_round_host(U1, tc1, tri, 3, 1, 1, m, 0, 1, MplpRoundOutputs{lab, &run, &energy, e2}, true);
        if (!(energy == inf) || lab[0] || lab[1] || lab[2] || run != 1) return fail("rounding one forbidden entry");
    }
    std::printf("ok\n");
    return 0;
}
