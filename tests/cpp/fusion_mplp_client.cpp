// fusion_mplp_client.cpp -- the C++ side of the label step's MPLP solve without a GPU (tests/test_fusion_mplp_cpu.py): the defaults of
// LevelOptions::fusion_mplp / fusion_sweeps / fusion_polish (include/msmhip_registration.hpp) and msmhip::fusion_mplp_step (include/msmhip.hpp) over a
// small table both sides can write down -- the octahedron's eight faces, dyadic costs -- printed with every bit (%a) for the test to compare with
// api.fusion_mplp_step.  A refusal comes back as msmhip::Error.
#include <cstdio>
#include <vector>

#include "msmhip.hpp"
#include "msmhip_registration.hpp"

int main() {
    using namespace msmhip;
    const LevelOptions o;
    std::printf("defaults %d %d %d\n", o.fusion_mplp ? 1 : 0, o.fusion_sweeps, o.fusion_polish);
    const std::vector<int32_t> triplets = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    const int N = 6, T = 8;
    std::vector<double> unary2(2 * (size_t)N), octets(8 * (size_t)T);
    for (int i = 0; i < N; ++i)
        for (int x = 0; x < 2; ++x) unary2[2 * (size_t)i + x] = ((7 * i + 3 * x) % 11) / 8.0;
    for (int t = 0; t < T; ++t)
        for (int e = 0; e < 8; ++e) octets[8 * (size_t)t + e] = ((5 * t + 3 * e * e) % 13 - 6) / 4.0;
    const FusionMplp r = fusion_mplp_step(N, unary2, octets.data(), triplets, 6, 3);
    std::printf("x");
    for (int32_t v : r.x) std::printf(" %d", v);
    std::printf("\nrun %d %d\nenergy %a bound %a\nenergies", r.sweeps_run, r.passes_run, r.energy, r.bound);
    for (double v : r.energies) std::printf(" %a", v);
    std::printf("\nbounds");
    for (double v : r.bounds) std::printf(" %a", v);
    std::printf("\n");
    try {
        fusion_mplp_step(N, unary2, octets.data(), triplets, 1025, 3);
        std::printf("not refused\n");
        return 1;
    } catch (const Error &e) {
        std::printf("refused %s\n", e.what());
    }
    return 0;
}
