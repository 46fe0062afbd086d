// mcmc_draw_host_check.cpp -- the host pieces of the proposals drawn on the device (newmsm_amd/csrc/mcmc_draw.hpp) on their own, so that they can be built
// and run under the sanitizers without HIP or Python:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/mcmc_draw_host_check.cpp -o mcmc_draw_host_check && ./mcmc_draw_host_check
// Checks the hand-written engine (seeding, regeneration in the kernel's phases, tempering) against std::mt19937 over 10 blocks, the candidate against
// std::generate_canonical, the thresholds against the label function on every double within 64 ulps of each, the mirror's stream against McmcProposals
// (std::mt19937 + std::geometric_distribution), and the block bound against the candidates the mirror consumed.  Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>

#include "../../newmsm_amd/csrc/mcmc_draw.hpp"
#include "../../newmsm_amd/csrc/mcmc_host.hpp"

using namespace msm;

namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

void check_engine(uint64_t seed) {
    std::mt19937 gen((std::mt19937::result_type)seed);
    uint32_t state[kMtWords];
    mt_seed(seed, state);
    size_t bad = 0;
    for (int block = 0; block < 10; ++block) {
        mt_regenerate(state);
        for (int i = 0; i < kMtWords; ++i) bad += mt_temper(state[i]) != gen();
    }
    EXPECT(bad == 0);
}

// a generator that hands out two given words: what generate_canonical<double, 53> makes of them, against candidate_bits
struct TwoWords {
    using result_type = uint32_t;
    uint32_t w[2];
    int i = 0;
    static constexpr result_type min() { return 0; }
    static constexpr result_type max() { return 0xffffffffu; }
    result_type operator()() { return w[i++ & 1]; }
};

void check_candidate(uint32_t w0, uint32_t w1) {
    TwoWords g{{w0, w1}};
    const double x = 1.0 - std::generate_canonical<double, 53>(g);
    uint64_t bits;
    std::memcpy(&bits, &x, sizeof(bits));
    EXPECT(bits == candidate_bits(w0, w1));
    EXPECT(bits >= kDrawLowestBits && bits <= kDrawOneBits);
}

void check_thresholds(int L, double mcparam) {
    std::vector<uint64_t> thr((size_t)L);
    mcmc_draw_thresholds(L, mcparam, thr.data());
    const double c = std::log(1.0 - mcparam);
    size_t bad = 0;
    for (int k = 1; k <= L; ++k) {
        if (k > 1) EXPECT(thr[(size_t)k - 1] <= thr[(size_t)k - 2]);
        const uint64_t t = thr[(size_t)k - 1];
        EXPECT(t >= kDrawLowestBits && t <= kDrawOneBits);
        const uint64_t lo = t - kDrawLowestBits < 64 ? kDrawLowestBits : t - 64, hi = kDrawOneBits - t < 64 ? kDrawOneBits : t + 64;
        for (uint64_t b = lo; b <= hi; ++b) bad += (b >= t) != (mcmc_draw_step(b, c) <= (double)(k - 1));
    }
    EXPECT(bad == 0);
    // the label of a pattern is the number of thresholds above it, and the host's own value wherever that is a label
    for (int k = 1; k <= L; ++k)
        for (uint64_t b : {thr[(size_t)k - 1], thr[(size_t)k - 1] - 1, kDrawLowestBits, kDrawOneBits}) {
            if (b < kDrawLowestBits) continue;
            int count = 0;
            for (int j = 0; j < L; ++j) count += b < thr[(size_t)j];
            EXPECT(label_of(b, thr.data(), L) == count);
            const double f = mcmc_draw_step(b, c);
            if (f < (double)L) EXPECT((double)count == f + 0.0);
            else EXPECT(count == L);
        }
}

void check_mirror(double mcparam, int L, uint64_t seed, size_t n) {
    McmcProposals p(seed, mcparam, L);
    McmcDrawMirror m(seed, mcparam, L);
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += p.next() != m.next();
    EXPECT(bad == 0);
    EXPECT(m.candidates >= n && m.blocks * (uint64_t)kDrawCandidates >= m.candidates);
    EXPECT((uint64_t)mcmc_draw_block_bound((long)n, L, mcparam) >= m.blocks);
}

}  // namespace

int main() {
    for (uint64_t seed : {(uint64_t)0, (uint64_t)1, (uint64_t)5489, (uint64_t)0xffffffffu, ((uint64_t)1 << 32) + 5}) check_engine(seed);
    {  // only the low 32 bits of a seed count
        uint32_t a[kMtWords], b[kMtWords];
        mt_seed(5, a);
        mt_seed(((uint64_t)1 << 32) + 5, b);
        EXPECT(std::memcmp(a, b, sizeof(a)) == 0);
    }
    for (uint32_t w0 : {0u, 1u, 0x7ffu, 0x800u, 0x801u, 0x80000000u, 0xfffff7ffu, 0xfffff800u, 0xfffffbffu, 0xfffffc00u, 0xffffffffu})
        for (uint32_t w1 : {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu}) check_candidate(w0, w1);
    std::srand(11);
    for (int i = 0; i < 20000; ++i) check_candidate((uint32_t)std::rand() * 2654435761u, (uint32_t)std::rand() * 40503u + (uint32_t)i);
    check_thresholds(19, (double)0.8f);
    check_thresholds(3, 0.05);
    check_thresholds(1, 0.5);
    check_thresholds(7, 0.2);
    check_thresholds(200, (double)0.3f);
    check_thresholds(19, 0.95);
    check_thresholds(4, 1.0);
    check_mirror((double)0.8f, 19, 17, 200000);
    check_mirror(0.05, 3, ((uint64_t)1 << 32) + 5, 100000);
    check_mirror(1.0, 4, 2, 1000);
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
