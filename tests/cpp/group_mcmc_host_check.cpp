// group_mcmc_host_check.cpp -- the host pieces of gMSM's Monte Carlo blocks (newmsm_amd/csrc/group_mcmc.hpp: the incidence of a pair list, the seed rule,
// the acceptance rule) on their own, so that they can be built and run under the sanitizers without HIP or Python:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/cpp/group_mcmc_host_check.cpp -o group_mcmc_host_check && ./group_mcmc_host_check
// Builds the incidence of estimate_pairs-shaped lists (S = 2, 3, 4; many-to-one second nodes, so some nodes have no pair), of an empty list and of a
// list with a repeated node against per-node lists collected the slow way; refuses nodes out of range; checks the seed rule against its formula and
// against the pairwise loops' seeds, and the acceptance rule on equal, lower, higher, NaN and infinite energies.  Exit status 0 and "ok" when all hold.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>

#define GROUP_MCMC_HOST_ONLY
#include "../../newmsm_amd/csrc/group_mcmc.hpp"

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

void check_incidence(const std::vector<int32_t> &pairs, int nodes) {
    const int64_t P = (int64_t)pairs.size() / 2;
    std::vector<int32_t> ptr, idx;
    EXPECT(group_mcmc_incidence(pairs.data(), P, nodes, ptr, idx));
    EXPECT((int)ptr.size() == nodes + 1 && ptr[0] == 0 && (size_t)ptr[(size_t)nodes] == idx.size());
    for (int n = 0; n < nodes; ++n) {
        std::vector<int32_t> want;
        for (int64_t p = 0; p < P; ++p)
            if (pairs[2 * p] == n || pairs[2 * p + 1] == n) want.push_back((int32_t)p);
        const std::vector<int32_t> got(idx.begin() + ptr[(size_t)n], idx.begin() + ptr[(size_t)n + 1]);
        EXPECT(got == want);
    }
}

// estimate_pairs' shape: for a < b and every node v of a, the pair (a N + v, b N + some node of b)
std::vector<int32_t> group_pairs(int S, int N, unsigned seed, int spread) {
    std::mt19937 gen(seed);
    std::vector<int32_t> pairs;
    for (int a = 0; a < S; ++a)
        for (int v = 0; v < N; ++v)
            for (int b = a + 1; b < S; ++b) {
                pairs.push_back(a * N + v);
                pairs.push_back(b * N + (int)(gen() % (unsigned)spread));  // spread < N: nodes beyond it have no incoming pair
            }
    return pairs;
}

}  // namespace

int main() {
    for (int S = 2; S <= 4; ++S) check_incidence(group_pairs(S, 42, 7u + (unsigned)S, 30), S * 42);
    check_incidence(group_pairs(2, 5, 3u, 1), 10);  // every pair ends in one node
    check_incidence({}, 7);
    check_incidence({3, 3, 0, 3, 3, 1}, 4);  // a pair that names a node twice is listed once
    {
        std::vector<int32_t> ptr, idx;
        const std::vector<int32_t> high = {0, 4}, low = {-1, 2};
        EXPECT(!group_mcmc_incidence(high.data(), 1, 4, ptr, idx));
        EXPECT(!group_mcmc_incidence(low.data(), 1, 4, ptr, idx));
    }
    // the seed rule
    EXPECT(group_mcmc_seed(42, 0, 0, 0, 3, 0) == 42);
    for (int it = 0; it < 3; ++it)
        for (int k = 0; k < 4; ++k) EXPECT(group_mcmc_seed(42, it, k, 0, 5, 0) == 42u + (uint64_t)it + (uint64_t)1000003 * (uint64_t)k);  // the pairwise loops' chains
    EXPECT(group_mcmc_seed(1, 2, 3, 1, 4, 2) == 1u + 2u + 3u * (uint64_t)1000003 + (uint64_t)15485863 * 6u);
    EXPECT(group_mcmc_seed(std::numeric_limits<uint64_t>::max(), 1, 0, 0, 2, 0) == 0);  // modulo 2^64
    EXPECT(group_mcmc_seed(0, 0, 255, 1, 64, 63) == (uint64_t)1000003 * 255u + (uint64_t)15485863 * 127u);
    // the acceptance rule
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    EXPECT(!group_mcmc_accept(1.0, 1.0));
    EXPECT(group_mcmc_accept(1.0, std::nextafter(1.0, 0.0)));
    EXPECT(!group_mcmc_accept(1.0, std::nextafter(1.0, 2.0)));
    EXPECT(!group_mcmc_accept(1.0, nan));
    EXPECT(!group_mcmc_accept(nan, 1.0));
    EXPECT(!group_mcmc_accept(nan, nan));
    EXPECT(group_mcmc_accept(inf, 1e7));
    EXPECT(!group_mcmc_accept(inf, inf));
    EXPECT(group_mcmc_accept(-0.0, -1.0) && !group_mcmc_accept(0.0, -0.0));
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
