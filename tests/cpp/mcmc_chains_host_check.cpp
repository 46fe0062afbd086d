// mcmc_chains_host_check.cpp -- the host pieces of several Monte Carlo chains in one launch (newmsm_amd/csrc/mcmc_host.hpp, host_parallel.hpp) on their own,
// so that they can be built and run under the sanitizers without HIP or Python, once with -fsanitize=address,undefined and once with -fsanitize=thread:
//     g++ -std=c++17 -O1 -g -pthread -fsanitize=thread tests/cpp/mcmc_chains_host_check.cpp -o mcmc_chains_host_check && ./mcmc_chains_host_check
// Draws the streams of 1, 5 and 17 chains on 1, 4 and 16 threads in chunks of 1 sweep, of 3 and of the whole run into the kernel's chunk layout and compares
// every label with McmcProposals drawn serially; checks the chunk length rule, the energy against a plain serial sum and the choice of the best chain on
// crafted energies.  Exit status 0 and "ok" when all hold.
#include <cmath>
#include <cstdio>
#include <limits>
#include <numeric>

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

// K streams drawn chunk by chunk on `threads` threads into chains x chunk x T, each label at its triplet's place; against the serial stream of every seed
void check_draw(int K, int threads, int chunk, int T, int sweeps, int L, double mcparam) {
    std::vector<uint64_t> seeds((size_t)K);
    for (int k = 0; k < K; ++k) seeds[(size_t)k] = 11 + (uint64_t)1000003 * (uint64_t)k;
    std::vector<int32_t> pos((size_t)T);  // a permutation that is not the identity: triplet t stands at (7 t + 3) mod T (T is no multiple of 7)
    for (int t = 0; t < T; ++t) pos[(size_t)t] = (int32_t)((7 * (long)t + 3) % T);
    std::vector<std::vector<uint16_t>> want((size_t)K);
    for (int k = 0; k < K; ++k) {
        McmcProposals p(seeds[(size_t)k], mcparam, L);
        want[(size_t)k].resize((size_t)sweeps * T);
        p.fill(want[(size_t)k].data(), want[(size_t)k].size());
    }
    McmcChainStreams streams(seeds.data(), K, mcparam, L);
    EXPECT(streams.chains() == K);
    std::vector<uint16_t> buf((size_t)K * chunk * T, (uint16_t)0xFFFF);
    size_t bad = 0;
    for (int done = 0; done < sweeps; done += chunk) {
        const int n = std::min(chunk, sweeps - done);
        streams.draw(buf.data(), chunk, n, T, pos.data(), threads);
        for (int k = 0; k < K; ++k)
            for (int s = 0; s < n; ++s)
                for (int t = 0; t < T; ++t)
                    bad += buf[((size_t)k * chunk + s) * T + (size_t)pos[(size_t)t]] != want[(size_t)k][(size_t)(done + s) * T + t];
    }
    EXPECT(bad == 0);
}

void check_energy() {
    const int N = 23, L = 4, T = 31;
    std::mt19937 gen(5);
    std::uniform_real_distribution<double> val(-3.0, 3.0);
    std::vector<double> U((size_t)L * N), tc((size_t)T * L * L * L);
    for (double &v : U) v = val(gen);
    for (double &v : tc) v = val(gen);
    std::vector<int32_t> tr(3 * (size_t)T), lab((size_t)N);
    for (int32_t &v : tr) v = (int32_t)(gen() % N);
    for (int32_t &v : lab) v = (int32_t)(gen() % L);
    std::vector<double> terms((size_t)N + T);
    mcmc_energy_terms(U.data(), tc.data(), tr.data(), N, L, T, lab.data(), terms.data());
    double u = 0.0, t3 = 0.0;
    for (int i = 0; i < N; ++i) u += U[(size_t)lab[(size_t)i] * N + i];
    for (int t = 0; t < T; ++t)
        t3 += tc[(((size_t)t * L + lab[(size_t)tr[3 * (size_t)t]]) * L + lab[(size_t)tr[3 * (size_t)t + 1]]) * L + lab[(size_t)tr[3 * (size_t)t + 2]]];
    const double want = u + 0.0 + t3, got = mcmc_energy_of_terms(terms.data(), N, T);
    EXPECT(got == want);
    EXPECT(mcmc_energy_of_terms(terms.data(), N, 0) == u + 0.0 + 0.0);
    // the order is part of the definition: 1e16 + 1 + 1 - 1e16 is 0 from the left and 2 pairwise
    const double order[4] = {1e16, 1.0, 1.0, -1e16};
    EXPECT(mcmc_energy_of_terms(order, 4, 0) == 0.0);
    EXPECT(mcmc_energy_of_terms(order, 1, 3) == 1e16 + ((0.0 + 1.0 + 1.0) + -1e16));
}

void check_best() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double one[] = {4.0};
    EXPECT(mcmc_best_chain(one, 1) == 0);
    const double ties[] = {3.0, 1.0, 2.0, 1.0, 1.0};
    EXPECT(mcmc_best_chain(ties, 5) == 1);  // the lower index of equal energies
    const double nan_first[] = {nan, -5.0, 1.0};
    EXPECT(mcmc_best_chain(nan_first, 3) == 0);  // nothing beats a NaN in slot 0
    const double nan_later[] = {2.0, nan, 1.0, nan};
    EXPECT(mcmc_best_chain(nan_later, 4) == 2);  // a NaN never beats anything
    const double infs[] = {inf, -inf, -inf};
    EXPECT(mcmc_best_chain(infs, 3) == 1);
    const double equal[] = {7.5, 7.5};
    EXPECT(mcmc_best_chain(equal, 2) == 0);
}

void check_chunk_length() {
    EXPECT(mcmc_chunk_sweeps(0, 5120, 2000, 1) == 102);                 // half a million proposals per chain
    EXPECT(mcmc_chunk_sweeps(0, 5120, 2000, 16) == 102);                // 16 x 102 x 5120 x 2 bytes < 16 MB
    EXPECT(mcmc_chunk_sweeps(0, 5120, 2000, 64) == (1 << 23) / (5120 * 64));  // reduced: 25 sweeps
    EXPECT((size_t)mcmc_chunk_sweeps(0, 5120, 2000, 256) * 5120 * 256 * 2 <= ((size_t)16 << 20));
    EXPECT(mcmc_chunk_sweeps(0, 80000 * 3, 10, 256) == 1);              // at least one sweep
    EXPECT(mcmc_chunk_sweeps(3, 320, 50, 17) == 3 && mcmc_chunk_sweeps(1, 320, 50, 17) == 1);  // the environment's value is per chain
    EXPECT(mcmc_chunk_sweeps(0, 20, 50, 5) == 50 && mcmc_chunk_sweeps(1000, 20, 50, 5) == 50);  // never more than the run
    EXPECT(mcmc_chunk_sweeps(0, 0, 5, 2) == 5);
    // one chain: the rule the single-chain sweeps had before they became the chains' with K = 1 (the 2^23 bound never binds below 2^19 per chain)
    for (long asked : {-5L, 0L, 1L, 3L, 102L, 1000000000L, 1L << 40})
        for (int T : {0, 1, 20, 320, 5120, 240000})
            for (int iters : {1, 50, 2000, 100000}) {
                const long per = std::max(T, 1);
                const long want = std::max(1L, std::min(std::min(asked > 0 ? asked : (1L << 19) / per, (1L << 30) / per), (long)iters));
                EXPECT(mcmc_chunk_sweeps(asked, T, iters, 1) == (int)want);
            }
}

}  // namespace

int main() {
    const int T = 37, sweeps = 10;
    for (int K : {1, 5, 17})
        for (int threads : {1, 4, 16})
            for (int chunk : {1, 3, sweeps}) check_draw(K, threads, chunk, T, sweeps, 19, 0.3);
    check_draw(5, 4, 3, T, sweeps, 3, 1.0);  // parameter 1: label 0 only
    EXPECT(mcmc_draw_threads(1) == 1 && mcmc_draw_threads(256) <= 16 && mcmc_draw_threads(3) <= 3);
    check_energy();
    check_best();
    check_chunk_length();
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
