// mcmc_host_check.cpp -- the host pieces of the Monte Carlo optimiser's GPU sweeps (newmsm_amd/csrc/mcmc_host.hpp) on their own, so that they can be built
// and run under the sanitizers without HIP or Python:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/mcmc_host_check.cpp -o mcmc_host_check && ./mcmc_host_check
// Checks the level schedule's three properties on lists that are meshes and lists that are not, replays a sweep level by level against the serial sweep,
// and compares the chunked proposal stream with the serial loop of std::mt19937 + std::geometric_distribution.  Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <set>

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

int check_schedule(const std::vector<int32_t> &tr, int N) {
    const int T = (int)(tr.size() / 3);
    McmcSchedule s;
    mcmc_build_schedule(tr.data(), N, T, s);
    EXPECT((int)s.order.size() == T && (int)s.level.size() == T && s.level_off.front() == 0 && s.level_off.back() == T);
    std::vector<int> seen((size_t)T, 0);
    for (int t : s.order) ++seen[(size_t)t];
    for (int t = 0; t < T; ++t) EXPECT(seen[(size_t)t] == 1);
    for (int l = 0; l < s.levels(); ++l) {
        std::set<int32_t> nodes;
        size_t named = 0;
        for (int i = s.level_off[(size_t)l]; i < s.level_off[(size_t)l + 1]; ++i) {
            const int t = s.order[(size_t)i];
            EXPECT(s.level[(size_t)t] == l);
            if (i > s.level_off[(size_t)l]) EXPECT(s.order[(size_t)i - 1] < t);
            const std::set<int32_t> own(tr.begin() + 3 * t, tr.begin() + 3 * t + 3);
            named += own.size();
            nodes.insert(own.begin(), own.end());
        }
        EXPECT(named == nodes.size());  // no two triplets of a level share a node
    }
    std::vector<int> last((size_t)N, -1);
    for (int t = 0; t < T; ++t) {
        int want = 0;
        for (int j = 0; j < 3; ++j) want = std::max(want, last[(size_t)tr[3 * (size_t)t + j]] + 1);
        EXPECT(s.level[(size_t)t] == want);
        for (int j = 0; j < 3; ++j) last[(size_t)tr[3 * (size_t)t + j]] = want;
    }
    return s.levels();
}

// a visit whose outcome depends on the labels it reads: the order of the visits that share a node shows in the result
void visit(std::vector<int> &lab, const int32_t *n, int p, int t) {
    const int h = (lab[(size_t)n[0]] * 7 + lab[(size_t)n[1]] * 3 + lab[(size_t)n[2]] + p + t) % 8;
    for (int j = 0; j < 3; ++j)
        if (h & (4 >> j)) lab[(size_t)n[j]] = p;
}

void check_walk(const std::vector<int32_t> &tr, int N, int L, int sweeps) {
    const int T = (int)(tr.size() / 3);
    McmcSchedule s;
    mcmc_build_schedule(tr.data(), N, T, s);
    McmcProposals a(5, 0.4, L), b(5, 0.4, L);
    std::vector<int> serial((size_t)N, 0), levelled((size_t)N, 0);
    std::vector<uint16_t> chunk((size_t)T);
    for (int sw = 0; sw < sweeps; ++sw) {
        for (int t = 0; t < T; ++t) visit(serial, &tr[3 * (size_t)t], a.next(), t);
        b.fill(chunk.data(), chunk.size());
        for (int l = 0; l < s.levels(); ++l)
            for (int i = s.level_off[(size_t)l + 1] - 1; i >= s.level_off[(size_t)l]; --i) {  // a level's triplets in any order: here backwards
                const int t = s.order[(size_t)i];
                visit(levelled, &tr[3 * (size_t)t], chunk[(size_t)t], t);
            }
    }
    EXPECT(serial == levelled);
}

void check_stream(double mcparam, int L, int T, int sweeps, int chunk_sweeps) {
    std::mt19937 gen(17);
    std::geometric_distribution<> dist(mcparam);
    McmcProposals p(17, mcparam, L);
    std::vector<uint16_t> chunk((size_t)chunk_sweeps * T);
    size_t bad = 0;
    for (int done = 0; done < sweeps; done += chunk_sweeps) {
        const size_t n = (size_t)std::min(chunk_sweeps, sweeps - done) * T;
        p.fill(chunk.data(), n);
        for (size_t i = 0; i < n; ++i) {
            int label;
            do { label = dist(gen); } while (label >= L);
            bad += chunk[i] != label;
        }
    }
    EXPECT(bad == 0);
}

}  // namespace

int main() {
    // a strip of triangles over 40 nodes and back again, a node named twice, identical triplets, a chain on one node, disjoint triplets, nothing at all
    std::vector<int32_t> strip;
    for (int i = 0; i + 2 < 40; ++i) strip.insert(strip.end(), {i, i + 1, i + 2});
    for (int i = 37; i >= 0; i -= 3) strip.insert(strip.end(), {i + 2, i, i + 1});
    check_schedule(strip, 40);
    check_walk(strip, 40, 5, 9);
    const std::vector<int32_t> odd = {0, 0, 1, 2, 3, 4, 2, 3, 4, 1, 1, 1, 4, 0, 5};
    EXPECT(check_schedule(odd, 6) == 3);
    check_walk(odd, 6, 3, 20);
    EXPECT(check_schedule(std::vector<int32_t>(21, 0), 1) == 7);
    std::vector<int32_t> disjoint(300);
    for (int i = 0; i < 300; ++i) disjoint[(size_t)i] = i;
    EXPECT(check_schedule(disjoint, 300) == 1);
    EXPECT(check_schedule({}, 3) == 0);
    std::srand(3);
    std::vector<int32_t> random_list(3 * 500);
    for (auto &v : random_list) v = std::rand() % 97;
    check_schedule(random_list, 97);
    check_walk(random_list, 97, 19, 6);
    for (double mcparam : {0.3, 0.8, 1.0})
        for (int L : {3, 19}) check_stream(mcparam, L, 320, 70, 3);
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
