// level_features_host_check.cpp -- the host pieces of msm_level_features (newmsm_amd/csrc/varnorm.hpp: the row body of variance_normalise and the one
// parallel section over the rows of all data sets) on their own, so that they can be built and run under the sanitizers without HIP or Python:
//     g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/level_features_host_check.cpp -o check && ./check
// Compares the batched section with the row body called row by row (byte for byte) for 1, 3, 4 and 17 rows, with and without masks, and checks the
// degenerate rows: a mask that keeps nothing, one kept value, a constant row.  Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../newmsm_amd/csrc/varnorm.hpp"

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

void check_batch(int n, int D, int V, bool masked, unsigned seed) {
    std::mt19937 rng(seed);
    std::normal_distribution<double> g(1.0, 2.0);
    std::vector<double> feat((size_t)n * D * V), mask((size_t)n * V);
    for (double &x : feat) x = g(rng);
    for (double &m : mask) m = (rng() % 10) ? 0.25 + (rng() % 4) * 0.25 : 0.0;
    std::vector<double> want = feat, got = feat;
    for (int r = 0; r < n * D; ++r) variance_normalise_row(want.data() + (size_t)r * V, V, masked ? mask.data() + (size_t)(r / D) * V : nullptr);
    variance_normalise_rows(got.data(), n, D, V, masked ? mask.data() : nullptr);
    EXPECT(std::memcmp(got.data(), want.data(), sizeof(double) * got.size()) == 0);
    if (!masked) {  // mean 0, unit sample variance
        double s = 0, q = 0;
        for (int i = 0; i < V; ++i) s += got[(size_t)i], q += got[(size_t)i] * got[(size_t)i];
        EXPECT(std::fabs(s / V) < 1e-12 && std::fabs(q / (V - 1) - 1.0) < 1e-9);
    }
}

void check_degenerate() {
    const int V = 37;
    std::vector<double> row(V), mask(V, 0.0), before;
    for (int i = 0; i < V; ++i) row[(size_t)i] = 0.5 * i - 3.0;
    before = row;
    variance_normalise_row(row.data(), V, mask.data());  // nothing kept: n - 1 wraps, var = 0 / 2^64, nothing is touched
    EXPECT(std::memcmp(row.data(), before.data(), sizeof(double) * V) == 0);
    mask[11] = 1.0;
    variance_normalise_row(row.data(), V, mask.data());  // one kept value: var = 0 / 0 is NaN, `var > 0` is false: the value minus its mean
    for (int i = 0; i < V; ++i) EXPECT(i == 11 ? row[(size_t)i] == 0.0 : row[(size_t)i] == before[(size_t)i]);
    std::vector<double> flat(V, 2.5);
    variance_normalise_row(flat.data(), V, nullptr);  // var == 0: the mean is taken off, nothing is divided
    for (int i = 0; i < V; ++i) EXPECT(flat[(size_t)i] == 0.0);
    variance_normalise_rows(nullptr, 0, 3, V, nullptr);  // no rows: no section
}

}  // namespace

int main() {
    for (int masked = 0; masked < 2; ++masked) {
        check_batch(1, 1, 501, masked != 0, 1);
        check_batch(3, 1, 501, masked != 0, 2);
        check_batch(2, 2, 501, masked != 0, 3);
        check_batch(17, 1, 130, masked != 0, 4);
        check_batch(5, 7, 64, masked != 0, 5);
    }
    check_degenerate();
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
