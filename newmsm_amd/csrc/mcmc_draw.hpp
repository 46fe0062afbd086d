// mcmc_draw.hpp -- the proposal stream of the Monte Carlo optimiser (McmcProposals, mcmc_host.hpp) rebuilt from integer work and single correctly rounded
// IEEE operations, so that a kernel can draw it bit for bit (mcmc_draw_kernels.hip; DESIGN.md 5.16 "Proposals on the device").  Plain C++ (no HIP header:
// tests/cpp/mcmc_draw_host_check.cpp builds it alone under the sanitizers); the per-candidate functions are __host__ __device__ under hipcc, so the host
// mirror below and the kernel share one text.
//
// The host's label is floor(log(1 - u) / log(1 - p)): a non-increasing step function of x = 1 - u.  Its steps are located once per call on the host with
// the host's own log (mcmc_draw_thresholds); a label is then the number of steps above x, found by comparing bit patterns.  No logarithm is taken anywhere
// but in the bisection.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define MSM_DRAW_HD __host__ __device__ __forceinline__
#else
#define MSM_DRAW_HD inline
#endif

namespace msm {

constexpr int kMtWords = 624;                  // the state of std::mt19937
constexpr int kMtShift = 397;                  // its m
constexpr int kDrawCandidates = kMtWords / 2;  // a regenerated state is 312 whole candidates (two words each)
constexpr uint64_t kDrawLowestBits = 0x3CA0000000000000ull;  // the bit pattern of 2^-53, the smallest 1 - u
constexpr uint64_t kDrawOneBits = 0x3FF0000000000000ull;     // of 1.0, the largest

// ---------------------------------------------------------------- per word and per candidate: the kernel's text

// word i of the next state from old word i, old word i + 1 and word i + 397 (old for i < 227, new after that)
MSM_DRAW_HD uint32_t mt_twist(uint32_t cur, uint32_t next, uint32_t far) {
    const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

MSM_DRAW_HD uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// generate_canonical<double, 53> of libstdc++ over two words, then 1.0 - u: the bits of x.  double(w1) * 2^32 is exact, the sum rounds once, the
// division by 2^64 is exact, the subtraction rounds once.
MSM_DRAW_HD uint64_t candidate_bits(uint32_t w0, uint32_t w1) {
    const double sum = (double)w0 + (double)w1 * 4294967296.0;
    double u = sum / 18446744073709551616.0;
    if (u >= 1.0) u = 0x1.fffffffffffffp-1;  // nextafter(1, 0)
    const double x = 1.0 - u;
    uint64_t bits;
    __builtin_memcpy(&bits, &x, sizeof(bits));
    return bits;
}

// the number of k in 1 .. L with bits < thr[k - 1]; thr is non-increasing, so this is the first index whose threshold is not above bits.  L itself: rejected.
MSM_DRAW_HD int label_of(uint64_t bits, const uint64_t *thr, int L) {
    int lo = 0, hi = L;  // thr[i] > bits for i < lo, thr[i] <= bits for i >= hi
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bits < thr[mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- host only

inline void mt_seed(uint64_t seed, uint32_t *state /* 624 */) {
    state[0] = (uint32_t)seed;  // std::mt19937 takes the low 32 bits
    for (int i = 1; i < kMtWords; ++i) state[i] = 1812433253u * (state[i - 1] ^ (state[i - 1] >> 30)) + (uint32_t)i;
}

// in place, in the kernel's phases: [0, 227) reads old words only, [227, 623) reads the new words 227 places back, word 623 the new word 0
inline void mt_regenerate(uint32_t *state /* 624 */) {
    for (int i = 0; i < kMtWords - kMtShift; ++i) state[i] = mt_twist(state[i], state[i + 1], state[i + kMtShift]);
    for (int i = kMtWords - kMtShift; i < kMtWords - 1; ++i) state[i] = mt_twist(state[i], state[i + 1], state[i + kMtShift - kMtWords]);
    state[kMtWords - 1] = mt_twist(state[kMtWords - 1], state[0], state[kMtShift - 1]);
}

// f(x) = floor(log(x) / c) of the bit pattern of x, as std::geometric_distribution computes it (c = log(1 - p), -inf for p = 1)
inline double mcmc_draw_step(uint64_t bits, double c) {
    double x;
    std::memcpy(&x, &bits, sizeof(x));
    return std::floor(std::log(x) / c);
}

// thr[k - 1] for k = 1 .. L: the bit pattern of the smallest double in [2^-53, 1] with f <= k - 1, by bisection on bit patterns (positive doubles order as
// their patterns do); 2^-53's pattern where f is that low already.  Non-increasing in k.
inline void mcmc_draw_thresholds(int L, double mcparam, uint64_t *thr) {
    const double c = std::log(1.0 - mcparam);
    uint64_t top = kDrawOneBits;  // f(1) = 0 <= k - 1 for every k; thr[k] <= thr[k - 1], so the search for k starts below the previous threshold
    for (int k = 1; k <= L; ++k) {
        const double level = (double)(k - 1);
        if (mcmc_draw_step(kDrawLowestBits, c) <= level) {
            for (; k <= L; ++k) thr[k - 1] = kDrawLowestBits;
            return;
        }
        uint64_t lo = kDrawLowestBits, hi = top;  // f(lo) > k - 1, f(hi) <= k - 1
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (mcmc_draw_step(mid, c) <= level) hi = mid;
            else lo = mid;
        }
        thr[k - 1] = top = hi;
    }
}

// 312-candidate blocks the kernel may generate for `need` accepted proposals: the mean of the negative-binomial candidate count, sixteen of its standard
// deviations, the up to 312 left-over candidates either side, and one block more
inline long mcmc_draw_block_bound(long need, int L, double mcparam) {
    const double a = mcparam >= 1.0 ? 1.0 : 1.0 - std::pow(1.0 - mcparam, (double)L);  // the acceptance probability
    const double n = (double)need;
    return (long)std::ceil((n / a + 16.0 * std::sqrt(n * (1.0 - a)) / a + 624.0) / 312.0) + 1;
}

// The whole stream from the pieces above and nothing else (no std::mt19937, no std::geometric_distribution): what the kernel computes, one candidate at a
// time.  `state` and `consumed` are the record a chain keeps between chunks.
struct McmcDrawMirror {
    uint32_t state[kMtWords];
    int consumed = kDrawCandidates;  // candidates of the current block already taken: a fresh engine has none left
    int L;
    std::vector<uint64_t> thr;
    uint64_t candidates = 0, blocks = 0;
    McmcDrawMirror(uint64_t seed, double mcparam, int L_) : L(L_), thr((size_t)L_) {
        mt_seed(seed, state);
        mcmc_draw_thresholds(L, mcparam, thr.data());
    }
    int next() {
        for (;;) {
            if (consumed == kDrawCandidates) {
                mt_regenerate(state);
                consumed = 0;
                ++blocks;
            }
            const uint32_t w0 = mt_temper(state[2 * consumed]), w1 = mt_temper(state[2 * consumed + 1]);
            ++consumed;
            ++candidates;
            const int label = label_of(candidate_bits(w0, w1), thr.data(), L);
            if (label < L) return label;
        }
    }
    void fill(uint16_t *out, size_t n) {  // L <= 65535 (checked by the callers)
        for (size_t i = 0; i < n; ++i) out[i] = (uint16_t)next();
    }
};

}  // namespace msm
