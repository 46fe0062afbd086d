// mcmc_draw_kernels.hip -- the proposal streams of the Monte Carlo optimiser's chains drawn on the device, bit for bit the host's (mcmc_draw.hpp, mcmc.hpp;
// DESIGN.md 5.16 "Proposals on the device").
//
// One workgroup per chain, the chain's std::mt19937 state (624 words) in LDS.  Per block of 312 candidates: the state is regenerated in the recurrence's
// three phases, every thread tempers two words into one candidate and classifies it against the host's thresholds, an ordered prefix sum over the accept
// flags numbers the accepted ones in stream order, and each goes to its place in the buffer the sweeps kernels read.  The arithmetic per candidate is
// mcmc_draw.hpp's and nothing else: integer work, one int -> double conversion each, one multiplication and one division by a power of two (exact), one
// addition and one subtraction (each correctly rounded); no logarithm.
//
// A chunk usually ends inside a block, so the state and the number of its candidates already taken go back to the chain's record; the next launch starts
// there and recomputes the rest of the block.  The workgroups never meet: no atomic but the status word's on the error path, every loop bounded by the
// host's counts (the proposals wanted and the block bound).
#include "mcmc.hpp"

namespace msm {

namespace {

constexpr int kDrawWaves = kMcmcDrawThreads / 64;

// LDS: s_thr (dynamic, L thresholds) when kThrLds, else none
template <bool kThrLds>
__global__ __launch_bounds__(kMcmcDrawThreads) void k_mcmc_draw(McmcDrawArgs d) {
    extern __shared__ __align__(16) uint64_t s_thr[];
    __shared__ uint32_t s_mt[kMtWords];
    __shared__ uint32_t s_wave[kDrawWaves];
    __shared__ uint32_t s_end;  // the candidates of the last block taken by the chunk
    const int tid = (int)threadIdx.x, k = (int)blockIdx.x;
    if (k >= d.chains) return;  // (the whole workgroup)
    McmcDrawRecord *__restrict__ rec = d.rec + k;
    for (int i = tid; i < kMtWords; i += kMcmcDrawThreads) s_mt[i] = rec->state[i];
    if (kThrLds)
        for (int i = tid; i < d.L; i += kMcmcDrawThreads) s_thr[i] = d.thr[i];
    const uint64_t *thr = kThrLds ? s_thr : d.thr;
    uint32_t consumed = rec->consumed;
    if (consumed > (uint32_t)kDrawCandidates) consumed = kDrawCandidates;  // (the host writes 0 .. 312)
    __syncthreads();
    uint16_t *__restrict__ out = d.prop + (size_t)k * d.chunk_sweeps * d.T;
    const uint32_t need = d.need, T = (uint32_t)d.T;
    uint32_t produced = 0;
    unsigned long long candidates = 0;
    long blocks = 0;
    bool finished = need == 0;
    // at most max_blocks regenerations, and one pass more over what the record left of its block
    for (long pass = 0; !finished && pass <= d.max_blocks; ++pass) {
        if (consumed >= (uint32_t)kDrawCandidates) {
            if (blocks >= d.max_blocks) break;
            // every word's old neighbours into registers before anything is overwritten: thread t owns words t, 227 + t and 454 + t (623 goes with 454 + 169)
            uint32_t a0 = 0, a1 = 0, b0 = 0, b1 = 0, c0 = 0, c1 = 0;
            if (tid < 227) {
                a0 = s_mt[tid];
                a1 = s_mt[tid + 1];
                b0 = s_mt[227 + tid];
                b1 = s_mt[228 + tid];
            }
            if (tid < 170) {
                c0 = s_mt[454 + tid];
                c1 = tid < 169 ? s_mt[455 + tid] : 0u;
            }
            __syncthreads();
            if (tid < 227) s_mt[tid] = mt_twist(a0, a1, s_mt[tid + kMtShift]);  // [0, 227): word i + 397 is old
            __syncthreads();
            if (tid < 227) s_mt[227 + tid] = mt_twist(b0, b1, s_mt[tid]);  // [227, 454): word i - 227 is new
            __syncthreads();
            if (tid < 169) s_mt[454 + tid] = mt_twist(c0, c1, s_mt[227 + tid]);  // [454, 623)
            if (tid == 169) s_mt[623] = mt_twist(c0, s_mt[0], s_mt[396]);       // 623: its neighbour is the new word 0
            __syncthreads();
            consumed = 0;
            ++blocks;
        }
        // candidate tid of the block, if the stream has not passed it yet
        const bool live = tid < kDrawCandidates && (uint32_t)tid >= consumed;
        int label = d.L;
        if (live) label = label_of(candidate_bits(mt_temper(s_mt[2 * tid]), mt_temper(s_mt[2 * tid + 1])), thr, d.L);
        const bool accept = live && label < d.L;
        // ordered prefix sum of the accept flags: within the wavefront by ballot, across the five wavefronts through LDS
        const unsigned long long votes = __ballot(accept);
        const int lane = tid & 63, wave = tid >> 6;
        const uint32_t before = (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(votes);
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kDrawWaves; ++w) {
            const uint32_t n = s_wave[w];
            if (w < wave) base += n;
            total += n;
        }
        const uint32_t j = produced + base + before;  // this proposal's number in the chunk
        if (accept && j < need) {
            const uint32_t sweep = j / T, t = j - sweep * T;
            const uint32_t p = d.pos ? (uint32_t)d.pos[t] : t;
            if (p < T) out[(size_t)sweep * T + p] = (uint16_t)label;
            else atomicMin(d.status, MSM_ERR_INVALID);  // (the host has checked: what is out of range indexes nothing)
            if (j == need - 1) s_end = (uint32_t)tid + 1;
        }
        finished = produced + total >= need;  // (uniform: every thread has read the same counts)
        __syncthreads();                      // s_wave is free for the next pass, s_end is written
        if (finished) {
            const uint32_t end = s_end;
            candidates += end - consumed;
            consumed = end;
        } else {
            candidates += (uint32_t)kDrawCandidates - consumed;
            consumed = kDrawCandidates;
            produced += total;
        }
    }
    if (!finished) atomicMin(d.status, MSM_ERR_CAPACITY);  // the block bound came first: the chunk is incomplete, the call fails
    for (int i = tid; i < kMtWords; i += kMcmcDrawThreads) rec->state[i] = s_mt[i];
    if (tid == 0) {
        rec->consumed = consumed;
        rec->candidates += candidates;
        rec->accepted += finished ? need : produced;
    }
}

}  // namespace

int launch_mcmc_draw(msm_ctx *ctx, const McmcDrawArgs &d, hipStream_t stream) {
    if (d.need == 0 || d.T <= 0) return MSM_OK;
    if (d.chains < 1 || d.chains > kMcmcMaxChains || d.L < 1 || d.L > 65535 || d.max_blocks < 0 || (size_t)d.need > (size_t)d.chunk_sweeps * (size_t)d.T)
        return fail(MSM_ERR_INVALID, "mcmc draw: bad launch (%d chains, %d labels, %u proposals of %d x %d)", d.chains, d.L, d.need, d.chunk_sweeps, d.T);
    if (d.L <= kMcmcDrawLdsLabels)
        hipLaunchKernelGGL(k_mcmc_draw<true>, dim3((unsigned)d.chains), dim3(kMcmcDrawThreads), sizeof(uint64_t) * (size_t)d.L, stream, d);
    else
        hipLaunchKernelGGL(k_mcmc_draw<false>, dim3((unsigned)d.chains), dim3(kMcmcDrawThreads), 0, stream, d);
    MSM_HIP(hipGetLastError());
    (void)ctx;
    return MSM_OK;
}

}  // namespace msm
