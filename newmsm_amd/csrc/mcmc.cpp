// mcmc.cpp -- the host side of the Monte Carlo optimiser's GPU sweeps (mcmc.hpp; kernel: mcmc_kernels.hip): the level schedule, the
// proposal streams of K chains from one start in chunks of whole sweeps, and the one loop that draws chunk c + 1 while the device walks chunk c (the
// streams drawn on the host workers, the chains' energies summed here, the best one kept; a single chain is K = 1), and the host-only chains, energy and
// selection.  With msm_ctx_set_mcmc_draw(ctx, 1) the streams are drawn by a kernel on a side stream instead (DeviceDraw; mcmc_draw.hpp,
// mcmc_draw_kernels.hip).
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "mcmc.hpp"

using namespace msm;

namespace msm {

// the refusals that recur, each reported under the name `what`
static int check_mcparam(const char *what, double mcparam) {
    if (!(mcparam > 0.0 && mcparam <= 1.0)) return fail(MSM_ERR_INVALID, "%s: the geometric distribution parameter must be in (0, 1]", what);
    return MSM_OK;
}

static int check_label_count(const char *what, int L) {
    if (L > 65535) return fail(MSM_ERR_INVALID, "%s: %d labels; the proposals travel as 16-bit values (at most 65535)", what, L);
    return MSM_OK;
}

int mcmc_check_node_count(const char *what, int N) {
    if (N > kMcmcMaxNodes) return fail(MSM_ERR_CAPACITY, "%s: the labels of %d nodes do not fit the LDS of one workgroup (at most %d)", what, N, kMcmcMaxNodes);
    return MSM_OK;
}

static int check_labels(const int32_t *labeling, int N, int L) {
    for (int i = 0; i < N; ++i)
        if (labeling[i] < 0 || labeling[i] >= L) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise: label of node %d out of range", i);
    return MSM_OK;
}

static int check_triplets(const int32_t *triplets, int N, int T) {
    for (int64_t i = 0; i < 3 * (int64_t)T; ++i)
        if (triplets[i] < 0 || triplets[i] >= N) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise: triplet node out of range");
    return MSM_OK;
}

int mcmc_check_arguments(const int32_t *triplets, int N, int L, int T, double mcparam, const int32_t *labeling) {
    MSM_TRY(check_mcparam("msm_mcmc_optimise", mcparam));
    MSM_TRY(check_labels(labeling, N, L));
    return check_triplets(triplets, N, T);
}

int mcmc_check_chains(const uint64_t *seeds, int K) {
    if (K < 1 || K > kMcmcMaxChains) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise_chains: %d chains (1 to %d)", K, kMcmcMaxChains);
    if (!seeds) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise_chains: null seeds");
    return MSM_OK;
}

// host -> device through the staging blocks in pieces (a table of 281 MB must not ask for one staging block of its size)
int upload_in_pieces(msm_ctx *ctx, void *dst, const void *src, size_t bytes) {
    const size_t piece = (size_t)16 << 20;
    for (size_t off = 0; off < bytes; off += piece)
        MSM_TRY(stage_h2d(ctx, (char *)dst + off, (const char *)src + off, std::min(piece, bytes - off)));
    return MSM_OK;
}

}  // namespace msm

namespace {

struct McmcScratch {
    DevBuf<double> U, tc;  // the host tables of msm_mcmc_optimise_gpu
    DevBuf<int4> sched;
    DevBuf<int32_t> level_off, labeling;
    DevBuf<uint16_t> prop;
    DevBuf<double> terms;        // K x (N + T) terms of the chains' energies
    std::vector<hipEvent_t> ev;  // a pair per chunk
    double stats[6] = {0, 0, 0, 0, 0, 0};
    int chains = 1, draw_threads = 1;  // of the last call
    // proposals drawn on the device (DeviceDraw below): the second proposal buffer, the thresholds, the chains' records, the triplets' places, the draw's
    // own status word, a side stream on which the draw of chunk c + 1 runs beside the sweeps of chunk c, and a pair of events per chunk around the kernel
    DevBuf<uint16_t> prop2;
    DevBuf<uint64_t> thr;
    DevBuf<McmcDrawRecord> rec;
    DevBuf<int32_t> pos;
    DevBuf<int> draw_status;
    hipStream_t draw_stream = nullptr;
    hipEvent_t draw_begin = nullptr;
    std::vector<hipEvent_t> draw_ev;
    double draw_stats[4] = {0, 0, 0, 0};
    ~McmcScratch() {
        if (draw_stream) {
            (void)hipStreamSynchronize(draw_stream);
            (void)hipStreamDestroy(draw_stream);
        }
        if (draw_begin) (void)hipEventDestroy(draw_begin);
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : draw_ev) (void)hipEventDestroy(e);
    }
};

McmcScratch &mcmc_scratch(msm_ctx *ctx) {
    if (!ctx->mcmc_scratch) ctx->mcmc_scratch = std::shared_ptr<void>(new McmcScratch(), [](void *p) { delete static_cast<McmcScratch *>(p); });
    return *static_cast<McmcScratch *>(ctx->mcmc_scratch.get());
}

// a pool of timing events, a pair per chunk: grown to `pairs` pairs, and the time between the two events of each of the first `pairs` pairs, summed
int grow_event_pairs(std::vector<hipEvent_t> &ev, int pairs) {
    while (ev.size() < 2 * (size_t)pairs) {
        hipEvent_t e;
        MSM_HIP(hipEventCreate(&e));
        ev.push_back(e);
    }
    return MSM_OK;
}

int sum_event_pairs(const std::vector<hipEvent_t> &ev, int pairs, double *ms) {
    *ms = 0.0;
    for (int c = 0; c < pairs; ++c) {
        float f = 0.f;
        MSM_HIP(hipEventElapsedTime(&f, ev[2 * (size_t)c], ev[2 * (size_t)c + 1]));
        *ms += f;
    }
    return MSM_OK;
}

// The proposals of K chains drawn on the device, chunk by chunk (k_mcmc_draw; DESIGN.md 5.16 "Proposals on the device").  begin() uploads what the host
// computes once per call -- the thresholds, the seeded engines, the triplets' places -- and lets the side stream wait for the context's; draw() queues
// chunk c there, behind `after` when the buffer it fills is still being walked; join() lets the context's stream wait for chunk c; collect() queues the
// downloads of the status word and the records on the context's stream and finish(), after that stream's sync, reads them.  Every draw has been joined
// when the entry point downloads, so the context's stream alone describes the call (msm_ctx_wait_stream's contract).
struct DeviceDraw {
    msm_ctx *ctx = nullptr;
    McmcScratch *s = nullptr;
    McmcDrawArgs d;
    double mcparam = 0.0;
    long forced_blocks = 0;  // MSMHIP_MCMC_DRAW_BLOCKS (testing): the block bound, whatever the formula says
    int chunks_drawn = 0;
    std::vector<McmcDrawRecord> recs;
    int status = 0;

    int begin(msm_ctx *ctx_, McmcScratch &s_, int L, double mcparam_, const uint64_t *seeds, int K, int T, int stride, const int32_t *pos, int chunks) {
        ctx = ctx_;
        s = &s_;
        mcparam = mcparam_;
        if (const char *e = std::getenv("MSMHIP_MCMC_DRAW_BLOCKS")) forced_blocks = std::max(0L, std::atol(e));
        std::vector<uint64_t> thr((size_t)L);
        mcmc_draw_thresholds(L, mcparam, thr.data());
        recs.assign((size_t)K, McmcDrawRecord());
        for (int k = 0; k < K; ++k) {
            McmcDrawRecord &r = recs[(size_t)k];
            mt_seed(seeds[k], r.state);
            r.consumed = kDrawCandidates;
            r.pad = 0;
            r.candidates = r.accepted = 0;
        }
        MSM_TRY(s->thr.upload_vec(thr, ctx));
        MSM_TRY(s->rec.upload_vec(recs, ctx));
        if (pos) MSM_TRY(s->pos.upload(pos, (size_t)T, ctx));
        if (s->draw_status.zero(1, ctx->stream) != hipSuccess) return stage_alloc_failed(sizeof(int));
        if (!s->draw_stream) MSM_HIP(hipStreamCreateWithFlags(&s->draw_stream, hipStreamNonBlocking));
        if (!s->draw_begin) MSM_HIP(hipEventCreateWithFlags(&s->draw_begin, hipEventDisableTiming));
        MSM_TRY(grow_event_pairs(s->draw_ev, chunks));
        MSM_HIP(hipEventRecord(s->draw_begin, ctx->stream));  // the uploads above, and whatever read the buffers before this call
        MSM_HIP(hipStreamWaitEvent(s->draw_stream, s->draw_begin, 0));
        d.rec = s->rec.p;
        d.thr = s->thr.p;
        d.pos = pos ? s->pos.p : nullptr;
        d.prop = nullptr;
        d.chains = K;
        d.L = L;
        d.T = T;
        d.chunk_sweeps = stride;
        d.need = 0;
        d.max_blocks = 0;
        d.status = s->draw_status.p;
        chunks_drawn = 0;
        return MSM_OK;
    }
    // chunk c: the next `sweeps` sweeps of every chain into dst (chains x d.chunk_sweeps x T), once `after` (an event of the context's stream, or null) has passed
    int draw(int c, uint16_t *dst, int sweeps, hipEvent_t after) {
        if (after) MSM_HIP(hipStreamWaitEvent(s->draw_stream, after, 0));
        d.prop = dst;
        d.need = (uint32_t)((size_t)sweeps * (size_t)d.T);
        d.max_blocks = forced_blocks > 0 ? forced_blocks : mcmc_draw_block_bound((long)d.need, d.L, mcparam);
        MSM_HIP(hipEventRecord(s->draw_ev[2 * (size_t)c], s->draw_stream));
        MSM_TRY(launch_mcmc_draw(ctx, d, s->draw_stream));
        MSM_HIP(hipEventRecord(s->draw_ev[2 * (size_t)c + 1], s->draw_stream));
        chunks_drawn = std::max(chunks_drawn, c + 1);
        return MSM_OK;
    }
    int join(int c) {
        MSM_HIP(hipStreamWaitEvent(ctx->stream, s->draw_ev[2 * (size_t)c + 1], 0));
        return MSM_OK;
    }
    int collect() {
        MSM_TRY(stage_d2h(ctx, &status, s->draw_status.p, sizeof(int)));
        MSM_TRY(s->rec.download(recs.data(), recs.size(), ctx));
        return MSM_OK;
    }
    // after the context's stream has been synchronised: the counters, and the draw's own error
    int finish(const char *what) {
        double ms = 0.0, candidates = 0.0, accepted = 0.0;
        MSM_TRY(sum_event_pairs(s->draw_ev, chunks_drawn, &ms));
        for (const McmcDrawRecord &r : recs) {
            candidates += (double)r.candidates;
            accepted += (double)r.accepted;
        }
        s->draw_stats[0] = ms;
        s->draw_stats[1] = candidates;
        s->draw_stats[2] = accepted;
        s->draw_stats[3] = (double)d.max_blocks;
        if (status == MSM_ERR_CAPACITY)
            return fail(MSM_ERR_CAPACITY, "%s: the proposal draw on the device reached its bound of %ld blocks of 312 candidates before a chunk was complete", what, d.max_blocks);
        if (status != 0) return fail(status, "%s: the proposal draw on the device reported status %d", what, status);
        return MSM_OK;
    }
};

// the end of a device-draw call: the context's status (read after the sync that also delivers the draw's), then the draw's own, which is the cause when both are raised
int finish_device_draw(msm_ctx *ctx, DeviceDraw &dd, const char *what) {
    const int st = check_status(ctx, what);
    if (st == MSM_ERR_HIP) return st;
    MSM_TRY(dd.finish(what));
    return st;
}

}  // namespace

namespace msm {

int mcmc_run_device(msm_ctx *ctx, const double *d_U, const double *d_tc, const int32_t *triplets, int N, int L, int T, double mcparam, int iters, uint64_t seed,
                    int32_t *labeling) {
    if (iters <= 0 || T <= 0) return MSM_OK;  // (the context's stats stay the previous call's)
    return mcmc_run_device_chains(ctx, d_U, d_tc, triplets, N, L, T, mcparam, iters, &seed, 1, labeling, nullptr, nullptr, nullptr, "msm_mcmc_optimise_gpu");
}

int mcmc_run_device_chains(msm_ctx *ctx, const double *d_U, const double *d_tc, const int32_t *triplets, int N, int L, int T, double mcparam, int iters,
                           const uint64_t *seeds, int K, int32_t *labeling, int32_t *labelings, double *energies, int32_t *best, const char *what) {
    MSM_TRY(check_label_count("msm_mcmc_optimise_gpu", L));
    MSM_TRY(mcmc_check_node_count("msm_mcmc_optimise_gpu", N));
    McmcScratch &s = mcmc_scratch(ctx);
    const bool sweep = iters > 0 && T > 0;  // otherwise every chain is the start: only the energies are computed
    const bool device_draw = ctx->mcmc_draw == 1 && sweep, host_draw = sweep && !device_draw;
    const bool want_energies = K > 1 || energies;  // a single chain is the best one whatever its energy: no term is computed or fetched for it
    McmcSchedule sch;
    mcmc_build_schedule(triplets, N, T, sch);
    std::vector<int4> rec((size_t)T);
    std::vector<int32_t> pos((size_t)T);  // where triplet t stands in the schedule
    for (int i = 0; i < T; ++i) {
        const int t = sch.order[(size_t)i];
        rec[(size_t)i] = make_int4(t, triplets[3 * (size_t)t], triplets[3 * (size_t)t + 1], triplets[3 * (size_t)t + 2]);
        pos[(size_t)t] = i;
    }
    // The host draws about as fast as the device walks, so the device idles for as long as the first chunk takes to draw: hence chunks
    // of half a million proposals per chain (mcmc_chunk_sweeps) and not more.
    long asked = 0;
    if (const char *e = std::getenv("MSMHIP_MCMC_CHUNK_SWEEPS")) asked = std::atol(e);
    const int chunk = mcmc_chunk_sweeps(asked, T, std::max(iters, 1), K);
    const int chunks = sweep ? (iters + chunk - 1) / chunk : 0;
    const int threads = mcmc_draw_threads(K);
    const size_t per_chunk = (size_t)K * chunk * T, nterms = (size_t)N + T;
    std::vector<int32_t> labs((size_t)K * N);  // the caller's labelling stays as it is when the call fails
    for (int k = 0; k < K; ++k) std::copy(labeling, labeling + N, labs.begin() + (size_t)k * N);
    MSM_TRY(s.sched.upload_vec(rec, ctx));
    MSM_TRY(s.level_off.upload_vec(sch.level_off, ctx));
    MSM_TRY(s.labeling.upload_vec(labs, ctx));
    if (s.prop.ensure(std::max<size_t>(per_chunk, 1)) != hipSuccess) return stage_alloc_failed(sizeof(uint16_t) * per_chunk);
    if (device_draw && s.prop2.ensure(per_chunk) != hipSuccess) return stage_alloc_failed(sizeof(uint16_t) * per_chunk);
    if (want_energies && s.terms.ensure((size_t)K * nterms) != hipSuccess) return stage_alloc_failed(sizeof(double) * (size_t)K * nterms);
    MSM_TRY(grow_event_pairs(s.ev, chunks));
    McmcChainArgs c;
    McmcArgs &a = c.a;
    a.U = d_U;
    a.tc = d_tc;
    a.sched = s.sched.p;
    a.level_off = s.level_off.p;
    a.prop = s.prop.p;
    a.labeling = s.labeling.p;
    a.N = N;
    a.L = L;
    a.T = T;
    a.levels = sch.levels();
    a.sweeps = 0;
    a.status = ctx->d_status;
    c.chains = K;
    c.chunk_sweeps = chunk;
    // The proposals of chunk k come from one of two sources.  Drawn on the device: queued on the side stream into buffer k & 1, behind the sweeps of
    // chunk k - 2, which read that buffer; the context's stream then waits for the draw.  Drawn here: every chain's next sweeps into buf in the kernel's
    // layout, the chains spread over the host workers (the wall clock of the threaded draw is kept); uploaded behind the previous chunk's kernel on the
    // stream, when the one device buffer is free (buf is consumed on return; a short last chunk leaves the tail of every chain's block unread).
    uint16_t *const bufs[2] = {s.prop.p, device_draw ? s.prop2.p : s.prop.p};
    DeviceDraw dd;
    McmcChainStreams streams(seeds, host_draw ? K : 0, mcparam, L);
    std::vector<uint16_t> buf(host_draw ? per_chunk : 0);
    double draw_ms = 0.0;
    auto draw = [&](int k, int sweeps) -> int {
        if (device_draw) return dd.draw(k, bufs[k & 1], sweeps, k >= 2 ? s.ev[2 * (size_t)(k - 2) + 1] : nullptr);
        const auto t0 = std::chrono::steady_clock::now();
        streams.draw(buf.data(), chunk, sweeps, T, pos.data(), threads);
        draw_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return MSM_OK;
    };
    auto deliver = [&](int k, int sweeps) -> int {
        if (device_draw) return dd.join(k);
        return upload_in_pieces(ctx, s.prop.p, buf.data(), sizeof(uint16_t) * (sweeps == chunk ? per_chunk : ((size_t)(K - 1) * chunk + sweeps) * T));
    };
    if (device_draw) MSM_TRY(dd.begin(ctx, s, L, mcparam, seeds, K, T, chunk, pos.data(), chunks));
    if (sweep) MSM_TRY(draw(0, std::min(chunk, iters)));
    for (int k = 0, done = 0; k < chunks; ++k) {
        const int sweeps = std::min(chunk, iters - done);
        done += sweeps;
        MSM_TRY(deliver(k, sweeps));
        a.prop = bufs[k & 1];
        a.sweeps = sweeps;
        MSM_HIP(hipEventRecord(s.ev[2 * (size_t)k], ctx->stream));
        MSM_TRY(launch_mcmc_chains(ctx, c));
        MSM_HIP(hipEventRecord(s.ev[2 * (size_t)k + 1], ctx->stream));
        if (done < iters) MSM_TRY(draw(k + 1, std::min(chunk, iters - done)));  // while the device walks chunk k
    }
    std::vector<double> terms(want_energies ? (size_t)K * nterms : 0), E((size_t)K, 0.0);
    if (want_energies) MSM_TRY(launch_mcmc_chain_terms(ctx, c, s.terms.p));
    MSM_TRY(s.labeling.download(labs.data(), labs.size(), ctx));
    if (want_energies) MSM_TRY(s.terms.download(terms.data(), terms.size(), ctx));
    if (device_draw) {
        MSM_TRY(dd.collect());
        MSM_TRY(finish_device_draw(ctx, dd, what));
    } else
        MSM_TRY(check_status(ctx, what));
    if (want_energies)
        for (int k = 0; k < K; ++k) E[(size_t)k] = mcmc_energy_of_terms(terms.data() + (size_t)k * nterms, N, T);
    const int b = mcmc_best_chain(E.data(), K);
    std::copy(labs.begin() + (size_t)b * N, labs.begin() + (size_t)(b + 1) * N, labeling);
    if (labelings) std::copy(labs.begin(), labs.end(), labelings);
    if (energies) std::copy(E.begin(), E.end(), energies);
    if (best) *best = b;
    double kernel_ms = 0.0;
    MSM_TRY(sum_event_pairs(s.ev, chunks, &kernel_ms));
    s.stats[0] = kernel_ms;
    s.stats[1] = sweep ? (double)iters * sch.levels() : 0.0;
    s.stats[2] = draw_ms;
    s.stats[3] = chunks;
    s.stats[4] = sch.levels();
    s.stats[5] = sch.widest();
    s.chains = K;
    s.draw_threads = device_draw ? 0 : threads;
    return MSM_OK;
}

}  // namespace msm

// what both msm_mcmc_optimise*_gpu do ahead of the sweeps: their checks, then both tables uploaded in pieces into the context's scratch.  skip_empty: a
// call without sweeps or triplets ends after the host optimiser's checks (the single-chain call; the chains call still computes the energies).
static int check_and_upload_tables(msm_ctx *ctx, const char *what, const double *unary, const double *tcosts, const int32_t *triplets, int N, int L, int T,
                                   double mcparam, int iters, const uint64_t *seeds, int K, const int32_t *labeling, bool skip_empty) {
    if (!ctx) return fail(MSM_ERR_INVALID, "%s: null context", what);
    if (!unary || !tcosts || !triplets || !labeling || N <= 0 || L <= 0 || T < 0 || iters < 0) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise: bad arguments");
    MSM_TRY(mcmc_check_chains(seeds, K));
    MSM_TRY(mcmc_check_arguments(triplets, N, L, T, mcparam, labeling));
    if (skip_empty && (iters == 0 || T == 0)) return MSM_OK;
    MSM_TRY(check_label_count("msm_mcmc_optimise_gpu", L));
    MSM_TRY(mcmc_check_node_count("msm_mcmc_optimise_gpu", N));
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    McmcScratch &s = mcmc_scratch(ctx);
    const size_t nU = (size_t)L * N, ntc = (size_t)T * L * L * L;
    if (s.U.ensure(nU) != hipSuccess) return stage_alloc_failed(sizeof(double) * nU);
    if (s.tc.ensure(ntc ? ntc : 1) != hipSuccess) return stage_alloc_failed(sizeof(double) * ntc);
    MSM_TRY(upload_in_pieces(ctx, s.U.p, unary, sizeof(double) * nU));
    return upload_in_pieces(ctx, s.tc.p, tcosts, sizeof(double) * ntc);
}

extern "C" {

int msm_mcmc_optimise_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, double mcparam,
                          int32_t iters, uint64_t seed, int32_t *labeling) {
    MSM_TRY(check_and_upload_tables(ctx, "msm_mcmc_optimise_gpu", unary, tcosts, triplets, N, L, T, mcparam, iters, &seed, 1, labeling, true));
    McmcScratch &s = mcmc_scratch(ctx);  // (nothing was uploaded for a call without sweeps or triplets: mcmc_run_device returns at once)
    return mcmc_run_device(ctx, s.U.p, s.tc.p, triplets, N, L, T, mcparam, iters, seed, labeling);
}

int msm_mcmc_optimise_chains_gpu(msm_ctx *ctx, const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T,
                                 double mcparam, int32_t iters, const uint64_t *seeds, int32_t K, int32_t *labeling, int32_t *labelings, double *energies,
                                 int32_t *best) {
    MSM_TRY(check_and_upload_tables(ctx, "msm_mcmc_optimise_chains_gpu", unary, tcosts, triplets, N, L, T, mcparam, iters, seeds, K, labeling, false));
    McmcScratch &s = mcmc_scratch(ctx);
    return mcmc_run_device_chains(ctx, s.U.p, s.tc.p, triplets, N, L, T, mcparam, iters, seeds, K, labeling, labelings, energies, best);
}

int msm_mcmc_optimise_chains(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, double mcparam,
                             int32_t iters, const uint64_t *seeds, int32_t K, int32_t *labeling, int32_t *labelings, double *energies, int32_t *best) {
    if (!unary || !tcosts || !triplets || !labeling || N <= 0 || L <= 0 || T < 0 || iters < 0) return fail(MSM_ERR_INVALID, "msm_mcmc_optimise: bad arguments");
    MSM_TRY(mcmc_check_chains(seeds, K));
    MSM_TRY(mcmc_check_arguments(triplets, N, L, T, mcparam, labeling));
    // K runs of the host optimiser from the one start, a chain per task on the host workers: a chain's result depends on its seed alone
    std::vector<int32_t> labs((size_t)K * N);
    std::vector<double> E((size_t)K);
    parallel_for(K, mcmc_draw_threads(K), [&](int k) {
        int32_t *lab = labs.data() + (size_t)k * N;
        std::copy(labeling, labeling + N, lab);
        mcmc_sweeps_host(unary, tcosts, triplets, N, L, T, mcparam, iters, seeds[k], lab);
        std::vector<double> terms((size_t)N + T);
        mcmc_energy_terms(unary, tcosts, triplets, N, L, T, lab, terms.data());
        E[(size_t)k] = mcmc_energy_of_terms(terms.data(), N, T);
    });
    const int b = mcmc_best_chain(E.data(), K);
    std::copy(labs.begin() + (size_t)b * N, labs.begin() + (size_t)(b + 1) * N, labeling);
    if (labelings) std::copy(labs.begin(), labs.end(), labelings);
    if (energies) std::copy(E.begin(), E.end(), energies);
    if (best) *best = b;
    return MSM_OK;
}

int msm_mcmc_energy(const double *unary, const double *tcosts, const int32_t *triplets, int32_t N, int32_t L, int32_t T, const int32_t *labeling, double *energy) {
    if (!unary || !labeling || !energy || N <= 0 || L <= 0 || T < 0 || (T > 0 && (!tcosts || !triplets))) return fail(MSM_ERR_INVALID, "msm_mcmc_energy: bad arguments");
    MSM_TRY(check_labels(labeling, N, L));
    MSM_TRY(check_triplets(triplets, N, T));
    std::vector<double> terms((size_t)N + T);
    mcmc_energy_terms(unary, tcosts, triplets, N, L, T, labeling, terms.data());
    *energy = mcmc_energy_of_terms(terms.data(), N, T);
    return MSM_OK;
}

int msm_mcmc_best(const double *energies, int32_t K, int32_t *best) {
    if (!energies || !best || K < 1) return fail(MSM_ERR_INVALID, "msm_mcmc_best: bad arguments");
    *best = mcmc_best_chain(energies, K);
    return MSM_OK;
}

int msm_mcmc_chains_info(msm_ctx *ctx, int32_t *K, int32_t *draw_threads) {
    if (!ctx) return fail(MSM_ERR_INVALID, "msm_mcmc_chains_info: null argument");
    if (K) *K = mcmc_scratch(ctx).chains;
    if (draw_threads) *draw_threads = mcmc_scratch(ctx).draw_threads;
    return MSM_OK;
}

int msm_mcmc_gpu_stats(msm_ctx *ctx, double stats[6]) {
    if (!ctx || !stats) return fail(MSM_ERR_INVALID, "msm_mcmc_gpu_stats: null argument");
    std::memcpy(stats, mcmc_scratch(ctx).stats, sizeof(double) * 6);
    return MSM_OK;
}

int msm_mcmc_proposals(int32_t L, double mcparam, uint64_t seed, int32_t T, int32_t sweeps, int32_t chunk_sweeps, uint16_t *out) {
    if (!out || L <= 0 || T < 0 || sweeps < 0) return fail(MSM_ERR_INVALID, "msm_mcmc_proposals: bad arguments");
    MSM_TRY(check_mcparam("msm_mcmc_optimise", mcparam));
    MSM_TRY(check_label_count("msm_mcmc_proposals", L));
    McmcProposals proposals(seed, mcparam, L);
    const int chunk = chunk_sweeps > 0 ? chunk_sweeps : std::max(sweeps, 1);
    for (int done = 0; done < sweeps; done += chunk) {
        const int n = std::min(chunk, sweeps - done);
        proposals.fill(out + (size_t)done * T, (size_t)n * T);
    }
    return MSM_OK;
}

int msm_ctx_set_mcmc_draw(msm_ctx *ctx, int32_t mode) {
    if (!ctx) return fail(MSM_ERR_INVALID, "msm_ctx_set_mcmc_draw: null context");
    if (mode != 0 && mode != 1) return fail(MSM_ERR_INVALID, "msm_ctx_set_mcmc_draw: mode %d (0: the proposals are drawn on the host, 1: on the device)", mode);
    ctx->mcmc_draw = mode;
    return MSM_OK;
}

int msm_ctx_get_mcmc_draw(msm_ctx *ctx, int32_t *mode) {
    if (!ctx || !mode) return fail(MSM_ERR_INVALID, "msm_ctx_get_mcmc_draw: null argument");
    *mode = ctx->mcmc_draw;
    return MSM_OK;
}

int msm_mcmc_draw_thresholds(int32_t L, double mcparam, uint64_t *thr) {
    if (!thr || L <= 0) return fail(MSM_ERR_INVALID, "msm_mcmc_draw_thresholds: bad arguments");
    MSM_TRY(check_mcparam("msm_mcmc_optimise", mcparam));
    mcmc_draw_thresholds(L, mcparam, thr);
    return MSM_OK;
}

int msm_mcmc_draw_block_bound(int64_t need, int32_t L, double mcparam, int64_t *blocks) {
    if (!blocks || L <= 0 || need < 0) return fail(MSM_ERR_INVALID, "msm_mcmc_draw_block_bound: bad arguments");
    MSM_TRY(check_mcparam("msm_mcmc_optimise", mcparam));
    *blocks = mcmc_draw_block_bound((long)need, L, mcparam);
    return MSM_OK;
}

int msm_mcmc_proposals_mirror_counted(int32_t L, double mcparam, uint64_t seed, int32_t T, int32_t sweeps, uint16_t *out, uint64_t *candidates) {
    if (!out || L <= 0 || T < 0 || sweeps < 0) return fail(MSM_ERR_INVALID, "msm_mcmc_proposals_mirror: bad arguments");
    MSM_TRY(check_mcparam("msm_mcmc_optimise", mcparam));
    MSM_TRY(check_label_count("msm_mcmc_proposals_mirror", L));
    McmcDrawMirror mirror(seed, mcparam, L);
    mirror.fill(out, (size_t)sweeps * T);
    if (candidates) *candidates = mirror.candidates;
    return MSM_OK;
}

int msm_mcmc_proposals_mirror(int32_t L, double mcparam, uint64_t seed, int32_t T, int32_t sweeps, uint16_t *out) {
    return msm_mcmc_proposals_mirror_counted(L, mcparam, seed, T, sweeps, out, nullptr);
}

int msm_mcmc_draw_gpu(msm_ctx *ctx, int32_t L, double mcparam, const uint64_t *seeds, int32_t K, int32_t T, int32_t sweeps, int32_t chunk_sweeps,
                      const int32_t *pos, uint16_t *out) {
    if (!ctx) return fail(MSM_ERR_INVALID, "msm_mcmc_draw_gpu: null context");
    if (!out || L <= 0 || T < 0 || sweeps < 0) return fail(MSM_ERR_INVALID, "msm_mcmc_draw_gpu: bad arguments");
    MSM_TRY(mcmc_check_chains(seeds, K));
    MSM_TRY(check_mcparam("msm_mcmc_optimise", mcparam));
    MSM_TRY(check_label_count("msm_mcmc_draw_gpu", L));
    if (pos) {  // a place per triplet, each taken once
        std::vector<char> seen((size_t)T, 0);
        for (int t = 0; t < T; ++t) {
            if (pos[t] < 0 || pos[t] >= T || seen[(size_t)pos[t]]) return fail(MSM_ERR_INVALID, "msm_mcmc_draw_gpu: pos is not a permutation of 0 .. T - 1");
            seen[(size_t)pos[t]] = 1;
        }
    }
    const size_t total = (size_t)K * (size_t)sweeps * (size_t)T;
    if (total > ((size_t)1 << 30)) return fail(MSM_ERR_CAPACITY, "msm_mcmc_draw_gpu: %zu proposals (at most 2^30 per call)", total);
    MSM_HIP(hipSetDevice(ctx->device));
    MSM_TRY(drop_ctx_pending(ctx));
    McmcScratch &s = mcmc_scratch(ctx);
    s.draw_stats[0] = s.draw_stats[1] = s.draw_stats[2] = s.draw_stats[3] = 0.0;
    if (total == 0) return MSM_OK;
    const int chunk = chunk_sweeps > 0 ? std::min(chunk_sweeps, sweeps) : sweeps;
    const int chunks = (sweeps + chunk - 1) / chunk;
    // the whole call's proposals in one device buffer, a chain's sweeps side by side: chunk c is drawn with the stride `sweeps`, `done` sweeps in
    if (s.prop.ensure(total) != hipSuccess) return stage_alloc_failed(sizeof(uint16_t) * total);
    DeviceDraw dd;
    MSM_TRY(dd.begin(ctx, s, L, mcparam, seeds, K, T, sweeps, pos, chunks));
    for (int c = 0, done = 0; c < chunks; ++c) {
        const int n = std::min(chunk, sweeps - done);
        MSM_TRY(dd.draw(c, s.prop.p + (size_t)done * T, n, nullptr));
        done += n;
    }
    MSM_TRY(dd.join(chunks - 1));
    std::vector<uint16_t> host(total);  // the caller's array stays as it is when the call fails
    MSM_TRY(stage_d2h(ctx, host.data(), s.prop.p, sizeof(uint16_t) * total));
    MSM_TRY(dd.collect());
    MSM_TRY(finish_device_draw(ctx, dd, "msm_mcmc_draw_gpu"));
    std::copy(host.begin(), host.end(), out);
    return MSM_OK;
}

int msm_mcmc_draw_stats(msm_ctx *ctx, double stats[4]) {
    if (!ctx || !stats) return fail(MSM_ERR_INVALID, "msm_mcmc_draw_stats: null argument");
    std::memcpy(stats, mcmc_scratch(ctx).draw_stats, sizeof(double) * 4);
    return MSM_OK;
}

int msm_mcmc_schedule(const int32_t *triplets, int32_t N, int32_t T, int32_t *level, int32_t *order, int32_t *level_off, int32_t *levels) {
    if (N <= 0 || T < 0 || (T > 0 && !triplets)) return fail(MSM_ERR_INVALID, "msm_mcmc_schedule: bad arguments");
    MSM_TRY(check_triplets(triplets, N, T));
    McmcSchedule s;
    mcmc_build_schedule(triplets, N, T, s);
    if (level) std::copy(s.level.begin(), s.level.end(), level);
    if (order) std::copy(s.order.begin(), s.order.end(), order);
    if (level_off) std::copy(s.level_off.begin(), s.level_off.end(), level_off);
    if (levels) *levels = s.levels();
    return MSM_OK;
}

}  // extern "C"
