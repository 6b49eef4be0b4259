// hs_runtime.hip.h -- part of libhsflow.so: graph cache, HIP-event profiler, Eps buffers and read-back,
// diagnostic stamps.
#pragma once

namespace {
// The graph cache is keyed by everything a captured launch sequence depends on (sizes, kernel shape,
// lambda, epsilon ...); a caller that varies those from call to call must not grow it without bound.
constexpr size_t kMaxGraphs = 32;
void drop_graphs(hsflow_ctx *c)
{
    if (c->graphs.empty()) return;
    hipStreamSynchronize(c->stream); // no replay of an old graph may still be running
    for (auto &kv : c->graphs) {
        if (kv.second.exec) hipGraphExecDestroy(kv.second.exec);
        if (kv.second.graph) hipGraphDestroy(kv.second.graph);
    }
    c->graphs.clear();
}

void trim_graph_cache(hsflow_ctx *c)
{
    if (c->graphs.size() >= kMaxGraphs) drop_graphs(c);
}

int check_ctx(hsflow_ctx *c, int pair)
{
    if (!c) return fail(nullptr, HSFLOW_E_ARG, "null context");
    if (pair < 0 || pair >= c->N) return fail(c, HSFLOW_E_ARG, "pair index out of range");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, HSFLOW_E_DEVICE, "hipSetDevice failed");
    // The launch wrappers report hipGetLastError() after a launch; that is the LAST error of this host thread, so a HIP call
    // that failed earlier -- anywhere in the process, already reported to its own caller -- must not surface here.
    (void)hipGetLastError();
    return HSFLOW_OK;
}

// Both frames of a pair from device memory into the context's planes: ONE launch on the context's stream (two 2-D copies
// cost two launches and their gaps: 5 % of a 1080p / 100 solve).
hipError_t launch_frame_copy(hsflow_ctx *c, int pair, const void *dprev, size_t ps, const void *dcurr, size_t cs)
{
    const dim3 grid((c->W + 1023) / 1024, (c->H + 3) / 4, 2), block(64, 4);
    const bool aligned = (((uintptr_t)dprev | (uintptr_t)dcurr | ps | cs) & 15u) == 0;
    uint8_t *dA = c->dA + pair * c->plane, *dB = c->dB + pair * c->plane;
    if (aligned)
        hipLaunchKernelGGL(hsk::k_copy_pair_u8<true>, grid, block, 0, c->stream, (const uint8_t *)dprev, (long long)ps, (const uint8_t *)dcurr,
                           (long long)cs, dA, dB, c->W, c->H, c->P);
    else
        hipLaunchKernelGGL(hsk::k_copy_pair_u8<false>, grid, block, 0, c->stream, (const uint8_t *)dprev, (long long)ps, (const uint8_t *)dcurr,
                           (long long)cs, dA, dB, c->W, c->H, c->P);
    return hipGetLastError();
}

// The context's one staging buffer (dScratch: host frames on their way to pre-processing, the derivative read-back): at
// least `need` bytes.  Grows only; nothing in flight may still use the old one, so the stream is waited for first.
int scratch_reserve(hsflow_ctx *c, size_t need)
{
    if (c->scratch_bytes >= need) return HSFLOW_OK;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(c->dScratch);
    c->dScratch = nullptr; c->scratch_bytes = 0;
    HS_HIP(c, hipMalloc(&c->dScratch, need));
    c->scratch_bytes = need;
    return HSFLOW_OK;
}

// dst planes (pitch P) = pre(format, src) for `frames` (1 or 2) frames that lie in device memory (a caller's, the staging
// slots, or a plane of the context), on the context's stream: ONE launch of k_pre_pair, whatever the format
// (HSFLOW_FRAMES_GRAY8 is a copy and not handled here).  Word loads per source where its base and stride allow them.
hipError_t launch_pre_fused(hsflow_ctx *c, int format, int frames, const void *sA, size_t psA, const void *sB, size_t psB, uint8_t *dA, uint8_t *dB)
{
    constexpr int S = HSFLOW_PRE_STRIP_ROWS;
    const dim3 grid((c->W + 255) / 256, ((c->H + S - 1) / S + 3) / 4, frames), block(64, 4);
    const unsigned words = ((((uintptr_t)sA | psA) & 3u) == 0 ? 1u : 0u) | (frames > 1 && (((uintptr_t)sB | psB) & 3u) == 0 ? 2u : 0u);
    const uint8_t *a = (const uint8_t *)sA, *b = (const uint8_t *)sB;
    switch (format) {
    case HSFLOW_FRAMES_GRAY8_BLUR:
        hipLaunchKernelGGL((hsk::k_pre_pair<false, true>), grid, block, 0, c->stream, a, (long long)psA, b, (long long)psB, dA, dB, c->W, c->H, c->P, words);
        break;
    case HSFLOW_FRAMES_BGR8:
        hipLaunchKernelGGL((hsk::k_pre_pair<true, false>), grid, block, 0, c->stream, a, (long long)psA, b, (long long)psB, dA, dB, c->W, c->H, c->P, words);
        break;
    case HSFLOW_FRAMES_BGR8_BLUR:
        hipLaunchKernelGGL((hsk::k_pre_pair<true, true>), grid, block, 0, c->stream, a, (long long)psA, b, (long long)psB, dA, dB, c->W, c->H, c->P, words);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// HSFLOW_PRE_SEQ_MAX of this call: the environment's (1 .. the header's, for measuring and for testing the chunking), else
// the header's; 0: unusable.
int pre_seq_max()
{
    static_assert(HSFLOW_PRE_SEQ_MAX >= 1 && HSFLOW_PRE_SEQ_MAX <= hsk::kPreSeqMax, "a chunk of frames must fit k_pre_sequence's argument block");
    const char *e = getenv("HSFLOW_PRE_SEQ_MAX");
    if (!e || !*e) return HSFLOW_PRE_SEQ_MAX;
    char *rest = nullptr;
    const long v = strtol(e, &rest, 10);
    if (*rest || v < 1 || v > HSFLOW_PRE_SEQ_MAX) return 0;
    return (int)v;
}

// Frames f_0 .. f_{n-1} in device memory (rows `stride` apart) into the pairs first_pair .. first_pair + n - 2 by the
// sequence rule of hs_pre_rule.h, on the context's stream: ONE launch of k_pre_sequence per chunk of at most `maxf`
// frames, whatever the format (a frame's results depend on that frame alone, so a chunk boundary needs no overlap).
hipError_t launch_pre_sequence(hsflow_ctx *c, int first_pair, int format, const void *const *frames, int n, size_t stride, int flags, int maxf)
{
    constexpr int S = HSFLOW_PRE_STRIP_ROWS;
    for (int j0 = 0; j0 < n; j0 += maxf) {
        const int m = std::min(maxf, n - j0);
        hsk::PreSeqFrames f = {};
        for (int i = 0; i < m; i++) {
            const int j = j0 + i;
            const hspre::SeqDst d = hspre::seq_dst(flags, j, n, j <= n - 2 ? c->dA + (size_t)(first_pair + j) * c->plane : nullptr,
                                                   j >= 1 ? c->dB + (size_t)(first_pair + j - 1) * c->plane : nullptr);
            f.src[i] = (const uint8_t *)frames[j];
            f.p0[i] = d.p0; f.p1[i] = d.p1; f.b[i] = d.b;
            if ((((uintptr_t)frames[j] | stride) & 3u) == 0) f.words |= 1u << i;
        }
        const dim3 grid((c->W + 255) / 256, ((c->H + S - 1) / S + 3) / 4, m), block(64, 4);
        switch (format) {
        case HSFLOW_FRAMES_GRAY8: hipLaunchKernelGGL((hsk::k_pre_sequence<false, false>), grid, block, 0, c->stream, f, (long long)stride, c->W, c->H, c->P); break;
        case HSFLOW_FRAMES_GRAY8_BLUR: hipLaunchKernelGGL((hsk::k_pre_sequence<false, true>), grid, block, 0, c->stream, f, (long long)stride, c->W, c->H, c->P); break;
        case HSFLOW_FRAMES_BGR8: hipLaunchKernelGGL((hsk::k_pre_sequence<true, false>), grid, block, 0, c->stream, f, (long long)stride, c->W, c->H, c->P); break;
        case HSFLOW_FRAMES_BGR8_BLUR: hipLaunchKernelGGL((hsk::k_pre_sequence<true, true>), grid, block, 0, c->stream, f, (long long)stride, c->W, c->H, c->P); break;
        default: return hipErrorInvalidValue;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Could the first Jacobi launch of a solve read these frames where they lie (hsk::FrameSrc)?  It reads a lane's four
// columns as one word, so both planes must be word-aligned with pitches that keep every row so; one pair per context.
// HSFLOW_KEEP_FRAME_COPY=1: never (A/B runs).  Whether the solve HAS such a launch it decides itself (resolve_lazy_frames).
bool frames_readable_in_place(const hsflow_ctx *c, const void *dprev, size_t ps, const void *dcurr, size_t cs)
{
    static const bool keep = getenv("HSFLOW_KEEP_FRAME_COPY") && atoi(getenv("HSFLOW_KEEP_FRAME_COPY")) != 0;
    return !keep && c->N == 1 && (((uintptr_t)dprev | (uintptr_t)dcurr | ps | cs) & 3u) == 0 && ps <= (size_t)INT32_MAX && cs <= (size_t)INT32_MAX;
}

// The frames of hsflow_solve_async_frames_device, once the solve knows its first launch: in_place -- that launch carries
// the derivative pass on the strip kernel, reads the caller's planes and stores the context's copy (*first: what the
// caller hands that one launch as LaunchIo::frames); otherwise the copy kernel goes out now, ahead of whatever reads
// dA / dB.  Never inside a capture or a dry run.
int resolve_lazy_frames(hsflow_ctx *c, bool in_place, hsflow_ctx::FrameRef *first = nullptr)
{
    if (!c->lazy.active) return HSFLOW_OK;
    c->lazy.active = false;
    if (in_place) {
        *first = c->lazy;
        first->active = true;
        c->copies_elided++;
        return HSFLOW_OK;
    }
    HS_HIP(c, launch_frame_copy(c, 0, c->lazy.A, (size_t)c->lazy.PA, c->lazy.B, (size_t)c->lazy.PB));
    return HSFLOW_OK;
}

struct Profiler { // brackets kernels with events when params.profile is set
    hsflow_ctx *c;
    bool on;
    std::vector<std::pair<int, size_t>> marks; // (kind, index of start event); kind 0 deriv, 1 jacobi
    size_t used = 0;
    hipEvent_t ev(size_t i)
    {
        while (c->events.size() <= i) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            c->events.push_back(e);
        }
        return c->events[i];
    }
    void begin(int kind)
    {
        if (!on) return;
        marks.push_back({kind, used});
        hipEventRecord(ev(used), c->stream);
        used++;
    }
    void end()
    {
        if (!on) return;
        hipEventRecord(ev(used), c->stream);
        used++;
    }
    void collect()
    {
        if (!on || marks.empty()) return;
        hipStreamSynchronize(c->stream);
        float d = 0, j = 0, t = 0;
        for (auto &m : marks) {
            float ms = 0;
            hipEventElapsedTime(&ms, c->events[m.second], c->events[m.second + 1]);
            (m.first == 0 ? d : j) += ms;
        }
        hipEventElapsedTime(&t, c->events[marks.front().second], c->events[used - 1]);
        c->info.deriv_ms = d;
        c->info.jacobi_ms = j;
        c->info.solve_ms = t;
    }
};

// --- the persistent launch (HSFLOW_KERNEL_PERSIST) -------------------------------------------------------------
// Buffers it needs (allocation only: called outside any capture).
int persist_reserve(hsflow_ctx *c)
{
    const size_t px = (size_t)c->plane * c->N;
    if (!c->dUp) HS_HIP(c, hipMalloc((void **)&c->dUp, px * sizeof(float)));
    if (!c->dVp) HS_HIP(c, hipMalloc((void **)&c->dVp, px * sizeof(float)));
    if (!c->dFlags) {
        HS_HIP(c, hipMalloc((void **)&c->dFlags, (size_t)(kMaxPersistTiles + 1) * sizeof(unsigned)));
        c->persist_tiles = 0;
    }
    if (!c->hErr) {
        HS_HIP(c, hipHostMalloc((void **)&c->hErr, 64, hipHostMallocMapped | hipHostMallocCoherent));
        HS_HIP(c, hipHostGetDevicePointer((void **)&c->hErrDev, c->hErr, 0));
        *c->hErr = 0u;
    }
    return HSFLOW_OK;
}

// The tiles' phase counters count up across solves and agree at every launch boundary as long as the grid stays the
// same; a different grid (or an aborted launch) starts from cleared counters.  Enqueued ahead of the launch, outside
// any capture.
int persist_prepare_flags(hsflow_ctx *c, int tiles)
{
    if (c->persist_tiles == tiles) return HSFLOW_OK;
    HS_HIP(c, hipMemsetAsync(c->dFlags, 0, (size_t)(kMaxPersistTiles + 1) * sizeof(unsigned), c->stream));
    c->persist_tiles = tiles;
    return HSFLOW_OK;
}

// A persistent launch gave up waiting (another grid held part of the CUs, a neighbour never came): the flow it left is
// invalid, and so is the derivative plane (a workgroup that never started left its part unwritten).  The context goes
// back to a launch per fuse_steps iterations for good.
void persist_failed(hsflow_ctx *c)
{
    if (c->hErr) *c->hErr = 0u;
    c->persist_tiles = 0;
    c->persist_off = true;
    c->persist_unchecked = false;
    c->coef_valid = false;
    c->plan_cache.clear();
}

// Did the last persistent launch(es) of this context give up?  Only meaningful once the stream has drained.
bool persist_error(const hsflow_ctx *c) { return c->hErr && *(volatile unsigned *)c->hErr != 0u; }

// After the stream has drained: looks at the error word an asynchronous persistent solve left unchecked.  True if that
// launch gave up (persist_failed has been dealt with then; the caller reports it or solves again).
bool persist_gave_up(hsflow_ctx *c)
{
    const bool gave_up = c->persist_unchecked && persist_error(c);
    c->persist_unchecked = false;
    if (gave_up) persist_failed(c);
    return gave_up;
}

// One persistent launch = `iters` sweeps in phases of sp.g.T: input dU[cur] (or zero), output dU[cur ^ 1]; the phases
// alternate between that buffer and the third one so that the last phase lands in it.  io.eps: a row of Eps words per phase.
int enqueue_persist(hsflow_ctx *c, const StripPlan &sp0, int iters, EpsMode eps, const LaunchIo &io, bool deriv, int zero_in, float coeff)
{
    StripPlan sp = sp0;
    sp.g.zero_in = zero_in;
    hsk::PersistArgs pa;
    const int T = sp.g.T;
    pa.n_phase = (iters + T - 1) / T;
    pa.T_last = iters - (pa.n_phase - 1) * T;
    pa.flags = c->dFlags;
    pa.err = c->hErrDev;
    // (HSFLOW_PERSIST_WAIT_TICKS: test hook -- with 0 every wait that is not already satisfied gives up, which drives the
    // abort and fall-back path)
    static const char *ticks_env = getenv("HSFLOW_PERSIST_WAIT_TICKS");
    pa.wait_ticks = ticks_env ? (unsigned)strtoul(ticks_env, nullptr, 10) : kPersistWaitTicks;
    const int a = c->cur, b = a ^ 1;
    const int lastb = (pa.n_phase - 1) & 1;
    pa.ub[lastb] = c->dU[b]; pa.vb[lastb] = c->dV[b];
    pa.ub[lastb ^ 1] = c->dUp; pa.vb[lastb ^ 1] = c->dVp;
    HS_HIP(c, launch_persist(c, sp, pa, eps, deriv, io, c->dU[a], c->dV[a], coeff));
    c->cur = b;
    return HSFLOW_OK;
}

// Asks, before anything of a solve is enqueued, whether the persistent kernel it will launch can be resident (and raises
// its LDS cap): a refusal then leaves the stream and the flow untouched.
int configure_persist(hsflow_ctx *c, const StripPlan &sp, EpsMode eps, bool deriv, float coeff)
{
    c->configuring = true;
    const hipError_t e = launch_persist(c, sp, hsk::PersistArgs{}, eps, deriv, default_io(c), nullptr, nullptr, coeff);
    c->configuring = false;
    HS_HIP(c, e);
    return HSFLOW_OK;
}

// Eps bookkeeping of an EPS-terminated solve: `sweeps` rows of `stride` words (one per workgroup) on the device, and
// the host buffer k_eps_reduce reduces the rows into, hEps[0..sweeps).  eps_reserve allocates only, so that what
// follows can be captured in a graph; eps_prepare also clears the rows.  Neither tells the launches anything: the caller
// hands them the rows (LaunchIo).
// host_words: words the reduction writes to the host (a per-pair reduction: sweeps x pairs), 0: one per row.
int eps_reserve(hsflow_ctx *c, int sweeps, int stride, size_t host_words = 0)
{
    const size_t need = (size_t)sweeps * stride;
    if (host_words < (size_t)sweeps) host_words = (size_t)sweeps;
    if (c->epsTilesCap < need) {
        drop_graphs(c); // captured launches hold the old address (this also waits for the stream)
        hipFree(c->dEpsTiles);
        c->dEpsTiles = nullptr; c->epsTilesCap = 0;
        HS_HIP(c, hipMalloc((void **)&c->dEpsTiles, need * sizeof(unsigned)));
        c->epsTilesCap = need;
    }
    if (c->hEpsCap < host_words) {
        drop_graphs(c);
        HS_HIP(c, hipStreamSynchronize(c->stream)); // nothing in flight may still write the old buffer
        if (c->hEps) hipHostFree(c->hEps);
        c->hEps = c->hEpsDev = nullptr; c->hEpsCap = 0;
        const size_t cap = std::max<size_t>(256, host_words * 2);
        HS_HIP(c, hipHostMalloc((void **)&c->hEps, cap * sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent));
        HS_HIP(c, hipHostGetDevicePointer((void **)&c->hEpsDev, c->hEps, 0));
        c->hEpsCap = cap;
    }
    return HSFLOW_OK;
}

int eps_clear(hsflow_ctx *c, int sweeps, int stride)
{
    HS_HIP(c, hipMemsetAsync(c->dEpsTiles, 0, (size_t)sweeps * stride * sizeof(unsigned), c->stream));
    return HSFLOW_OK;
}

int eps_prepare(hsflow_ctx *c, int sweeps, int stride)
{
    const int st = eps_reserve(c, sweeps, stride);
    return st ? st : eps_clear(c, sweeps, stride);
}

// Reduces the rows of per-workgroup words to one word per row, straight into the host's buffer (no copy node).
// mark: the kernel's last workgroup also writes the context's marker (hsflow_set_async_reduce; the caller counts it).
int eps_collect_enqueue(hsflow_ctx *c, const EpsLayout &w, bool mark = false)
{
    if (c->configuring) return HSFLOW_OK;
    if (w.pairs > 0) { // one word per (row, pair): hEps[row * pairs + pair]
        // (pairs of fewer than 8 workgroups: a lane each; the rows of one pass differ by a short last launch at most)
        const int per_lane = std::max(w.cnt_first, w.cnt_last) / w.pairs < 8 ? 1 : 0;
        const int pair_blocks = per_lane ? (w.pairs + 255) / 256 : (w.pairs + 3) / 4;
        if ((long long)w.slots * pair_blocks > (long long)INT32_MAX)
            return fail(c, HSFLOW_E_SIZE, "the per-pair Eps reduction of this many launches x pairs exceeds the grid limit");
        hipLaunchKernelGGL(hsk::k_eps_reduce_pairs, dim3((unsigned)w.slots * (unsigned)pair_blocks), dim3(256), 0, c->stream, c->dEpsTiles,
                           w.stride, c->hEpsDev, w.n_first, w.cnt_first, w.cnt_last, w.pairs, pair_blocks, per_lane, mark ? c->dSeq : nullptr,
                           mark ? c->hMarkDev : nullptr);
        HS_HIP(c, hipGetLastError());
        return HSFLOW_OK;
    }
    hipLaunchKernelGGL(hsk::k_eps_reduce, dim3(w.slots), dim3(256), 0, c->stream, c->dEpsTiles, w.stride, c->hEpsDev, w.n_first,
                       w.cnt_first, w.cnt_last, mark ? c->dSeq : nullptr, mark ? c->hMarkDev : nullptr);
    HS_HIP(c, hipGetLastError());
    return HSFLOW_OK;
}

// The exact pass: every row is `stride` words, cleared where a launch had fewer workgroups (eps_prepare).
int eps_collect(hsflow_ctx *c, int sweeps, int stride, std::vector<unsigned> &host)
{
    int st = eps_collect_enqueue(c, EpsLayout{sweeps, stride, 0, 0, stride});
    if (st) return st;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    host.assign(c->hEps, c->hEps + sweeps);
    return HSFLOW_OK;
}

// Witness slots of a speculative ITER|EPS pass (host copy): true if they prove that the early stop
// cannot have fired before the budget ran out; *last = Eps of the final sweep.
// last_is_exact: the last slot is the measured Eps of the final sweep (a stop there IS the budget, so it proves
// nothing and fails nothing); otherwise every slot is a witness word and all of them must clear epsilon.
// step: words between two slots (a per-pair reduction lays them out [slot][pair]: w = the pair's first word, step = pairs).
bool witness_proven(const unsigned *w, int slots, double epsilon, float *last, bool last_is_exact, int step = 1)
{
    float e = 0.f;
    for (int i = 0; i < slots; i++) {
        std::memcpy(&e, &w[(size_t)i * step], sizeof(float));
        if (!((double)e >= epsilon) && !(last_is_exact && i == slots - 1)) return false;
    }
    *last = e;
    return true;
}

int plan_eps_stride(int kernel, const JPlan &pl) { return (kernel == HSFLOW_KERNEL_STRIP || kernel == HSFLOW_KERNEL_FOLD) ? pl.s.tiles : 1; }

// Diagnostic only: with HSFLOW_DEBUG_STAMPS=<file> every strip launch records per-workgroup phase
// stamps (8 x u64) and hsflow_solve appends those of the LAST launch to <file> as text.
constexpr int kStampTiles = 65536;
void dump_stamps(hsflow_ctx *c, int tiles)
{
    const char *path = getenv("HSFLOW_DEBUG_STAMPS");
    if (!path || !c->dStamps) return;
    tiles = std::min(tiles, kStampTiles);
    std::vector<unsigned long long> h((size_t)tiles * 8);
    if (hipMemcpy(h.data(), c->dStamps, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    FILE *f = fopen(path, "a");
    if (!f) return;
    fprintf(f, "# solve tiles=%d T=%d R=%d threads=%d\n", tiles, c->info.fuse_steps, c->info.groups_per_thread, c->info.threads);
    for (int i = 0; i < tiles; i++) {
        const unsigned long long *o = &h[(size_t)i * 8];
        fprintf(f, "%d %llu %llu %llu %llu %llu %llu %llu\n", i, o[1] - o[0], o[2] - o[1], o[3] - o[2], o[3] - o[0],
                o[5] - o[4], o[6], o[7]);
    }
    // the persistent launch: cycles spent in sweeps / publish (stores drained, barrier) / wait (counters) / halo reload,
    // summed over the phases, per workgroup
    if (c->info.persistent && tiles <= 8192) {
        std::vector<unsigned long long> pq((size_t)tiles * 32);
        if (hipMemcpy(pq.data(), c->dStamps + (size_t)tiles * 8, pq.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
            for (int i = 0; i < tiles; i++)
                fprintf(f, "P %d %llu %llu %llu %llu %d %llu %llu\n", i, pq[(size_t)i * 32], pq[(size_t)i * 32 + 1], pq[(size_t)i * 32 + 2],
                        pq[(size_t)i * 32 + 3], c->info.persistent, pq[(size_t)i * 32 + 4], pq[(size_t)i * 32 + 5]);
    }
    // per-sweep end stamps of the strip kernel (cycles since the end of the load phase), HSFLOW_DEBUG_STAMPS_SWEEPS=1
    if (getenv("HSFLOW_DEBUG_STAMPS_SWEEPS") && tiles <= 8192 && c->info.kernel == HSFLOW_KERNEL_STRIP) {
        const int T = std::min(c->info.fuse_steps, 32);
        std::vector<unsigned long long> sw((size_t)tiles * 32);
        if (hipMemcpy(sw.data(), c->dStamps + (size_t)tiles * 8, sw.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            for (int i = 0; i < tiles; i++) {
                fprintf(f, "S %d", i);
                for (int k = 0; k < T; k++) fprintf(f, " %llu", sw[(size_t)i * 32 + k] - h[(size_t)i * 8 + 1]);
                fprintf(f, "\n");
            }
        }
    }
    fclose(f);
}

int pick_T(int max_iter, int requested)
{
    if (requested > 0) return std::min(requested, kMaxFuse);
    // default sweeps per launch; prefer a divisor of max_iter near 8 so that launches are uniform
    const int pref[] = {8, 10, 7, 9, 6, 12, 5, 4};
    for (int t : pref)
        if (max_iter % t == 0) return t;
    return std::min(8, std::max(1, max_iter));
}

} // namespace
