// hs_solve.hip.h -- part of libhsflow.so: the solve paths (classic mode; CV mode with a fixed sweep count,
// speculative ITER|EPS with witness launches, EPS-only chunks) and the deferred check of asynchronous solves.
#pragma once

namespace {
int solve_impl(hsflow_ctx *c, const hsflow_params *pp, bool async);
int prepare_solve(hsflow_ctx *c, const hsflow_params &p, bool async, SolveSetup &S);

// After the stream has drained: did an asynchronous persistent launch give up?  Its flow is invalid then; the context
// goes back to a launch per fuse_steps iterations and the caller is told.
int check_persist(hsflow_ctx *c)
{
    if (!persist_gave_up(c)) return HSFLOW_OK;
    return fail(c, HSFLOW_E_DEVICE, "a persistent launch of an asynchronous solve timed out (another grid on the device?): its flow is invalid; "
                                    "this context now launches per fuse_steps iterations, solve again");
}

// Waits until the marker kernel that wrote `target` has run (k_mark_done: everything enqueued before it is done, and what the
// reduction kernel wrote to host memory is visible).  Polls page-locked memory; gives the stream a proper wait after 2 s.
int wait_marker(hsflow_ctx *c, unsigned target)
{
    if (!c->hMark) { HS_HIP(c, hipStreamSynchronize(c->stream)); return HSFLOW_OK; }
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while ((int)(__atomic_load_n(c->hMark, __ATOMIC_ACQUIRE) - target) < 0) {
        if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            HS_HIP(c, hipStreamSynchronize(c->stream));
            break;
        }
    }
    return HSFLOW_OK;
}

// Pair `pair`'s u and v planes (n planes each, from that pair on) from (su, sv) to (du, dv), on the context's stream.
hipError_t copy_pair_flow(hsflow_ctx *c, float *du, float *dv, const float *su, const float *sv, int pair, int n = 1)
{
    const long long o = (long long)pair * c->plane;
    const size_t bytes = (size_t)c->plane * n * sizeof(float);
    const hipError_t e = hipMemcpyAsync(du + o, su + o, bytes, hipMemcpyDeviceToDevice, c->stream);
    return e != hipSuccess ? e : hipMemcpyAsync(dv + o, sv + o, bytes, hipMemcpyDeviceToDevice, c->stream);
}

// dUb / dVb: the backup of a starting flow (save_start; the chunk input of the per-pair stop on the one-sweep kernel).
int reserve_start_backup(hsflow_ctx *c)
{
    const size_t px = (size_t)c->plane * c->N;
    if (!c->dUb) HS_HIP(c, hipMalloc((void **)&c->dUb, px * sizeof(float)));
    if (!c->dVb) HS_HIP(c, hipMalloc((void **)&c->dVb, px * sizeof(float)));
    return HSFLOW_OK;
}

// ITER|EPS with use_previous: the ping-pong buffers get overwritten, so the starting flow is kept in dUb / dVb
// (allocated by solve_iter_eps) for an exact pass that has to start over from it ...
int save_start(hsflow_ctx *c)
{
    if (c->configuring) return HSFLOW_OK;
    HS_HIP(c, copy_pair_flow(c, c->dUb, c->dVb, c->dU[c->cur], c->dV[c->cur], 0, c->N));
    return HSFLOW_OK;
}

// ... which copies it back into the current buffer.
int restore_start(hsflow_ctx *c)
{
    HS_HIP(c, copy_pair_flow(c, c->dU[c->cur], c->dV[c->cur], c->dUb, c->dVb, 0, c->N));
    return HSFLOW_OK;
}

// Do the derivatives have to be computed, or does the coefficient plane hold those of this mode and may be reused?
bool needs_deriv(const hsflow_ctx *c, const hsflow_params &p, int mode) { return !(p.reuse_derivatives && c->coef_valid && c->coef_mode == mode); }

// The bits of GraphKey::use_prev: what, besides the shapes, decides which launches a captured sequence holds.
// (p.use_previous enters as p.use_previous * kKeyUsePrev.)
enum : int {
    kKeyDeriv = 1,       // the sequence computes the derivatives
    kKeyUsePrev = 2,
    kKeyAsync = 4,       // CV mode: an asynchronous witness pass (Witness last launch, reduction owed)
    kKeyUnpack = 4,      // classic mode: the derivative planes are unpacked
    kKeyAsyncReduce = 8, // ... with the reduction in the stream
    kKeyInPlace = 16,    // the first launch went out by itself (it reads the caller's frames): the launches after it
    kKeyPerPair = 32,    // the witness words are reduced per pair
};

// The key of a captured launch sequence: the call's parameters, the kernel and sweeps per launch of its setup, the launch
// shape in c->info, the kKey* bits, the coefficient (Ilambda, or alpha in classic mode) and a witness pass's threshold.
GraphKey graph_key(const hsflow_ctx *c, const hsflow_params &p, int kernel, int T, int flags, float coeff, float eps_thr = -1.f)
{
    const hsflow_info &i = c->info;
    return GraphKey{p.mode, kernel, p.max_iter, T, i.tile_w, i.tile_h, i.threads, i.groups_per_thread, p.use_previous ? c->cur : 0,
                    p.use_previous * kKeyUsePrev + flags, coeff, eps_thr};
}

// EPS termination without a usable sweep budget stops only on Eps < epsilon.  A positive epsilon below the fp32 limit
// cycle of the iteration (Eps stalls around 1e-7 * |flow|) would keep the host launching for ever -- the original does
// exactly that; here a solve (a pair, under the per-pair stop) gives up with HSFLOW_E_NOTERM (flow, iterations_done and
// last_eps stay valid) once Eps has not reached a new minimum for kStallSweeps sweeps or after kMaxSweeps.
constexpr long long kStallSweeps = 4096, kMaxSweeps = 1LL << 24;
struct StallWatch {
    float best = INFINITY; // the lowest Eps so far ...
    long long at = 0;      // ... and the sweep it occurred in
    void seen(float e, long long sweep) { if (e < best) { best = e; at = sweep; } }
    bool give_up(long long ran, long long budget) const { return budget > kMaxSweeps && (ran - at >= kStallSweeps || ran >= kMaxSweeps); }
};

// ------------------------------------------------------------------------------------------------------------------
// Per-pair stop (hsflow_set_pair_termination): under EPS termination every pair of a batch stops on its own Eps, as
// cvCalcOpticalFlowHS called pair by pair does (OpticalFlowOpenCV.cpp:29,94).  The speculative witness pass runs over
// all pairs exactly as for a batch that stops as one -- same launches, same graph -- and its words are reduced per pair
// (k_eps_reduce_pairs).  A proven pair stands at the budget.  The pairs that are not proven go through the exact pass
// TOGETHER (solve_pairs_exact): chunk launches over a device list of the pairs still running, one read-back of their
// per-pair Eps per chunk, a replay from the chunk's intact input for exactly the missing sweeps of a pair whose stop lies
// in the chunk, which is then dropped from the list.  A stopped pair's final flow is copied into the other ping-pong
// buffer too: whichever buffer the context calls current, every pair's final flow lies in it.
// ------------------------------------------------------------------------------------------------------------------
enum class PairStart : int { Zero = 0, Saved = 1, Current = 2 }; // zero flow; dUb / dVb (save_start); the flow held now

// hsflow_info of a per-pair solve: iterations_done the maximum over the pairs, last_eps that of the lowest pair that ran
// that long, eps_rerun 1 if any pair was re-run.
void pairs_to_info(hsflow_ctx *c)
{
    int most = 0, rerun = 0;
    for (const hsflow_ctx::PairResult &r : c->pair_res) { most = std::max(most, r.iterations_done); rerun |= r.eps_rerun; }
    for (const hsflow_ctx::PairResult &r : c->pair_res)
        if (r.iterations_done == most) { c->info.last_eps = r.eps_owed ? NAN : r.last_eps; break; }
    c->info.iterations_done = most;
    c->info.eps_rerun = rerun;
    c->pair_res_valid = true;
}

// The exact pass for the pairs of `list`, together.  Chunk length: the plan's sweeps per launch (a shorter tail at the end
// of the budget); the one-sweep kernel runs HSFLOW_PAIR_STOP_SIMPLE_CHUNK launches between read-backs and keeps the
// chunk's input in dUb / dVb (its ping-pong overwrites it).  Afterwards the stream is idle and hsflow_info is that of the
// whole solve.  rerun: a witness pass ran before and proved nothing for these pairs.
int solve_pairs_exact(hsflow_ctx *c, const SolveSetup &S, const std::vector<int> &list, PairStart start, bool rerun)
{
    const hsflow_params &p = S.eff;
    const int N = c->N, kernel = S.kernel;
    const bool multi = S.multi, strip = kernel == HSFLOW_KERNEL_STRIP || kernel == HSFLOW_KERNEL_FOLD;
    const int T = multi ? S.T : HSFLOW_PAIR_STOP_SIMPLE_CHUNK;
    const long long budget = S.budget;
    int st = HSFLOW_OK;
    if (list.empty()) { pairs_to_info(c); return HSFLOW_OK; }
    if (!c->dPairs) { // the identity, then room for the list of active pairs and for the lists of a chunk's replays
        std::vector<int> ident((size_t)N);
        for (int i = 0; i < N; i++) ident[(size_t)i] = i;
        HS_HIP(c, hipMalloc((void **)&c->dPairs, 3 * (size_t)N * sizeof(int)));
        HS_HIP(c, hipMemcpy(c->dPairs, ident.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice));
    }
    if (!multi && (st = reserve_start_backup(c))) return st;
    const int stride = strip ? std::max(S.plan.s.tiles, S.tail.T ? S.tail.s.tiles : 0) : N;
    if ((st = eps_reserve(c, T, stride, (size_t)T * N))) return st;
    int cur = c->cur; // the buffer that holds the active pairs' flow
    bool zero = start == PairStart::Zero;
    if (start == PairStart::Saved)
        for (int pair : list) HS_HIP(c, copy_pair_flow(c, c->dU[cur], c->dV[cur], c->dUb, c->dVb, pair));
    std::vector<int> active = list, next, rlist;
    std::map<int, std::vector<int>> replays;    // sweeps to replay -> the pairs that stopped there in this chunk
    std::vector<std::pair<int, int>> stopped;   // (pair, buffer its final flow lies in)
    std::vector<unsigned> words;
    std::vector<StallWatch> stall((size_t)N);
    long long done = 0;
    int launches = 0, stalled = -1;
    for (int pair : list) c->pair_res[(size_t)pair].eps_rerun = rerun ? 1 : 0;
    while (!active.empty()) {
        const int n_act = (int)active.size();
        const int chunk = (int)std::min<long long>(T, budget - done);
        HS_HIP(c, hipMemcpyAsync(c->dPairs + N, active.data(), (size_t)n_act * sizeof(int), hipMemcpyHostToDevice, c->stream));
        const int a0 = cur;
        const JPlan &cp = chunk == T ? S.plan : S.tail;
        // the chunk's launches: the active pairs; strip / fold a row of `stride` words per sweep (every launch writes all its
        // words), the other kernels one word per (sweep, active pair), cleared first
        LaunchIo io{c->dEpsTiles, strip ? stride : n_act, 0.f, strip ? 0 : 1, c->dPairs + N, n_act};
        if (multi) {
            if (!strip && (st = eps_clear(c, chunk, n_act))) return st;
            HS_HIP(c, launch_j(c, cp, EpsMode::EverySweep, io, c->dU[cur], c->dV[cur], c->dU[cur ^ 1], c->dV[cur ^ 1], S.coeff, zero ? 1 : 0));
            cur ^= 1;
            launches++;
        } else {
            if (!zero) // the chunk's input, for a replay
                for (int pair : active) HS_HIP(c, copy_pair_flow(c, c->dUb, c->dVb, c->dU[cur], c->dV[cur], pair));
            if ((st = eps_clear(c, chunk, n_act))) return st;
            for (int s = 0; s < chunk; s++) {
                io.eps = c->dEpsTiles + (size_t)s * n_act;
                HS_HIP(c, launch_simple(c, true, io, c->dU[cur], c->dV[cur], c->dU[cur ^ 1], c->dV[cur ^ 1], S.coeff, (zero && s == 0) ? 1 : 0));
                cur ^= 1;
                launches++;
            }
        }
        c->sweeps_run += chunk;
        // one read-back for all active pairs: words[s * n_act + k]
        words.resize((size_t)chunk * n_act);
        if (strip) {
            const int tiles = cp.s.tiles / N * n_act;
            st = eps_collect_enqueue(c, EpsLayout{chunk, stride, 0, 0, tiles, n_act});
            if (st) return st;
            HS_HIP(c, hipStreamSynchronize(c->stream));
            std::memcpy(words.data(), c->hEps, words.size() * sizeof(unsigned));
        } else {
            HS_HIP(c, hipMemcpyAsync(words.data(), c->dEpsTiles, words.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            HS_HIP(c, hipStreamSynchronize(c->stream));
        }
        next.clear();
        replays.clear();
        stopped.clear();
        for (int k = 0; k < n_act; k++) {
            const int pair = active[(size_t)k];
            hsflow_ctx::PairResult &r = c->pair_res[(size_t)pair];
            r.sweeps += chunk;
            int hit = -1;
            float e = 0.f;
            for (int s = 0; s < chunk && hit < 0; s++) {
                std::memcpy(&e, &words[(size_t)s * n_act + k], sizeof(float));
                if ((double)e < p.epsilon) hit = s;
                else stall[(size_t)pair].seen(e, done + s);
            }
            r.last_eps = e;
            r.eps_owed = false;
            bool stop = hit >= 0;
            const int k1 = (hit >= 0 && hit < chunk - 1) ? hit + 1 : 0; // the stop lies inside the chunk: a replay of hit + 1 sweeps
            if (k1) {
                replays[k1].push_back(pair);
                r.sweeps += k1;
            }
            const long long ran = hit >= 0 ? done + hit + 1 : done + chunk;
            if (!stop && S.use_iter && p.max_iter > 0 && ran >= budget) stop = true;
            if (!stop && stall[(size_t)pair].give_up(ran, budget)) {
                stop = true;
                r.status = HSFLOW_E_NOTERM;
                if (stalled < 0) stalled = pair;
            }
            r.iterations_done = (int)std::min<long long>(ran, INT32_MAX);
            if (stop) {
                r.in_both = true;
                // where the pair's final flow lies: behind the chunk, or behind its replay from the chunk's input
                stopped.push_back({pair, !k1 ? cur : multi ? (a0 ^ 1) : (a0 ^ (k1 & 1))});
            } else next.push_back(pair);
        }
        // the replays: exactly hit + 1 sweeps from the chunk's intact input, ONE launch sequence for all pairs that share the count
        rlist.clear();
        for (const auto &g : replays) rlist.insert(rlist.end(), g.second.begin(), g.second.end());
        if (!rlist.empty())
            HS_HIP(c, hipMemcpyAsync(c->dPairs + 2 * (size_t)N, rlist.data(), rlist.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        size_t at = 0;
        for (const auto &g : replays) {
            const int k1 = g.first, n = (int)g.second.size();
            LaunchIo io = default_io(c); // (a replay records no Eps)
            io.pairs = c->dPairs + 2 * (size_t)N + at;
            io.n_pairs = n;
            at += (size_t)n;
            if (multi) {
                JPlan rp;
                if (!make_jplan(c, kernel, k1, p, rp)) return fail(c, HSFLOW_E_SIZE, "no feasible launch plan for the replay");
                HS_HIP(c, launch_j(c, rp, EpsMode::None, io, c->dU[a0], c->dV[a0], c->dU[a0 ^ 1], c->dV[a0 ^ 1], S.coeff, zero ? 1 : 0));
                launches++;
            } else {
                if (!zero)
                    for (int pair : g.second) HS_HIP(c, copy_pair_flow(c, c->dU[a0], c->dV[a0], c->dUb, c->dVb, pair));
                int from = a0;
                for (int s = 0; s < k1; s++) {
                    HS_HIP(c, launch_simple(c, false, io, c->dU[from], c->dV[from], c->dU[from ^ 1], c->dV[from ^ 1], S.coeff, (zero && s == 0) ? 1 : 0));
                    from ^= 1;
                    launches++;
                }
            }
            c->sweeps_run += k1;
        }
        for (const auto &sp : stopped) // a stopped pair's final flow into the other buffer as well
            HS_HIP(c, copy_pair_flow(c, c->dU[sp.second ^ 1], c->dV[sp.second ^ 1], c->dU[sp.second], c->dV[sp.second], sp.first));
        active.swap(next); // (the list uploaded this round is not written again before the next round's read-back)
        done += chunk;
        zero = false;
    }
    c->info.jacobi_launches += launches;
    pairs_to_info(c);
    if (stalled >= 0)
        return fail(c, HSFLOW_E_NOTERM, "EPS termination: Eps of pair " + std::to_string(stalled) + " stopped decreasing above epsilon (fp32 limit "
                                        "cycle) -- its flow of the sweeps done so far is kept; every other pair has stopped "
                                        "(hsflow_get_pair_result)");
    return HSFLOW_OK;
}

// Does this solve stop pair by pair?  (Not the per-sweep pass of hsflow_solve_probe*, nor a one-pair context.)
bool stops_per_pair(const hsflow_ctx *c) { return c->per_pair && c->N > 1 && !c->force_exact; }

// Per-pair verdicts over the witness words of a pass that was reduced per pair (hEps[slot * N + pair]): fills pair_res
// for the proven pairs (standing at the budget) and lists the others.  last_is_exact: as witness_proven.
void pair_verdicts(hsflow_ctx *c, const EpsLayout &words, double epsilon, int iters, bool last_is_exact, std::vector<int> &unproven)
{
    c->pair_res.assign((size_t)c->N, hsflow_ctx::PairResult());
    unproven.clear();
    for (int i = 0; i < c->N; i++) {
        hsflow_ctx::PairResult &r = c->pair_res[(size_t)i];
        float last = 0.f;
        const bool proven = witness_proven(c->hEps + i, words.slots, epsilon, &last, last_is_exact, c->N);
        r.iterations_done = iters;
        r.sweeps = iters;
        r.last_eps = last_is_exact ? last : NAN;
        r.eps_owed = !last_is_exact; // (measure_last_eps; a pair that takes the exact pass measures its own)
        if (!proven) unproven.push_back(i);
    }
}

// Settles an ITER|EPS solve that hsflow_solve_async left unverified: waits for the stream, looks at the
// witness words and, if they do not prove "no early stop", runs the exact pass from the saved start.
// verdict_only: report whether the witness words prove "no early stop" and leave it at that (no exact pass; the flow of
// the whole budget stands) -- for a driver that decides over several contexts (row slabs: hsflow_take_verdict).
int settle_pending(hsflow_ctx *c, int *verdict_only = nullptr)
{
    if (!c->pend.active) return HSFLOW_OK;
    c->pend.active = false;
    HS_HIP(c, hipSetDevice(c->device));
    // the witness words of that solve's launches are still per workgroup: an asynchronous solve enqueues no
    // reduction (a stream of solves would pay a kernel and a boundary per solve for words nobody reads); now
    // that somebody wants the verdict, reduce them into the host's buffer and wait
    if (!c->pend.reduced) { // (hsflow_set_async_reduce: the solve enqueued the reduction itself, right behind its last launch)
        int st0 = eps_collect_enqueue(c, c->pend.words);
        if (st0) return st0;
        HS_HIP(c, hipStreamSynchronize(c->stream));
    } else {
        // ... and a marker behind it: only THAT is waited for, not what other contexts may have enqueued on the same stream
        // since (the slots of a pair pipeline share streams: pair_pipeline.cpp)
        int stw = wait_marker(c, c->pend.mark);
        if (stw) return stw;
    }
    if (c->pend.words.pairs > 0) { // every pair on its own verdict (hsflow_set_pair_termination)
        std::vector<int> unproven;
        pair_verdicts(c, c->pend.words, c->pend.params.epsilon, c->pend.iters, false, unproven);
        pairs_to_info(c);
        if (verdict_only) *verdict_only = unproven.empty() ? 1 : 0;
        if (verdict_only || unproven.empty()) return HSFLOW_OK; // (last_eps of the proven pairs: measure_last_eps)
        SolveSetup S; // (the plan of that solve once more: the chunk launches are its kernel's)
        hsflow_params q = c->pend.params;
        const int st = prepare_solve(c, q, false, S);
        if (st) return st;
        return solve_pairs_exact(c, S, unproven, q.use_previous ? PairStart::Saved : PairStart::Zero, true);
    }
    float last = 0.f;
    const bool gave_up = persist_gave_up(c); // a persistent launch that timed out proves nothing
    if (!gave_up && witness_proven(c->hEps, c->pend.words.slots, c->pend.params.epsilon, &last, false)) {
        c->info.iterations_done = c->pend.iters;
        c->info.last_eps = NAN; // not measured by an asynchronous solve; hsflow_get_info measures it on demand (c->lastl)
        if (verdict_only) *verdict_only = 1;
        return HSFLOW_OK;
    }
    if (verdict_only && !gave_up) { // not proven, and the caller decides what follows
        *verdict_only = 0;
        c->info.iterations_done = c->pend.iters;
        c->info.last_eps = NAN;
        return HSFLOW_OK;
    }
    c->lastl.valid = false;
    hsflow_params q = c->pend.params;
    q.reuse_derivatives = gave_up ? 0 : 1; // the coefficient plane of that solve is still in place
    if (q.kernel == HSFLOW_KERNEL_PERSIST) q.kernel = HSFLOW_KERNEL_STRIP;
    if (q.use_previous) {
        c->cur = c->pend.cur0;
        int str = restore_start(c);
        if (str) return str;
    }
    const long long sweeps = c->sweeps_run; // (those of the witness pass)
    c->force_exact = true;
    const int st = solve_impl(c, &q, false);
    c->force_exact = false;
    c->info.eps_rerun = 1;
    c->info.jacobi_launches += c->pend.launches;
    c->sweeps_run += sweeps;
    return st;
}

// last_eps of an asynchronous ITER|EPS solve, on demand: the solve ran witness launches only (they prove "no early
// stop" but measure nothing).  Its last launch left its input buffer intact, so that launch is simply run again with
// the final sweep's Eps measured (EpsMode::WitnessLast); it rewrites the flow with the same values.
int measure_last_eps(hsflow_ctx *c)
{
    if (!c->lastl.valid) return HSFLOW_OK;
    c->lastl.valid = false;
    const hsflow_ctx::LastLaunch &L = c->lastl;
    if (c->pair_res_valid) { // (a per-pair solve whose pairs were all re-run owes nothing)
        bool owed = false;
        for (const hsflow_ctx::PairResult &r : c->pair_res) owed = owed || r.eps_owed;
        if (!owed) return HSFLOW_OK;
    }
    const int stride = L.plan.s.tiles;
    int st = eps_reserve(c, 2, stride, c->pair_res_valid ? 2 * (size_t)c->N : 0);
    if (st) return st;
    const int b = c->cur, a = b ^ 1;
    const float *ui = L.from_third ? c->dUp : c->dU[a], *vi = L.from_third ? c->dVp : c->dV[a];
    HS_HIP(c, launch_j(c, L.plan, EpsMode::WitnessLast, LaunchIo{c->dEpsTiles, stride, L.eps_thr}, ui, vi, c->dU[b], c->dV[b], L.coeff, L.zero_in));
    if (c->pair_res_valid) { // a per-pair solve: the proven pairs' last sweep, each over its own workgroups
        if ((st = eps_collect_enqueue(c, EpsLayout{2, stride, 0, 0, stride, c->N}))) return st;
        // the launch also ran over the pairs that stopped early: their final flow comes back from the other buffer
        for (int i = 0; i < c->N; i++)
            if (c->pair_res[(size_t)i].in_both) HS_HIP(c, copy_pair_flow(c, c->dU[b], c->dV[b], c->dU[a], c->dV[a], i));
        HS_HIP(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < c->N; i++) {
            hsflow_ctx::PairResult &r = c->pair_res[(size_t)i];
            if (!r.eps_owed) continue;
            std::memcpy(&r.last_eps, &c->hEps[(size_t)c->N + i], sizeof(float));
            r.eps_owed = false;
        }
        pairs_to_info(c);
        return HSFLOW_OK;
    }
    if ((st = eps_collect_enqueue(c, EpsLayout{2, stride, 0, 0, stride}))) return st;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    float last = 0.f;
    std::memcpy(&last, &c->hEps[1], sizeof(float));
    c->info.last_eps = last;
    return HSFLOW_OK;
}

// Replays the hipGraph cached under `key`, capturing it first if needed.  `enqueue` issues the launch sequence on
// c->stream and reports how many Jacobi launches it made.  Kernel attributes cannot be set inside a capture, so ahead
// of one the sequence is walked once as a dry run (hsflow_ctx::configuring), which sets those of exactly the kernel
// variants the sequence launches.  On return c->cur is where the sequence leaves the flow.
template <class Enqueue>
int run_captured(hsflow_ctx *c, const GraphKey &key, Enqueue enqueue, int *launches)
{
    if (!c->stream)
        return fail(c, HSFLOW_E_ARG, "use_graph: the default (NULL) stream cannot be captured; create the "
                                     "context on a non-default stream or with own_stream");
    auto it = c->graphs.find(key);
    if (it == c->graphs.end()) {
        const int cur0 = c->cur;
        int n = 0;
        c->configuring = true;
        int st = enqueue(&n);
        c->configuring = false;
        c->cur = cur0;
        if (st) return st;
        HS_HIP(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        st = enqueue(&n);
        hipGraph_t graph = nullptr;
        const hipError_t e = hipStreamEndCapture(c->stream, &graph);
        if (st) { if (graph) hipGraphDestroy(graph); c->cur = cur0; return st; }
        if (e != hipSuccess) { c->cur = cur0; return fail(c, HSFLOW_E_DEVICE, std::string("hipStreamEndCapture: ") + hipGetErrorString(e)); }
        GraphEntry ge{};
        ge.graph = graph;
        ge.cur_after = c->cur;
        ge.launches = n;
        HS_HIP(c, hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0));
        trim_graph_cache(c);
        it = c->graphs.emplace(key, ge).first;
    }
    HS_HIP(c, hipGraphLaunch(it->second.exec, c->stream));
    c->cur = it->second.cur_after;
    *launches = it->second.launches;
    return HSFLOW_OK;
}

// CLASSIC mode (Kernels.cl semantics, v restored): derivatives once, then max_iter fused average+update sweeps --
// several per launch on a register strip (k_classic_strip) or an LDS tile (k_jacobi_classic_fused), or one per launch
// (k_jacobi_classic).  The reference loop has no other stop rule (HSOpticalFlowOpenCL.cpp:750-751), so only ITER
// termination is accepted.  The launch sequence can be one hipGraph (use_graph), like the CV-mode solve.
struct ClassicSetup {
    int kernel, T; // kernel actually used (AUTO resolved), sweeps per full launch
    ClassicStripPlan splan, stail;
    FusedPlan fplan, ftail;
};

// Checks the parameters, picks the kernel and the launch plans and writes the plan into c->info (hsflow_plan_query
// stops here; no device is touched).
int prepare_classic(hsflow_ctx *c, const hsflow_params &p, ClassicSetup &S)
{
    if (p.term_type != HSFLOW_TERM_ITER) return fail(c, HSFLOW_E_ARG, "CLASSIC mode supports ITER termination only");
    if (p.max_iter <= 0) return fail(c, HSFLOW_E_NOTERM, "ITER termination with max_iter <= 0 would never stop");
    if (!(p.alpha > 0.f) || !std::isfinite(p.alpha)) return fail(c, HSFLOW_E_ARG, "alpha must be positive");
    const float a2 = p.alpha * p.alpha; // Kernels.cl:85
    // which kernel: the register strip wherever the image has an aligned shape for it (classic_strip_geom), else the LDS tile
    int kernel = p.kernel;
    if (kernel != HSFLOW_KERNEL_AUTO && kernel != HSFLOW_KERNEL_SIMPLE && kernel != HSFLOW_KERNEL_FUSED && kernel != HSFLOW_KERNEL_STRIP)
        return fail(c, HSFLOW_E_ARG, "CLASSIC mode has the simple, the fused (LDS tile) and the strip kernels only");
    int T = 1;
    if (kernel == HSFLOW_KERNEL_AUTO || kernel == HSFLOW_KERNEL_STRIP) {
        T = p.fuse_steps > 0 ? std::min(p.fuse_steps, kMaxFuse) : pick_classic_strip_T(c, p.max_iter, p.strip_rows, p.threads);
        const bool tiles_apply = T > 0 && (kernel == HSFLOW_KERNEL_STRIP || (!p.tile_w && !p.tile_h));
        if (T <= 0) T = 1;
        // (the strip kernels divide with a precomputed reciprocal: legal while alpha^2 is nowhere near the ends of the
        // exponent range, hs_kernels_classic_strip.hip.h)
        const bool alpha_ok = a2 >= 0x1p-40f && a2 <= 0x1p40f;
        bool ok = alpha_ok && tiles_apply && make_classic_strip_plan(c, T, p.strip_rows, p.threads, S.splan);
        const int rem = p.max_iter % T;
        if (ok && rem) ok = make_classic_strip_plan(c, rem, p.strip_rows, p.threads, S.stail);
        if (ok) kernel = HSFLOW_KERNEL_STRIP;
        else if (kernel == HSFLOW_KERNEL_STRIP)
            return fail(c, alpha_ok ? HSFLOW_E_SIZE : HSFLOW_E_ARG,
                        alpha_ok ? "CLASSIC mode: no strip shape for this image / fuse_steps / strip_rows / threads"
                                 : "CLASSIC mode: the strip kernel takes 2^-20 <= alpha <= 2^20");
        else kernel = HSFLOW_KERNEL_FUSED;
    }
    if (kernel == HSFLOW_KERNEL_FUSED) {
        // 18 LDS values per plane and group and an IEEE division make a sweep dearer than in CV mode:
        // the halo pays off up to about 6 sweeps per launch (tools/sweep_classic.py on MI355X)
        T = p.fuse_steps > 0 ? std::min(p.fuse_steps, kMaxFuse) : std::min(6, p.max_iter);
        if (!make_plan(c, T, p.tile_w, p.tile_h, p.threads, S.fplan))
            return fail(c, HSFLOW_E_SIZE, "no feasible tile for the requested fuse_steps / tile / threads");
        const int rem = p.max_iter % T;
        if (rem && !make_plan(c, rem, p.tile_w, p.tile_h, p.threads, S.ftail))
            return fail(c, HSFLOW_E_SIZE, "no feasible tile for the tail launch");
    }
    if (kernel == HSFLOW_KERNEL_SIMPLE) T = 1;
    S.kernel = kernel;
    S.T = T;
    hsflow_info &i = c->info;
    i.kernel = kernel; i.fuse_steps = T;
    if (kernel == HSFLOW_KERNEL_STRIP) {
        i.tile_w = S.splan.g.CW; i.tile_h = S.splan.g.CH; i.threads = S.splan.g.NW * 64;
        i.groups_per_thread = S.splan.R; i.tiles = S.splan.tiles; i.lds_bytes = S.splan.lds_bytes;
    } else if (kernel == HSFLOW_KERNEL_FUSED) {
        i.tile_w = S.fplan.g.CW; i.tile_h = S.fplan.g.CH; i.threads = S.fplan.NT;
        i.groups_per_thread = S.fplan.K; i.tiles = S.fplan.tiles; i.lds_bytes = S.fplan.lds_bytes;
    } else {
        i.tile_w = i.tile_h = 0; i.threads = 256; i.groups_per_thread = 1; i.tiles = 0; i.lds_bytes = 0;
    }
    i.jacobi_launches = (p.max_iter + T - 1) / T;
    return HSFLOW_OK;
}

int solve_classic(hsflow_ctx *c, const hsflow_params &p, bool async)
{
    ClassicSetup S;
    int st = prepare_classic(c, p, S);
    if (st) return st;
    if (p.profile && (p.use_graph || async)) return fail(c, HSFLOW_E_ARG, "CLASSIC mode: profiling needs a synchronous solve without use_graph");
    Profiler prof{c, p.profile != 0};
    const dim3 block(64, 4);
    auto grid = [&](int pairs) { return dim3((c->W + 255) / 256, (c->H + 3) / 4, pairs); }; // for_pair_batches
    const bool do_deriv = needs_deriv(c, p, HSFLOW_MODE_CLASSIC);
    const float a2 = p.alpha * p.alpha; // Kernels.cl:85
    const bool write_v = p.mode != HSFLOW_MODE_CLASSIC_AS_SHIPPED;
    const bool zero0 = !p.use_previous;
    const int kernel = S.kernel, T = S.T;
    const ClassicStripPlan &splan = S.splan, &stail = S.stail;
    const FusedPlan &fplan = S.fplan, &ftail = S.ftail;
    // The derivatives live as one packed word per pixel (k_deriv_classic_packed; what the strip kernel loads); the
    // LDS-tile and the one-sweep kernels read three fp32 planes, unpacked once per derivative pass when they run.
    const bool need_planes = kernel != HSFLOW_KERNEL_STRIP;
    if (need_planes) {
        const size_t px = (size_t)c->plane * c->N;
        for (int i = 0; i < 3; i++)
            if (!c->dE[i]) HS_HIP(c, hipMalloc((void **)&c->dE[i], px * sizeof(float)));
    }
    const bool do_unpack = need_planes && (do_deriv || !c->dE_valid);
    auto enqueue = [&](int *n) -> int {
        if (do_deriv) {
            prof.begin(0);
            HS_HIP(c, for_pair_batches(c, [&](long long o, int pairs) {
                hipLaunchKernelGGL(hsk::k_deriv_classic_packed, grid(pairs), block, 0, c->stream, c->dA + o, c->dB + o, c->dCoef + o,
                                   c->W, c->H, c->P, c->plane);
            }));
            prof.end();
        }
        if (do_unpack) {
            HS_HIP(c, for_pair_batches(c, [&](long long o, int pairs) {
                hipLaunchKernelGGL(hsk::k_unpack_classic_deriv, grid(pairs), block, 0, c->stream, c->dCoef + o, c->dE[0] + o, c->dE[1] + o,
                                   c->dE[2] + o, c->W, c->H, c->P, c->plane);
            }));
        }
        int zero = zero0 ? 1 : 0;
        if (zero) c->cur = 0;
        int done = 0, launches = 0;
        while (done < p.max_iter) {
            const int chunk = std::min(T, p.max_iter - done);
            const int a = c->cur, b = a ^ 1;
            prof.begin(1);
            hipError_t e;
            if (kernel == HSFLOW_KERNEL_STRIP) {
                ClassicStripPlan cp = chunk == T ? splan : stail;
                cp.g.zero_in = zero;
                e = launch_classic_strip(c, cp, write_v, c->dU[a], c->dV[a], c->dU[b], c->dV[b], a2);
            } else if (kernel == HSFLOW_KERNEL_FUSED) {
                FusedPlan cp = chunk == T ? fplan : ftail;
                cp.g.zero_in = zero;
                e = launch_classic_fused(c, cp, write_v, c->dU[a], c->dV[a], c->dU[b], c->dV[b], a2);
            } else {
                auto kern = zero ? (write_v ? hsk::k_jacobi_classic<true, true> : hsk::k_jacobi_classic<true, false>)
                                 : (write_v ? hsk::k_jacobi_classic<false, true> : hsk::k_jacobi_classic<false, false>);
                e = for_pair_batches(c, [&](long long o, int pairs) {
                    hipLaunchKernelGGL(kern, grid(pairs), block, 0, c->stream, c->dE[0] + o, c->dE[1] + o, c->dE[2] + o, c->dU[a] + o,
                                       c->dV[a] + o, c->dU[b] + o, c->dV[b] + o, c->W, c->H, c->P, c->plane, a2);
                });
            }
            prof.end();
            HS_HIP(c, e);
            c->cur = b;
            zero = 0;
            done += chunk;
            launches++;
        }
        *n = launches;
        return HSFLOW_OK;
    };
    hsflow_info &i = c->info;
    int launches = 0;
    if (p.use_graph) {
        const GraphKey key = graph_key(c, p, kernel, T, (do_deriv ? kKeyDeriv : 0) + (do_unpack ? kKeyUnpack : 0), p.alpha);
        if ((st = run_captured(c, key, enqueue, &launches))) return st;
    } else if ((st = enqueue(&launches))) return st;
    c->coef_valid = true;
    c->coef_mode = HSFLOW_MODE_CLASSIC;
    c->dE_valid = do_unpack || (c->dE_valid && !do_deriv);
    i.jacobi_launches = launches;
    c->sweeps_run += p.max_iter;
    i.iterations_done = p.max_iter; i.last_eps = 0.f; i.deriv_ms = i.jacobi_ms = i.solve_ms = 0.f;
    if (!async) {
        HS_HIP(c, hipStreamSynchronize(c->stream));
        prof.collect();
    }
    return HSFLOW_OK;
}

// A pass of `sweeps` sweeps with the setup's kernel: launches of `plan` and, where the count leaves a remainder, a last
// one of `tail`; the one-sweep kernel takes a launch per sweep.  Records nothing; the caller fills in what its pass adds.
Pass sweeps_pass(const SolveSetup &S, int sweeps, const JPlan &plan, const JPlan &tail, bool zero)
{
    Pass P;
    P.sweeps = sweeps;
    P.n = S.multi ? (sweeps + plan.T - 1) / plan.T : sweeps;
    if (S.multi) { P.plan = &plan; P.last = sweeps % plan.T ? &tail : &plan; }
    P.coeff = S.coeff;
    P.zero = zero;
    return P;
}

// The plan of a budget pass's last launch.
const JPlan &last_plan(const SolveSetup &S) { return S.tail.T ? S.tail : S.plan; }

// How launch 0 of a solve's first pass is formed.  The derivative pass rides in it where the kernel can do it (not when
// profiling: deriv_ms / jacobi_ms then keep their meaning).  The frames of hsflow_solve_async_frames_device are read in
// place by it where it is the strip kernel with the derivative pass, else copied now, ahead of whatever reads dA / dB.
// (Launch 0 is a launch of P.plan: a setup's T never exceeds its budget.)
int form_first_launch(hsflow_ctx *c, const hsflow_params &p, Pass &P)
{
    P.deriv = needs_deriv(c, p, HSFLOW_MODE_CV);
    P.fuse = P.deriv && !p.profile && P.plan && strip_deriv_fusable(c, *P.plan);
    c->info.deriv_fused = P.fuse;
    P.in_place = c->lazy.active && P.fuse && !P.persist && P.plan->kind == HSFLOW_KERNEL_STRIP;
    return resolve_lazy_frames(c, P.in_place, &P.frames);
}

// Enqueues launches [first, last) of a pass (no host synchronisation, nothing allocated: capturable).  The range with
// launch 0 opens the pass: the starting flow saved, the derivative kernel unless launch 0 carries that pass, a cold start
// from buffer 0 -- u = v = 0 there means that launch 0 is TOLD its input is zero, instead of two planes cleared and read
// back.  The range with the last launch closes it: the reduction of the Eps rows.  A later range takes c->cur as the
// earlier one left it.
int enqueue_pass(hsflow_ctx *c, const Pass &P, int first, int last, Profiler &prof)
{
    int st = HSFLOW_OK;
    if (first == 0) {
        if (P.save_start && (st = save_start(c))) return st;
        if (P.deriv && !P.fuse) {
            prof.begin(0);
            HS_HIP(c, launch_deriv(c));
            prof.end();
        }
        if (P.zero) c->cur = 0;
    }
    // launch (phase) L writes row L of the Eps rows (no clearing: every launch writes all its words, the reduction reads
    // only those)
    auto io_of = [&](int L) {
        LaunchIo io = P.eps_rows ? LaunchIo{P.eps_rows + (size_t)L * P.stride, P.stride, P.thr} : default_io(c);
        if (L == 0 && P.in_place) io.frames = &P.frames;
        return io;
    };
    if (P.persist) { // the whole pass as one launch, a row of Eps words per phase
        prof.begin(1);
        st = enqueue_persist(c, P.plan->s, P.sweeps, P.eps, io_of(0), P.fuse, P.zero ? 1 : 0, P.coeff);
        prof.end();
        if (st) return st;
    } else for (int L = first; L < last; L++) {
        const bool is_last = L == P.n - 1;
        const int a = c->cur, b = a ^ 1, zero_in = (L == 0 && P.zero) ? 1 : 0;
        prof.begin(1);
        const hipError_t e = P.plan ? launch_j(c, is_last ? *P.last : *P.plan, is_last ? P.eps_last : P.eps, io_of(L), c->dU[a], c->dV[a],
                                               c->dU[b], c->dV[b], P.coeff, zero_in, L == 0 && P.fuse)
                                    : launch_simple(c, false, io_of(L), c->dU[a], c->dV[a], c->dU[b], c->dV[b], P.coeff, zero_in);
        prof.end();
        HS_HIP(c, e);
        c->cur = b;
    }
    return last == P.n && P.reduce ? eps_collect_enqueue(c, *P.reduce, P.mark) : HSFLOW_OK;
}

// Puts a solve's pass on the stream and reports its Jacobi launches.  use_graph: replayed from the graph cache
// (run_captured), under a key of the setup, the pass and the caller's kKey* bits.  A launch 0 that reads the caller's
// frames carries THIS submission's pointers, which a cached graph cannot: it goes out by itself, and the graph holds the
// launches after it (none: nothing worth a graph).
int issue_pass(hsflow_ctx *c, const SolveSetup &S, const Pass &P, int key_flags, Profiler &prof, int *launches)
{
    const hsflow_params &p = S.eff;
    int st = HSFLOW_OK, first = 0;
    const int n = *launches = P.persist ? 1 : P.n;
    if (!p.use_graph || p.profile) {
        if (P.persist && (st = configure_persist(c, P.plan->s, P.eps, P.fuse, P.coeff))) return st;
        return enqueue_pass(c, P, 0, P.n, prof);
    }
    // (the key before anything moves c->cur)
    const GraphKey key = graph_key(c, p, P.persist ? HSFLOW_KERNEL_PERSIST : S.kernel, S.T,
                                   key_flags + (P.deriv ? kKeyDeriv : 0) + (P.in_place ? kKeyInPlace : 0), S.coeff, P.eps_rows ? P.thr : -1.f);
    if (P.in_place) {
        if ((st = enqueue_pass(c, P, 0, 1, prof)) || P.n == 1) return st;
        first = 1;
    }
    return run_captured(c, key, [&](int *m) { *m = n; return enqueue_pass(c, P, first, P.n, prof); }, launches);
}

// ITER termination: a fixed sweep count, nothing on the host between launches (optionally one hipGraph).
int solve_fixed(hsflow_ctx *c, const SolveSetup &S, Profiler &prof, bool async)
{
    const hsflow_params &p = S.eff;
    const int iters = (int)S.budget;
    int st = HSFLOW_OK;
    if (S.persist) { // buffers and phase counters: outside any capture
        if ((st = persist_reserve(c)) || (st = persist_prepare_flags(c, S.plan.s.tiles))) return st;
    }
    Pass P = sweeps_pass(S, iters, S.plan, S.tail, !p.use_previous);
    P.persist = S.persist;
    if ((st = form_first_launch(c, p, P)) || (st = issue_pass(c, S, P, 0, prof, &c->info.jacobi_launches))) return st;
    c->coef_valid = true;
    c->coef_mode = HSFLOW_MODE_CV;
    c->info.iterations_done = iters;
    c->sweeps_run += iters;
    if (S.persist && async) c->persist_unchecked = true; // looked at when the stream is next drained (check_persist)
    if (!async) {
        HS_HIP(c, hipStreamSynchronize(c->stream));
        if (S.persist && persist_error(c)) { // a wait timed out: back to a launch per fuse_steps iterations, for good
            persist_failed(c);
            c->cur ^= 1; // the starting flow is intact (the phases wrote the other two buffers)
            hsflow_params q = p;
            if (q.kernel == HSFLOW_KERNEL_PERSIST) q.kernel = HSFLOW_KERNEL_STRIP;
            q.reuse_derivatives = 0;
            return solve_impl(c, &q, false);
        }
        prof.collect();
        if (c->dStamps && (S.kernel == HSFLOW_KERNEL_STRIP || S.kernel == HSFLOW_KERNEL_FOLD)) dump_stamps(c, S.plan.s.tiles);
    }
    return HSFLOW_OK;
}

// Index of the first of n Eps words below epsilon, -1 if there is none.  *last: that word, else the last one.
int first_eps_hit(const unsigned *w, int n, double epsilon, float *last)
{
    for (int s = 0; s < n; s++) {
        std::memcpy(last, &w[s], sizeof(float));
        if ((double)*last < epsilon) return s;
    }
    return -1;
}

// The threshold of witness launches, and whether launches of T sweeps can use it: hs_stop_rule.h.
using hsstop::witness_threshold;
using hsstop::witness_usable;

// The witness pass of ITER|EPS: the budget runs at full speed, nothing on the host between launches.  All launches but
// the last run the kernels' witness mode, which costs almost nothing over the ITER-only kernel and yields one number per
// launch that proves "Eps >= epsilon in every one of my sweeps" when it is >= epsilon.  If every bound holds, the early
// stop cannot have fired before the budget ran out (a stop AT the final sweep is the budget) and the result stands.
// Synchronous solves report last_eps at once: their last launch measures its final sweep too (WitnessLast: two words per
// workgroup, the witness and that sweep's Eps).  Asynchronous solves run witness launches only and leave the check owed
// (c->pend: settle_pending); their last_eps is measured if and when hsflow_get_info asks for it (c->lastl:
// measure_last_eps).
// stride: words per row; *launches: Jacobi launches enqueued.
// *rerun: nothing is proven (a flat or converged input) -- the starting flow is back in place for the exact pass.
int witness_pass(hsflow_ctx *c, const SolveSetup &S, int stride, Profiler &prof, bool async, int *launches, bool *rerun,
                 std::vector<int> *unproven = nullptr)
{
    const hsflow_params &p = S.eff;
    const bool per_pair = stops_per_pair(c); // the words are reduced per pair, and each pair gets its own verdict
    const int iters = (int)S.budget, cur0 = c->cur;
    const JPlan &plan = S.plan, &lastp = last_plan(S);
    int st = HSFLOW_OK;
    const bool persist = S.persist && async; // (prepare_solve grants it to asynchronous solves only)
    if (persist && ((st = persist_reserve(c)) || (st = persist_prepare_flags(c, plan.s.tiles)))) return st;
    Pass P = sweeps_pass(S, iters, plan, S.tail, !p.use_previous); // (persist: its launches are the phases; the witness words are laid out alike)
    P.persist = persist;
    P.eps = EpsMode::Witness;
    P.eps_last = async ? EpsMode::Witness : EpsMode::WitnessLast;
    P.stride = stride;
    P.thr = witness_threshold(p.epsilon);
    P.save_start = p.use_previous != 0;
    // (persist: the tail phase keeps the plan's geometry)
    const EpsLayout words{P.n - 1 + (async ? 1 : 2), stride, P.n - 1, plan_eps_stride(S.kernel, plan),
                          plan_eps_stride(S.kernel, persist ? plan : lastp), per_pair ? c->N : 0};
    if ((st = eps_reserve(c, words.slots, stride, per_pair ? (size_t)words.slots * c->N : 0))) return st;
    P.eps_rows = c->dEpsTiles;
    // an asynchronous solve leaves the reduction of the witness words until somebody settles the check (settle_pending),
    // unless the in-stream reduction is on: its last workgroup then writes the marker too
    if (!async || c->async_reduce) P.reduce = &words;
    P.mark = async && c->hMark != nullptr;
    const int flags = (async ? kKeyAsync : 0) + (async && c->async_reduce ? kKeyAsyncReduce : 0) + (per_pair ? kKeyPerPair : 0);
    if ((st = form_first_launch(c, p, P)) || (st = issue_pass(c, S, P, flags, prof, launches))) return st;
    c->coef_valid = true;
    c->coef_mode = HSFLOW_MODE_CV;
    if (persist) c->persist_unchecked = true;
    c->info.iterations_done = iters;
    c->info.jacobi_launches = *launches;
    c->sweeps_run += iters;
    if (async) { // the check is owed: hsflow_synchronize (or the next call that needs results) settles it
        // what measure_last_eps needs: the last launch again (persist: the last phase as an ordinary launch, from the third buffer)
        const int zero_in = (P.n == 1 && P.zero && !persist) ? 1 : 0; // a single launch from zero flow
        c->lastl = hsflow_ctx::LastLaunch{true, lastp, zero_in, S.coeff, P.thr, persist};
        c->pend.active = true;
        c->pend.params = p;
        c->pend.iters = iters; c->pend.launches = *launches; c->pend.cur0 = cur0;
        c->pend.words = words;
        c->pend.reduced = c->async_reduce;
        c->pend.marked_by_reduce = c->async_reduce && c->hMark != nullptr;
        return HSFLOW_OK;
    }
    HS_HIP(c, hipStreamSynchronize(c->stream));
    if (per_pair) { // the proven pairs stand at the budget, where this pass left them; the others take the exact pass (caller)
        pair_verdicts(c, words, p.epsilon, iters, true, *unproven);
        pairs_to_info(c);
        *rerun = !unproven->empty();
        if (!*rerun) prof.collect();
        return HSFLOW_OK;
    }
    float last = 0.f;
    if (witness_proven(c->hEps, words.slots, p.epsilon, &last, true)) {
        c->info.last_eps = last;
        prof.collect();
        return HSFLOW_OK;
    }
    // not proven: restore the starting flow and measure every sweep
    *rerun = true;
    c->info.eps_rerun = 1;
    c->cur = cur0;
    return p.use_previous ? restore_start(c) : HSFLOW_OK;
}

// The exact pass of ITER|EPS: every sweep records its Eps on the device (one row of `stride` words per sweep, reserved
// and cleared by the caller, solve_iter_eps); one read-back at the end finds the first sweep k with Eps_k < epsilon.  If
// there is none the result stands; otherwise exactly k sweeps are re-run from the saved starting flow, which reproduces the oracle's
// stopping sweep.  launches: those of a witness pass that proved nothing, which this pass then follows.
int exact_pass(hsflow_ctx *c, const SolveSetup &S, int stride, Profiler &prof, int launches)
{
    const hsflow_params &p = S.eff;
    const int iters = (int)S.budget, T = S.T;
    int st = HSFLOW_OK, zero_in = p.use_previous ? 0 : 1, done = 0;
    if (c->probe_pairs && c->N > 1 && (st = eps_reserve(c, iters, stride, (size_t)iters * c->N))) return st;
    const bool strip_words = S.kernel == HSFLOW_KERNEL_STRIP || S.kernel == HSFLOW_KERNEL_FOLD;
    const bool pair_words = c->probe_pairs && c->N > 1 && !strip_words; // (stride = N: solve_iter_eps)
    if (zero_in) c->cur = 0;
    while (done < iters) {
        const int chunk = S.multi ? std::min(T, iters - done) : 1;
        const JPlan &cp = chunk == T ? S.plan : S.tail;
        const int a = c->cur, b = a ^ 1;
        const LaunchIo io{c->dEpsTiles + (size_t)done * stride, stride, 0.f, pair_words ? 1 : 0};
        prof.begin(1);
        hipError_t e = S.multi ? launch_j(c, cp, EpsMode::EverySweep, io, c->dU[a], c->dV[a], c->dU[b], c->dV[b], S.coeff, zero_in)
                               : launch_simple(c, true, io, c->dU[a], c->dV[a], c->dU[b], c->dV[b], S.coeff, zero_in);
        prof.end();
        HS_HIP(c, e);
        c->cur = b;
        zero_in = 0;
        done += chunk;
        launches++;
    }
    c->sweeps_run += iters;
    std::vector<unsigned> heps;
    if ((st = eps_collect(c, iters, stride, heps))) return st;
    c->sweep_eps.resize((size_t)iters); // (hsflow_solve_probe hands these out)
    std::memcpy(c->sweep_eps.data(), heps.data(), (size_t)iters * sizeof(float));
    if (pair_words) { // the rows ARE per pair (the batch's Eps above is their maximum, by k_eps_reduce over N words a row)
        c->sweep_eps_pairs.resize((size_t)iters * c->N);
        HS_HIP(c, hipMemcpy(c->sweep_eps_pairs.data(), c->dEpsTiles, (size_t)iters * c->N * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (c->probe_pairs && c->N > 1 && strip_words) {
        // hsflow_solve_probe_pairs: the same rows once more, per pair (the rows of a short last launch hold fewer words)
        const EpsLayout pw{iters, stride, iters / T * T, plan_eps_stride(S.kernel, S.plan), plan_eps_stride(S.kernel, last_plan(S)), c->N};
        if ((st = eps_collect_enqueue(c, pw))) return st;
        HS_HIP(c, hipStreamSynchronize(c->stream));
        c->sweep_eps_pairs.resize((size_t)iters * c->N);
        std::memcpy(c->sweep_eps_pairs.data(), c->hEps, (size_t)iters * c->N * sizeof(float));
    }
    float last = 0.f;
    const int hit = first_eps_hit(heps.data(), iters, p.epsilon, &last);
    if (hit >= 0 && hit + 1 < iters) { // converged early: redo exactly hit+1 sweeps from the start
        const int k = hit + 1;
        if (p.use_previous && (st = restore_start(c))) return st;
        JPlan kp, kt; // (a data-dependent length: planned on demand)
        if (S.multi) {
            const int Tk = std::min(T, k);
            if (!make_jplan(c, S.kernel, Tk, p, kp)) return fail(c, HSFLOW_E_SIZE, "no feasible launch plan for the re-run");
            if (k % Tk && !make_jplan(c, S.kernel, k % Tk, p, kt)) return fail(c, HSFLOW_E_SIZE, "no feasible launch plan for the re-run tail");
        }
        const Pass rerun = sweeps_pass(S, k, kp, kt, !p.use_previous);
        if ((st = enqueue_pass(c, rerun, 0, rerun.n, prof))) return st;
        launches += rerun.n;
        c->sweeps_run += k;
        HS_HIP(c, hipStreamSynchronize(c->stream));
        c->info.iterations_done = k;
    } else {
        c->info.iterations_done = hit >= 0 ? hit + 1 : iters;
    }
    c->info.last_eps = last;
    c->info.jacobi_launches = launches;
    prof.collect();
    return HSFLOW_OK;
}

// Per-pair stop without a witness pass (the simple and the LDS-tile kernel, EPS alone): the derivative pass for all pairs,
// then every pair through the exact pass from the flow it starts with.
int solve_pairs_all(hsflow_ctx *c, const SolveSetup &S)
{
    const hsflow_params &p = S.eff;
    int st = resolve_lazy_frames(c, false);
    if (st) return st;
    if (needs_deriv(c, p, HSFLOW_MODE_CV)) HS_HIP(c, launch_deriv(c));
    c->coef_valid = true;
    c->coef_mode = HSFLOW_MODE_CV;
    c->pair_res.assign((size_t)c->N, hsflow_ctx::PairResult());
    c->info.jacobi_launches = 0;
    std::vector<int> all((size_t)c->N);
    for (int i = 0; i < c->N; i++) all[(size_t)i] = i;
    return solve_pairs_exact(c, S, all, p.use_previous ? PairStart::Current : PairStart::Zero, false);
}

// ITER|EPS -- the way the reference calls the solver (OpticalFlowOpenCV.cpp:29).  On real image pairs Eps never drops
// below 1e-6 within the sweep budget, so the budget is run SPECULATIVELY wherever the kernel has a witness mode
// (witness_pass); the exact pass measures every sweep where there is none, where a solve is being settled
// (force_exact) and where the witness proved nothing.
int solve_iter_eps(hsflow_ctx *c, const SolveSetup &S, Profiler &prof, bool async)
{
    const hsflow_params &p = S.eff;
    const int iters = (int)S.budget, kernel = S.kernel;
    int st = HSFLOW_OK;
    if (p.use_previous && (st = reserve_start_backup(c))) return st; // the starting flow is kept (save_start)
    // every launch of this solve uses the same number of workgroups or fewer (tail): stride = max
    int stride = S.multi ? plan_eps_stride(kernel, S.plan) : 1;
    // hsflow_solve_probe_pairs on the simple / LDS-tile kernel: one word per (sweep, pair) instead of one per sweep
    const bool pair_words = c->probe_pairs && c->N > 1 && kernel != HSFLOW_KERNEL_STRIP && kernel != HSFLOW_KERNEL_FOLD;
    if (pair_words) stride = c->N;
    if (S.tail.T) stride = std::max(stride, plan_eps_stride(kernel, S.tail));
    int launches = 0;
    if (stops_per_pair(c)) { // every pair on its own Eps: the pairs the witness pass could not vouch for, or all of them
        std::vector<int> list;
        if (S.witness) {
            bool rerun = false;
            if ((st = witness_pass(c, S, stride, prof, async, &launches, &rerun, &list)) || !rerun) return st;
            st = solve_pairs_exact(c, S, list, p.use_previous ? PairStart::Saved : PairStart::Zero, true);
            prof.collect(); // (profile = 1: the times of the witness pass; the chunk launches behind it are not bracketed)
            return st;
        }
        return solve_pairs_all(c, S);
    }
    if (S.witness) {
        bool rerun = false;
        if ((st = witness_pass(c, S, stride, prof, async, &launches, &rerun)) || !rerun) return st;
        if ((st = eps_prepare(c, iters, stride))) return st;
    } else {
        if ((st = resolve_lazy_frames(c, false))) return st;
        if (p.use_previous && (st = save_start(c))) return st;
        if ((st = eps_prepare(c, iters, stride))) return st;
        if (needs_deriv(c, p, HSFLOW_MODE_CV)) {
            prof.begin(0);
            HS_HIP(c, launch_deriv(c));
            prof.end();
        }
        c->coef_valid = true;
        c->coef_mode = HSFLOW_MODE_CV;
    }
    return exact_pass(c, S, stride, prof, launches);
}


// EPS without a usable sweep budget (CV_TERMCRIT_EPS alone): Eps_k = max |u_k - u_{k-1}|, |v_k - v_{k-1}|
// is produced per sweep by the kernel; the host looks at it after every chunk and, if the
// threshold was crossed inside the chunk, replays the chunk up to that sweep (its input buffer
// is still intact), which reproduces the oracle's stopping sweep exactly.
int solve_eps_chunks(hsflow_ctx *c, const SolveSetup &S, Profiler &prof)
{
    const hsflow_params &p = S.eff;
    const int kernel = S.kernel, T = S.T;
    const bool multi = S.multi;
    const long long budget = S.budget;
    int st = HSFLOW_OK;
    if (!p.use_previous) {
        c->cur = 0;
        HS_HIP(c, hipMemsetAsync(c->dU[0], 0, (size_t)c->plane * c->N * sizeof(float), c->stream));
        HS_HIP(c, hipMemsetAsync(c->dV[0], 0, (size_t)c->plane * c->N * sizeof(float), c->stream));
    }
    if (needs_deriv(c, p, HSFLOW_MODE_CV)) {
        prof.begin(0);
        HS_HIP(c, launch_deriv(c));
        prof.end();
    }
    c->coef_valid = true;
    c->coef_mode = HSFLOW_MODE_CV;
    long long done = 0;
    int launches = 0;
    float last = 0.f;
    bool stop = false;
    StallWatch stall; // (without a sweep budget the only other exit is Eps < epsilon)
    bool stalled = false;
    while (!stop) {
        const int chunk = (int)std::min<long long>(T, budget - done);
        const JPlan &cp = chunk == T ? S.plan : S.tail;
        const int a = c->cur, b = a ^ 1;
        const int n = multi ? chunk : 1;
        const int stride = multi ? plan_eps_stride(kernel, cp) : 1;
        if ((st = eps_prepare(c, n, stride))) return st;
        const LaunchIo io{c->dEpsTiles, stride};
        prof.begin(1);
        if (!multi)
            HS_HIP(c, launch_simple(c, true, io, c->dU[a], c->dV[a], c->dU[b], c->dV[b], S.coeff));
        else
            HS_HIP(c, launch_j(c, cp, EpsMode::EverySweep, io, c->dU[a], c->dV[a], c->dU[b], c->dV[b], S.coeff));
        prof.end();
        launches++;
        c->sweeps_run += n;
        std::vector<unsigned> heps;
        if ((st = eps_collect(c, n, stride, heps))) return st;
        const int hit = first_eps_hit(heps.data(), n, p.epsilon, &last);
        for (int s = 0; s < n && hit < 0; s++) { // (the stall rule)
            float e;
            std::memcpy(&e, &heps[(size_t)s], sizeof(float));
            stall.seen(e, done + s);
        }
        if (hit >= 0 && hit < n - 1) { // crossed inside the chunk: redo exactly hit+1 sweeps
            JPlan rp;
            if (!make_jplan(c, kernel, hit + 1, p, rp))
                return fail(c, HSFLOW_E_SIZE, "no feasible launch plan for the replay");
            prof.begin(1);
            HS_HIP(c, launch_j(c, rp, EpsMode::None, default_io(c), c->dU[a], c->dV[a], c->dU[b], c->dV[b], S.coeff));
            prof.end();
            launches++;
            c->sweeps_run += hit + 1;
            done += hit + 1;
            stop = true;
        } else {
            done += n;
            if (hit >= 0) stop = true;
        }
        c->cur = b;
        if (S.use_iter && p.max_iter > 0 && done >= budget) stop = true;
        if (!stop && stall.give_up(done, budget)) stop = stalled = true;
    }
    HS_HIP(c, hipStreamSynchronize(c->stream));
    c->info.iterations_done = (int)std::min<long long>(done, INT32_MAX);
    c->info.last_eps = last;
    c->info.jacobi_launches = launches;
    prof.collect();
    if (stalled)
        return fail(c, HSFLOW_E_NOTERM, "EPS termination: Eps stopped decreasing above epsilon (fp32 limit cycle) -- "
                                        "the flow of the sweeps done so far is kept");
    return HSFLOW_OK;
}

// CV mode: the checks of the arguments themselves.  Run on every solve, also where the plan comes from the cache: the cache
// key leaves out what does not enter the plan (profile among it), so a cached plan vouches for none of this.
int check_solve_args(hsflow_ctx *c, const hsflow_params &p, bool async)
{
    const bool use_iter = (p.term_type & HSFLOW_TERM_ITER) != 0, use_eps = (p.term_type & HSFLOW_TERM_EPS) != 0;
    if (!use_iter && !use_eps) return fail(c, HSFLOW_E_ARG, "term_type must include ITER and/or EPS");
    if (use_iter && p.max_iter <= 0 && !use_eps)
        return fail(c, HSFLOW_E_NOTERM, "ITER termination with max_iter <= 0 would never stop");
    if (!(p.lambda > 0.f) || !std::isfinite(p.lambda)) return fail(c, HSFLOW_E_ARG, "lambda must be positive");
    // EPS with no sweep budget (EPS alone, or ITER|EPS with max_iter <= 0, which the original treats the same way,
    // cv210.dll VA 0x1012f10b-0x1012f14a) stops only on Eps < epsilon: with epsilon <= 0 or NaN that never happens
    // and the original spins forever.  Refused here; a positive epsilon below the fp32 limit cycle of the
    // iteration is caught at run time (solve_eps_chunks).
    if (use_eps && !(use_iter && p.max_iter > 0) && !(p.epsilon > 0.0 && std::isfinite(p.epsilon)))
        return fail(c, HSFLOW_E_NOTERM, "EPS termination without a sweep budget needs a finite epsilon > 0");
    if (async && p.profile) return fail(c, HSFLOW_E_ARG, "solve_async does not support profiling");
    return HSFLOW_OK;
}

// CV mode: argument checks, kernel choice (AUTO rule) and launch plan.  Touches no device state, so the
// planner can also be queried without a GPU (hsflow_plan_query).  Fills c->info's plan fields.
int prepare_solve(hsflow_ctx *c, const hsflow_params &p, bool async, SolveSetup &S)
{
    int st = check_solve_args(c, p, async);
    if (st) return st;
    const bool use_iter = (p.term_type & HSFLOW_TERM_ITER) != 0, use_eps = (p.term_type & HSFLOW_TERM_EPS) != 0;
    // Ilambda = fl32(1/fl32(lambda)), cv210.dll VA 0x1012e054-0x1012e085.  Kept out of the denormal range
    // (lambda > 8.5e37): v_rsq_f32 in sweep_coefs flushes denormals, and where it matters -- a pixel with
    // Ix = Iy = 0 -- any finite value gives the same update (al = be = 0).
    const float coeff = std::max(1.0f / p.lambda, FLT_MIN);
    // AUTO: the register-strip kernel; below ~1.5 Mpixel per context its folded form (128-column strips:
    // twice the tiles across, so small frames reach more CUs -- measured 5-25 % faster from 160x120 to
    // 1600x900 at 100 sweeps, tools/crossover.py).
    bool small_frame = (long long)c->W * c->H * c->N <= 1500000LL;
    // A context that plans for a share of the chip (hsflow_set_cu_share: pair pipeline slots) wants the cheaper of the two
    // in CU-time, whatever the frame size: the folded kernel's 128-column strips pay twice the column halo.
    if (plan_shared(c) && p.kernel == HSFLOW_KERNEL_AUTO && (p.term_type & HSFLOW_TERM_ITER) && p.max_iter > 0 && p.max_iter <= (1 << 16) && p.fuse_steps <= 0) {
        double cs = 1e300, cf = 1e300;
        pick_strip_T(c, p.max_iter, p, 0, &cs);
        pick_strip_T(c, p.max_iter, p, 1, &cf);
        small_frame = cf < cs;
    }
    // PERSIST is the strip kernel as one launch per solve; AUTO takes it where it can run (persist_obstacle)
    const bool persist_asked = p.kernel == HSFLOW_KERNEL_PERSIST;
    if (use_eps && eps_windowed(c)) small_frame = false; // (the Eps row window is the strip kernel's)
    const int kernel = persist_asked ? HSFLOW_KERNEL_STRIP
                                     : p.kernel != HSFLOW_KERNEL_AUTO ? p.kernel : (small_frame ? HSFLOW_KERNEL_FOLD : HSFLOW_KERNEL_STRIP);
    if (kernel != HSFLOW_KERNEL_SIMPLE && kernel != HSFLOW_KERNEL_FUSED && kernel != HSFLOW_KERNEL_STRIP &&
        kernel != HSFLOW_KERNEL_FOLD)
        return fail(c, HSFLOW_E_ARG, "unknown kernel selector");
    if (use_eps && eps_windowed(c) && (kernel == HSFLOW_KERNEL_FOLD || kernel == HSFLOW_KERNEL_FUSED))
        return fail(c, HSFLOW_E_ARG, "EPS termination over a row window (hsflow_set_eps_rows) runs on the strip or the simple kernel");
    const bool multi = kernel != HSFLOW_KERNEL_SIMPLE;
    if (async && use_eps && !(use_iter && p.max_iter > 0 && p.max_iter <= (1 << 16) &&
                              (kernel == HSFLOW_KERNEL_STRIP || kernel == HSFLOW_KERNEL_FOLD) && !c->force_exact))
        return fail(c, HSFLOW_E_ARG, "solve_async with EPS termination needs ITER|EPS with a sweep budget and the strip / fold kernel "
                                     "(ITER-only termination works with every kernel)");
    // With ITER the sweep budget is max_iter (a budget <= 0 with EPS never triggers ITER);
    // EPS-only runs use chunks until Eps < epsilon.
    const long long budget = (use_iter && p.max_iter > 0) ? p.max_iter : (1LL << 40);

    int T = 1;
    JPlan plan, tail;
    hsflow_params eff = p;
    // ITER|EPS with a sweep budget on a kernel with a witness mode
    const bool spec = use_eps && use_iter && p.max_iter > 0 && (kernel == HSFLOW_KERNEL_STRIP || kernel == HSFLOW_KERNEL_FOLD);
    // It runs witness launches, which watch an edge row of each strip: a plan whose core tile is thinner
    // than a strip may have no wavefront with a core row there (thin frames, very short launches); another shape
    // then takes its place as far as the caller left rows / wavefronts open (make_witness_jplan).
    auto plan_sweeps = [&](int sweeps, JPlan &out) {
        if (!make_jplan(c, kernel, sweeps, p, out)) return false;
        JPlan alt;
        if (spec && !strip_has_witness(out) && make_witness_jplan(c, kernel, sweeps, p, alt)) out = alt;
        return true;
    };
    if (multi) {
        const int horizon = budget > (1 << 30) ? 64 : (int)budget; // EPS-only runs: plan for chunks
        if (p.fuse_steps > 0) T = std::min(p.fuse_steps, kMaxFuse);
        else if (kernel == HSFLOW_KERNEL_STRIP || kernel == HSFLOW_KERNEL_FOLD)
            T = (use_eps && !(use_iter && p.max_iter > 0)) ? std::min(8, horizon)
                                                          : pick_strip_T(c, horizon, p, kernel == HSFLOW_KERNEL_FOLD);
        else T = pick_T(horizon, 0);
        if (budget < T) T = (int)budget;
        // The strip kernels carry 4^k * u inside a launch (hs_kernels_strip.hip.h).  The largest flow and
        // constant term a pixel can have grow like sqrt(lambda); beyond lambda = 1e20 keep the launches
        // short so that 4^(T+1) times those stays far inside the float range.  That bounds what the solver itself
        // produces from zero flow, up to kMaxFuse sweeps per launch; it says nothing about flow a caller wrote or an
        // earlier solve with a larger lambda left: a warm solve on such planes measures them and hands down the most
        // sweeps a launch may have (c->t_cap, flow_launch_cap).
        if ((kernel == HSFLOW_KERNEL_STRIP || kernel == HSFLOW_KERNEL_FOLD) && coeff < 1e-20f) T = std::min(T, 8);
        if ((kernel == HSFLOW_KERNEL_STRIP || kernel == HSFLOW_KERNEL_FOLD) && c->t_cap > 0) T = std::min(T, c->t_cap);
        if (!plan_sweeps(T, plan))
            return fail(c, HSFLOW_E_SIZE, "no feasible launch plan for the requested tile/threads/rows/fuse_steps");
        // the short last launch of a real sweep budget: planned here, once per parameter set like the full launch
        if (use_iter && p.max_iter > 0 && budget % T && !plan_sweeps((int)(budget % T), tail))
            return fail(c, HSFLOW_E_SIZE, "no feasible launch plan for the tail launch");
        plan_to_info(c, plan);
    } else {
        c->info.fuse_steps = 1; c->info.tile_w = c->info.tile_h = 0; c->info.threads = 256;
        c->info.groups_per_thread = 1; c->info.tiles = 0; c->info.lds_bytes = 0;
    }
    c->info.kernel = kernel;
    bool persist = false;
    // AUTO keeps the launch per fuse_steps: measured on MI355X at 1080p / 100 the persistent launch spends as long at a
    // phase boundary (write-through publish 2.6 us + counters 3.2 us + halo reload 4 us) as the stream does at a kernel
    // boundary -- ITER 0.148 against 0.149 ms, ITER|EPS slower -- so it runs on request only
    // (HSFLOW_PERSIST_AUTO=1 lets AUTO take it, for experiments).
    static const bool persist_auto = getenv("HSFLOW_PERSIST_AUTO") != nullptr;
    if (persist_asked || (persist_auto && p.kernel == HSFLOW_KERNEL_AUTO && kernel == HSFLOW_KERNEL_STRIP)) {
        const char *why = !(use_iter && p.max_iter > 0 && budget <= (1 << 16)) ? "needs a sweep budget (ITER)"
                                                                               : persist_obstacle(c, plan.s, (int)budget, p, async, use_eps);
        if (!why && use_eps && !strip_has_witness(plan)) why = "this launch plan cannot run witness phases";
        if (!why && use_eps && stops_per_pair(c)) why = "every pair of the batch stops on its own"; // (solve_impl_inner says more when it was asked for)
        if (!why) persist = true;
        else if (persist_asked) return fail(c, HSFLOW_E_SIZE, std::string("HSFLOW_KERNEL_PERSIST: ") + why);
    }
    c->info.persistent = persist ? (int)((budget + T - 1) / T) : 0;
    // The budget runs as witness launches where plan and tail can (a tail of one sweep is measured, not witnessed: the
    // synchronous pass's WitnessLast; an asynchronous pass needs it able; persist: the tail phase keeps the plan's geometry)
    const bool witness = spec && !c->force_exact && strip_has_witness(plan) &&
                         !(tail.T && !persist && (async || tail.T > 1) && !strip_has_witness(tail));
    if (async && use_eps && !witness)
        return fail(c, HSFLOW_E_ARG, "solve_async with ITER|EPS: this launch plan (core tile thinner than a strip) cannot run witness launches; "
                                     "use hsflow_solve or other tuning parameters");
    S = SolveSetup{coeff, kernel, multi, use_iter, use_eps, budget, T, plan, tail, witness, persist, eff};
    return HSFLOW_OK;
}

int solve_impl_inner(hsflow_ctx *c, const hsflow_params *pp, bool async, bool *took_over);

// ---- tame planes: warm starts from flow the solver did not make ------------------------------------------------------
// The largest finite |value| of the flow planes, every pair (NaN and Inf do not count: no scale changes them or what
// they do to their neighbours).  One small launch, one word back, and the host waits for it: only on contexts whose
// planes are not tame (hsflow_ctx::flow_tame).
int measure_flow_absmax(hsflow_ctx *c, float &m)
{
    if (!c->dFlowMax) HS_HIP(c, hipMalloc((void **)&c->dFlowMax, sizeof(unsigned)));
    if (!c->hFlowMax) HS_HIP(c, hipHostMalloc((void **)&c->hFlowMax, sizeof(unsigned), hipHostMallocDefault));
    HS_HIP(c, hipMemsetAsync(c->dFlowMax, 0, sizeof(unsigned), c->stream));
    const long long rows = (long long)c->N * c->H;
    hipLaunchKernelGGL(hsk::k_flow_absmax, dim3((c->W + 255) / 256, (unsigned)std::min<long long>(rows, 256)), dim3(256), 0, c->stream,
                       c->dU[c->cur], c->dV[c->cur], c->W, rows, c->P, c->dFlowMax);
    HS_HIP(c, hipGetLastError());
    HS_HIP(c, hipMemcpyAsync(c->hFlowMax, c->dFlowMax, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HS_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(&m, c->hFlowMax, sizeof(m));
    return HSFLOW_OK;
}

// The most sweeps a strip / fold launch may have on planes whose largest |value| is m (0: not even one).
// With N_k the largest Euclidean length of a pixel's (u, v) after k sweeps: the neighbour average does not lengthen it,
// the update takes away part of its component along (Ix, Iy) and adds a constant no longer than |ga| <= 255 / sqrt(Ilambda)
// (sweep_coefs: |It| <= 255, s <= 1 / sqrt(Ilambda)), so N_k <= sqrt(2) m + k g.  After k sweeps of a launch the kernel
// holds 4^k * flow, and the largest numbers sweep k + 1 forms are the neighbour sum 4^(k+1) * average, the inner product q
// of update_cv, at most 4^(k+1) * (N_k + g) as |al|, |be| <= 1, and sweep_diff's 4 * old - new, at most 2 * 4^(k+1) * N:
// all below 4^(k+1) * 2 * (sqrt(2) m + (k + 1) g) < 4^(T+1) * 4 * (m + n g) / sqrt(2) over a launch of T sweeps in a solve
// of n.  So 4^(T+1) * (m + n g) < FLT_MAX / 4 keeps every one of them finite with a factor sqrt(2) to spare for rounding.
// (n: the sweep budget, at most 2^20 -- an EPS-only solve that long has its flow at a fixed point, not growing.)
int flow_launch_cap(float m, float coeff, long long budget)
{
    if (!(m < INFINITY)) return 0;
    const double g = 255.0 / std::sqrt((double)coeff);
    const double bound = (double)m + (double)std::min<long long>(budget, 1LL << 20) * g;
    int T = 0;
    while (T < kMaxFuse && std::ldexp(bound, 2 * (T + 2)) < (double)FLT_MAX / 4) T++;
    return T;
}

int solve_impl(hsflow_ctx *c, const hsflow_params *pp, bool async)
{
    // A solve that takes an owed early-stop check over (below) drops it first; should it then fail before it has
    // registered its own, the owed check comes back -- the flow of the earlier solve is still unverified.
    const hsflow_ctx::Pending owed = c ? c->pend : hsflow_ctx::Pending();
    bool took_over = false;
    const int st = solve_impl_inner(c, pp, async, &took_over);
    if (st && took_over && !c->pend.active) c->pend = owed;
    if (c) c->last_marked = false;
    if (!st && async && c->async_reduce && c->hMark) { // a marker behind everything this solve enqueued (hsflow_wait_solve, settle_pending)
        const bool by_reduce = c->pend.active && c->pend.marked_by_reduce; // (the reduction kernel of an ITER|EPS solve wrote it)
        if (!by_reduce) hipLaunchKernelGGL(hsk::k_mark_done, dim3(1), dim3(64), 0, c->stream, c->dSeq, c->hMarkDev);
        if (by_reduce || hipGetLastError() == hipSuccess) {
            c->mark_issued++;
            c->last_marked = true;
            c->flow_after_mark = false; // (the new marker is behind whatever was enqueued before this solve)
            if (c->pend.active) c->pend.mark = c->mark_issued;
        } else if (c->pend.active) c->pend.reduced = false; // (no marker: the owed check is settled the slow way)
    }
    return st;
}

int solve_impl_inner(hsflow_ctx *c, const hsflow_params *pp, bool async, bool *took_over)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    // An unverified asynchronous solve comes first -- unless this call repeats it exactly: while a check is owed
    // the inputs cannot have changed (every entry point that changes frames or flow settles first), so an
    // asynchronous solve with bit-identical parameters that starts from zero flow recomputes the very same
    // result and leaves the very same witness words; the owed check simply passes on to it and the host does
    // not wait for the stream (a caller that streams solves never pays a round trip per solve).
    const bool repeat = c->pend.active && async && !c->force_exact && pp && pp->struct_size == sizeof(hsflow_params) &&
                        !pp->use_previous && std::memcmp(pp, &c->pend.params, sizeof(hsflow_params)) == 0;
    if (repeat) { c->pend.active = false; *took_over = true; }
    else if ((st = settle_pending(c))) return st;
    c->lastl.valid = false;
    c->pair_res_valid = false;
    c->sweeps_run = 0;
    if (!pp || pp->struct_size != sizeof(hsflow_params))
        return fail(c, HSFLOW_E_ARG, "params null or struct_size mismatch");
    bool measured_small = false; // the planes were measured and hold nothing the solver could not have made itself
    hsflow_params tamed; // (this call's parameters with the one-sweep kernel in place of the caller's, where no strip launch fits)
    if (!c->frames_set) return fail(c, HSFLOW_E_STATE, "frames were not set");
    if (pp->mode == HSFLOW_MODE_CLASSIC || pp->mode == HSFLOW_MODE_CLASSIC_AS_SHIPPED) {
        if ((st = resolve_lazy_frames(c, false))) return st; // (the classic kernels read the context's planes)
        c->flow_tame = false; // (its flow is bounded by nothing the CV planner knows)
        return solve_classic(c, *pp, async);
    }
    // Tame planes.  A cold solve, and a warm one on tame planes, pass through here without a launch or a wait.
    c->t_cap = 0;
    if (pp->mode == HSFLOW_MODE_CV && pp->lambda > 0.f) { // (anything else is refused below)
        const float coeff = std::max(1.0f / pp->lambda, FLT_MIN);
        const bool strip_like = pp->kernel == HSFLOW_KERNEL_AUTO || pp->kernel == HSFLOW_KERNEL_STRIP || pp->kernel == HSFLOW_KERNEL_FOLD ||
                                pp->kernel == HSFLOW_KERNEL_PERSIST;
        if (pp->use_previous && !c->flow_tame && strip_like) {
            float m = 0.f;
            if ((st = measure_flow_absmax(c, m))) return st;
            // Tame planes reach 65536 sweeps x 2.6e12 (the constant term at lambda = 1e20), about 1.7e17: planes with nothing
            // finite above 1e15 are as good as the solver's own, and count as tame again once this solve is accepted
            measured_small = m <= 1e15f;
            const bool budgeted = (pp->term_type & HSFLOW_TERM_ITER) && pp->max_iter > 0;
            c->t_cap = flow_launch_cap(m, coeff, budgeted ? pp->max_iter : (1LL << 40));
            if (c->t_cap == 0) { // not one sweep of scaled state fits: the one-sweep kernel, which keeps the canonical scale;
                tamed = *pp;     // complete when the call returns, also where it was asked for asynchronously
                tamed.kernel = HSFLOW_KERNEL_SIMPLE;
                tamed.fuse_steps = tamed.tile_w = tamed.tile_h = tamed.threads = tamed.strip_rows = 0;
                pp = &tamed;
                if (pp->term_type & HSFLOW_TERM_EPS) async = false;
            }
        }
    }
    const hsflow_params &p = *pp;
    if (p.mode != HSFLOW_MODE_CV) return fail(c, HSFLOW_E_ARG, "unknown mode");
    if (stops_per_pair(c) && (p.term_type & HSFLOW_TERM_EPS) && p.kernel == HSFLOW_KERNEL_PERSIST)
        return fail(c, HSFLOW_E_ARG, "HSFLOW_KERNEL_PERSIST with hsflow_set_pair_termination on a batch under EPS termination: the persistent "
                                     "launch holds every pair of the batch until its last phase, so no pair can stop on its own; "
                                     "use HSFLOW_KERNEL_STRIP, or switch the per-pair stop off");
    c->info.eps_rerun = 0;
    c->info.deriv_fused = 0;
    // The plan of a solve depends on the parameters, not on the frames: a stream of solves with the same parameters plans
    // once (the planner tries every sweep count x rows x wavefronts: tens of microseconds of host time per solve, which is
    // what bounded a stream of small frames).  Not cached: a persistent launch (it depends on who else is alive).
    SolveSetup S;
    PlanKey key;
    std::memset(&key, 0, sizeof(key)); // (compared bytewise: padding too)
    key.p = p;
    key.p.use_previous = key.p.reuse_derivatives = key.p.use_graph = key.p.profile = 0; // (do not enter the plan)
    key.async = async ? 1 : 0;
    key.exact = c->force_exact ? 1 : 0;
    key.t_cap = c->t_cap;
    const bool cacheable = p.kernel != HSFLOW_KERNEL_PERSIST && !getenv("HSFLOW_PERSIST_AUTO");
    const PlanEntry *hit = nullptr;
    if (cacheable)
        for (const PlanEntry &e : c->plan_cache)
            if (std::memcmp(&e.key, &key, sizeof(key)) == 0) { hit = &e; break; }
    if (hit) {
        if ((st = check_solve_args(c, p, async))) return st;
        S = hit->S;
        S.eff = p; // (the cached copy carries the first caller's use_previous / reuse_derivatives / use_graph)
        hsflow_info &i = c->info;
        const hsflow_info &j = hit->info;
        i.kernel = j.kernel; i.fuse_steps = j.fuse_steps; i.tile_w = j.tile_w; i.tile_h = j.tile_h; i.threads = j.threads;
        i.groups_per_thread = j.groups_per_thread; i.tiles = j.tiles; i.lds_bytes = j.lds_bytes; i.persistent = j.persistent;
    } else {
        if ((st = prepare_solve(c, p, async, S))) return st;
        if (cacheable) {
            if (c->plan_cache.size() >= 16) c->plan_cache.erase(c->plan_cache.begin());
            c->plan_cache.push_back(PlanEntry{key, S, c->info});
        }
    }
    // (the solve is accepted: from here on the planes are what it makes of them)
    if (!p.use_previous) c->flow_tame = S.coeff >= 1e-20f;
    else if (S.coeff < 1e-20f) c->flow_tame = false;
    else if (measured_small) c->flow_tame = true;
    c->info.deriv_ms = c->info.jacobi_ms = c->info.solve_ms = 0.f;
    c->info.last_eps = 0.f;
    Profiler prof{c, p.profile != 0};
    if (!S.use_eps) return solve_fixed(c, S, prof, async);
    // A threshold that S.T sweeps of scaling would carry out of the float range (epsilon from about 2^(127 - 2 T) up), or
    // a NaN: the witness launches could prove nothing, or worse (hs_stop_rule.h).  No witness pass then: every sweep is
    // measured, launch by launch, and the solve is complete when the call returns, also where it was asked for
    // asynchronously -- nothing stays owed.  (S.T is the longest launch of the pass: a tail is shorter.)
    if (S.witness && !witness_usable(p.epsilon, S.T)) {
        S.witness = S.persist = false;
        c->info.persistent = 0;
        async = false;
    }
    constexpr long long kSpecMax = 1 << 16; // speculative ITER|EPS: the whole budget in one go
    if (S.use_iter && p.max_iter > 0 && S.budget <= kSpecMax) return solve_iter_eps(c, S, prof, async);
    if (stops_per_pair(c)) // (no budget to speculate on: every pair through its own chunk loop, stall rule included)
        return solve_pairs_all(c, S);
    if ((st = resolve_lazy_frames(c, false))) return st;
    return solve_eps_chunks(c, S, prof);
}

} // namespace
