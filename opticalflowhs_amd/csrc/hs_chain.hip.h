// hs_chain.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_chain_flow* and
// hsflow_track_points*, pixels and points followed through the flows of up to HSFLOW_CHAIN_MAX_PAIRS pairs where the
// solver left them (hs_chain_rule.h).  Per call: one launch (hs_kernels_chain.hip.h), with statistics one memset of the
// record in front of it.  On top of hs_postops.hip.h: its three ordering rules hold word for word.  A context that never
// chains allocates and launches nothing here.
#pragma once

namespace {

static_assert(sizeof(hsflow_chain_stats) == 64 && sizeof(hsflow_chain_stats) == sizeof(hsk::ChainStatsWords) && sizeof(hsflow_chain_stats) == kStatsBytes,
              "hsflow_chain_stats is 64 bytes on both sides");
static_assert(offsetof(hsflow_chain_stats, sum_age) == 32 && offsetof(hsflow_chain_stats, max_mag2_bits) == 40, "hsflow_chain_stats: the kernel's layout");
static_assert(sizeof(hsflow_chain_params) == 16, "hsflow_chain_params is 16 bytes");
static_assert(HSFLOW_CHAIN_MAX_PAIRS == hschain::kMaxPairs, "the header's constant is the rule's");
static_assert(HSFLOW_CHAIN_ALIVE == hschain::kAlive && HSFLOW_CHAIN_LEFT == hschain::kLeft && HSFLOW_CHAIN_UNTRUSTED == hschain::kUntrusted &&
                  HSFLOW_CHAIN_UNKNOWN == hschain::kUnknown,
              "the header's classes are the rule's");

// The inputs of a chain that a caller names plane by plane (host or device memory alike).
struct ChainIn {
    int n;
    const void *const *u, *const *v; // n each
    size_t fs;
    const void *const *s; // n, or NULL; a NULL entry: no test for that plane
    size_t ss;
    const void *U0, *V0; // both or neither
    size_t s0s;
};

// The outputs of a dense chain.
struct ChainOut {
    void *U, *V;
    size_t os;
    void *status;
    size_t sts;
    void *age;
    size_t as;
    const void *stats;
};

int check_chain_params(hsflow_ctx *c, const hsflow_chain_params *cp)
{
    if (!cp || cp->struct_size != sizeof(hsflow_chain_params)) return fail(c, HSFLOW_E_ARG, "chain params null or struct_size mismatch");
    return HSFLOW_OK;
}

int check_chain_n(hsflow_ctx *c, int n)
{
    if (n < 1 || n > HSFLOW_CHAIN_MAX_PAIRS) return fail(c, HSFLOW_E_ARG, "a chain takes 1 .. " + std::to_string(HSFLOW_CHAIN_MAX_PAIRS) + " planes");
    return HSFLOW_OK;
}

int check_chain_pairs(hsflow_ctx *c, const int *pairs, int n)
{
    const int st = check_chain_n(c, n);
    if (st) return st;
    if (!pairs) return fail(c, HSFLOW_E_ARG, "null pair list");
    for (int k = 0; k < n; k++)
        if (pairs[k] < 0 || pairs[k] >= c->N) return fail(c, HSFLOW_E_ARG, "plane " + std::to_string(k) + ": pair index out of range");
    return HSFLOW_OK;
}

// The state list alone (the forms on a context's own flows take nothing else of ChainIn).
int check_chain_state(hsflow_ctx *c, int n, const void *const *s, size_t ss, int W)
{
    if (!s) return HSFLOW_OK;
    for (int k = 0; k < n; k++)
        if (s[k] && ss < (size_t)W) return fail(c, HSFLOW_E_SIZE, "state stride smaller than width");
    return HSFLOW_OK;
}

int check_chain_start(hsflow_ctx *c, const void *U0, const void *V0, size_t s0s, int W)
{
    if ((U0 != nullptr) != (V0 != nullptr)) return fail(c, HSFLOW_E_ARG, "the two start planes are given together or not at all");
    if (!U0) return HSFLOW_OK;
    if ((((uintptr_t)U0 | (uintptr_t)V0) & 3u) != 0) return fail(c, HSFLOW_E_ARG, "the start planes must be 4-byte aligned");
    if (s0s < (size_t)W * 4 || (s0s & 3u)) return fail(c, HSFLOW_E_SIZE, "start stride smaller than 4*width or no multiple of 4");
    return HSFLOW_OK;
}

// The planes a caller names: the lists, their entries, the strides.
int check_chain_in(hsflow_ctx *c, const ChainIn &in, int W)
{
    int st = check_chain_n(c, in.n);
    if (st) return st;
    if (!in.u || !in.v) return fail(c, HSFLOW_E_ARG, "null flow plane list");
    for (int k = 0; k < in.n; k++) {
        if (!in.u[k] || !in.v[k]) return fail(c, HSFLOW_E_ARG, "plane " + std::to_string(k) + ": null flow plane");
        if ((((uintptr_t)in.u[k] | (uintptr_t)in.v[k]) & 3u) != 0) return fail(c, HSFLOW_E_ARG, "plane " + std::to_string(k) + ": the flow planes must be 4-byte aligned");
    }
    if (in.fs < (size_t)W * 4 || (in.fs & 3u)) return fail(c, HSFLOW_E_SIZE, "flow stride smaller than 4*width or no multiple of 4");
    if ((st = check_chain_state(c, in.n, in.s, in.ss, W))) return st;
    return check_chain_start(c, in.U0, in.V0, in.s0s, W);
}

int check_chain_out(hsflow_ctx *c, const ChainOut &o, int W)
{
    if ((o.U != nullptr) != (o.V != nullptr)) return fail(c, HSFLOW_E_ARG, "the two flow outputs are asked for together or not at all");
    if (!o.U && !o.status && !o.age && !o.stats) return fail(c, HSFLOW_E_ARG, "neither the flow nor the status nor the age nor statistics asked for");
    if (o.U && (((uintptr_t)o.U | (uintptr_t)o.V) & 3u) != 0) return fail(c, HSFLOW_E_ARG, "the output flow planes must be 4-byte aligned");
    if (o.U && (o.os < (size_t)W * 4 || (o.os & 3u))) return fail(c, HSFLOW_E_SIZE, "output flow stride smaller than 4*width or no multiple of 4");
    if (o.status && o.sts < (size_t)W) return fail(c, HSFLOW_E_SIZE, "status stride smaller than width");
    if (o.age && o.as < (size_t)W) return fail(c, HSFLOW_E_SIZE, "age stride smaller than width");
    return HSFLOW_OK;
}

using ChainSpans = std::vector<MedSpan>; // (hs_median.hip.h: the bytes a plane covers)

void chain_out_spans(const ChainOut &o, int W, int H, ChainSpans *out)
{
    out->push_back(med_span(o.U, o.os, (size_t)W * 4, H));
    out->push_back(med_span(o.V, o.os, (size_t)W * 4, H));
    out->push_back(med_span(o.status, o.sts, (size_t)W, H));
    out->push_back(med_span(o.age, o.as, (size_t)W, H));
    out->push_back(med_span(o.stats, 0, kStatsBytes, 1));
}

void chain_state_spans(int n, const void *const *s, size_t ss, int W, int H, ChainSpans *in)
{
    for (int k = 0; s && k < n; k++) in->push_back(med_span(s[k], ss, (size_t)W, H));
}

void chain_in_spans(const ChainIn &i, int W, int H, ChainSpans *in)
{
    for (int k = 0; k < i.n; k++) {
        in->push_back(med_span(i.u[k], i.fs, (size_t)W * 4, H));
        in->push_back(med_span(i.v[k], i.fs, (size_t)W * 4, H));
    }
    chain_state_spans(i.n, i.s, i.ss, W, H, in);
    in->push_back(med_span(i.U0, i.s0s, (size_t)W * 4, H));
    in->push_back(med_span(i.V0, i.s0s, (size_t)W * 4, H));
}

// The flows of the context's pairs in both buffers of the ping-pong (which one holds the flow is known behind
// settle_pending only).
void chain_ctx_spans(hsflow_ctx *c, const int *pairs, int n, ChainSpans *in)
{
    for (int k = 0; k < n; k++)
        for (int b = 0; b < 2; b++) {
            in->push_back(med_span(c->dU[b] + (long long)pairs[k] * c->plane, (size_t)c->P * 4, (size_t)c->W * 4, c->H));
            in->push_back(med_span(c->dV[b] + (long long)pairs[k] * c->plane, (size_t)c->P * 4, (size_t)c->W * 4, c->H));
        }
}

int check_chain_overlap(hsflow_ctx *c, const ChainSpans &in, const ChainSpans &out)
{
    for (const MedSpan &o : out)
        for (const MedSpan &i : in)
            if (med_overlap(o, i)) return fail(c, HSFLOW_E_ARG, "an output of the chain may not overlap an input");
    return HSFLOW_OK;
}

unsigned chain_values(const hsflow_chain_params &cp)
{
    return (unsigned)cp.value[0] | (unsigned)cp.value[1] << 8 | (unsigned)cp.value[2] << 16 | (unsigned)cp.value[3] << 24;
}

int chain_wide(const void *p, const void *q, size_t stride, unsigned mask) { return (((uintptr_t)p | (uintptr_t)q | stride) & mask) == 0; }

void chain_stats_out(hsflow_chain_stats *stats, const hschain::Sums &sums)
{
    std::memset(stats, 0, sizeof(*stats));
    for (int k = 0; k < 4; k++) stats->cls[k] = sums.cls[k];
    stats->sum_age = sums.sum_age;
    stats->max_mag2_bits = sums.max_bits;
}

// What the last check of a device form does before c->cur is named: the record's alignment, then the owed ITER|EPS check
// (hs_postops.hip.h, rule 1).
int chain_device_begin(hsflow_ctx *c, const void *d_stats)
{
    if (((uintptr_t)d_stats & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the statistics record must be 8-byte aligned");
    return settle_pending(c);
}

// The planes of the context's pairs (behind settle_pending).
void chain_ctx_planes(hsflow_ctx *c, const int *pairs, int n, const void *const *s, hsk::ChainPlanes *pl)
{
    const float *U = c->dU[c->cur], *V = c->dV[c->cur];
    for (int k = 0; k < n; k++) {
        pl->u[k] = U + (long long)pairs[k] * c->plane;
        pl->v[k] = V + (long long)pairs[k] * c->plane;
        pl->s[k] = s ? (const uint8_t *)s[k] : nullptr;
    }
}

void chain_list_planes(const ChainIn &in, hsk::ChainPlanes *pl)
{
    for (int k = 0; k < in.n; k++) {
        pl->u[k] = (const float *)in.u[k];
        pl->v[k] = (const float *)in.v[k];
        pl->s[k] = in.s ? (const uint8_t *)in.s[k] : nullptr;
    }
}

// The launch of a dense chain.  All pointers are device memory; the caller has checked every argument.
int enqueue_chain_dense(hsflow_ctx *c, const hsk::ChainPlanes &pl, int n, size_t fs, size_t ss, const void *U0, const void *V0, size_t s0s,
                        const hsflow_chain_params &cp, const ChainOut &o, void *d_stats)
{
    hsk::ChainDense d{};
    d.U0 = (const float *)U0; d.V0 = (const float *)V0;
    d.U = (float *)o.U; d.V = (float *)o.V;
    d.status = (uint8_t *)o.status; d.age = (uint8_t *)o.age;
    d.fs = (long long)fs; d.ss = (long long)ss; d.s0s = (long long)s0s; d.os = (long long)o.os; d.sts = (long long)o.sts; d.as = (long long)o.as;
    d.n = n; d.W = c->W; d.H = c->H;
    d.value = chain_values(cp);
    if (U0 ? chain_wide(U0, V0, s0s, 15u) : chain_wide(pl.u[0], pl.v[0], fs, 15u)) d.wide |= hsk::kChainWideStart;
    if (o.U && chain_wide(o.U, o.V, o.os, 15u)) d.wide |= hsk::kChainWideOut;
    if (o.status && word_aligned(o.status, o.sts)) d.wide |= hsk::kChainWideStatus;
    if (o.age && word_aligned(o.age, o.as)) d.wide |= hsk::kChainWideAge;
    dim3 grid;
    const int st = stats_grid(c, (c->W + 1023) / 1024, c->H, 1, d_stats, &grid);
    if (st) return st;
    HS_HIP(c, hsk::launch_chain_dense(grid, c->stream, pl, d, (hsk::ChainStatsWords *)d_stats));
    c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
    return HSFLOW_OK;
}

// The launch for m points.
int enqueue_chain_points(hsflow_ctx *c, const hsk::ChainPlanes &pl, int n, size_t fs, size_t ss, const hsflow_chain_params &cp, const float *xy, int m,
                         float *track, float *last, uint8_t *status, uint8_t *age, void *d_stats)
{
    hsk::ChainPoints d{};
    d.xy = xy; d.track = track; d.last = last; d.status = status; d.age = age;
    d.fs = (long long)fs; d.ss = (long long)ss;
    d.n = n; d.m = m; d.W = c->W; d.H = c->H;
    d.value = chain_values(cp);
    d.wide = (((uintptr_t)xy & 7u) == 0 ? 1u : 0u) | (track && ((uintptr_t)track & 7u) == 0 ? 2u : 0u) | (last && ((uintptr_t)last & 7u) == 0 ? 4u : 0u);
    if (d_stats) HS_HIP(c, hipMemsetAsync(d_stats, 0, kStatsBytes, c->stream));
    HS_HIP(c, hsk::launch_chain_points(dim3((unsigned)((m + 255) / 256)), c->stream, pl, d, (hsk::ChainStatsWords *)d_stats));
    c->last_marked = false; // (rule 2)
    return HSFLOW_OK;
}

int check_chain_points(hsflow_ctx *c, const float *xy, int m, const void *track, const void *last, const void *status, const void *age, const void *stats)
{
    if (m < 1 || m > hschain::kMaxPoints) return fail(c, HSFLOW_E_ARG, "a call takes 1 .. 2^24 points");
    if (!xy) return fail(c, HSFLOW_E_ARG, "null point list");
    if ((((uintptr_t)xy | (uintptr_t)track | (uintptr_t)last) & 3u) != 0) return fail(c, HSFLOW_E_ARG, "the points, the track and the last positions must be 4-byte aligned");
    if (!track && !last && !status && !age && !stats) return fail(c, HSFLOW_E_ARG, "neither the track nor the last positions nor status nor age nor statistics asked for");
    return HSFLOW_OK;
}

void chain_points_spans(int n, const float *xy, int m, const void *track, const void *last, const void *status, const void *age, const void *stats,
                        ChainSpans *in, ChainSpans *out)
{
    in->push_back(med_span(xy, 0, (size_t)m * 8, 1));
    out->push_back(med_span(track, 0, (size_t)(n + 1) * (size_t)m * 8, 1));
    out->push_back(med_span(last, 0, (size_t)m * 8, 1));
    out->push_back(med_span(status, 0, (size_t)m, 1));
    out->push_back(med_span(age, 0, (size_t)m, 1));
    out->push_back(med_span(stats, 0, kStatsBytes, 1));
}

// The state planes of a synchronous form into the staging (slot 0, packed: rows W bytes, planes W * H bytes apart), the
// device pointers into dev[].  The caller has reserved the slot.
int chain_upload_state(hsflow_ctx *c, int n, const uint8_t *const *state, size_t ss, const void **dev)
{
    const size_t brow = (size_t)c->W, bplane = brow * c->H;
    for (int k = 0; k < n; k++) {
        dev[k] = nullptr;
        if (!state || !state[k]) continue;
        uint8_t *p = c->chain.stage[0] + (size_t)k * bplane;
        HS_HIP(c, copy_rows_async(c, p, brow, state[k], ss, brow, c->H, hipMemcpyHostToDevice));
        dev[k] = p;
    }
    return HSFLOW_OK;
}

bool chain_any(int n, const uint8_t *const *state)
{
    for (int k = 0; state && k < n; k++)
        if (state[k]) return true;
    return false;
}

int chain_stage(hsflow_ctx *c, int slot, size_t bytes) { return stage_reserve(c, &c->chain.stage[slot], &c->chain.stage_bytes[slot], bytes); }

void chain_release(hsflow_ctx *c)
{
    for (uint8_t *p : c->chain.stage) hipFree(p);
    stats_release(c->chain.dStats, c->chain.hStats);
    c->chain = hsflow_ctx::ChainScratch();
}

} // namespace

extern "C" {

void hsflow_default_chain_params(hsflow_chain_params *cp)
{
    if (!cp) return;
    std::memset(cp, 0, sizeof(*cp));
    cp->struct_size = sizeof(*cp);
    cp->value[0] = 255;
}

int hsflow_chain_flow_host(int n, const float *const *u, const float *const *v, size_t flow_stride, const uint8_t *const *state, size_t state_stride, int width,
                           int height, const float *U0, const float *V0, size_t start_stride, const hsflow_chain_params *cp, float *U, float *V,
                           size_t out_stride, uint8_t *status, size_t status_stride, uint8_t *age, size_t age_stride, hsflow_chain_stats *stats)
{
    int st = check_chain_params(nullptr, cp);
    if (st) return st;
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_chain_flow_host: width and height must be positive");
    const ChainIn in = {n, (const void *const *)u, (const void *const *)v, flow_stride, (const void *const *)state, state_stride, U0, V0, start_stride};
    const ChainOut out = {U, V, out_stride, status, status_stride, age, age_stride, stats};
    if ((st = check_chain_in(nullptr, in, width))) return st;
    if ((st = check_chain_out(nullptr, out, width))) return st;
    ChainSpans is, os;
    chain_in_spans(in, width, height, &is);
    chain_out_spans(out, width, height, &os);
    if ((st = check_chain_overlap(nullptr, is, os))) return st;
    hschain::Plane planes[hschain::kMaxPairs];
    for (int k = 0; k < n; k++) planes[k] = hschain::Plane{u[k], v[k], state ? state[k] : nullptr, (long long)flow_stride, (long long)state_stride};
    hschain::Sums sums;
    hschain::chain_rows(planes, n, width, height, U0, V0, start_stride, cp->value, U, V, out_stride, status, status_stride, age, age_stride, &sums);
    if (stats) chain_stats_out(stats, sums);
    return HSFLOW_OK;
}

int hsflow_track_points_host(int n, const float *const *u, const float *const *v, size_t flow_stride, const uint8_t *const *state, size_t state_stride, int width,
                             int height, const hsflow_chain_params *cp, const float *xy, int m, float *track, float *last, uint8_t *status, uint8_t *age,
                             hsflow_chain_stats *stats)
{
    int st = check_chain_params(nullptr, cp);
    if (st) return st;
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_track_points_host: width and height must be positive");
    const ChainIn in = {n, (const void *const *)u, (const void *const *)v, flow_stride, (const void *const *)state, state_stride, nullptr, nullptr, 0};
    if ((st = check_chain_in(nullptr, in, width))) return st;
    if ((st = check_chain_points(nullptr, xy, m, track, last, status, age, stats))) return st;
    ChainSpans is, os;
    chain_in_spans(in, width, height, &is);
    chain_points_spans(n, xy, m, track, last, status, age, stats, &is, &os);
    if ((st = check_chain_overlap(nullptr, is, os))) return st;
    hschain::Plane planes[hschain::kMaxPairs];
    for (int k = 0; k < n; k++) planes[k] = hschain::Plane{u[k], v[k], state ? state[k] : nullptr, (long long)flow_stride, (long long)state_stride};
    hschain::Sums sums;
    hschain::track_rows(planes, n, width, height, xy, m, cp->value, track, last, status, age, &sums);
    if (stats) chain_stats_out(stats, sums);
    return HSFLOW_OK;
}

int hsflow_chain_planes_device(hsflow_ctx *c, int n, const void *const *d_u, const void *const *d_v, size_t flow_stride, const void *const *d_state,
                               size_t state_stride, const void *d_U0, const void *d_V0, size_t start_stride, const hsflow_chain_params *cp, void *d_U, void *d_V,
                               size_t out_stride, void *d_status, size_t status_stride, void *d_age, size_t age_stride, hsflow_chain_stats *d_stats)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_chain_params(c, cp))) return st;
    const ChainIn in = {n, d_u, d_v, flow_stride, d_state, state_stride, d_U0, d_V0, start_stride};
    const ChainOut out = {d_U, d_V, out_stride, d_status, status_stride, d_age, age_stride, d_stats};
    if ((st = check_chain_in(c, in, c->W))) return st;
    if ((st = check_chain_out(c, out, c->W))) return st;
    ChainSpans is, os;
    chain_in_spans(in, c->W, c->H, &is);
    chain_out_spans(out, c->W, c->H, &os);
    if ((st = check_chain_overlap(c, is, os))) return st;
    if ((st = chain_device_begin(c, d_stats))) return st;
    hsk::ChainPlanes pl{};
    chain_list_planes(in, &pl);
    return enqueue_chain_dense(c, pl, n, flow_stride, state_stride, d_U0, d_V0, start_stride, *cp, out, d_stats);
}

int hsflow_chain_flow_device(hsflow_ctx *c, const int *pairs, int n, const void *const *d_state, size_t state_stride, const void *d_U0, const void *d_V0,
                             size_t start_stride, const hsflow_chain_params *cp, void *d_U, void *d_V, size_t out_stride, void *d_status, size_t status_stride,
                             void *d_age, size_t age_stride, hsflow_chain_stats *d_stats)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_chain_params(c, cp))) return st;
    if ((st = check_chain_pairs(c, pairs, n))) return st;
    if ((st = check_chain_state(c, n, d_state, state_stride, c->W))) return st;
    if ((st = check_chain_start(c, d_U0, d_V0, start_stride, c->W))) return st;
    const ChainOut out = {d_U, d_V, out_stride, d_status, status_stride, d_age, age_stride, d_stats};
    if ((st = check_chain_out(c, out, c->W))) return st;
    ChainSpans is, os;
    chain_ctx_spans(c, pairs, n, &is);
    chain_state_spans(n, d_state, state_stride, c->W, c->H, &is);
    is.push_back(med_span(d_U0, start_stride, (size_t)c->W * 4, c->H));
    is.push_back(med_span(d_V0, start_stride, (size_t)c->W * 4, c->H));
    chain_out_spans(out, c->W, c->H, &os);
    if ((st = check_chain_overlap(c, is, os))) return st;
    if ((st = chain_device_begin(c, d_stats))) return st;
    hsk::ChainPlanes pl{};
    chain_ctx_planes(c, pairs, n, d_state, &pl);
    return enqueue_chain_dense(c, pl, n, (size_t)c->P * 4, state_stride, d_U0, d_V0, start_stride, *cp, out, d_stats);
}

int hsflow_chain_flow(hsflow_ctx *c, const int *pairs, int n, const uint8_t *const *state, size_t state_stride, const float *U0, const float *V0,
                      size_t start_stride, const hsflow_chain_params *cp, float *U, float *V, size_t out_stride, uint8_t *status, size_t status_stride,
                      uint8_t *age, size_t age_stride, hsflow_chain_stats *stats)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_chain_params(c, cp))) return st;
    if ((st = check_chain_pairs(c, pairs, n))) return st;
    if ((st = check_chain_state(c, n, (const void *const *)state, state_stride, c->W))) return st;
    if ((st = check_chain_start(c, U0, V0, start_stride, c->W))) return st;
    const ChainOut out = {U, V, out_stride, status, status_stride, age, age_stride, stats};
    if ((st = check_chain_out(c, out, c->W))) return st;
    {
        ChainSpans is, os;
        chain_state_spans(n, (const void *const *)state, state_stride, c->W, c->H, &is);
        is.push_back(med_span(U0, start_stride, (size_t)c->W * 4, c->H));
        is.push_back(med_span(V0, start_stride, (size_t)c->W * 4, c->H));
        chain_out_spans(out, c->W, c->H, &os);
        if ((st = check_chain_overlap(c, is, os))) return st;
    }
    if ((st = settle_pending(c))) return st;
    const size_t frow = (size_t)c->W * 4, brow = (size_t)c->W, fbytes = frow * c->H, bbytes = brow * c->H;
    hsflow_ctx::ChainScratch &s = c->chain;
    // the slots: 0 the state planes, 1 / 2 the start planes, 3 / 4 U and V, 5 status, 6 age
    if (chain_any(n, state) && (st = chain_stage(c, 0, bbytes * n))) return st;
    if (U0 && ((st = chain_stage(c, 1, fbytes)) || (st = chain_stage(c, 2, fbytes)))) return st;
    if (U && ((st = chain_stage(c, 3, fbytes)) || (st = chain_stage(c, 4, fbytes)))) return st;
    if (status && (st = chain_stage(c, 5, bbytes))) return st;
    if (age && (st = chain_stage(c, 6, bbytes))) return st;
    if (stats && (st = stats_reserve(c, (void **)&s.dStats, (void **)&s.hStats))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    const void *dstate[hschain::kMaxPairs];
    if ((st = chain_upload_state(c, n, state, state_stride, dstate))) return st;
    if (U0) {
        HS_HIP(c, copy_rows_async(c, s.stage[1], frow, U0, start_stride, frow, c->H, hipMemcpyHostToDevice));
        HS_HIP(c, copy_rows_async(c, s.stage[2], frow, V0, start_stride, frow, c->H, hipMemcpyHostToDevice));
    }
    hsk::ChainPlanes pl{};
    chain_ctx_planes(c, pairs, n, dstate, &pl);
    const ChainOut dev = {U ? s.stage[3] : nullptr, U ? s.stage[4] : nullptr, frow, status ? s.stage[5] : nullptr, brow, age ? s.stage[6] : nullptr, brow, nullptr};
    if ((st = enqueue_chain_dense(c, pl, n, (size_t)c->P * 4, brow, U0 ? s.stage[1] : nullptr, U0 ? s.stage[2] : nullptr, frow, *cp, dev, stats ? s.dStats : nullptr)))
        return st;
    if (U) {
        HS_HIP(c, copy_rows_async(c, U, out_stride, s.stage[3], frow, frow, c->H, hipMemcpyDeviceToHost));
        HS_HIP(c, copy_rows_async(c, V, out_stride, s.stage[4], frow, frow, c->H, hipMemcpyDeviceToHost));
    }
    if (status) HS_HIP(c, copy_rows_async(c, status, status_stride, s.stage[5], brow, brow, c->H, hipMemcpyDeviceToHost));
    if (age) HS_HIP(c, copy_rows_async(c, age, age_stride, s.stage[6], brow, brow, c->H, hipMemcpyDeviceToHost));
    if (stats && (st = stats_copy_back(c, s.hStats, s.dStats))) return st;
    return sync_finish(c, marked, stats, s.hStats);
}

int hsflow_track_points_device(hsflow_ctx *c, const int *pairs, int n, const void *const *d_state, size_t state_stride, const hsflow_chain_params *cp,
                               const float *d_xy, int m, float *d_track, float *d_last, uint8_t *d_status, uint8_t *d_age, hsflow_chain_stats *d_stats)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_chain_params(c, cp))) return st;
    if ((st = check_chain_pairs(c, pairs, n))) return st;
    if ((st = check_chain_state(c, n, d_state, state_stride, c->W))) return st;
    if ((st = check_chain_points(c, d_xy, m, d_track, d_last, d_status, d_age, d_stats))) return st;
    ChainSpans is, os;
    chain_ctx_spans(c, pairs, n, &is);
    chain_state_spans(n, d_state, state_stride, c->W, c->H, &is);
    chain_points_spans(n, d_xy, m, d_track, d_last, d_status, d_age, d_stats, &is, &os);
    if ((st = check_chain_overlap(c, is, os))) return st;
    if ((st = chain_device_begin(c, d_stats))) return st;
    hsk::ChainPlanes pl{};
    chain_ctx_planes(c, pairs, n, d_state, &pl);
    return enqueue_chain_points(c, pl, n, (size_t)c->P * 4, state_stride, *cp, d_xy, m, d_track, d_last, d_status, d_age, d_stats);
}

int hsflow_track_points(hsflow_ctx *c, const int *pairs, int n, const uint8_t *const *state, size_t state_stride, const hsflow_chain_params *cp, const float *xy,
                        int m, float *track, float *last, uint8_t *status, uint8_t *age, hsflow_chain_stats *stats)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_chain_params(c, cp))) return st;
    if ((st = check_chain_pairs(c, pairs, n))) return st;
    if ((st = check_chain_state(c, n, (const void *const *)state, state_stride, c->W))) return st;
    if ((st = check_chain_points(c, xy, m, track, last, status, age, stats))) return st;
    {
        ChainSpans is, os;
        chain_state_spans(n, (const void *const *)state, state_stride, c->W, c->H, &is);
        chain_points_spans(n, xy, m, track, last, status, age, stats, &is, &os);
        if ((st = check_chain_overlap(c, is, os))) return st;
    }
    if ((st = settle_pending(c))) return st;
    const size_t brow = (size_t)c->W, bbytes = brow * c->H, pbytes = (size_t)m * 8, tbytes = (size_t)(n + 1) * pbytes;
    hsflow_ctx::ChainScratch &s = c->chain;
    // the slots: 0 the state planes, 1 the points, 3 the track, 4 the last positions, 5 status, 6 age
    if (chain_any(n, state) && (st = chain_stage(c, 0, bbytes * n))) return st;
    if ((st = chain_stage(c, 1, pbytes))) return st;
    if (track && (st = chain_stage(c, 3, tbytes))) return st;
    if (last && (st = chain_stage(c, 4, pbytes))) return st;
    if (status && (st = chain_stage(c, 5, (size_t)m))) return st;
    if (age && (st = chain_stage(c, 6, (size_t)m))) return st;
    if (stats && (st = stats_reserve(c, (void **)&s.dStats, (void **)&s.hStats))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    const void *dstate[hschain::kMaxPairs];
    if ((st = chain_upload_state(c, n, state, state_stride, dstate))) return st;
    HS_HIP(c, hipMemcpyAsync(s.stage[1], xy, pbytes, hipMemcpyHostToDevice, c->stream));
    hsk::ChainPlanes pl{};
    chain_ctx_planes(c, pairs, n, dstate, &pl);
    if ((st = enqueue_chain_points(c, pl, n, (size_t)c->P * 4, brow, *cp, (const float *)s.stage[1], m, track ? (float *)s.stage[3] : nullptr,
                                   last ? (float *)s.stage[4] : nullptr, status ? s.stage[5] : nullptr, age ? s.stage[6] : nullptr, stats ? s.dStats : nullptr)))
        return st;
    if (track) HS_HIP(c, hipMemcpyAsync(track, s.stage[3], tbytes, hipMemcpyDeviceToHost, c->stream));
    if (last) HS_HIP(c, hipMemcpyAsync(last, s.stage[4], pbytes, hipMemcpyDeviceToHost, c->stream));
    if (status) HS_HIP(c, hipMemcpyAsync(status, s.stage[5], (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (age) HS_HIP(c, hipMemcpyAsync(age, s.stage[6], (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (stats && (st = stats_copy_back(c, s.hStats, s.dStats))) return st;
    return sync_finish(c, marked, stats, s.hStats);
}

} // extern "C"
