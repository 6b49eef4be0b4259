// hs_median.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_median*, the median filter and
// the hole filling of a flow where the solver left it (hs_median_rule.h).  Per chunk of at most HSFLOW_JPEG_BATCH_MAX
// fields and per pass: one launch (hs_kernels_median.hip.h), with statistics one memset of the chunk's records in front of
// it.  The single forms are batches of one.  A context that never filters allocates and launches nothing here.
#pragma once

namespace {

static_assert(sizeof(hsflow_median_stats) == 64 && sizeof(hsflow_median_stats) == sizeof(hsk::MedianStatsWords), "hsflow_median_stats is 64 bytes on both sides");
static_assert(offsetof(hsflow_median_stats, newly_filled) == 24 && offsetof(hsflow_median_stats, changed) == 32, "hsflow_median_stats: the kernel's layout");
static_assert(sizeof(hsflow_median_params) == 16, "hsflow_median_params is 16 bytes");
static_assert(hsk::kMedianBatchMax == hsk::kRenderBatchMax, "one chunk size for every batched form");
static_assert(HSFLOW_MEDIAN_FILTER == hsmed::kFilter && HSFLOW_MEDIAN_FILL == hsmed::kFill && HSFLOW_MEDIAN_MAX_PASSES == hsmed::kMaxPasses, "the header's constants are the rule's");

int check_median_params(hsflow_ctx *c, const hsflow_median_params *mp)
{
    if (!mp || mp->struct_size != sizeof(hsflow_median_params)) return fail(c, HSFLOW_E_ARG, "median params null or struct_size mismatch");
    if (mp->radius != 1 && mp->radius != 2) return fail(c, HSFLOW_E_ARG, "median radius must be 1 or 2");
    if (mp->mode != HSFLOW_MEDIAN_FILTER && mp->mode != HSFLOW_MEDIAN_FILL) return fail(c, HSFLOW_E_ARG, "unknown median mode");
    const int side = 2 * mp->radius + 1;
    if (mp->min_votes < 1 || mp->min_votes > side * side) return fail(c, HSFLOW_E_ARG, "median min_votes must be 1 .. (2 radius + 1)^2");
    return HSFLOW_OK;
}

int check_median_passes(hsflow_ctx *c, int passes)
{
    if (passes < 1 || passes > HSFLOW_MEDIAN_MAX_PASSES) return fail(c, HSFLOW_E_ARG, "median passes must be 1 .. " + std::to_string(HSFLOW_MEDIAN_MAX_PASSES));
    return HSFLOW_OK;
}

// The checks every form shares once the optional planes are known: what there is to do and the row sizes.
int check_median_planes(hsflow_ctx *c, int W, bool has_state, size_t state_stride, bool has_u, bool has_v, size_t out_stride, bool has_state_out,
                        size_t state_out_stride, bool has_stats)
{
    if (has_u != has_v) return fail(c, HSFLOW_E_ARG, "the two flow outputs are asked for together or not at all");
    if (!has_u && !has_state_out && !has_stats) return fail(c, HSFLOW_E_ARG, "neither the flow nor the state nor statistics asked for");
    if (has_state && state_stride < (size_t)W) return fail(c, HSFLOW_E_SIZE, "state stride smaller than width");
    if (has_u && (out_stride < (size_t)W * 4 || (out_stride & 3u))) return fail(c, HSFLOW_E_SIZE, "output flow stride smaller than 4*width or no multiple of 4");
    if (has_state_out && state_out_stride < (size_t)W) return fail(c, HSFLOW_E_SIZE, "output state stride smaller than width");
    return HSFLOW_OK;
}

// The bytes a plane of H rows of rowb bytes, `stride` apart, covers.
struct MedSpan {
    uintptr_t lo, hi;
};
MedSpan med_span(const void *p, size_t stride, size_t rowb, int H) { return MedSpan{(uintptr_t)p, p ? (uintptr_t)p + stride * (size_t)(H - 1) + rowb : 0}; }
bool med_overlap(const MedSpan &a, const MedSpan &b) { return a.hi && b.hi && a.lo < b.hi && b.lo < a.hi; }

// No output may overlap an input (the kernel reads a neighbourhood that another workgroup writes).
int check_median_overlap(hsflow_ctx *c, const MedSpan (&in)[3], const MedSpan (&out)[3])
{
    for (const MedSpan &o : out)
        for (const MedSpan &i : in)
            if (med_overlap(o, i)) return fail(c, HSFLOW_E_ARG, "an output of the median may not overlap an input");
    return HSFLOW_OK;
}

// One pass over cnt fields (cnt <= kRenderBatchMax).  Strides in bytes.  d_stats: the chunk's first record, or NULL.  The
// caller has checked every argument.
int enqueue_median_chunk(hsflow_ctx *c, int cnt, const hsflow_median_params &mp, const hsk::MedianBatchFields &f, size_t is, size_t ss, size_t os, size_t sos,
                         void *d_stats)
{
    hsk::MedianStatsWords *stats = (hsk::MedianStatsWords *)d_stats;
    dim3 grid;
    const int st = stats_grid(c, (c->W + hsk::kMedTileX - 1) / hsk::kMedTileX, (c->H + hsk::kMedTileY - 1) / hsk::kMedTileY, cnt, stats, &grid);
    if (st) return st;
    HS_HIP(c, hsk::launch_median_batch(mp.radius, mp.mode == HSFLOW_MEDIAN_FILL, grid, c->stream, f, (long long)is, (long long)ss, (long long)os, (long long)sos, c->W,
                                       c->H, mp.min_votes, stats));
    c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
    return HSFLOW_OK;
}

// The scratch of hsflow_median_apply and hsflow_median, allocated by the first call that needs a piece and kept.
int median_reserve(hsflow_ctx *c, int flow_pairs, int byte_planes, bool stats)
{
    hsflow_ctx::MedianScratch &m = c->median;
    const size_t fbytes = (size_t)c->W * 4 * c->H, bbytes = (size_t)c->W * c->H;
    for (int k = 0; k < flow_pairs; k++) {
        if (!m.u[k]) HS_HIP(c, hipMalloc((void **)&m.u[k], fbytes));
        if (!m.v[k]) HS_HIP(c, hipMalloc((void **)&m.v[k], fbytes));
    }
    for (int k = 0; k < byte_planes; k++)
        if (!m.s[k]) HS_HIP(c, hipMalloc((void **)&m.s[k], bbytes));
    return stats ? stats_reserve(c, (void **)&m.dStats, (void **)&m.hStats) : HSFLOW_OK;
}

// `passes` passes from the planes (u, v, rows is bytes apart) and the state (or NULL) through the scratch; the scratch is
// packed (rows 4 W and W bytes).  Flow pass j (1-based) lands in flow_dst(j), its state in the byte plane the pass before
// did not write; the last pass writes its state to last_state (or nowhere) and the record.  flow_dst: see the callers.
template <class FlowDst>
int median_passes(hsflow_ctx *c, const hsflow_median_params &mp, int passes, const float *u, const float *v, size_t is, const uint8_t *state, size_t ss,
                  FlowDst flow_dst, uint8_t *first_state_plane, uint8_t *second_state_plane, uint8_t *last_state, size_t last_ss, void *d_stats)
{
    const size_t brow = (size_t)c->W;
    for (int j = 1; j <= passes; j++) {
        const bool last = j == passes;
        hsk::MedianBatchFields f{};
        float *uo = nullptr, *vo = nullptr;
        size_t os = 0;
        flow_dst(j, &uo, &vo, &os);
        uint8_t *so = last ? last_state : (j & 1) ? first_state_plane : second_state_plane;
        f.u[0] = u; f.v[0] = v; f.state[0] = state;
        f.u_out[0] = uo; f.v_out[0] = vo; f.state_out[0] = so;
        const int st = enqueue_median_chunk(c, 1, mp, f, is, ss, os, last ? last_ss : brow, last ? d_stats : nullptr);
        if (st) return st;
        u = uo; v = vo; is = os;
        state = so; ss = brow;
    }
    return HSFLOW_OK;
}

// What hsflow_median_batch_device and hsflow_median_planes_device share.  pairs: the inputs are the flows of the context's
// pairs first_pair ..; else u / v / is for the one field (n is then 1).
int median_on_device(hsflow_ctx *c, int first_pair, int n, const float *u, const float *v, size_t is, const hsflow_median_params *mp, const void *const *d_state,
                     size_t state_stride, void *const *d_u_out, void *const *d_v_out, size_t out_stride, void *const *d_state_out, size_t state_out_stride,
                     hsflow_median_stats *d_stats)
{
    int st = HSFLOW_OK, maxb = 0;
    const bool pairs = u == nullptr;
    if ((st = check_median_params(c, mp))) return st;
    if ((st = check_median_planes(c, c->W, d_state != nullptr, state_stride, d_u_out != nullptr, d_v_out != nullptr, out_stride, d_state_out != nullptr,
                                  state_out_stride, d_stats != nullptr)))
        return st;
    const size_t frow = (size_t)c->W * 4, brow = (size_t)c->W;
    for (int i = 0; i < n; i++) {
        if ((d_state && !d_state[i]) || (d_u_out && (!d_u_out[i] || !d_v_out[i])) || (d_state_out && !d_state_out[i]))
            return fail(c, HSFLOW_E_ARG, "field " + std::to_string(i) + ": null plane pointer");
        if (d_u_out && (((uintptr_t)d_u_out[i] | (uintptr_t)d_v_out[i]) & 3u))
            return fail(c, HSFLOW_E_ARG, "field " + std::to_string(i) + ": the output flow planes must be 4-byte aligned");
    }
    // (the alignment here, not in batch_device_begin: it is checked ahead of the overlaps)
    if (((uintptr_t)d_stats & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the statistics records must be 8-byte aligned");
    // every output of the batch against every input of the batch (the pairs' planes in both buffers of the ping-pong)
    for (int i = 0; i < n; i++) {
        const MedSpan out[3] = {med_span(d_u_out ? d_u_out[i] : nullptr, out_stride, frow, c->H), med_span(d_v_out ? d_v_out[i] : nullptr, out_stride, frow, c->H),
                                med_span(d_state_out ? d_state_out[i] : nullptr, state_out_stride, brow, c->H)};
        for (int k = 0; k < n; k++) {
            const MedSpan state = med_span(d_state ? d_state[k] : nullptr, state_stride, brow, c->H);
            if (pairs) {
                for (int b = 0; b < 2; b++) {
                    const MedSpan in[3] = {med_span(c->dU[b] + (long long)(first_pair + k) * c->plane, (size_t)c->P * 4, frow, c->H),
                                           med_span(c->dV[b] + (long long)(first_pair + k) * c->plane, (size_t)c->P * 4, frow, c->H), state};
                    if ((st = check_median_overlap(c, in, out))) return st;
                }
            } else {
                const MedSpan in[3] = {med_span(u, is, frow, c->H), med_span(v, is, frow, c->H), state};
                if ((st = check_median_overlap(c, in, out))) return st;
            }
        }
    }
    if ((st = batch_device_begin(c, nullptr, &maxb))) return st;
    const float *U = c->dU[c->cur], *V = c->dV[c->cur];
    for (const hsjpeg_plan::Chunk &ch : hsjpeg_plan::chunks(n, maxb)) {
        hsk::MedianBatchFields f{};
        for (int k = 0; k < ch.count; k++) {
            const int i = ch.first + k;
            const long long pair = first_pair + i;
            f.u[k] = pairs ? U + pair * c->plane : u;
            f.v[k] = pairs ? V + pair * c->plane : v;
            f.state[k] = d_state ? (const uint8_t *)d_state[i] : nullptr;
            f.u_out[k] = d_u_out ? (float *)d_u_out[i] : nullptr;
            f.v_out[k] = d_v_out ? (float *)d_v_out[i] : nullptr;
            f.state_out[k] = d_state_out ? (uint8_t *)d_state_out[i] : nullptr;
        }
        if ((st = enqueue_median_chunk(c, ch.count, *mp, f, pairs ? (size_t)c->P * 4 : is, state_stride, out_stride, state_out_stride,
                                       d_stats ? d_stats + ch.first : nullptr)))
            return st;
    }
    return HSFLOW_OK;
}

} // namespace

extern "C" {

void hsflow_default_median_params(hsflow_median_params *mp)
{
    if (!mp) return;
    std::memset(mp, 0, sizeof(*mp));
    mp->struct_size = sizeof(*mp);
    mp->radius = 1;
    mp->mode = HSFLOW_MEDIAN_FILTER;
    mp->min_votes = 1;
}

int hsflow_median_host(const float *u, size_t u_stride, const float *v, size_t v_stride, const uint8_t *state, size_t state_stride, int width, int height,
                       const hsflow_median_params *mp, int passes, float *u_out, float *v_out, size_t out_stride, uint8_t *state_out, size_t state_out_stride,
                       hsflow_median_stats *stats)
{
    int st = check_median_params(nullptr, mp);
    if (st) return st;
    if ((st = check_median_passes(nullptr, passes))) return st;
    if (!u || !v) return fail(nullptr, HSFLOW_E_ARG, "hsflow_median_host: null flow plane");
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_median_host: width and height must be positive");
    const size_t frow = (size_t)width * 4, brow = (size_t)width;
    if (u_stride < frow || v_stride < frow || ((u_stride | v_stride) & 3u)) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_median_host: flow stride smaller than 4*width or no multiple of 4");
    if ((st = check_median_planes(nullptr, width, state != nullptr, state_stride, u_out != nullptr, v_out != nullptr, out_stride, state_out != nullptr,
                                  state_out_stride, stats != nullptr)))
        return st;
    const MedSpan in[3] = {med_span(u, u_stride, frow, height), med_span(v, v_stride, frow, height), med_span(state, state_stride, brow, height)};
    const MedSpan out[3] = {med_span(u_out, out_stride, frow, height), med_span(v_out, out_stride, frow, height), med_span(state_out, state_out_stride, brow, height)};
    if ((st = check_median_overlap(nullptr, in, out))) return st;
    const int fill = mp->mode == HSFLOW_MEDIAN_FILL;
    hsmed::Sums sums = {0, 0, 0, 0, 0};
    if (passes == 1) {
        hsmed::median_rows(mp->radius, u, u_stride, v, v_stride, state, state_stride, width, height, fill, mp->min_votes, u_out, v_out, out_stride, state_out,
                           state_out_stride, &sums);
    } else {
        // packed planes between the passes: two flow pairs and two states, the last pass into the caller's
        const size_t px = (size_t)width * height;
        std::vector<float> fu[2], fv[2];
        std::vector<uint8_t> fs[2];
        for (int k = 0; k < 2; k++) { fu[k].resize(px); fv[k].resize(px); fs[k].resize(px); }
        const float *cu = u, *cv = v;
        const uint8_t *cs = state;
        size_t us = u_stride, vs = v_stride, ss = state_stride;
        for (int j = 1; j <= passes; j++) {
            const bool last = j == passes;
            const int k = j & 1;
            if (last) {
                hsmed::median_rows(mp->radius, cu, us, cv, vs, cs, ss, width, height, fill, mp->min_votes, u_out, v_out, out_stride, state_out, state_out_stride, &sums);
            } else {
                hsmed::median_rows(mp->radius, cu, us, cv, vs, cs, ss, width, height, fill, mp->min_votes, fu[k].data(), fv[k].data(), frow, fs[k].data(), brow, nullptr);
                cu = fu[k].data(); cv = fv[k].data(); cs = fs[k].data();
                us = vs = frow; ss = brow;
            }
        }
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->kept = sums.kept; stats->filled = sums.filled; stats->unfilled = sums.unfilled;
        stats->newly_filled = sums.newly_filled; stats->changed = sums.changed;
    }
    return HSFLOW_OK;
}

int hsflow_median_batch_device(hsflow_ctx *c, int first_pair, int n, const hsflow_median_params *mp, const void *const *d_state, size_t state_stride,
                               void *const *d_u_out, void *const *d_v_out, size_t out_stride, void *const *d_state_out, size_t state_out_stride,
                               hsflow_median_stats *d_stats)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_batch_pairs(c, first_pair, n))) return st;
    return median_on_device(c, first_pair, n, nullptr, nullptr, 0, mp, d_state, state_stride, d_u_out, d_v_out, out_stride, d_state_out, state_out_stride, d_stats);
}

int hsflow_median_device(hsflow_ctx *c, int pair, const hsflow_median_params *mp, const void *d_state, size_t state_stride, void *d_u_out, void *d_v_out,
                         size_t out_stride, void *d_state_out, size_t state_out_stride, hsflow_median_stats *d_stats)
{
    const void *const state[1] = {d_state};
    void *const uo[1] = {d_u_out}, *const vo[1] = {d_v_out}, *const so[1] = {d_state_out};
    return hsflow_median_batch_device(c, pair, 1, mp, d_state ? state : nullptr, state_stride, d_u_out ? uo : nullptr, d_v_out ? vo : nullptr, out_stride,
                                      d_state_out ? so : nullptr, state_out_stride, d_stats);
}

int hsflow_median_planes_device(hsflow_ctx *c, const hsflow_median_params *mp, const void *d_u, const void *d_v, size_t in_stride, const void *d_state,
                                size_t state_stride, void *d_u_out, void *d_v_out, size_t out_stride, void *d_state_out, size_t state_out_stride,
                                hsflow_median_stats *d_stats)
{
    const int st = check_ctx(c, 0);
    if (st) return st;
    if (!d_u || !d_v) return fail(c, HSFLOW_E_ARG, "null flow plane");
    if ((((uintptr_t)d_u | (uintptr_t)d_v) & 3u) != 0) return fail(c, HSFLOW_E_ARG, "the flow planes must be 4-byte aligned");
    if (in_stride < (size_t)c->W * 4 || (in_stride & 3u)) return fail(c, HSFLOW_E_SIZE, "flow stride smaller than 4*width or no multiple of 4");
    const void *const state[1] = {d_state};
    void *const uo[1] = {d_u_out}, *const vo[1] = {d_v_out}, *const so[1] = {d_state_out};
    return median_on_device(c, 0, 1, (const float *)d_u, (const float *)d_v, in_stride, mp, d_state ? state : nullptr, state_stride, d_u_out ? uo : nullptr,
                            d_v_out ? vo : nullptr, out_stride, d_state_out ? so : nullptr, state_out_stride, d_stats);
}

int hsflow_median_apply(hsflow_ctx *c, int pair, const hsflow_median_params *mp, int passes, const void *d_state, size_t state_stride, void *d_state_out,
                        size_t state_out_stride, hsflow_median_stats *d_stats)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = check_median_params(c, mp))) return st;
    if ((st = check_median_passes(c, passes))) return st;
    if ((st = check_median_planes(c, c->W, d_state != nullptr, state_stride, true, true, (size_t)c->W * 4, d_state_out != nullptr, state_out_stride, d_stats != nullptr)))
        return st;
    if (((uintptr_t)d_stats & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the statistics records must be 8-byte aligned");
    const size_t frow = (size_t)c->W * 4, brow = (size_t)c->W, pitchb = (size_t)c->P * 4;
    {
        const MedSpan out[3] = {med_span(d_state_out, state_out_stride, brow, c->H), MedSpan{0, 0}, MedSpan{0, 0}};
        for (int b = 0; b < 2; b++) {
            const MedSpan in[3] = {med_span(c->dU[b] + (long long)pair * c->plane, pitchb, frow, c->H), med_span(c->dV[b] + (long long)pair * c->plane, pitchb, frow, c->H),
                                   med_span(d_state, state_stride, brow, c->H)};
            if ((st = check_median_overlap(c, in, out))) return st;
        }
    }
    // the way of hsflow_set_flow_device: an unverified asynchronous solve still needs the old flow, the planes are the
    // caller's from now on (the next warm strip / fold solve measures them), last_eps can no longer be measured
    if ((st = settle_pending(c))) return st;
    if ((st = median_reserve(c, 1, passes > 1 ? 2 : 0, false))) return st;
    c->lastl.valid = false;
    c->flow_tame = false;
    hsflow_ctx::MedianScratch &m = c->median;
    float *U = c->dU[c->cur] + (long long)pair * c->plane, *V = c->dV[c->cur] + (long long)pair * c->plane;
    // the flow goes to and fro between the scratch pair (odd passes) and the pair's own planes (even passes)
    auto flow_dst = [&](int j, float **uo, float **vo, size_t *os) {
        if (j & 1) { *uo = m.u[0]; *vo = m.v[0]; *os = frow; }
        else { *uo = U; *vo = V; *os = pitchb; }
    };
    if ((st = median_passes(c, *mp, passes, U, V, pitchb, (const uint8_t *)d_state, state_stride, flow_dst, m.s[0], m.s[1], (uint8_t *)d_state_out, state_out_stride,
                            d_stats)))
        return st;
    if (passes & 1) {
        HS_HIP(c, hipMemcpy2DAsync(U, pitchb, m.u[0], frow, frow, c->H, hipMemcpyDeviceToDevice, c->stream));
        HS_HIP(c, hipMemcpy2DAsync(V, pitchb, m.v[0], frow, frow, c->H, hipMemcpyDeviceToDevice, c->stream));
    }
    c->flow_after_mark = true;
    return HSFLOW_OK;
}

int hsflow_median(hsflow_ctx *c, int pair, const hsflow_median_params *mp, int passes, const uint8_t *state, size_t state_stride, float *u, float *v,
                  size_t out_stride, uint8_t *state_out, size_t state_out_stride, hsflow_median_stats *stats)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = check_median_params(c, mp))) return st;
    if ((st = check_median_passes(c, passes))) return st;
    if ((st = check_median_planes(c, c->W, state != nullptr, state_stride, u != nullptr, v != nullptr, out_stride, state_out != nullptr, state_out_stride,
                                  stats != nullptr)))
        return st;
    const size_t frow = (size_t)c->W * 4, brow = (size_t)c->W;
    {
        const MedSpan in[3] = {med_span(state, state_stride, brow, c->H), MedSpan{0, 0}, MedSpan{0, 0}};
        const MedSpan out[3] = {med_span(u, out_stride, frow, c->H), med_span(v, out_stride, frow, c->H), med_span(state_out, state_out_stride, brow, c->H)};
        if ((st = check_median_overlap(c, in, out))) return st;
    }
    if ((st = settle_pending(c))) return st;
    // the flow of pass j in scratch pair (j & 1) ^ 1 (the context's own flow stays as it is), the states in the two byte planes:
    // the uploaded one is free again once the first pass has read it
    const bool need_flow = u != nullptr || passes > 1, need_bytes = state != nullptr || state_out != nullptr || passes > 1;
    hsflow_ctx::MedianScratch &m = c->median;
    if ((st = median_reserve(c, need_flow ? (passes > 1 ? 2 : 1) : 0, need_bytes ? 2 : 0, stats != nullptr))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    if (state) HS_HIP(c, copy_rows_async(c, m.s[0], brow, state, state_stride, brow, c->H, hipMemcpyHostToDevice));
    const bool last_flow = u != nullptr;
    auto flow_dst = [&](int j, float **uo, float **vo, size_t *os) {
        const bool wanted = j < passes || last_flow;
        *uo = wanted ? m.u[(j & 1) ^ 1] : nullptr; *vo = wanted ? m.v[(j & 1) ^ 1] : nullptr; *os = frow;
    };
    // pass 1 reads s[0] (the upload) and writes s[1], pass 2 writes s[0], ...: first plane s[1], second s[0]
    uint8_t *const last_state = state_out ? m.s[passes & 1] : nullptr;
    const float *U = c->dU[c->cur] + (long long)pair * c->plane, *V = c->dV[c->cur] + (long long)pair * c->plane;
    if ((st = median_passes(c, *mp, passes, U, V, (size_t)c->P * 4, state ? m.s[0] : nullptr, brow, flow_dst, m.s[1], m.s[0], last_state, brow,
                            stats ? m.dStats : nullptr)))
        return st;
    if (u) {
        HS_HIP(c, copy_rows_async(c, u, out_stride, m.u[(passes & 1) ^ 1], frow, frow, c->H, hipMemcpyDeviceToHost));
        HS_HIP(c, copy_rows_async(c, v, out_stride, m.v[(passes & 1) ^ 1], frow, frow, c->H, hipMemcpyDeviceToHost));
    }
    if (state_out) HS_HIP(c, copy_rows_async(c, state_out, state_out_stride, last_state, brow, brow, c->H, hipMemcpyDeviceToHost));
    if (stats && (st = stats_copy_back(c, m.hStats, m.dStats))) return st;
    return sync_finish(c, marked, stats, m.hStats);
}

} // extern "C"
