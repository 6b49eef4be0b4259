// hs_link.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_link_regions*, the regions of frame k
// linked to those of frame k + 1 by the flow, where label planes and flow lie (hs_link_rule.h), and hsflow_link_tracks_host.
// The engine works on planes (enqueue_link); the forms on a context's pairs hand it the context's flow.  Per chunk of steps
// one fixed sequence of launches (hsk::launch_link), no memset call, no wait.  On top of hs_postops.hip.h: its three
// ordering rules hold word for word.  A context that never links allocates and launches nothing here.
#pragma once

namespace {

static_assert(sizeof(hsflow_link_result) == 64 && sizeof(hsflow_link_result) == sizeof(hsln::Result) && sizeof(hsflow_link_result) == kStatsBytes,
              "hsflow_link_result is 64 bytes on both sides");
static_assert(sizeof(hsflow_link_record) == 16 && sizeof(hsflow_link_record) == sizeof(hsln::Link), "hsflow_link_record is 16 bytes on both sides");
static_assert(sizeof(hsflow_link_side) == 32 && sizeof(hsflow_link_side) == sizeof(hsln::Side), "hsflow_link_side is 32 bytes on both sides");
static_assert(offsetof(hsflow_link_side, best) == 8 && offsetof(hsflow_link_side, gone_px) == 16, "hsflow_link_side: the kernel's layout");
static_assert(offsetof(hsflow_link_result, n_mutual) == 12 && offsetof(hsflow_link_result, voted_px) == 16 && offsetof(hsflow_link_result, over_a_px) == 40,
              "hsflow_link_result: the kernel's layout");
static_assert(sizeof(hsflow_link_params) == 16, "hsflow_link_params is 16 bytes");
static_assert(HSFLOW_LINK_MAX_CELLS == hsln::kMaxCells && HSFLOW_LINK_FLAG_OVERFLOW == hsln::kFlagOverflow, "the header's constants are the rule's");

int check_link_params(hsflow_ctx *c, const hsflow_link_params *lp, uint32_t link_capacity)
{
    if (!lp || lp->struct_size != sizeof(hsflow_link_params)) return fail(c, HSFLOW_E_ARG, "link params null or struct_size mismatch");
    if (lp->reserved) return fail(c, HSFLOW_E_ARG, "link params: reserved must be 0");
    if (lp->cap_a < 1u || lp->cap_b < 1u) return fail(c, HSFLOW_E_ARG, "link cap_a and cap_b must be at least 1");
    if (lp->cap_a > hsln::kMaxCap || lp->cap_b > hsln::kMaxCap) return fail(c, HSFLOW_E_SIZE, "a link cap above 2^30");
    if ((uint64_t)lp->cap_a * lp->cap_b > (uint64_t)hsln::kMaxCells) return fail(c, HSFLOW_E_SIZE, "link cap_a * cap_b above 2^24 cells");
    if (link_capacity > hsln::kMaxCells) return fail(c, HSFLOW_E_SIZE, "a link_capacity above 2^24 records");
    return HSFLOW_OK;
}

// The steps of a call as the caller names them (host or device memory alike): n of each; step i links a[i] to b[i].  The
// lists of links and sides may be NULL and may hold NULL entries.
struct LnSteps {
    int n;
    const void *const *a, *const *b;
    size_t as, bs;
    const void *const *u, *const *v; // NULL: the context's pairs
    size_t fs;
    void *const *links;
    uint32_t link_capacity;
    void *const *side_a, *const *side_b;
    const void *results; // n headers, or NULL
};

int check_link_steps(hsflow_ctx *c, const LnSteps &f, int W)
{
    bool asked = f.results != nullptr;
    for (int k = 0; k < f.n; k++) {
        const std::string who = "step " + std::to_string(k) + ": ";
        if (!f.a[k] || !f.b[k]) return fail(c, HSFLOW_E_ARG, who + "null label plane");
        if ((((uintptr_t)f.a[k] | (uintptr_t)f.b[k]) & 3u) != 0) return fail(c, HSFLOW_E_ARG, who + "the label planes must be 4-byte aligned");
        if (f.u) {
            if (!f.u[k] || !f.v[k]) return fail(c, HSFLOW_E_ARG, who + "null flow plane");
            if ((((uintptr_t)f.u[k] | (uintptr_t)f.v[k]) & 3u) != 0) return fail(c, HSFLOW_E_ARG, who + "the flow planes must be 4-byte aligned");
        }
        for (void *const *list : {f.links, f.side_a, f.side_b})
            if (list && list[k]) {
                // (a link array of no records is no output: nothing would be written to it)
                if (list != f.links || f.link_capacity > 0u) asked = true;
                if (((uintptr_t)list[k] & 7u) != 0) return fail(c, HSFLOW_E_ARG, who + "the link and side records must be 8-byte aligned");
            }
    }
    if (f.as < (size_t)W * 4 || (f.as & 3u) || f.bs < (size_t)W * 4 || (f.bs & 3u)) return fail(c, HSFLOW_E_SIZE, "labels stride smaller than 4*width or no multiple of 4");
    if (f.u && (f.fs < (size_t)W * 4 || (f.fs & 3u))) return fail(c, HSFLOW_E_SIZE, "flow stride smaller than 4*width or no multiple of 4");
    if (((uintptr_t)f.results & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the result headers must be 8-byte aligned");
    if (!asked) return fail(c, HSFLOW_E_ARG, "neither links nor sides nor a result asked for");
    return HSFLOW_OK;
}

// No output may overlap an input or another output (first_pair >= 0: the context's flows of the pairs, in both buffers of
// the ping-pong).
int check_link_overlap(hsflow_ctx *c, const LnSteps &f, const hsflow_link_params &lp, int first_pair, int W, int H)
{
    std::vector<MedSpan> in, out;
    for (int k = 0; k < f.n; k++) {
        in.push_back(med_span(f.a[k], f.as, (size_t)W * 4, H));
        in.push_back(med_span(f.b[k], f.bs, (size_t)W * 4, H));
        if (f.u) {
            in.push_back(med_span(f.u[k], f.fs, (size_t)W * 4, H));
            in.push_back(med_span(f.v[k], f.fs, (size_t)W * 4, H));
        } else {
            for (int b = 0; b < 2; b++) {
                in.push_back(med_span(c->dU[b] + (long long)(first_pair + k) * c->plane, (size_t)c->P * 4, (size_t)W * 4, H));
                in.push_back(med_span(c->dV[b] + (long long)(first_pair + k) * c->plane, (size_t)c->P * 4, (size_t)W * 4, H));
            }
        }
        if (f.links && f.link_capacity) out.push_back(med_span(f.links[k], 0, sizeof(hsflow_link_record) * (size_t)f.link_capacity, 1));
        if (f.side_a) out.push_back(med_span(f.side_a[k], 0, sizeof(hsflow_link_side) * (size_t)lp.cap_a, 1));
        if (f.side_b) out.push_back(med_span(f.side_b[k], 0, sizeof(hsflow_link_side) * (size_t)lp.cap_b, 1));
    }
    out.push_back(med_span(f.results, 0, sizeof(hsflow_link_result) * (size_t)f.n, 1));
    for (size_t a = 0; a < out.size(); a++) {
        for (const MedSpan &i : in)
            if (med_overlap(out[a], i)) return fail(c, HSFLOW_E_ARG, "an output of the linking may not overlap an input");
        for (size_t b = a + 1; b < out.size(); b++)
            if (med_overlap(out[a], out[b])) return fail(c, HSFLOW_E_ARG, "the outputs of the linking may not overlap one another");
    }
    return HSFLOW_OK;
}

// The steps of one set of launches: min(8, 2^24 / cells), at least 1 -- the tables of a set stay within 64 MiB of cells.
int link_chunk(const hsflow_link_params &lp)
{
    const uint32_t fit = hsln::kMaxCells / (lp.cap_a * lp.cap_b);
    return fit < 1u ? 1 : fit < (uint32_t)hsk::kLnBatchMax ? (int)fit : hsk::kLnBatchMax;
}

// The kernels' scratch for n steps.  Allocated by the first call, grown, kept; k_ln_clear zeroes the tables of every call.
int link_scratch(hsflow_ctx *c, int n, const hsflow_link_params &lp, hsk::LnPlanes *pl)
{
    hsflow_ctx::LinkScratch &g = c->link;
    const hsln::Table t = hsln::table_of(lp.cap_a, lp.cap_b);
    const size_t n_tab = t.words(), n_counts = ((size_t)t.cells + 255) / 256, n_aux = (size_t)hsk::ln_aux_words(lp.cap_a, lp.cap_b);
    const size_t bytes = (n_tab + n_counts + n_aux) * 4 * (size_t)n;
    if (g.bytes < bytes) {
        hipFree(g.scr); // (holds until the device is idle: an earlier call may still be using the tables)
        g.scr = nullptr; g.bytes = 0;
        HS_HIP(c, hipMalloc(&g.scr, bytes));
        g.bytes = bytes;
    }
    uint32_t *base = (uint32_t *)g.scr;
    pl->tab = base;
    pl->counts = base + n_tab * (size_t)n;
    pl->aux = pl->counts + n_counts * (size_t)n;
    pl->n_tab = (long long)n_tab; pl->n_counts = (long long)n_counts; pl->n_aux = (long long)n_aux;
    return HSFLOW_OK;
}

// The launches of a call.  All pointers are device memory; the caller has checked every argument and, for the context's own
// flows, settled an owed check.
int enqueue_link(hsflow_ctx *c, const LnSteps &f, const hsflow_link_params &lp, int first_pair)
{
    const int most = link_chunk(lp), chunk = f.n < most ? f.n : most;
    hsk::LnPlanes pl{};
    const int st = link_scratch(c, chunk, lp, &pl);
    if (st) return st;
    pl.W = c->W; pl.H = c->H;
    pl.as = (long long)f.as; pl.bs = (long long)f.bs; pl.fs = f.u ? (long long)f.fs : (long long)c->P * 4;
    pl.cap_a = lp.cap_a; pl.cap_b = lp.cap_b; pl.link_capacity = f.link_capacity;
    for (int first = 0; first < f.n; first += chunk) {
        const int cnt = f.n - first < chunk ? f.n - first : chunk;
        for (int k = 0; k < hsk::kLnBatchMax; k++) {
            const int i = first + k;
            const bool on = k < cnt;
            pl.a[k] = on ? (const int32_t *)f.a[i] : nullptr;
            pl.b[k] = on ? (const int32_t *)f.b[i] : nullptr;
            pl.u[k] = !on ? nullptr : f.u ? (const float *)f.u[i] : c->dU[c->cur] + (long long)(first_pair + i) * c->plane;
            pl.v[k] = !on ? nullptr : f.u ? (const float *)f.v[i] : c->dV[c->cur] + (long long)(first_pair + i) * c->plane;
            pl.links[k] = on && f.links && f.link_capacity ? (hsln::Link *)f.links[i] : nullptr;
            pl.side_a[k] = on && f.side_a ? (hsln::Side *)f.side_a[i] : nullptr;
            pl.side_b[k] = on && f.side_b ? (hsln::Side *)f.side_b[i] : nullptr;
            pl.results[k] = on && f.results ? (hsln::Result *)f.results + i : nullptr;
        }
        // every voting workgroup ends in atomics on its step's table: several rows per workgroup, as the statistics kernels
        dim3 vote;
        stats_rows(c, (c->W + 255) / 256, c->H, cnt, true, &vote);
        c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
        HS_HIP(c, hsk::launch_link(c->stream, pl, cnt, vote));
    }
    return HSFLOW_OK;
}

int link_stage(hsflow_ctx *c, int slot, size_t bytes) { return stage_reserve(c, &c->link.stage[slot], &c->link.stage_bytes[slot], bytes); }

void link_release(hsflow_ctx *c)
{
    hipFree(c->link.scr);
    for (uint8_t *p : c->link.stage) hipFree(p);
    stats_release(c->link.dRes, c->link.hRes);
    c->link = hsflow_ctx::LinkScratch();
}

} // namespace

extern "C" {

void hsflow_default_link_params(hsflow_link_params *lp)
{
    if (!lp) return;
    std::memset(lp, 0, sizeof(*lp));
    lp->struct_size = sizeof(*lp);
    lp->cap_a = 64;
    lp->cap_b = 64;
}

int hsflow_link_regions_host(const int32_t *labels_a, size_t stride_a, const int32_t *labels_b, size_t stride_b, const float *u, const float *v, size_t flow_stride,
                             int width, int height, const hsflow_link_params *lp, hsflow_link_record *links, uint32_t link_capacity, hsflow_link_side *side_a,
                             hsflow_link_side *side_b, hsflow_link_result *result)
{
    int st = check_link_params(nullptr, lp, link_capacity);
    if (st) return st;
    if ((st = check_regions_size(nullptr, width, height))) return st;
    if (!u || !v) return fail(nullptr, HSFLOW_E_ARG, "null flow plane");
    const void *const pa[1] = {labels_a}, *const pb[1] = {labels_b}, *const pu[1] = {u}, *const pv[1] = {v};
    void *const pk[1] = {links}, *const psa[1] = {side_a}, *const psb[1] = {side_b};
    const LnSteps f = {1, pa, pb, stride_a, stride_b, pu, pv, flow_stride, links ? pk : nullptr, link_capacity, side_a ? psa : nullptr, side_b ? psb : nullptr, result};
    if ((st = check_link_steps(nullptr, f, width))) return st;
    if ((st = check_link_overlap(nullptr, f, *lp, -1, width, height))) return st;
    const hsln::Step step = {labels_a, stride_a, labels_b, stride_b, u, v, flow_stride, width, height};
    hsln::link_rows(step, lp->cap_a, lp->cap_b, (hsln::Link *)links, link_capacity, (hsln::Side *)side_a, (hsln::Side *)side_b, (hsln::Result *)result);
    return HSFLOW_OK;
}

int hsflow_link_regions_planes_device(hsflow_ctx *c, const void *d_labels_a, size_t stride_a, const void *d_labels_b, size_t stride_b, const void *d_u,
                                      const void *d_v, size_t flow_stride, const hsflow_link_params *lp, hsflow_link_record *d_links, uint32_t link_capacity,
                                      hsflow_link_side *d_side_a, hsflow_link_side *d_side_b, hsflow_link_result *d_result)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_link_params(c, lp, link_capacity))) return st;
    if ((st = check_regions_size(c, c->W, c->H))) return st;
    if (!d_u || !d_v) return fail(c, HSFLOW_E_ARG, "null flow plane");
    const void *const pa[1] = {d_labels_a}, *const pb[1] = {d_labels_b}, *const pu[1] = {d_u}, *const pv[1] = {d_v};
    void *const pk[1] = {d_links}, *const psa[1] = {d_side_a}, *const psb[1] = {d_side_b};
    const LnSteps f = {1, pa, pb, stride_a, stride_b, pu, pv, flow_stride, d_links ? pk : nullptr, link_capacity, d_side_a ? psa : nullptr, d_side_b ? psb : nullptr,
                       d_result};
    if ((st = check_link_steps(c, f, c->W))) return st;
    if ((st = check_link_overlap(c, f, *lp, -1, c->W, c->H))) return st;
    if ((st = settle_pending(c))) return st;
    return enqueue_link(c, f, *lp, 0);
}

int hsflow_link_regions_batch_device(hsflow_ctx *c, int first_pair, int n_steps, const void *const *d_labels, size_t labels_stride, const hsflow_link_params *lp,
                                     void *const *d_links, uint32_t link_capacity, void *const *d_side_a, void *const *d_side_b, hsflow_link_result *d_results)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_batch_pairs(c, first_pair, n_steps))) return st;
    if ((st = check_link_params(c, lp, link_capacity))) return st;
    if ((st = check_regions_size(c, c->W, c->H))) return st;
    if (!d_labels) return fail(c, HSFLOW_E_ARG, "null list of label planes");
    const LnSteps f = {n_steps, d_labels, d_labels + 1, labels_stride, labels_stride, nullptr, nullptr, 0, d_links, link_capacity, d_side_a, d_side_b, d_results};
    if ((st = check_link_steps(c, f, c->W))) return st;
    if ((st = check_link_overlap(c, f, *lp, first_pair, c->W, c->H))) return st;
    if ((st = settle_pending(c))) return st; // (hs_postops.hip.h, rule 1, before c->cur is named)
    return enqueue_link(c, f, *lp, first_pair);
}

int hsflow_link_regions_device(hsflow_ctx *c, int pair, const void *d_labels_a, const void *d_labels_b, size_t labels_stride, const hsflow_link_params *lp,
                               hsflow_link_record *d_links, uint32_t link_capacity, hsflow_link_side *d_side_a, hsflow_link_side *d_side_b,
                               hsflow_link_result *d_result)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    const void *const pl[2] = {d_labels_a, d_labels_b};
    void *const pk[1] = {d_links}, *const psa[1] = {d_side_a}, *const psb[1] = {d_side_b};
    return hsflow_link_regions_batch_device(c, pair, 1, pl, labels_stride, lp, d_links ? pk : nullptr, link_capacity, d_side_a ? psa : nullptr,
                                            d_side_b ? psb : nullptr, d_result);
}

int hsflow_link_regions(hsflow_ctx *c, int pair, const int32_t *labels_a, size_t stride_a, const int32_t *labels_b, size_t stride_b, const hsflow_link_params *lp,
                        hsflow_link_record *links, uint32_t link_capacity, hsflow_link_side *side_a, hsflow_link_side *side_b, hsflow_link_result *result)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = check_link_params(c, lp, link_capacity))) return st;
    if ((st = check_regions_size(c, c->W, c->H))) return st;
    {
        const void *const pa[1] = {labels_a}, *const pb[1] = {labels_b};
        void *const pk[1] = {links}, *const psa[1] = {side_a}, *const psb[1] = {side_b};
        const LnSteps h = {1, pa, pb, stride_a, stride_b, nullptr, nullptr, 0, links ? pk : nullptr, link_capacity, side_a ? psa : nullptr, side_b ? psb : nullptr, result};
        if ((st = check_link_steps(c, h, c->W))) return st;
    }
    if ((st = settle_pending(c))) return st;
    const bool want_links = links && link_capacity;
    const size_t lrow = (size_t)c->W * 4, kbytes = sizeof(hsflow_link_record) * (size_t)link_capacity;
    const size_t abytes = sizeof(hsflow_link_side) * (size_t)lp->cap_a, bbytes = sizeof(hsflow_link_side) * (size_t)lp->cap_b;
    hsflow_ctx::LinkScratch &g = c->link;
    if ((st = link_stage(c, 0, lrow * c->H)) || (st = link_stage(c, 1, lrow * c->H))) return st;
    if (want_links && (st = link_stage(c, 2, kbytes))) return st;
    if (side_a && (st = link_stage(c, 3, abytes))) return st;
    if (side_b && (st = link_stage(c, 4, bbytes))) return st;
    // (the header tells how many links were written: it is always taken)
    if ((st = stats_reserve(c, (void **)&g.dRes, (void **)&g.hRes))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    HS_HIP(c, copy_rows_async(c, g.stage[0], lrow, labels_a, stride_a, lrow, c->H, hipMemcpyHostToDevice));
    HS_HIP(c, copy_rows_async(c, g.stage[1], lrow, labels_b, stride_b, lrow, c->H, hipMemcpyHostToDevice));
    const void *const pa[1] = {g.stage[0]}, *const pb[1] = {g.stage[1]};
    void *const pk[1] = {g.stage[2]}, *const psa[1] = {g.stage[3]}, *const psb[1] = {g.stage[4]};
    const LnSteps f = {1, pa, pb, lrow, lrow, nullptr, nullptr, 0, want_links ? pk : nullptr, link_capacity, side_a ? psa : nullptr, side_b ? psb : nullptr, g.dRes};
    if ((st = enqueue_link(c, f, *lp, pair))) return st;
    if (side_a) HS_HIP(c, hipMemcpyAsync(side_a, g.stage[3], abytes, hipMemcpyDeviceToHost, c->stream));
    if (side_b) HS_HIP(c, hipMemcpyAsync(side_b, g.stage[4], bbytes, hipMemcpyDeviceToHost, c->stream));
    if ((st = stats_copy_back(c, g.hRes, g.dRes))) return st;
    if (want_links) {
        // only the links that were written cross: the rest of the caller's array stays as it is
        if ((st = sync_wait(c))) return st;
        const size_t written = g.hRes->n_written;
        if (written) HS_HIP(c, hipMemcpyAsync(links, g.stage[2], sizeof(hsflow_link_record) * written, hipMemcpyDeviceToHost, c->stream));
    }
    return sync_finish(c, marked, result, g.hRes);
}

int hsflow_link_tracks_host(const hsflow_link_side *const *side_a, const hsflow_link_side *const *side_b, const uint32_t *n_regions, int n_steps, uint32_t cap,
                            uint32_t min_share_256, uint32_t *ids, uint32_t *n_tracks)
{
    if (n_steps < 0 || !n_regions || !ids) return fail(nullptr, HSFLOW_E_ARG, "link tracks: n_steps below 0, or null n_regions or ids");
    if (cap < 1u) return fail(nullptr, HSFLOW_E_ARG, "link tracks: cap must be at least 1");
    if (cap > hsln::kMaxCap) return fail(nullptr, HSFLOW_E_SIZE, "link tracks: a cap above 2^30");
    if (min_share_256 > 256u) return fail(nullptr, HSFLOW_E_ARG, "link tracks: min_share_256 is 0 .. 256");
    if (n_steps > 0 && (!side_a || !side_b)) return fail(nullptr, HSFLOW_E_ARG, "link tracks: null list of side records");
    for (int i = 0; i < n_steps; i++)
        if (!side_a[i] || !side_b[i]) return fail(nullptr, HSFLOW_E_ARG, "link tracks: null side records of step " + std::to_string(i));
    const uint32_t n = hsln::link_tracks((const hsln::Side *const *)side_a, (const hsln::Side *const *)side_b, n_regions, n_steps, cap, min_share_256, ids);
    if (n_tracks) *n_tracks = n;
    return HSFLOW_OK;
}

} // extern "C"
