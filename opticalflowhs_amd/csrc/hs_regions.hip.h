// hs_regions.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_regions*, the connected regions of
// a foreground mask -- the moving objects -- labelled and measured where mask and flow lie (hs_regions_rule.h).  The engine
// works on planes (enqueue_regions); the forms on a context's pairs hand it the context's flow.  Per chunk of at most
// hsk::kRgBatchMax fields one fixed sequence of launches (hsk::launch_regions), no memset, no wait.  On top of
// hs_postops.hip.h: its three ordering rules hold word for word.  A context that never labels allocates and launches
// nothing here.
#pragma once

namespace {

static_assert(sizeof(hsflow_regions_result) == 64 && sizeof(hsflow_regions_result) == sizeof(hsrg::Result) && sizeof(hsflow_regions_result) == kStatsBytes,
              "hsflow_regions_result is 64 bytes on both sides");
static_assert(sizeof(hsflow_regions_record) == 64 && sizeof(hsflow_regions_record) == sizeof(hsrg::Record), "hsflow_regions_record is 64 bytes on both sides");
static_assert(offsetof(hsflow_regions_record, x0) == 8 && offsetof(hsflow_regions_record, sum_x) == 16 && offsetof(hsflow_regions_record, n_flow) == 32 &&
                  offsetof(hsflow_regions_record, sum_qu) == 40 && offsetof(hsflow_regions_record, reserved1) == 56,
              "hsflow_regions_record: the kernel's layout");
static_assert(offsetof(hsflow_regions_result, fg_px) == 16 && offsetof(hsflow_regions_result, largest_area) == 40, "hsflow_regions_result: the kernel's layout");
static_assert(sizeof(hsflow_regions_params) == 32, "hsflow_regions_params is 32 bytes");
static_assert(HSFLOW_REGIONS_MAX_SIDE == hsrg::kMaxSide && HSFLOW_REGIONS_FLAG_OVERFLOW == hsrg::kFlagOverflow, "the header's constants are the rule's");

int check_regions_params(hsflow_ctx *c, const hsflow_regions_params *rp, hsrg::Rule *rule)
{
    if (!rp || rp->struct_size != sizeof(hsflow_regions_params)) return fail(c, HSFLOW_E_ARG, "regions params null or struct_size mismatch");
    if (rp->reserved[0] || rp->reserved[1]) return fail(c, HSFLOW_E_ARG, "regions params: reserved fields must be 0");
    if (rp->connectivity != 4 && rp->connectivity != 8) return fail(c, HSFLOW_E_ARG, "regions connectivity must be 4 or 8");
    if (rp->fg_lo < 0 || rp->fg_hi > 255 || rp->fg_lo > rp->fg_hi) return fail(c, HSFLOW_E_ARG, "regions fg_lo .. fg_hi must be a range inside 0 .. 255");
    if (rp->min_area < 1u) return fail(c, HSFLOW_E_ARG, "regions min_area must be at least 1");
    const float thr = rp->join_px * rp->join_px;
    if (!(std::isfinite(rp->join_px) && rp->join_px >= 0.0f && std::isfinite(thr))) return fail(c, HSFLOW_E_ARG, "regions join_px and its square must be finite and not negative");
    if (rp->join_px > 0.0f && !(thr > 0.0f)) return fail(c, HSFLOW_E_ARG, "regions join_px above 0 whose square is 0");
    *rule = hsrg::Rule{rp->connectivity, (unsigned)rp->fg_lo, (unsigned)rp->fg_hi, rp->min_area, thr};
    return HSFLOW_OK;
}

int check_regions_size(hsflow_ctx *c, int W, int H)
{
    if (W < 1 || H < 1) return fail(c, HSFLOW_E_SIZE, "regions: width and height must be positive");
    if (W > HSFLOW_REGIONS_MAX_SIDE || H > HSFLOW_REGIONS_MAX_SIDE || (long long)W * H > hsrg::kMaxPixels)
        return fail(c, HSFLOW_E_SIZE, "regions: a frame wider or higher than 16384, or of more than 2^30 pixels");
    return HSFLOW_OK;
}

// The fields of a call as the caller names them (host or device memory alike): n of each; the lists of masks, label planes
// and record arrays may be NULL and may hold NULL entries.
struct RgFields {
    int n;
    const void *const *mask;
    size_t ms;
    const void *const *u, *const *v; // NULL with own_flow: the context's pairs; NULL without: no flow
    bool own_flow;
    size_t fs;
    void *const *labels;
    size_t ls;
    void *const *records;
    uint32_t capacity;
    const void *results; // n headers, or NULL
};

int check_regions_fields(hsflow_ctx *c, const RgFields &f, const hsrg::Rule &rule, int W)
{
    bool asked = f.results != nullptr;
    if ((f.u != nullptr) != (f.v != nullptr)) return fail(c, HSFLOW_E_ARG, "the two flow planes are given together or not at all");
    if (rule.thr > 0.0f && !f.u && !f.own_flow) return fail(c, HSFLOW_E_ARG, "join_px above 0 needs the flow planes");
    if ((uint64_t)f.capacity > (uint64_t)hsrg::kMaxPixels) return fail(c, HSFLOW_E_SIZE, "a capacity above 2^30 records");
    for (int k = 0; k < f.n; k++) {
        const std::string who = "field " + std::to_string(k) + ": ";
        if (f.u) {
            if (!f.u[k] || !f.v[k]) return fail(c, HSFLOW_E_ARG, who + "null flow plane");
            if ((((uintptr_t)f.u[k] | (uintptr_t)f.v[k]) & 3u) != 0) return fail(c, HSFLOW_E_ARG, who + "the flow planes must be 4-byte aligned");
        }
        if (f.mask && f.mask[k] && f.ms < (size_t)W) return fail(c, HSFLOW_E_SIZE, "mask stride smaller than width");
        if (f.labels && f.labels[k]) {
            asked = true;
            if (((uintptr_t)f.labels[k] & 3u) != 0) return fail(c, HSFLOW_E_ARG, who + "the label plane must be 4-byte aligned");
            if (f.ls < (size_t)W * 4 || (f.ls & 3u)) return fail(c, HSFLOW_E_SIZE, "labels stride smaller than 4*width or no multiple of 4");
        }
        if (f.records && f.records[k]) {
            asked = true;
            if (((uintptr_t)f.records[k] & 7u) != 0) return fail(c, HSFLOW_E_ARG, who + "the records must be 8-byte aligned");
        }
    }
    if (f.u && (f.fs < (size_t)W * 4 || (f.fs & 3u))) return fail(c, HSFLOW_E_SIZE, "flow stride smaller than 4*width or no multiple of 4");
    if (((uintptr_t)f.results & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the result headers must be 8-byte aligned");
    if (!asked) return fail(c, HSFLOW_E_ARG, "neither labels nor records nor a result asked for");
    return HSFLOW_OK;
}

// No output may overlap an input or another output (first_pair >= 0: the context's flows of the pairs, in both buffers of
// the ping-pong).
int check_regions_overlap(hsflow_ctx *c, const RgFields &f, int first_pair, int W, int H)
{
    std::vector<MedSpan> in, out;
    for (int k = 0; k < f.n; k++) {
        if (f.u) {
            in.push_back(med_span(f.u[k], f.fs, (size_t)W * 4, H));
            in.push_back(med_span(f.v[k], f.fs, (size_t)W * 4, H));
        } else if (f.own_flow) {
            for (int b = 0; b < 2; b++) {
                in.push_back(med_span(c->dU[b] + (long long)(first_pair + k) * c->plane, (size_t)c->P * 4, (size_t)W * 4, H));
                in.push_back(med_span(c->dV[b] + (long long)(first_pair + k) * c->plane, (size_t)c->P * 4, (size_t)W * 4, H));
            }
        }
        if (f.mask) in.push_back(med_span(f.mask[k], f.ms, (size_t)W, H));
        if (f.labels) out.push_back(med_span(f.labels[k], f.ls, (size_t)W * 4, H));
        if (f.records && f.capacity) out.push_back(med_span(f.records[k], 0, sizeof(hsflow_regions_record) * (size_t)f.capacity, 1));
    }
    out.push_back(med_span(f.results, 0, sizeof(hsflow_regions_result) * (size_t)f.n, 1));
    for (size_t a = 0; a < out.size(); a++) {
        for (const MedSpan &i : in)
            if (med_overlap(out[a], i)) return fail(c, HSFLOW_E_ARG, "an output of the labelling may not overlap an input");
        for (size_t b = a + 1; b < out.size(); b++)
            if (med_overlap(out[a], out[b])) return fail(c, HSFLOW_E_ARG, "the outputs of the labelling may not overlap one another");
    }
    return HSFLOW_OK;
}

// The kernels' scratch for n fields of the context's size: per field a parent and an area plane and the scan's counts, then
// the RgAcc records.  Allocated by the first call, grown, kept; no call reads a word it has not written itself.
int regions_scratch(hsflow_ctx *c, int n, hsk::RgPlanes *pl)
{
    hsflow_ctx::RegionsScratch &g = c->regions;
    const size_t plane = (size_t)c->W * c->H, counts = (size_t)((c->W + 255) / 256) * c->H;
    const size_t words = (2 * plane + counts) * (size_t)n, bytes = words * 4 + sizeof(hsk::RgAcc) * (size_t)hsk::kRgBatchMax + 8;
    if (g.bytes < bytes) {
        hipFree(g.scr); // (holds until the device is idle: an earlier call may still be using the planes)
        g.scr = nullptr; g.bytes = 0;
        HS_HIP(c, hipMalloc(&g.scr, bytes));
        g.bytes = bytes;
    }
    uint32_t *base = (uint32_t *)g.scr;
    pl->parent = base;
    pl->area = base + plane * (size_t)n;
    pl->counts = base + 2 * plane * (size_t)n;
    pl->acc = (hsk::RgAcc *)(((uintptr_t)(base + words) + 7u) & ~(uintptr_t)7u);
    pl->plane = (long long)plane;
    pl->n_counts = (long long)counts;
    return HSFLOW_OK;
}

// The launches of a call.  All pointers are device memory; the caller has checked every argument and, for the context's own
// flows, settled an owed check.
int enqueue_regions(hsflow_ctx *c, const RgFields &f, int first_pair, const hsrg::Rule &rule)
{
    const int chunk = f.n < hsk::kRgBatchMax ? f.n : hsk::kRgBatchMax;
    hsk::RgPlanes pl{};
    const int st = regions_scratch(c, chunk, &pl);
    if (st) return st;
    pl.W = c->W; pl.H = c->H;
    pl.ms = (long long)f.ms; pl.fs = f.u ? (long long)f.fs : (long long)c->P * 4; pl.ls = (long long)f.ls;
    pl.capacity = f.capacity;
    pl.lo = rule.lo; pl.hi = rule.hi; pl.min_area = rule.min_area; pl.conn = rule.conn; pl.thr = rule.thr;
    for (int first = 0; first < f.n; first += chunk) {
        const int cnt = f.n - first < chunk ? f.n - first : chunk;
        for (int k = 0; k < hsk::kRgBatchMax; k++) {
            const int i = first + k;
            const bool on = k < cnt;
            pl.mask[k] = on && f.mask ? (const uint8_t *)f.mask[i] : nullptr;
            pl.u[k] = !on ? nullptr : f.u ? (const float *)f.u[i] : f.own_flow ? c->dU[c->cur] + (long long)(first_pair + i) * c->plane : nullptr;
            pl.v[k] = !on ? nullptr : f.u ? (const float *)f.v[i] : f.own_flow ? c->dV[c->cur] + (long long)(first_pair + i) * c->plane : nullptr;
            pl.labels[k] = on && f.labels ? (int32_t *)f.labels[i] : nullptr;
            pl.records[k] = on && f.records && f.capacity ? (hsrg::Record *)f.records[i] : nullptr;
            pl.results[k] = on && f.results ? (hsrg::Result *)f.results + i : nullptr;
        }
        c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
        HS_HIP(c, hsk::launch_regions(c->stream, pl, cnt));
    }
    return HSFLOW_OK;
}

int regions_stage(hsflow_ctx *c, int slot, size_t bytes) { return stage_reserve(c, &c->regions.stage[slot], &c->regions.stage_bytes[slot], bytes); }

void regions_release(hsflow_ctx *c)
{
    hipFree(c->regions.scr);
    for (uint8_t *p : c->regions.stage) hipFree(p);
    stats_release(c->regions.dRes, c->regions.hRes);
    c->regions = hsflow_ctx::RegionsScratch();
}

} // namespace

extern "C" {

void hsflow_default_regions_params(hsflow_regions_params *rp)
{
    if (!rp) return;
    std::memset(rp, 0, sizeof(*rp));
    rp->struct_size = sizeof(*rp);
    rp->connectivity = 8;
    rp->fg_lo = 1;
    rp->fg_hi = 255;
    rp->min_area = 1;
    rp->join_px = 0.0f;
}

int hsflow_regions_host(const uint8_t *mask, size_t mask_stride, const float *u, const float *v, size_t flow_stride, int width, int height,
                        const hsflow_regions_params *rp, int32_t *labels, size_t labels_stride, hsflow_regions_record *records, uint32_t capacity,
                        hsflow_regions_result *result)
{
    hsrg::Rule rule;
    int st = check_regions_params(nullptr, rp, &rule);
    if (st) return st;
    if ((st = check_regions_size(nullptr, width, height))) return st;
    if ((u != nullptr) != (v != nullptr)) return fail(nullptr, HSFLOW_E_ARG, "the two flow planes are given together or not at all");
    const void *const pm[1] = {mask}, *const pu[1] = {u}, *const pv[1] = {v};
    void *const pl[1] = {labels}, *const pr[1] = {records};
    const RgFields f = {1, mask ? pm : nullptr, mask_stride, u ? pu : nullptr, u ? pv : nullptr, false, flow_stride, labels ? pl : nullptr, labels_stride,
                        records ? pr : nullptr, capacity, result};
    if ((st = check_regions_fields(nullptr, f, rule, width))) return st;
    if ((st = check_regions_overlap(nullptr, f, -1, width, height))) return st;
    const hsrg::Field field = {mask, mask_stride, u, v, flow_stride, width, height};
    hsrg::label_rows(field, rule, labels, labels_stride, (hsrg::Record *)records, capacity, (hsrg::Result *)result);
    return HSFLOW_OK;
}

int hsflow_regions_planes_device(hsflow_ctx *c, const void *d_mask, size_t mask_stride, const void *d_u, const void *d_v, size_t flow_stride,
                                 const hsflow_regions_params *rp, void *d_labels, size_t labels_stride, hsflow_regions_record *d_records, uint32_t capacity,
                                 hsflow_regions_result *d_result)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    hsrg::Rule rule;
    if ((st = check_regions_params(c, rp, &rule))) return st;
    if ((st = check_regions_size(c, c->W, c->H))) return st;
    if ((d_u != nullptr) != (d_v != nullptr)) return fail(c, HSFLOW_E_ARG, "the two flow planes are given together or not at all");
    const void *const pm[1] = {d_mask}, *const pu[1] = {d_u}, *const pv[1] = {d_v};
    void *const pl[1] = {d_labels}, *const pr[1] = {d_records};
    const RgFields f = {1, d_mask ? pm : nullptr, mask_stride, d_u ? pu : nullptr, d_u ? pv : nullptr, false, flow_stride, d_labels ? pl : nullptr, labels_stride,
                        d_records ? pr : nullptr, capacity, d_result};
    if ((st = check_regions_fields(c, f, rule, c->W))) return st;
    if ((st = check_regions_overlap(c, f, -1, c->W, c->H))) return st;
    if ((st = settle_pending(c))) return st;
    return enqueue_regions(c, f, 0, rule);
}

int hsflow_regions_batch_device(hsflow_ctx *c, int first_pair, int n, const void *const *d_mask, size_t mask_stride, const hsflow_regions_params *rp,
                                void *const *d_labels, size_t labels_stride, void *const *d_records, uint32_t capacity, hsflow_regions_result *d_results)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_batch_pairs(c, first_pair, n))) return st;
    hsrg::Rule rule;
    if ((st = check_regions_params(c, rp, &rule))) return st;
    if ((st = check_regions_size(c, c->W, c->H))) return st;
    const RgFields f = {n, d_mask, mask_stride, nullptr, nullptr, true, 0, d_labels, labels_stride, d_records, capacity, d_results};
    if ((st = check_regions_fields(c, f, rule, c->W))) return st;
    if ((st = check_regions_overlap(c, f, first_pair, c->W, c->H))) return st;
    if ((st = settle_pending(c))) return st; // (hs_postops.hip.h, rule 1, before c->cur is named)
    return enqueue_regions(c, f, first_pair, rule);
}

int hsflow_regions_device(hsflow_ctx *c, int pair, const void *d_mask, size_t mask_stride, const hsflow_regions_params *rp, void *d_labels, size_t labels_stride,
                          hsflow_regions_record *d_records, uint32_t capacity, hsflow_regions_result *d_result)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    const void *const pm[1] = {d_mask};
    void *const pl[1] = {d_labels}, *const pr[1] = {d_records};
    return hsflow_regions_batch_device(c, pair, 1, d_mask ? pm : nullptr, mask_stride, rp, d_labels ? pl : nullptr, labels_stride, d_records ? pr : nullptr, capacity,
                                       d_result);
}

int hsflow_regions(hsflow_ctx *c, int pair, const uint8_t *mask, size_t mask_stride, const hsflow_regions_params *rp, int32_t *labels, size_t labels_stride,
                   hsflow_regions_record *records, uint32_t capacity, hsflow_regions_result *result)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    hsrg::Rule rule;
    if ((st = check_regions_params(c, rp, &rule))) return st;
    if ((st = check_regions_size(c, c->W, c->H))) return st;
    {
        const void *const pm[1] = {mask};
        void *const pl[1] = {labels}, *const pr[1] = {records};
        const RgFields h = {1, mask ? pm : nullptr, mask_stride, nullptr, nullptr, true, 0, labels ? pl : nullptr, labels_stride, records ? pr : nullptr, capacity, result};
        if ((st = check_regions_fields(c, h, rule, c->W))) return st;
    }
    if ((st = settle_pending(c))) return st;
    const bool want_records = records && capacity;
    const size_t brow = (size_t)c->W, lrow = (size_t)c->W * 4, rbytes = sizeof(hsflow_regions_record) * (size_t)capacity;
    hsflow_ctx::RegionsScratch &g = c->regions;
    if (mask && (st = regions_stage(c, 0, brow * c->H))) return st;
    if (labels && (st = regions_stage(c, 1, lrow * c->H))) return st;
    if (want_records && (st = regions_stage(c, 2, rbytes))) return st;
    // (the header tells how many records were written: it is always taken)
    if ((st = stats_reserve(c, (void **)&g.dRes, (void **)&g.hRes))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    if (mask) HS_HIP(c, copy_rows_async(c, g.stage[0], brow, mask, mask_stride, brow, c->H, hipMemcpyHostToDevice));
    const void *const pm[1] = {g.stage[0]};
    void *const pl[1] = {g.stage[1]}, *const pr[1] = {g.stage[2]};
    const RgFields f = {1, mask ? pm : nullptr, brow, nullptr, nullptr, true, 0, labels ? pl : nullptr, lrow, want_records ? pr : nullptr, capacity, g.dRes};
    if ((st = enqueue_regions(c, f, pair, rule))) return st;
    if (labels) HS_HIP(c, copy_rows_async(c, labels, labels_stride, g.stage[1], lrow, lrow, c->H, hipMemcpyDeviceToHost));
    if ((st = stats_copy_back(c, g.hRes, g.dRes))) return st;
    if (want_records) {
        // only the records that were written cross: the rest of the caller's array stays as it is
        if ((st = sync_wait(c))) return st;
        const size_t written = g.hRes->n_written;
        if (written) HS_HIP(c, hipMemcpyAsync(records, g.stage[2], sizeof(hsflow_regions_record) * written, hipMemcpyDeviceToHost, c->stream));
    }
    return sync_finish(c, marked, result, g.hRes);
}

} // extern "C"
