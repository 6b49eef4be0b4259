// hs_corners.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_corners*, the corners of a gray
// frame -- the points worth following -- found where the frames lie (hs_corners_rule.h).  The engine works on planes
// (enqueue_corners); the forms on a context's pairs hand it the context's own pre-processed planes.  Per chunk of at most
// hsk::kCnBatchMax fields one memset of the accumulators and one fixed sequence of launches (hsk::launch_corners), no wait.
// On top of hs_postops.hip.h: its three ordering rules hold word for word.  A context that never asks for corners allocates
// and launches nothing here.
#pragma once

namespace {

static_assert(sizeof(hsflow_corners_result) == 64 && sizeof(hsflow_corners_result) == sizeof(hscn::Result) && sizeof(hsflow_corners_result) == kStatsBytes,
              "hsflow_corners_result is 64 bytes on both sides");
static_assert(sizeof(hsflow_corners_record) == 16 && sizeof(hsflow_corners_record) == sizeof(hscn::Record), "hsflow_corners_record is 16 bytes on both sides");
static_assert(offsetof(hsflow_corners_record, index) == 4 && offsetof(hsflow_corners_record, score) == 8, "hsflow_corners_record: the kernel's layout");
static_assert(offsetof(hsflow_corners_result, smax) == 16 && offsetof(hsflow_corners_result, allowed_px) == 32, "hsflow_corners_result: the kernel's layout");
static_assert(sizeof(hsflow_corners_params) == 64 && offsetof(hsflow_corners_params, min_score) == 40, "hsflow_corners_params is 64 bytes");
static_assert(HSFLOW_CORNERS_MAX_SIDE == hscn::kMaxSide && HSFLOW_CORNERS_MAX_CANDIDATES == hscn::kMaxCandidates && HSFLOW_CORNERS_MAX_CAPACITY == hscn::kMaxCapacity &&
                  HSFLOW_CORNERS_FLAG_OVERFLOW == hscn::kFlagOverflow && HSFLOW_CORNERS_FLAG_TRUNCATED == hscn::kFlagTruncated &&
                  HSFLOW_CORNERS_MIN_EIGEN == hscn::kMinEigen && HSFLOW_CORNERS_HARRIS == hscn::kHarris,
              "the header's constants are the rule's");

int check_corners_params(hsflow_ctx *c, const hsflow_corners_params *cp, hscn::Rule *rule)
{
    if (!cp || cp->struct_size != sizeof(hsflow_corners_params)) return fail(c, HSFLOW_E_ARG, "corners params null or struct_size mismatch");
    if (cp->reserved0 || cp->reserved[0] || cp->reserved[1]) return fail(c, HSFLOW_E_ARG, "corners params: reserved fields must be 0");
    if (cp->kind != HSFLOW_CORNERS_MIN_EIGEN && cp->kind != HSFLOW_CORNERS_HARRIS) return fail(c, HSFLOW_E_ARG, "corners kind must be MIN_EIGEN or HARRIS");
    if (cp->block_r < 1 || cp->block_r > hscn::kMaxBlockR) return fail(c, HSFLOW_E_ARG, "corners block_r must be 1 .. 3");
    if (cp->nms_r < 1 || cp->nms_r > hscn::kMaxNmsR) return fail(c, HSFLOW_E_ARG, "corners nms_r must be 1 .. 8");
    if (cp->quality_q16 > 65535u) return fail(c, HSFLOW_E_ARG, "corners quality_q16 must be 0 .. 65535");
    if (cp->border < 0) return fail(c, HSFLOW_E_ARG, "corners border must not be negative");
    if (cp->fg_lo < 0 || cp->fg_hi > 255 || cp->fg_lo > cp->fg_hi) return fail(c, HSFLOW_E_ARG, "corners fg_lo .. fg_hi must be a range inside 0 .. 255");
    if (cp->max_candidates < 1u || cp->max_candidates > hscn::kMaxCandidates) return fail(c, HSFLOW_E_ARG, "corners max_candidates must be 1 .. 65536");
    if (cp->min_score < 1) return fail(c, HSFLOW_E_ARG, "corners min_score must be at least 1");
    *rule = hscn::Rule{cp->kind, cp->block_r, cp->nms_r, cp->quality_q16, cp->border, (unsigned)cp->fg_lo, (unsigned)cp->fg_hi, cp->max_candidates, cp->min_score};
    return HSFLOW_OK;
}

int check_corners_size(hsflow_ctx *c, int W, int H)
{
    if (W < 1 || H < 1) return fail(c, HSFLOW_E_SIZE, "corners: width and height must be positive");
    if (W > HSFLOW_CORNERS_MAX_SIDE || H > HSFLOW_CORNERS_MAX_SIDE) return fail(c, HSFLOW_E_SIZE, "corners: a frame wider or higher than 16384");
    return HSFLOW_OK;
}

// The fields of a call as the caller names them (host or device memory alike): n of each; gray NULL: the context's own
// planes; the lists of masks, record and xy arrays may be NULL and may hold NULL entries.
struct CnFields {
    int n;
    const void *const *gray;
    size_t gs;
    const void *const *mask;
    size_t ms;
    void *const *records;
    uint32_t capacity;
    void *const *xy;
    const void *results; // n headers, or NULL
};

int check_corners_fields(hsflow_ctx *c, const CnFields &f, int W)
{
    bool asked = f.results != nullptr;
    if ((uint64_t)f.capacity > (uint64_t)hscn::kMaxCapacity) return fail(c, HSFLOW_E_SIZE, "a capacity above 2^24 corners");
    if (f.gray && f.gs < (size_t)W) return fail(c, HSFLOW_E_SIZE, "gray stride smaller than width");
    for (int k = 0; k < f.n; k++) {
        const std::string who = "field " + std::to_string(k) + ": ";
        if (f.gray && !f.gray[k]) return fail(c, HSFLOW_E_ARG, who + "null gray plane");
        if (f.mask && f.mask[k] && f.ms < (size_t)W) return fail(c, HSFLOW_E_SIZE, "mask stride smaller than width");
        if (f.records && f.records[k]) {
            asked = true;
            if (((uintptr_t)f.records[k] & 7u) != 0) return fail(c, HSFLOW_E_ARG, who + "the records must be 8-byte aligned");
        }
        if (f.xy && f.xy[k]) {
            asked = true;
            if (((uintptr_t)f.xy[k] & 3u) != 0) return fail(c, HSFLOW_E_ARG, who + "the xy array must be 4-byte aligned");
        }
    }
    if (((uintptr_t)f.results & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the result headers must be 8-byte aligned");
    if (!asked) return fail(c, HSFLOW_E_ARG, "neither records nor xy nor a result asked for");
    return HSFLOW_OK;
}

// No output may overlap an input or another output (first_pair >= 0: the context's frames of the pairs).
int check_corners_overlap(hsflow_ctx *c, const CnFields &f, int first_pair, int W, int H)
{
    std::vector<MedSpan> in, out;
    for (int k = 0; k < f.n; k++) {
        if (f.gray) in.push_back(med_span(f.gray[k], f.gs, (size_t)W, H));
        else if (first_pair >= 0) {
            in.push_back(med_span(c->dA + (long long)(first_pair + k) * c->plane, (size_t)c->P, (size_t)W, H));
            in.push_back(med_span(c->dB + (long long)(first_pair + k) * c->plane, (size_t)c->P, (size_t)W, H));
        }
        if (f.mask) in.push_back(med_span(f.mask[k], f.ms, (size_t)W, H));
        if (f.records && f.capacity) out.push_back(med_span(f.records[k], 0, sizeof(hsflow_corners_record) * (size_t)f.capacity, 1));
        if (f.xy && f.capacity) out.push_back(med_span(f.xy[k], 0, 8 * (size_t)f.capacity, 1));
    }
    out.push_back(med_span(f.results, 0, sizeof(hsflow_corners_result) * (size_t)f.n, 1));
    for (size_t a = 0; a < out.size(); a++) {
        for (const MedSpan &i : in)
            if (med_overlap(out[a], i)) return fail(c, HSFLOW_E_ARG, "an output of the corner detection may not overlap an input");
        for (size_t b = a + 1; b < out.size(); b++)
            if (med_overlap(out[a], out[b])) return fail(c, HSFLOW_E_ARG, "the outputs of the corner detection may not overlap one another");
    }
    return HSFLOW_OK;
}

// The kernels' scratch for n fields of the context's size: per field the score plane, the candidates, the ballot words and
// the offsets of the segments, then the CnAcc records.  Allocated by the first call, grown, kept.
int corners_scratch(hsflow_ctx *c, int n, hsk::CnPlanes *pl)
{
    hsflow_ctx::CornersScratch &g = c->corners;
    const size_t plane = (size_t)c->W * c->H, segs = (size_t)((c->W + hsk::kCnSegW - 1) / hsk::kCnSegW) * c->H;
    const size_t per_field = plane * 8 + sizeof(hsk::CnCand) * (size_t)hsk::kCnMaxCandidates + segs * 32 + ((segs * 4 + 7) & ~(size_t)7);
    const size_t bytes = per_field * (size_t)n + sizeof(hsk::CnAcc) * (size_t)hsk::kCnBatchMax;
    if (g.bytes < bytes) {
        hipFree(g.scr); // (holds until the device is idle: an earlier call may still be using the planes)
        g.scr = nullptr; g.bytes = 0;
        HS_HIP(c, hipMalloc(&g.scr, bytes));
        g.bytes = bytes;
    }
    uint8_t *p = (uint8_t *)g.scr;
    pl->score = (long long *)p; p += plane * 8 * (size_t)n;
    pl->cand = (hsk::CnCand *)p; p += sizeof(hsk::CnCand) * (size_t)hsk::kCnMaxCandidates * (size_t)n;
    pl->bits = (unsigned long long *)p; p += segs * 32 * (size_t)n;
    pl->offsets = (uint32_t *)p; p += ((segs * 4 + 7) & ~(size_t)7) * (size_t)n;
    pl->acc = (hsk::CnAcc *)p;
    pl->plane = (long long)plane;
    pl->n_segs = (long long)segs;
    return HSFLOW_OK;
}

// The launches of a call.  All pointers are device memory; the caller has checked every argument.  which: 0 the prev, 1 the
// curr plane of the context's pairs (f.gray NULL).
int enqueue_corners(hsflow_ctx *c, const CnFields &f, int first_pair, int which, const hscn::Rule &rule)
{
    const int chunk = f.n < hsk::kCnBatchMax ? f.n : hsk::kCnBatchMax;
    hsk::CnPlanes pl{};
    const int st = corners_scratch(c, chunk, &pl);
    if (st) return st;
    pl.W = c->W; pl.H = c->H;
    pl.gs = f.gray ? (long long)f.gs : (long long)c->P;
    pl.ms = (long long)f.ms;
    pl.capacity = f.capacity;
    pl.rule = rule;
    for (int first = 0; first < f.n; first += chunk) {
        const int cnt = f.n - first < chunk ? f.n - first : chunk;
        for (int k = 0; k < hsk::kCnBatchMax; k++) {
            const int i = first + k;
            const bool on = k < cnt;
            pl.gray[k] = !on ? nullptr : f.gray ? (const uint8_t *)f.gray[i] : (which ? c->dB : c->dA) + (long long)(first_pair + i) * c->plane;
            pl.mask[k] = on && f.mask ? (const uint8_t *)f.mask[i] : nullptr;
            pl.records[k] = on && f.records && f.capacity ? (hscn::Record *)f.records[i] : nullptr;
            pl.xy[k] = on && f.xy && f.capacity ? (float *)f.xy[i] : nullptr;
            pl.results[k] = on && f.results ? (hscn::Result *)f.results + i : nullptr;
        }
        c->last_marked = false; // (hs_postops.hip.h, rule 2)
        HS_HIP(c, hsk::launch_corners(c->stream, pl, cnt));
    }
    return HSFLOW_OK;
}

int corners_stage(hsflow_ctx *c, int slot, size_t bytes) { return stage_reserve(c, &c->corners.stage[slot], &c->corners.stage_bytes[slot], bytes); }

void corners_release(hsflow_ctx *c)
{
    hipFree(c->corners.scr);
    for (uint8_t *p : c->corners.stage) hipFree(p);
    stats_release(c->corners.dRes, c->corners.hRes);
    c->corners = hsflow_ctx::CornersScratch();
}

int check_corners_which(hsflow_ctx *c, int which)
{
    if (which != 0 && which != 1) return fail(c, HSFLOW_E_ARG, "corners: which must be 0 (prev) or 1 (curr)");
    if (!c->frames_set) return fail(c, HSFLOW_E_STATE, "frames were not set");
    return HSFLOW_OK;
}

} // namespace

extern "C" {

void hsflow_default_corners_params(hsflow_corners_params *cp)
{
    if (!cp) return;
    std::memset(cp, 0, sizeof(*cp));
    cp->struct_size = sizeof(*cp);
    cp->kind = HSFLOW_CORNERS_MIN_EIGEN;
    cp->block_r = 1;
    cp->nms_r = 3;
    cp->quality_q16 = 655;
    cp->border = 0;
    cp->fg_lo = 1;
    cp->fg_hi = 255;
    cp->max_candidates = HSFLOW_CORNERS_MAX_CANDIDATES;
    cp->min_score = 1;
}

int hsflow_corners_host(const uint8_t *gray, size_t stride, int width, int height, const uint8_t *mask, size_t mask_stride, const hsflow_corners_params *cp,
                        hsflow_corners_record *records, uint32_t capacity, float *xy, hsflow_corners_result *result)
{
    hscn::Rule rule;
    int st = check_corners_params(nullptr, cp, &rule);
    if (st) return st;
    if ((st = check_corners_size(nullptr, width, height))) return st;
    if (!gray) return fail(nullptr, HSFLOW_E_ARG, "null gray plane");
    const void *const pg[1] = {gray}, *const pm[1] = {mask};
    void *const pr[1] = {records}, *const px[1] = {xy};
    const CnFields f = {1, pg, stride, mask ? pm : nullptr, mask_stride, records ? pr : nullptr, capacity, xy ? px : nullptr, result};
    if ((st = check_corners_fields(nullptr, f, width))) return st;
    if ((st = check_corners_overlap(nullptr, f, -1, width, height))) return st;
    hscn::corners_rows(gray, stride, width, height, mask, mask_stride, rule, (hscn::Record *)records, capacity, xy, (hscn::Result *)result);
    return HSFLOW_OK;
}

int hsflow_corners_planes_device(hsflow_ctx *c, const void *d_gray, size_t stride, const void *d_mask, size_t mask_stride, const hsflow_corners_params *cp,
                                 hsflow_corners_record *d_records, uint32_t capacity, float *d_xy, hsflow_corners_result *d_result)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    hscn::Rule rule;
    if ((st = check_corners_params(c, cp, &rule))) return st;
    if ((st = check_corners_size(c, c->W, c->H))) return st;
    if (!d_gray) return fail(c, HSFLOW_E_ARG, "null gray plane");
    const void *const pg[1] = {d_gray}, *const pm[1] = {d_mask};
    void *const pr[1] = {d_records}, *const px[1] = {d_xy};
    const CnFields f = {1, pg, stride, d_mask ? pm : nullptr, mask_stride, d_records ? pr : nullptr, capacity, d_xy ? px : nullptr, d_result};
    if ((st = check_corners_fields(c, f, c->W))) return st;
    if ((st = check_corners_overlap(c, f, -1, c->W, c->H))) return st;
    if ((st = settle_pending(c))) return st;
    return enqueue_corners(c, f, 0, 0, rule);
}

int hsflow_corners_batch_device(hsflow_ctx *c, int first_pair, int n, int which, const void *const *d_mask, size_t mask_stride, const hsflow_corners_params *cp,
                                void *const *d_records, uint32_t capacity, void *const *d_xy, hsflow_corners_result *d_results)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_batch_pairs(c, first_pair, n))) return st;
    hscn::Rule rule;
    if ((st = check_corners_params(c, cp, &rule))) return st;
    if ((st = check_corners_size(c, c->W, c->H))) return st;
    if ((st = check_corners_which(c, which))) return st;
    const CnFields f = {n, nullptr, 0, d_mask, mask_stride, d_records, capacity, d_xy, d_results};
    if ((st = check_corners_fields(c, f, c->W))) return st;
    if ((st = check_corners_overlap(c, f, first_pair, c->W, c->H))) return st;
    if ((st = settle_pending(c))) return st; // (hs_postops.hip.h, rule 1)
    if ((st = resolve_lazy_frames(c, false))) return st;
    return enqueue_corners(c, f, first_pair, which, rule);
}

int hsflow_corners_device(hsflow_ctx *c, int pair, int which, const void *d_mask, size_t mask_stride, const hsflow_corners_params *cp,
                          hsflow_corners_record *d_records, uint32_t capacity, float *d_xy, hsflow_corners_result *d_result)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    const void *const pm[1] = {d_mask};
    void *const pr[1] = {d_records}, *const px[1] = {d_xy};
    return hsflow_corners_batch_device(c, pair, 1, which, d_mask ? pm : nullptr, mask_stride, cp, d_records ? pr : nullptr, capacity, d_xy ? px : nullptr, d_result);
}

int hsflow_corners(hsflow_ctx *c, int pair, int which, const uint8_t *mask, size_t mask_stride, const hsflow_corners_params *cp, hsflow_corners_record *records,
                   uint32_t capacity, float *xy, hsflow_corners_result *result)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    hscn::Rule rule;
    if ((st = check_corners_params(c, cp, &rule))) return st;
    if ((st = check_corners_size(c, c->W, c->H))) return st;
    if ((st = check_corners_which(c, which))) return st;
    {
        const void *const pm[1] = {mask};
        void *const pr[1] = {records}, *const px[1] = {xy};
        const CnFields h = {1, nullptr, 0, mask ? pm : nullptr, mask_stride, records ? pr : nullptr, capacity, xy ? px : nullptr, result};
        if ((st = check_corners_fields(c, h, c->W))) return st;
    }
    if ((st = settle_pending(c))) return st;
    if ((st = resolve_lazy_frames(c, false))) return st;
    const bool want_records = records && capacity, want_xy = xy && capacity;
    const size_t brow = (size_t)c->W, rbytes = sizeof(hsflow_corners_record) * (size_t)capacity, xbytes = 8 * (size_t)capacity;
    hsflow_ctx::CornersScratch &g = c->corners;
    if (mask && (st = corners_stage(c, 0, brow * c->H))) return st;
    if (want_records && (st = corners_stage(c, 1, rbytes))) return st;
    if (want_xy && (st = corners_stage(c, 2, xbytes))) return st;
    // (the header tells how many records were written: it is always taken)
    if ((st = stats_reserve(c, (void **)&g.dRes, (void **)&g.hRes))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    if (mask) HS_HIP(c, copy_rows_async(c, g.stage[0], brow, mask, mask_stride, brow, c->H, hipMemcpyHostToDevice));
    const void *const pm[1] = {g.stage[0]};
    void *const pr[1] = {g.stage[1]}, *const px[1] = {g.stage[2]};
    const CnFields f = {1, nullptr, 0, mask ? pm : nullptr, brow, want_records ? pr : nullptr, capacity, want_xy ? px : nullptr, g.dRes};
    if ((st = enqueue_corners(c, f, pair, which, rule))) return st;
    if (want_xy) HS_HIP(c, hipMemcpyAsync(xy, g.stage[2], xbytes, hipMemcpyDeviceToHost, c->stream));
    if ((st = stats_copy_back(c, g.hRes, g.dRes))) return st;
    if (want_records) {
        // only the records that were written cross: the rest of the caller's array stays as it is
        if ((st = sync_wait(c))) return st;
        const size_t written = g.hRes->n_written;
        if (written) HS_HIP(c, hipMemcpyAsync(records, g.stage[1], sizeof(hsflow_corners_record) * written, hipMemcpyDeviceToHost, c->stream));
    }
    return sync_finish(c, marked, result, g.hRes);
}

} // extern "C"
