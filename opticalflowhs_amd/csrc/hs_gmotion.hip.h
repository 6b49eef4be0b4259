// hs_gmotion.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_gmotion_*, the global motion of a
// flow field fitted where the solver left it (hs_gmotion_rule.h), the mask and the residual flow it leaves, and a picture
// warped by the model.  The engine works on planes (enqueue_gmotion); the forms on a context's pairs hand it the
// context's planes.  Per chunk of at most hsk::kGmBatchMax fields: per pass one k_gm_accum and one k_gm_solve (AUTO: one
// k_gm_hist and one k_gm_solve more), then k_gm_apply -- no memset between them.  On top of hs_postops.hip.h: its three
// ordering rules hold word for word.  A context that never fits allocates and launches nothing here.
#pragma once

#include <cassert>

namespace {

static_assert(sizeof(hsflow_gmotion_result) == 64 && sizeof(hsflow_gmotion_result) == sizeof(hsk::GmResultWords) && sizeof(hsflow_gmotion_result) == kStatsBytes,
              "hsflow_gmotion_result is 64 bytes on both sides");
static_assert(offsetof(hsflow_gmotion_result, threshold) == 24 && offsetof(hsflow_gmotion_result, flags) == 28 && offsetof(hsflow_gmotion_result, cls) == 32,
              "hsflow_gmotion_result: the kernel's layout");
static_assert(sizeof(hsflow_gmotion_params) == 40, "hsflow_gmotion_params is 40 bytes");
static_assert(HSFLOW_GMOTION_TRANSLATION == hsgm::kTranslation && HSFLOW_GMOTION_SIMILARITY == hsgm::kSimilarity && HSFLOW_GMOTION_AFFINE == hsgm::kAffine &&
                  HSFLOW_GMOTION_ZERO == hsgm::kZero && HSFLOW_GMOTION_THRESHOLD_FIXED == hsgm::kFixed && HSFLOW_GMOTION_THRESHOLD_AUTO == hsgm::kAuto &&
                  HSFLOW_GMOTION_MAX_PASSES == hsgm::kMaxPasses && HSFLOW_GMOTION_MAX_SIDE == hsgm::kMaxSide && HSFLOW_GMOTION_FLAG_FALLBACK == hsgm::kFlagFallback,
              "the header's constants are the rule's");
static_assert(HSFLOW_GMOTION_INLIER == hsgm::kInlier && HSFLOW_GMOTION_OUTLIER == hsgm::kOutlier && HSFLOW_GMOTION_UNTRUSTED == hsgm::kUntrusted &&
                  HSFLOW_GMOTION_UNKNOWN == hsgm::kUnknown,
              "the header's classes are the rule's");

int check_gmotion_params(hsflow_ctx *c, const hsflow_gmotion_params *gp, hsgm::Fit *fit)
{
    if (!gp || gp->struct_size != sizeof(hsflow_gmotion_params)) return fail(c, HSFLOW_E_ARG, "gmotion params null or struct_size mismatch");
    if (gp->model != HSFLOW_GMOTION_TRANSLATION && gp->model != HSFLOW_GMOTION_SIMILARITY && gp->model != HSFLOW_GMOTION_AFFINE)
        return fail(c, HSFLOW_E_ARG, "unknown gmotion model");
    if (gp->passes < 1 || gp->passes > HSFLOW_GMOTION_MAX_PASSES) return fail(c, HSFLOW_E_ARG, "gmotion passes must be 1 .. " + std::to_string(HSFLOW_GMOTION_MAX_PASSES));
    if (gp->threshold_mode != HSFLOW_GMOTION_THRESHOLD_FIXED && gp->threshold_mode != HSFLOW_GMOTION_THRESHOLD_AUTO)
        return fail(c, HSFLOW_E_ARG, "unknown gmotion threshold mode");
    if (gp->reserved[0] || gp->reserved[1]) return fail(c, HSFLOW_E_ARG, "gmotion params: reserved fields must be 0");
    const float thr = gp->inlier_px * gp->inlier_px;
    if (gp->threshold_mode == HSFLOW_GMOTION_THRESHOLD_FIXED) {
        if (!(std::isfinite(gp->inlier_px) && gp->inlier_px > 0.0f && std::isfinite(thr) && thr > 0.0f))
            return fail(c, HSFLOW_E_ARG, "gmotion inlier_px and its square must be finite and positive");
    } else if (!(std::isfinite(gp->scale2) && gp->scale2 > 0.0f && gp->scale2 <= 1e6f && std::isfinite(gp->min_thr2) && gp->min_thr2 > 0.0f)) {
        return fail(c, HSFLOW_E_ARG, "gmotion scale2 must be in (0, 1e6] and min_thr2 finite and positive");
    }
    *fit = hsgm::Fit{gp->model, gp->passes, gp->threshold_mode, thr, gp->scale2, gp->min_thr2};
    return HSFLOW_OK;
}

int check_gmotion_size(hsflow_ctx *c, int W, int H)
{
    if (W < 1 || H < 1) return fail(c, HSFLOW_E_SIZE, "gmotion: width and height must be positive");
    if (W > HSFLOW_GMOTION_MAX_SIDE || H > HSFLOW_GMOTION_MAX_SIDE || (long long)W * H > hsgm::kMaxPixels)
        return fail(c, HSFLOW_E_SIZE, "gmotion: a frame wider or higher than 16384, or of more than 2^30 pixels");
    return HSFLOW_OK;
}

// The fields of a fit as the caller names them (host or device memory alike): n of each; the lists of state, mask and
// residual planes may be NULL and may hold NULL entries.
struct GmFields {
    int n;
    const void *const *u, *const *v; // NULL: the context's own pairs
    size_t fs;
    const void *const *state;
    size_t ss;
    void *const *mask;
    size_t ms;
    void *const *ru, *const *rv;
    size_t rs;
    const void *results; // n records, or NULL
};

int check_gmotion_fields(hsflow_ctx *c, const GmFields &f, int W)
{
    bool asked = f.results != nullptr;
    if ((f.ru != nullptr) != (f.rv != nullptr)) return fail(c, HSFLOW_E_ARG, "the two residual planes are asked for together or not at all");
    for (int k = 0; k < f.n; k++) {
        const std::string who = "field " + std::to_string(k) + ": ";
        if (f.u) {
            if (!f.u[k] || !f.v[k]) return fail(c, HSFLOW_E_ARG, who + "null flow plane");
            if ((((uintptr_t)f.u[k] | (uintptr_t)f.v[k]) & 3u) != 0) return fail(c, HSFLOW_E_ARG, who + "the flow planes must be 4-byte aligned");
        }
        if (f.ru) {
            if ((f.ru[k] != nullptr) != (f.rv[k] != nullptr)) return fail(c, HSFLOW_E_ARG, who + "the two residual planes are asked for together or not at all");
            if ((((uintptr_t)f.ru[k] | (uintptr_t)f.rv[k]) & 3u) != 0) return fail(c, HSFLOW_E_ARG, who + "the residual planes must be 4-byte aligned");
            asked = asked || f.ru[k];
            if (f.ru[k] && (f.rs < (size_t)W * 4 || (f.rs & 3u))) return fail(c, HSFLOW_E_SIZE, "residual stride smaller than 4*width or no multiple of 4");
        }
        if (f.mask && f.mask[k]) {
            asked = true;
            if (f.ms < (size_t)W) return fail(c, HSFLOW_E_SIZE, "mask stride smaller than width");
        }
        if (f.state && f.state[k] && f.ss < (size_t)W) return fail(c, HSFLOW_E_SIZE, "state stride smaller than width");
    }
    if (f.u && (f.fs < (size_t)W * 4 || (f.fs & 3u))) return fail(c, HSFLOW_E_SIZE, "flow stride smaller than 4*width or no multiple of 4");
    if (!asked) return fail(c, HSFLOW_E_ARG, "neither a result nor a mask nor the residual planes asked for");
    return HSFLOW_OK;
}

// No output may overlap an input (first_pair >= 0: the context's flows of the pairs, in both buffers of the ping-pong).
int check_gmotion_overlap(hsflow_ctx *c, const GmFields &f, int first_pair, int W, int H)
{
    std::vector<MedSpan> in, out;
    for (int k = 0; k < f.n; k++) {
        if (f.u) {
            in.push_back(med_span(f.u[k], f.fs, (size_t)W * 4, H));
            in.push_back(med_span(f.v[k], f.fs, (size_t)W * 4, H));
        } else {
            for (int b = 0; b < 2; b++) {
                in.push_back(med_span(c->dU[b] + (long long)(first_pair + k) * c->plane, (size_t)c->P * 4, (size_t)W * 4, H));
                in.push_back(med_span(c->dV[b] + (long long)(first_pair + k) * c->plane, (size_t)c->P * 4, (size_t)W * 4, H));
            }
        }
        if (f.state) in.push_back(med_span(f.state[k], f.ss, (size_t)W, H));
        if (f.mask) out.push_back(med_span(f.mask[k], f.ms, (size_t)W, H));
        if (f.ru) {
            out.push_back(med_span(f.ru[k], f.rs, (size_t)W * 4, H));
            out.push_back(med_span(f.rv[k], f.rs, (size_t)W * 4, H));
        }
    }
    out.push_back(med_span(f.results, 0, sizeof(hsflow_gmotion_result) * (size_t)f.n, 1));
    for (const MedSpan &o : out)
        for (const MedSpan &i : in)
            if (med_overlap(o, i)) return fail(c, HSFLOW_E_ARG, "an output of the fit may not overlap an input");
    return HSFLOW_OK;
}

unsigned gmotion_values(const hsflow_gmotion_params &gp)
{
    return (unsigned)gp.value[0] | (unsigned)gp.value[1] << 8 | (unsigned)gp.value[2] << 16 | (unsigned)gp.value[3] << 24;
}

bool gm_wide16(const void *p, const void *q, size_t stride) { return (((uintptr_t)p | (uintptr_t)q | stride) & 15u) == 0; }

// The kernels' records for n fields, zero sums and histograms.  Allocated by the first call, grown, kept.
int gmotion_scratch(hsflow_ctx *c, int n)
{
    hsflow_ctx::GmotionScratch &g = c->gmotion;
    if (g.cap < n) {
        hipFree(g.scr); // (holds until the device is idle: an earlier fit may still be using the records)
        g.scr = nullptr; g.cap = 0;
        HS_HIP(c, hipMalloc(&g.scr, sizeof(hsk::GmScratch) * (size_t)n));
        g.cap = n;
        g.dirty = true;
    }
    if (g.dirty) HS_HIP(c, hipMemsetAsync(g.scr, 0, sizeof(hsk::GmScratch) * (size_t)g.cap, c->stream));
    g.dirty = false;
    return HSFLOW_OK;
}

// The launches of a fit.  All pointers are device memory; the caller has checked every argument and, for the context's own
// flows (f.u NULL), settled an owed check.
int enqueue_gmotion(hsflow_ctx *c, const GmFields &f, int first_pair, const hsflow_gmotion_params &gp, const hsgm::Fit &fit)
{
    const int W = c->W, H = c->H, chunk = f.n < hsk::kGmBatchMax ? f.n : hsk::kGmBatchMax;
    const int st = gmotion_scratch(c, chunk);
    if (st) return st;
    hsflow_ctx::GmotionScratch &g = c->gmotion;
    hsk::GmScratch *scr = (hsk::GmScratch *)g.scr;
    for (int first = 0; first < f.n; first += chunk) {
        const int cnt = f.n - first < chunk ? f.n - first : chunk;
        hsk::GmPlanes pl{};
        pl.W = W; pl.H = H;
        pl.fs = f.u ? (long long)f.fs : (long long)c->P * 4; pl.ss = (long long)f.ss; pl.ms = (long long)f.ms; pl.rs = (long long)f.rs;
        pl.value = gmotion_values(gp);
        for (int k = 0; k < cnt; k++) {
            const int i = first + k;
            pl.u[k] = f.u ? (const float *)f.u[i] : c->dU[c->cur] + (long long)(first_pair + i) * c->plane;
            pl.v[k] = f.u ? (const float *)f.v[i] : c->dV[c->cur] + (long long)(first_pair + i) * c->plane;
            pl.s[k] = f.state ? (const uint8_t *)f.state[i] : nullptr;
            pl.mask[k] = f.mask ? (uint8_t *)f.mask[i] : nullptr;
            pl.ru[k] = f.ru ? (float *)f.ru[i] : nullptr;
            pl.rv[k] = f.ru ? (float *)f.rv[i] : nullptr;
            if (gm_wide16(pl.u[k], pl.v[k], (size_t)pl.fs)) pl.wide_in |= 1u << k;
            if (pl.s[k] && word_aligned(pl.s[k], f.ss)) pl.wide_state |= 1u << k;
            if (pl.mask[k] && word_aligned(pl.mask[k], f.ms)) pl.wide_mask |= 1u << k;
            if (pl.ru[k] && gm_wide16(pl.ru[k], pl.rv[k], f.rs)) pl.wide_res |= 1u << k;
        }
        dim3 grid;
        stats_rows(c, (W + 1023) / 1024, H, cnt, true, &grid);
        assert(((long long)H + grid.y - 1) / grid.y <= hsk::kGmRowsPerLane); // (stats_rows: at most 8 rows per workgroup while H <= 65535 * 8; check_gmotion_size holds H <= 16384)
        hsk::GmResultWords *results = f.results ? (hsk::GmResultWords *)f.results + first : nullptr;
        const bool aut = fit.mode == hsgm::kAuto;
        g.dirty = true; // (until the last launch is in the stream: a failure in between leaves sums or histograms behind)
        c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
        for (int j = 0; j < fit.passes; j++) {
            if (j > 0 && aut) {
                HS_HIP(c, hsk::launch_gm_hist(grid, c->stream, pl, scr));
                HS_HIP(c, hsk::launch_gm_solve(c->stream, scr, cnt, hsk::kGmSolveThreshold, fit.kind, fit.mode, fit.fixed_thr, fit.scale2, fit.min_thr2, nullptr));
            }
            HS_HIP(c, hsk::launch_gm_accum(grid, c->stream, pl, scr, j == 0));
            // the model, and with it the threshold of FIXED (AUTO's comes from the histogram under this model)
            HS_HIP(c, hsk::launch_gm_solve(c->stream, scr, cnt, hsk::kGmSolveModel | (aut ? 0 : hsk::kGmSolveThreshold | hsk::kGmSolveResult), fit.kind, fit.mode,
                                           fit.fixed_thr, fit.scale2, fit.min_thr2, j == fit.passes - 1 ? results : nullptr));
        }
        if (aut) {
            HS_HIP(c, hsk::launch_gm_hist(grid, c->stream, pl, scr));
            HS_HIP(c, hsk::launch_gm_solve(c->stream, scr, cnt, hsk::kGmSolveThreshold | hsk::kGmSolveResult, fit.kind, fit.mode, fit.fixed_thr, fit.scale2,
                                           fit.min_thr2, results));
        }
        HS_HIP(c, hsk::launch_gm_apply(grid, c->stream, pl, scr, results));
        g.dirty = false;
    }
    return HSFLOW_OK;
}

int check_gmotion_model(hsflow_ctx *c, const float *model, hsgm::Model *m)
{
    if (!model) return fail(c, HSFLOW_E_ARG, "null model");
    for (int k = 0; k < 6; k++) {
        if (!std::isfinite(model[k])) return fail(c, HSFLOW_E_ARG, "a model parameter is not finite");
        m->p[k] = model[k];
    }
    return HSFLOW_OK;
}

// The launch of a warp by a model.  All pointers are device memory; the caller has checked every argument.
int enqueue_gmotion_warp(hsflow_ctx *c, const hsgm::Model &m, const hsflow_warp_params &wp, const void *src, size_t ss, const void *ref, size_t rs, void *dst,
                         size_t ds, void *d_stats)
{
    dim3 grid;
    const int st = stats_grid(c, (c->W + 1023) / 1024, c->H, 1, d_stats, &grid);
    if (st) return st;
    HS_HIP(c, hsk::launch_gm_warp(grid, c->stream, wp.channels, m, (const uint8_t *)src, (const uint8_t *)ref, (uint8_t *)dst, dst && word_aligned(dst, ds),
                                  (long long)ss, (long long)rs, (long long)ds, c->W, c->H, wp.t, wp.border, warp_fill(wp), (unsigned long long *)d_stats));
    c->last_marked = false; // (rule 2: the call is in the stream behind the solve like every operator's)
    return HSFLOW_OK;
}

int gmotion_stage(hsflow_ctx *c, int slot, size_t bytes) { return stage_reserve(c, &c->gmotion.stage[slot], &c->gmotion.stage_bytes[slot], bytes); }

void gmotion_release(hsflow_ctx *c)
{
    hipFree(c->gmotion.scr);
    for (uint8_t *p : c->gmotion.stage) hipFree(p);
    stats_release(c->gmotion.dRes, c->gmotion.hRes);
    stats_release(c->gmotion.dStats, c->gmotion.hStats);
    c->gmotion = hsflow_ctx::GmotionScratch();
}

} // namespace

extern "C" {

void hsflow_default_gmotion_params(hsflow_gmotion_params *gp)
{
    if (!gp) return;
    std::memset(gp, 0, sizeof(*gp));
    gp->struct_size = sizeof(*gp);
    gp->model = HSFLOW_GMOTION_AFFINE;
    gp->passes = 3;
    gp->threshold_mode = HSFLOW_GMOTION_THRESHOLD_FIXED;
    gp->inlier_px = 1.0f;
    gp->scale2 = 6.0f;
    gp->min_thr2 = 0.0625f;
    gp->value[0] = 255;
}

int hsflow_gmotion_fit_host(const float *u, const float *v, size_t flow_stride, const uint8_t *state, size_t state_stride, int width, int height,
                            const hsflow_gmotion_params *gp, uint8_t *mask, size_t mask_stride, float *res_u, float *res_v, size_t res_stride,
                            hsflow_gmotion_result *result)
{
    hsgm::Fit fit;
    int st = check_gmotion_params(nullptr, gp, &fit);
    if (st) return st;
    if ((st = check_gmotion_size(nullptr, width, height))) return st;
    const void *const pu[1] = {u}, *const pv[1] = {v}, *const ps[1] = {state};
    void *const pm[1] = {mask}, *const pru[1] = {res_u}, *const prv[1] = {res_v};
    const GmFields f = {1, pu, pv, flow_stride, state ? ps : nullptr, state_stride, mask ? pm : nullptr, mask_stride, (res_u || res_v) ? pru : nullptr,
                        (res_u || res_v) ? prv : nullptr, res_stride, result};
    if ((st = check_gmotion_fields(nullptr, f, width))) return st;
    if ((st = check_gmotion_overlap(nullptr, f, -1, width, height))) return st;
    const hsgm::Field field = {u, v, flow_stride, state, state_stride, width, height};
    hsgm::Result r;
    hsgm::fit_rows(field, fit, gp->value, mask, mask_stride, res_u, res_v, res_stride, &r);
    if (result) {
        std::memset(result, 0, sizeof(*result));
        for (int k = 0; k < 6; k++) result->p[k] = r.m.p[k];
        result->threshold = r.thr;
        result->flags = r.flags;
        for (int k = 0; k < 4; k++) result->cls[k] = r.cls[k];
    }
    return HSFLOW_OK;
}

int hsflow_gmotion_fit_planes_device(hsflow_ctx *c, const void *d_u, const void *d_v, size_t flow_stride, const void *d_state, size_t state_stride,
                                     const hsflow_gmotion_params *gp, void *d_mask, size_t mask_stride, void *d_res_u, void *d_res_v, size_t res_stride,
                                     hsflow_gmotion_result *d_result)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    hsgm::Fit fit;
    if ((st = check_gmotion_params(c, gp, &fit))) return st;
    if ((st = check_gmotion_size(c, c->W, c->H))) return st;
    const void *const pu[1] = {d_u}, *const pv[1] = {d_v}, *const ps[1] = {d_state};
    void *const pm[1] = {d_mask}, *const pru[1] = {d_res_u}, *const prv[1] = {d_res_v};
    const GmFields f = {1, pu, pv, flow_stride, d_state ? ps : nullptr, state_stride, d_mask ? pm : nullptr, mask_stride, (d_res_u || d_res_v) ? pru : nullptr,
                        (d_res_u || d_res_v) ? prv : nullptr, res_stride, d_result};
    if ((st = check_gmotion_fields(c, f, c->W))) return st;
    if ((st = check_gmotion_overlap(c, f, -1, c->W, c->H))) return st;
    if (((uintptr_t)d_result & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the result record must be 8-byte aligned");
    if ((st = settle_pending(c))) return st;
    return enqueue_gmotion(c, f, 0, *gp, fit);
}

int hsflow_gmotion_fit_batch_device(hsflow_ctx *c, int first_pair, int n, const void *const *d_state, size_t state_stride, const hsflow_gmotion_params *gp,
                                    void *const *d_mask, size_t mask_stride, void *const *d_res_u, void *const *d_res_v, size_t res_stride,
                                    hsflow_gmotion_result *d_results)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_batch_pairs(c, first_pair, n))) return st;
    hsgm::Fit fit;
    if ((st = check_gmotion_params(c, gp, &fit))) return st;
    if ((st = check_gmotion_size(c, c->W, c->H))) return st;
    const GmFields f = {n, nullptr, nullptr, 0, d_state, state_stride, d_mask, mask_stride, d_res_u, d_res_v, res_stride, d_results};
    if ((st = check_gmotion_fields(c, f, c->W))) return st;
    if ((st = check_gmotion_overlap(c, f, first_pair, c->W, c->H))) return st;
    if (((uintptr_t)d_results & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the result records must be 8-byte aligned");
    if ((st = settle_pending(c))) return st; // (hs_postops.hip.h, rule 1, before c->cur is named)
    return enqueue_gmotion(c, f, first_pair, *gp, fit);
}

int hsflow_gmotion_fit_device(hsflow_ctx *c, int pair, const void *d_state, size_t state_stride, const hsflow_gmotion_params *gp, void *d_mask,
                              size_t mask_stride, void *d_res_u, void *d_res_v, size_t res_stride, hsflow_gmotion_result *d_result)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    const void *const ps[1] = {d_state};
    void *const pm[1] = {d_mask}, *const pru[1] = {d_res_u}, *const prv[1] = {d_res_v};
    return hsflow_gmotion_fit_batch_device(c, pair, 1, d_state ? ps : nullptr, state_stride, gp, d_mask ? pm : nullptr, mask_stride,
                                           (d_res_u || d_res_v) ? pru : nullptr, (d_res_u || d_res_v) ? prv : nullptr, res_stride, d_result);
}

int hsflow_gmotion_fit(hsflow_ctx *c, int pair, const uint8_t *state, size_t state_stride, const hsflow_gmotion_params *gp, uint8_t *mask, size_t mask_stride,
                       float *res_u, float *res_v, size_t res_stride, hsflow_gmotion_result *result)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    hsgm::Fit fit;
    if ((st = check_gmotion_params(c, gp, &fit))) return st;
    if ((st = check_gmotion_size(c, c->W, c->H))) return st;
    {
        const void *const ps[1] = {state};
        void *const pm[1] = {mask}, *const pru[1] = {res_u}, *const prv[1] = {res_v};
        const GmFields h = {1, nullptr, nullptr, 0, state ? ps : nullptr, state_stride, mask ? pm : nullptr, mask_stride, (res_u || res_v) ? pru : nullptr,
                            (res_u || res_v) ? prv : nullptr, res_stride, result};
        if ((st = check_gmotion_fields(c, h, c->W))) return st;
    }
    if ((st = settle_pending(c))) return st;
    const size_t frow = (size_t)c->W * 4, brow = (size_t)c->W, fbytes = frow * c->H, bbytes = brow * c->H;
    hsflow_ctx::GmotionScratch &g = c->gmotion;
    if (state && (st = gmotion_stage(c, 0, bbytes))) return st;
    if (mask && (st = gmotion_stage(c, 1, bbytes))) return st;
    if (res_u && ((st = gmotion_stage(c, 2, fbytes)) || (st = gmotion_stage(c, 3, fbytes)))) return st;
    if (result && (st = stats_reserve(c, (void **)&g.dRes, (void **)&g.hRes))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    if (state) HS_HIP(c, copy_rows_async(c, g.stage[0], brow, state, state_stride, brow, c->H, hipMemcpyHostToDevice));
    const void *const ps[1] = {g.stage[0]};
    void *const pm[1] = {g.stage[1]}, *const pru[1] = {g.stage[2]}, *const prv[1] = {g.stage[3]};
    const GmFields f = {1, nullptr, nullptr, 0, state ? ps : nullptr, brow, mask ? pm : nullptr, brow, res_u ? pru : nullptr, res_u ? prv : nullptr, frow,
                        result ? g.dRes : nullptr};
    if ((st = enqueue_gmotion(c, f, pair, *gp, fit))) return st;
    if (mask) HS_HIP(c, copy_rows_async(c, mask, mask_stride, g.stage[1], brow, brow, c->H, hipMemcpyDeviceToHost));
    if (res_u) {
        HS_HIP(c, copy_rows_async(c, res_u, res_stride, g.stage[2], frow, frow, c->H, hipMemcpyDeviceToHost));
        HS_HIP(c, copy_rows_async(c, res_v, res_stride, g.stage[3], frow, frow, c->H, hipMemcpyDeviceToHost));
    }
    if (result && (st = stats_copy_back(c, g.hRes, g.dRes))) return st;
    return sync_finish(c, marked, result, g.hRes);
}

int hsflow_gmotion_warp_host(const float *model, int width, int height, const hsflow_warp_params *wp, const uint8_t *src, size_t src_stride, const uint8_t *ref,
                             size_t ref_stride, uint8_t *dst, size_t dst_stride, hsflow_warp_stats *stats)
{
    int st = check_warp_params(nullptr, wp);
    if (st) return st;
    hsgm::Model m;
    if ((st = check_gmotion_model(nullptr, model, &m))) return st;
    if (!src) return fail(nullptr, HSFLOW_E_ARG, "hsflow_gmotion_warp_host: null source");
    if (dst && (dst == src || dst == ref)) return fail(nullptr, HSFLOW_E_ARG, "hsflow_gmotion_warp_host: the destination is the source or the reference");
    if ((st = check_gmotion_size(nullptr, width, height))) return st;
    if ((st = check_warp_pictures(nullptr, wp, width, false, ref != nullptr, dst != nullptr, stats != nullptr, src_stride, ref_stride, dst_stride))) return st;
    hswarp::Sums sums;
    if (wp->channels == 1)
        hsgm::warp_rows<1>(m, width, height, wp->t, wp->border, warp_fill(*wp), src, src_stride, ref, ref_stride, dst, dst_stride, stats ? &sums : nullptr);
    else
        hsgm::warp_rows<3>(m, width, height, wp->t, wp->border, warp_fill(*wp), src, src_stride, ref, ref_stride, dst, dst_stride, stats ? &sums : nullptr);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->inside = sums.inside; stats->outside = sums.outside; stats->unknown = sums.unknown;
        stats->sad_warped = sums.sad_warped; stats->sad_plain = sums.sad_plain;
        stats->max_warped = sums.max_warped; stats->max_plain = sums.max_plain;
    }
    return HSFLOW_OK;
}

int hsflow_gmotion_warp_device(hsflow_ctx *c, const float *model, const hsflow_warp_params *wp, const void *d_src, size_t src_stride, const void *d_ref,
                               size_t ref_stride, void *d_dst, size_t dst_stride, hsflow_warp_stats *d_stats)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_warp_params(c, wp))) return st;
    hsgm::Model m;
    if ((st = check_gmotion_model(c, model, &m))) return st;
    if (!d_src) return fail(c, HSFLOW_E_ARG, "null source");
    if (d_dst && (d_dst == d_src || d_dst == d_ref)) return fail(c, HSFLOW_E_ARG, "the destination is the source or the reference");
    if ((st = check_warp_pictures(c, wp, c->W, false, d_ref != nullptr, d_dst != nullptr, d_stats != nullptr, src_stride, ref_stride, dst_stride))) return st;
    if (((uintptr_t)d_stats & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the statistics record must be 8-byte aligned");
    if ((st = settle_pending(c))) return st;
    return enqueue_gmotion_warp(c, m, *wp, d_src, src_stride, d_ref, ref_stride, d_dst, dst_stride, d_stats);
}

int hsflow_gmotion_warp(hsflow_ctx *c, const float *model, const hsflow_warp_params *wp, const uint8_t *src, size_t src_stride, const uint8_t *ref,
                        size_t ref_stride, uint8_t *dst, size_t dst_stride, hsflow_warp_stats *stats)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_warp_params(c, wp))) return st;
    hsgm::Model m;
    if ((st = check_gmotion_model(c, model, &m))) return st;
    if (!src) return fail(c, HSFLOW_E_ARG, "null source");
    if (dst && (dst == src || dst == ref)) return fail(c, HSFLOW_E_ARG, "the destination is the source or the reference");
    if ((st = check_warp_pictures(c, wp, c->W, false, ref != nullptr, dst != nullptr, stats != nullptr, src_stride, ref_stride, dst_stride))) return st;
    if ((st = settle_pending(c))) return st;
    const size_t rowb = (size_t)c->W * (size_t)wp->channels, bytes = rowb * c->H;
    hsflow_ctx::GmotionScratch &g = c->gmotion;
    if ((st = gmotion_stage(c, 4, bytes))) return st;
    if (ref && (st = gmotion_stage(c, 5, bytes))) return st;
    if (dst && (st = gmotion_stage(c, 6, bytes))) return st;
    if (stats && (st = stats_reserve(c, (void **)&g.dStats, (void **)&g.hStats))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    HS_HIP(c, copy_rows_async(c, g.stage[4], rowb, src, src_stride, rowb, c->H, hipMemcpyHostToDevice));
    if (ref) HS_HIP(c, copy_rows_async(c, g.stage[5], rowb, ref, ref_stride, rowb, c->H, hipMemcpyHostToDevice));
    if ((st = enqueue_gmotion_warp(c, m, *wp, g.stage[4], rowb, ref ? g.stage[5] : nullptr, rowb, dst ? g.stage[6] : nullptr, rowb, stats ? g.dStats : nullptr)))
        return st;
    if (dst) HS_HIP(c, copy_rows_async(c, dst, dst_stride, g.stage[6], rowb, rowb, c->H, hipMemcpyDeviceToHost));
    if (stats && (st = stats_copy_back(c, g.hStats, g.dStats))) return st;
    return sync_finish(c, marked, stats, g.hStats);
}

int hsflow_gmotion_compose_host(const float *m1, const float *m2, float *out)
{
    hsgm::Model a, b, r;
    int st = check_gmotion_model(nullptr, m1, &a);
    if (st) return st;
    if ((st = check_gmotion_model(nullptr, m2, &b))) return st;
    if (!out) return fail(nullptr, HSFLOW_E_ARG, "hsflow_gmotion_compose_host: null output");
    hsgm::compose(a, b, &r);
    for (int k = 0; k < 6; k++) out[k] = r.p[k];
    return HSFLOW_OK;
}

int hsflow_gmotion_invert_host(const float *m, float *out)
{
    hsgm::Model a, r;
    const int st = check_gmotion_model(nullptr, m, &a);
    if (st) return st;
    if (!out) return fail(nullptr, HSFLOW_E_ARG, "hsflow_gmotion_invert_host: null output");
    if (!hsgm::invert(a, &r)) return fail(nullptr, HSFLOW_E_ARG, "hsflow_gmotion_invert_host: the model's linear part is singular");
    for (int k = 0; k < 6; k++) out[k] = r.p[k];
    return HSFLOW_OK;
}

} // extern "C"
