// hs_fb.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_fb*, the forward-backward
// consistency of two flows where the solver left them (hs_fb_rule.h), and hsflow_set_frames_reversed, which makes the
// reversed pair of a bidirectional solve from frames that are already on the device.  Per chunk of at most
// HSFLOW_JPEG_BATCH_MAX checks: one launch (hs_kernels_fb.hip.h), with statistics one memset of the chunk's records in
// front of it.  The single forms are batches of one.  A context that never checks allocates and launches nothing here.
#pragma once

namespace {

static_assert(sizeof(hsflow_fb_stats) == 64 && sizeof(hsflow_fb_stats) == sizeof(hsk::FbStatsWords), "hsflow_fb_stats is 64 bytes on both sides");
static_assert(offsetof(hsflow_fb_stats, sum_err2_q) == 32 && offsetof(hsflow_fb_stats, max_err2_bits) == 40, "hsflow_fb_stats: the kernel's layout");
static_assert(sizeof(hsflow_fb_params) == 16, "hsflow_fb_params is 16 bytes");

int check_fb_params(hsflow_ctx *c, const hsflow_fb_params *fp)
{
    if (!fp || fp->struct_size != sizeof(hsflow_fb_params)) return fail(c, HSFLOW_E_ARG, "fb params null or struct_size mismatch");
    if (!(std::isfinite(fp->alpha) && fp->alpha >= 0.0f && fp->alpha <= hsfb::kMaxAlpha)) return fail(c, HSFLOW_E_ARG, "fb alpha must be finite and 0 .. 1e6");
    if (!(std::isfinite(fp->beta) && fp->beta >= 0.0f && fp->beta <= hsfb::kMaxBeta)) return fail(c, HSFLOW_E_ARG, "fb beta must be finite and 0 .. 1e30");
    return HSFLOW_OK;
}

// The checks every form shares once the outputs are known: what there is to do and the row sizes.
int check_fb_outputs(hsflow_ctx *c, const hsflow_fb_params *fp, int W, bool has_mask, bool has_err2, bool has_stats, size_t mask_stride, size_t err2_stride)
{
    const int st = check_fb_params(c, fp);
    if (st) return st;
    if (!has_mask && !has_err2 && !has_stats) return fail(c, HSFLOW_E_ARG, "neither a mask nor err2 nor statistics asked for");
    if (has_mask && mask_stride < (size_t)W) return fail(c, HSFLOW_E_SIZE, "mask stride smaller than width");
    if (has_err2 && (err2_stride < (size_t)W * 4 || (err2_stride & 3u))) return fail(c, HSFLOW_E_SIZE, "err2 stride smaller than 4*width or no multiple of 4");
    return HSFLOW_OK;
}

int check_fb_planes(hsflow_ctx *c, int W, const void *ub, const void *vb, size_t b_stride)
{
    if (!ub || !vb) return fail(c, HSFLOW_E_ARG, "null backward flow plane");
    if ((((uintptr_t)ub | (uintptr_t)vb) & 3u) != 0) return fail(c, HSFLOW_E_ARG, "the backward flow planes must be 4-byte aligned");
    if (b_stride < (size_t)W * 4 || (b_stride & 3u)) return fail(c, HSFLOW_E_SIZE, "backward flow stride smaller than 4*width or no multiple of 4");
    return HSFLOW_OK;
}

unsigned fb_values(const hsflow_fb_params &fp)
{
    return (unsigned)fp.value[0] | (unsigned)fp.value[1] << 8 | (unsigned)fp.value[2] << 16 | (unsigned)fp.value[3] << 24;
}

template <bool ERR, bool STATS>
void launch_fb(hsflow_ctx *c, const dim3 &grid, const hsk::FbBatchChecks &chk, size_t bs, size_t ms, size_t es, const hsflow_fb_params &fp,
               hsk::FbStatsWords *stats)
{
    hipLaunchKernelGGL((hsk::k_fb_batch<ERR, STATS>), grid, dim3(256), 0, c->stream, chk, (long long)c->P, (long long)bs, (long long)ms, (long long)es, c->W,
                       c->H, fp.alpha, fp.beta, fb_values(fp), stats);
}

// The launch for cnt checks (cnt <= kRenderBatchMax).  bs: the backward planes' stride in bytes.  d_stats: the chunk's
// first record, or NULL.  The caller has checked every argument.
int enqueue_fb_chunk(hsflow_ctx *c, int cnt, const hsflow_fb_params &fp, const hsk::FbBatchChecks &chk, bool with_err2, size_t bs, size_t ms, size_t es,
                     void *d_stats)
{
    hsk::FbStatsWords *stats = (hsk::FbStatsWords *)d_stats;
    dim3 grid;
    const int st = stats_grid(c, (c->W + 1023) / 1024, c->H, cnt, stats, &grid);
    if (st) return st;
    if (with_err2) {
        if (stats) launch_fb<true, true>(c, grid, chk, bs, ms, es, fp, stats);
        else launch_fb<true, false>(c, grid, chk, bs, ms, es, fp, stats);
    } else {
        if (stats) launch_fb<false, true>(c, grid, chk, bs, ms, es, fp, stats);
        else launch_fb<false, false>(c, grid, chk, bs, ms, es, fp, stats);
    }
    HS_HIP(c, hipGetLastError());
    c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
    return HSFLOW_OK;
}

int fb_wide16(const void *p, size_t stride) { return (((uintptr_t)p | stride) & 15u) == 0; }

// The synchronous form: pair fwd_pair forwards against pair bwd_pair of the context, or with bwd_pair < 0 against the
// backward planes ub / vb (device memory, rows bs bytes apart); the results to host memory.  The caller has checked the
// pairs and the planes.  The context's own planes are named only behind settle_pending: a re-run that an owed ITER|EPS
// check asks for may end in the other buffer of the pair (c->cur).
int fb_to_host(hsflow_ctx *c, int fwd_pair, int bwd_pair, const float *ub, const float *vb, size_t bs, const hsflow_fb_params *fp, uint8_t *mask, size_t mask_stride,
               float *err2, size_t err2_stride, hsflow_fb_stats *stats)
{
    int st = check_fb_outputs(c, fp, c->W, mask != nullptr, err2 != nullptr, stats != nullptr, mask_stride, err2_stride);
    if (st) return st;
    if ((st = settle_pending(c))) return st;
    if (bwd_pair >= 0) {
        ub = c->dU[c->cur] + bwd_pair * c->plane; vb = c->dV[c->cur] + bwd_pair * c->plane;
        bs = (size_t)c->P * 4;
    }
    const size_t mrow = (size_t)c->W, erow = (size_t)c->W * 4;
    hsflow_ctx::FbScratch &f = c->fb;
    if (mask && (st = stage_reserve(c, &f.mask, &f.mask_bytes, mrow * c->H))) return st;
    if (err2 && (st = stage_reserve(c, &f.err2, &f.err2_bytes, erow * c->H))) return st;
    if (stats && (st = stats_reserve(c, (void **)&f.dStats, (void **)&f.hStats))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    hsk::FbBatchChecks chk{};
    chk.uf[0] = c->dU[c->cur] + fwd_pair * c->plane; chk.vf[0] = c->dV[c->cur] + fwd_pair * c->plane;
    chk.ub[0] = ub; chk.vb[0] = vb;
    chk.mask[0] = mask ? f.mask : nullptr;
    chk.err2[0] = err2 ? (float *)f.err2 : nullptr;
    chk.wide_mask = mask ? (uint32_t)word_aligned(f.mask, mrow) : 0u;
    chk.wide_err2 = err2 ? (uint32_t)fb_wide16(f.err2, erow) : 0u;
    if ((st = enqueue_fb_chunk(c, 1, *fp, chk, err2 != nullptr, bs, mrow, erow, stats ? f.dStats : nullptr))) return st;
    if (mask) HS_HIP(c, copy_rows_async(c, mask, mask_stride, f.mask, mrow, mrow, c->H, hipMemcpyDeviceToHost));
    if (err2) HS_HIP(c, copy_rows_async(c, err2, err2_stride, f.err2, erow, erow, c->H, hipMemcpyDeviceToHost));
    if (stats && (st = stats_copy_back(c, f.hStats, f.dStats))) return st;
    return sync_finish(c, marked, stats, f.hStats);
}

// What the device forms share.  bwd_pairs: the backward flow is that of the context's pairs; else ub / vb / bs for every
// check (n is then 1).
int fb_on_device(hsflow_ctx *c, int n, const int *fwd_pairs, const int *bwd_pairs, const float *ub, const float *vb, size_t bs, const hsflow_fb_params *fp,
                 void *const *d_mask, size_t mask_stride, void *const *d_err2, size_t err2_stride, hsflow_fb_stats *d_stats)
{
    int st = HSFLOW_OK, maxb = 0;
    if (n < 1) return fail(c, HSFLOW_E_ARG, "a batch needs at least one check");
    if (!fwd_pairs || (!bwd_pairs && !ub)) return fail(c, HSFLOW_E_ARG, "null pair list");
    for (int i = 0; i < n; i++)
        if (fwd_pairs[i] < 0 || fwd_pairs[i] >= c->N || (bwd_pairs && (bwd_pairs[i] < 0 || bwd_pairs[i] >= c->N)))
            return fail(c, HSFLOW_E_ARG, "check " + std::to_string(i) + ": pair index out of range");
    if ((st = check_fb_outputs(c, fp, c->W, d_mask != nullptr, d_err2 != nullptr, d_stats != nullptr, mask_stride, err2_stride))) return st;
    for (int i = 0; i < n; i++) {
        if ((d_mask && !d_mask[i]) || (d_err2 && !d_err2[i])) return fail(c, HSFLOW_E_ARG, "check " + std::to_string(i) + ": null output pointer");
        if (d_err2 && ((uintptr_t)d_err2[i] & 3u)) return fail(c, HSFLOW_E_ARG, "check " + std::to_string(i) + ": err2 must be 4-byte aligned");
    }
    if ((st = batch_device_begin(c, d_stats, &maxb))) return st;
    const float *U = c->dU[c->cur], *V = c->dV[c->cur];
    for (const hsjpeg_plan::Chunk &ch : hsjpeg_plan::chunks(n, maxb)) {
        hsk::FbBatchChecks chk{};
        for (int k = 0; k < ch.count; k++) {
            const int i = ch.first + k;
            const long long fwd = fwd_pairs[i];
            chk.uf[k] = U + fwd * c->plane; chk.vf[k] = V + fwd * c->plane;
            chk.ub[k] = bwd_pairs ? U + (long long)bwd_pairs[i] * c->plane : ub;
            chk.vb[k] = bwd_pairs ? V + (long long)bwd_pairs[i] * c->plane : vb;
            chk.mask[k] = d_mask ? (uint8_t *)d_mask[i] : nullptr;
            chk.err2[k] = d_err2 ? (float *)d_err2[i] : nullptr;
            if (d_mask && word_aligned(d_mask[i], mask_stride)) chk.wide_mask |= 1u << k;
            if (d_err2 && fb_wide16(d_err2[i], err2_stride)) chk.wide_err2 |= 1u << k;
        }
        if ((st = enqueue_fb_chunk(c, ch.count, *fp, chk, d_err2 != nullptr, bwd_pairs ? (size_t)c->P * 4 : bs, mask_stride, err2_stride,
                                   d_stats ? d_stats + ch.first : nullptr)))
            return st;
    }
    return HSFLOW_OK;
}

} // namespace

extern "C" {

void hsflow_default_fb_params(hsflow_fb_params *fp)
{
    if (!fp) return;
    std::memset(fp, 0, sizeof(*fp));
    fp->struct_size = sizeof(*fp);
    fp->alpha = 0.01f;
    fp->beta = 0.5f;
    fp->value[0] = 255;
}

int hsflow_fb_host(const float *uf, size_t uf_stride, const float *vf, size_t vf_stride, const float *ub, size_t ub_stride, const float *vb, size_t vb_stride,
                   int width, int height, const hsflow_fb_params *fp, uint8_t *mask, size_t mask_stride, float *err2, size_t err2_stride,
                   hsflow_fb_stats *stats)
{
    int st = check_fb_params(nullptr, fp);
    if (st) return st;
    if (!uf || !vf || !ub || !vb) return fail(nullptr, HSFLOW_E_ARG, "hsflow_fb_host: null flow plane");
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_fb_host: width and height must be positive");
    const size_t rowb = (size_t)width * 4;
    if (uf_stride < rowb || vf_stride < rowb || ub_stride < rowb || vb_stride < rowb || ((uf_stride | vf_stride | ub_stride | vb_stride) & 3u))
        return fail(nullptr, HSFLOW_E_SIZE, "hsflow_fb_host: flow stride smaller than 4*width or no multiple of 4");
    if ((st = check_fb_outputs(nullptr, fp, width, mask != nullptr, err2 != nullptr, stats != nullptr, mask_stride, err2_stride))) return st;
    hsfb::Sums sums;
    hsfb::fb_rows(uf, uf_stride, vf, vf_stride, ub, ub_stride, vb, vb_stride, width, height, fp->alpha, fp->beta, fp->value, mask, mask_stride, err2,
                  err2_stride, stats ? &sums : nullptr);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->consistent = sums.cls[0]; stats->inconsistent = sums.cls[1]; stats->outside = sums.cls[2]; stats->unknown = sums.cls[3];
        stats->sum_err2_q = sums.sum_q;
        stats->max_err2_bits = sums.max_bits;
    }
    return HSFLOW_OK;
}

int hsflow_fb_batch_device(hsflow_ctx *c, int n, const int *fwd_pairs, const int *bwd_pairs, const hsflow_fb_params *fp, void *const *d_mask,
                           size_t mask_stride, void *const *d_err2, size_t err2_stride, hsflow_fb_stats *d_stats)
{
    const int st = check_ctx(c, 0);
    if (st) return st;
    if (!bwd_pairs) return fail(c, HSFLOW_E_ARG, "null pair list");
    return fb_on_device(c, n, fwd_pairs, bwd_pairs, nullptr, nullptr, 0, fp, d_mask, mask_stride, d_err2, err2_stride, d_stats);
}

int hsflow_fb_device(hsflow_ctx *c, int fwd_pair, int bwd_pair, const hsflow_fb_params *fp, void *d_mask, size_t mask_stride, void *d_err2,
                     size_t err2_stride, hsflow_fb_stats *d_stats)
{
    void *const mask[1] = {d_mask}, *const err2[1] = {d_err2};
    return hsflow_fb_batch_device(c, 1, &fwd_pair, &bwd_pair, fp, d_mask ? mask : nullptr, mask_stride, d_err2 ? err2 : nullptr, err2_stride, d_stats);
}

int hsflow_fb_planes_device(hsflow_ctx *c, int fwd_pair, const void *d_ub, const void *d_vb, size_t b_stride, const hsflow_fb_params *fp, void *d_mask,
                            size_t mask_stride, void *d_err2, size_t err2_stride, hsflow_fb_stats *d_stats)
{
    int st = check_ctx(c, fwd_pair);
    if (st) return st;
    if ((st = check_fb_planes(c, c->W, d_ub, d_vb, b_stride))) return st;
    void *const mask[1] = {d_mask}, *const err2[1] = {d_err2};
    return fb_on_device(c, 1, &fwd_pair, nullptr, (const float *)d_ub, (const float *)d_vb, b_stride, fp, d_mask ? mask : nullptr, mask_stride,
                        d_err2 ? err2 : nullptr, err2_stride, d_stats);
}

int hsflow_fb(hsflow_ctx *c, int fwd_pair, int bwd_pair, const hsflow_fb_params *fp, uint8_t *mask, size_t mask_stride, float *err2, size_t err2_stride,
              hsflow_fb_stats *stats)
{
    int st = check_ctx(c, fwd_pair);
    if (st) return st;
    if ((st = check_ctx(c, bwd_pair))) return st;
    return fb_to_host(c, fwd_pair, bwd_pair, nullptr, nullptr, 0, fp, mask, mask_stride, err2, err2_stride, stats);
}

int hsflow_fb_planes(hsflow_ctx *c, int fwd_pair, const void *d_ub, const void *d_vb, size_t b_stride, const hsflow_fb_params *fp, uint8_t *mask,
                     size_t mask_stride, float *err2, size_t err2_stride, hsflow_fb_stats *stats)
{
    int st = check_ctx(c, fwd_pair);
    if (st) return st;
    if ((st = check_fb_planes(c, c->W, d_ub, d_vb, b_stride))) return st;
    return fb_to_host(c, fwd_pair, -1, (const float *)d_ub, (const float *)d_vb, b_stride, fp, mask, mask_stride, err2, err2_stride, stats);
}

int hsflow_set_frames_reversed(hsflow_ctx *c, int dst_pair, int src_pair)
{
    int st = check_ctx(c, dst_pair);
    if (st) return st;
    if ((st = check_ctx(c, src_pair))) return st;
    if (dst_pair == src_pair) return fail(c, HSFLOW_E_ARG, "a pair cannot be reversed onto itself");
    if (!c->frames_set) return fail(c, HSFLOW_E_STATE, "frames were not set");
    // an owed check still needs the old inputs, and a source pair whose copy was elided gets its planes first
    if ((st = settle_pending(c))) return st;
    if ((st = resolve_lazy_frames(c, false))) return st;
    // the one input path: prev := the source's curr plane, curr := its prev plane, plain gray from device memory
    return frames_in(c, dst_pair, pair_in(HSFLOW_FRAMES_GRAY8, c->dB + src_pair * c->plane, (size_t)c->P, c->dA + src_pair * c->plane, (size_t)c->P, false, true));
}

} // extern "C"
