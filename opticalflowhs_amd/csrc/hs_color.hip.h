// hs_color.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_color_flow*, the dense colour
// picture of the flow (hs_color_rule.h: the Middlebury wheel) drawn from the flow where the solver left it.  Per chunk of
// at most HSFLOW_JPEG_BATCH_MAX pictures: with the scale taken from the picture one memset of the chunk's scale words and
// two launches, with a fixed scale one launch (hs_kernels_color.hip.h).  The single forms are batches of one.  A context
// that never colours allocates and launches nothing here.
#pragma once

namespace {

int check_color_params(hsflow_ctx *c, const hsflow_color_params *cp)
{
    if (!cp || cp->struct_size != sizeof(hsflow_color_params)) return fail(c, HSFLOW_E_ARG, "color params null or struct_size mismatch");
    if (cp->scale_mode != HSFLOW_COLOR_SCALE_AUTO && cp->scale_mode != HSFLOW_COLOR_SCALE_FIXED) return fail(c, HSFLOW_E_ARG, "unknown color scale mode");
    if (cp->scale_mode == HSFLOW_COLOR_SCALE_FIXED && !(std::isfinite(cp->max_flow) && cp->max_flow > 0.f))
        return fail(c, HSFLOW_E_ARG, "color max_flow must be finite and > 0");
    return HSFLOW_OK;
}

// The scale words of a chunk: kRenderBatchMax of them, whatever the chunk size.
int color_reserve(hsflow_ctx *c)
{
    if (!c->dColorScale) HS_HIP(c, hipMalloc((void **)&c->dColorScale, sizeof(unsigned) * hsk::kRenderBatchMax));
    return HSFLOW_OK;
}

// The launches for the pairs first_pair .. first_pair + cnt - 1 (cnt <= kRenderBatchMax), picture i into pics.rgb[i].  The
// caller has checked every argument and color_reserve has run.
int enqueue_color_chunk(hsflow_ctx *c, int first_pair, int cnt, const hsflow_color_params &cp, const hsk::RenderBatchPics &pics, size_t stride)
{
    const float *u = c->dU[c->cur] + first_pair * c->plane, *v = c->dV[c->cur] + first_pair * c->plane;
    const bool fixed = cp.scale_mode == HSFLOW_COLOR_SCALE_FIXED;
    const dim3 grid((c->W + 1023) / 1024, c->H < 65535 ? c->H : 65535, (unsigned)cnt);
    if (!fixed) {
        HS_HIP(c, hipMemsetAsync(c->dColorScale, 0, sizeof(unsigned) * (size_t)cnt, c->stream));
        hipLaunchKernelGGL(hsk::k_color_max_batch, grid, dim3(256), 0, c->stream, u, v, c->plane, c->W, c->H, c->P, c->dColorScale);
        HS_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(hsk::k_color_batch, grid, dim3(256), 0, c->stream, u, v, c->plane, pics, (long long)stride, c->W, c->H, c->P,
                       fixed ? (const unsigned *)nullptr : c->dColorScale, fixed ? cp.max_flow : 0.f);
    HS_HIP(c, hipGetLastError());
    c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
    return HSFLOW_OK;
}

} // namespace

extern "C" {

void hsflow_default_color_params(hsflow_color_params *cp)
{
    if (!cp) return;
    std::memset(cp, 0, sizeof(*cp));
    cp->struct_size = sizeof(*cp);
    cp->scale_mode = HSFLOW_COLOR_SCALE_AUTO;
}

int hsflow_color_flow_host(const float *u, size_t u_stride, const float *v, size_t v_stride, int width, int height, const hsflow_color_params *cp,
                           uint8_t *rgb, size_t stride, float *scale_used)
{
    int st = check_color_params(nullptr, cp);
    if (st) return st;
    if (!u || !v || !rgb) return fail(nullptr, HSFLOW_E_ARG, "hsflow_color_flow_host: null pointer");
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_color_flow_host: width and height must be positive");
    if (u_stride < (size_t)width * 4 || v_stride < (size_t)width * 4 || ((u_stride | v_stride) & 3u))
        return fail(nullptr, HSFLOW_E_SIZE, "hsflow_color_flow_host: flow stride smaller than 4*width or no multiple of 4");
    if (stride < (size_t)width * 3) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_color_flow_host: picture stride smaller than 3*width");
    const float m = hscolor::color_rows(u, u_stride, v, v_stride, width, height, cp->scale_mode == HSFLOW_COLOR_SCALE_FIXED ? cp->max_flow : 0.f, rgb, stride);
    if (scale_used) *scale_used = m;
    return HSFLOW_OK;
}

int hsflow_color_flow_batch_device(hsflow_ctx *c, int first_pair, int n, const hsflow_color_params *cp, void *const *d_rgb, size_t stride)
{
    int st = check_ctx(c, 0), maxb = 0;
    if (st) return st;
    if ((st = check_batch_pairs(c, first_pair, n))) return st;
    if ((st = check_color_params(c, cp))) return st;
    if (!d_rgb) return fail(c, HSFLOW_E_ARG, "null picture list");
    for (int i = 0; i < n; i++)
        if (!d_rgb[i]) return fail(c, HSFLOW_E_ARG, "picture " + std::to_string(i) + ": null picture pointer");
    if (stride < (size_t)c->W * 3) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    if ((st = batch_device_begin(c, nullptr, &maxb))) return st;
    if ((st = color_reserve(c))) return st;
    for (const hsjpeg_plan::Chunk &ch : hsjpeg_plan::chunks(n, maxb)) {
        hsk::RenderBatchPics pics{};
        for (int k = 0; k < ch.count; k++) {
            pics.rgb[k] = (uint8_t *)d_rgb[ch.first + k];
            if (word_aligned(d_rgb[ch.first + k], stride)) pics.wide |= 1u << k;
        }
        if ((st = enqueue_color_chunk(c, first_pair + ch.first, ch.count, *cp, pics, stride))) return st;
    }
    return HSFLOW_OK;
}

int hsflow_color_flow_device(hsflow_ctx *c, int pair, const hsflow_color_params *cp, void *d_rgb, size_t stride)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!d_rgb) return fail(c, HSFLOW_E_ARG, "null picture pointer");
    void *const list[1] = {d_rgb};
    return hsflow_color_flow_batch_device(c, pair, 1, cp, list, stride);
}

int hsflow_color_flow(hsflow_ctx *c, int pair, const hsflow_color_params *cp, uint8_t *rgb, size_t stride, float *scale_used)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = check_color_params(c, cp))) return st;
    if (!rgb) return fail(c, HSFLOW_E_ARG, "null picture pointer");
    const size_t rowb = (size_t)c->W * 3;
    if (stride < rowb) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    if ((st = settle_pending(c))) return st;
    if ((st = color_reserve(c))) return st;
    if (!c->dRgb) HS_HIP(c, hipMalloc((void **)&c->dRgb, rowb * c->H));
    if (!c->hColorScale) HS_HIP(c, hipHostMalloc((void **)&c->hColorScale, 64, hipHostMallocDefault));
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    const bool fixed = cp->scale_mode == HSFLOW_COLOR_SCALE_FIXED;
    hsk::RenderBatchPics pics{};
    pics.rgb[0] = c->dRgb;
    pics.wide = (uint32_t)word_aligned(c->dRgb, rowb);
    if ((st = enqueue_color_chunk(c, pair, 1, *cp, pics, rowb))) return st;
    HS_HIP(c, copy_rows_async(c, rgb, stride, c->dRgb, rowb, rowb, c->H, hipMemcpyDeviceToHost));
    if (scale_used && !fixed) HS_HIP(c, hipMemcpyAsync(c->hColorScale, c->dColorScale, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    if ((st = sync_wait(c))) return st;
    if (scale_used) *scale_used = fixed ? cp->max_flow : hscolor::auto_scale(*c->hColorScale);
    sync_restore(c, marked);
    return check_persist(c);
}

} // extern "C"
