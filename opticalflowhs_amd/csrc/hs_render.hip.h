// hs_render.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_render_flow[_device], the
// flow picture of the reference (OpticalFlowOpenCV.cpp:33-46, HSOpticalFlowOpenCL.cpp:759-769) drawn from the flow
// where the solver left it.  Two launches on the context's stream (hs_kernels_render.hip.h); a context that never
// renders allocates and launches nothing here.  hsflow_render_flow_batch_device: the pictures of consecutive pairs by
// two launches per chunk of at most HSFLOW_JPEG_BATCH_MAX.
#pragma once

namespace {

int check_render_params(hsflow_ctx *c, const hsflow_render_params *rp)
{
    if (!rp || rp->struct_size != sizeof(hsflow_render_params)) return fail(c, HSFLOW_E_ARG, "render params null or struct_size mismatch");
    if (rp->step < 1) return fail(c, HSFLOW_E_ARG, "render step must be >= 1");
    if (!std::isfinite(rp->threshold) || rp->threshold < 0.f) return fail(c, HSFLOW_E_ARG, "render threshold must be finite and >= 0");
    if (!std::isfinite(rp->scale)) return fail(c, HSFLOW_E_ARG, "render scale must be finite");
    return HSFLOW_OK;
}

// Both launches, enqueued on c's stream.  The caller has checked every argument.
int enqueue_render(hsflow_ctx *c, int pair, const hsflow_render_params &rp, uint8_t *d_rgb, size_t stride)
{
    const size_t words = (size_t)c->plane;
    if (!c->dPrio) {
        HS_HIP(c, hipMalloc((void **)&c->dPrio, words * sizeof(unsigned)));
        c->prio_planes = 1;
        c->prio_dirty = true;
    }
    if (c->prio_dirty) { // (every plane there is: a batched render may have left any of them dirty)
        HS_HIP(c, hipMemsetAsync(c->dPrio, 0, words * sizeof(unsigned) * (size_t)c->prio_planes, c->stream));
        c->prio_dirty = false;
    }
    const int gx = (c->W + rp.step - 1) / rp.step, gy = (c->H + rp.step - 1) / rp.step;
    const unsigned n = (unsigned)((long long)gx * gy); // <= W * H <= 2^30: 2n + 2 fits a word
    const unsigned dot = rp.dot_rgb[0] | (unsigned)rp.dot_rgb[1] << 8 | (unsigned)rp.dot_rgb[2] << 16;
    const unsigned line = rp.line_rgb[0] | (unsigned)rp.line_rgb[1] << 8 | (unsigned)rp.line_rgb[2] << 16;
    c->prio_dirty = true; // until the resolve pass has been enqueued behind the scatter pass
    hipLaunchKernelGGL(hsk::k_render_scatter, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, c->dU[c->cur] + pair * c->plane,
                       c->dV[c->cur] + pair * c->plane, c->dPrio, c->W, c->H, c->P, c->P, rp.step, gx, n, rp.threshold, rp.scale);
    HS_HIP(c, hipGetLastError());
    const int wide = word_aligned(d_rgb, stride);
    const dim3 grid((c->W + 1023) / 1024, c->H < 65535 ? c->H : 65535);
    hipLaunchKernelGGL(hsk::k_render_resolve, grid, dim3(256), 0, c->stream, c->dPrio, d_rgb, (long long)stride, c->W, c->H, c->P, dot, line, wide);
    HS_HIP(c, hipGetLastError());
    c->prio_dirty = false;
    c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
    return HSFLOW_OK;
}

// One priority plane per picture of a chunk of `planes`.  Grown behind a wait for the stream: what is in flight still uses
// the old ones.
int render_batch_reserve(hsflow_ctx *c, int planes)
{
    if (c->prio_planes >= planes) return HSFLOW_OK;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(c->dPrio);
    c->dPrio = nullptr; c->prio_planes = 0;
    HS_HIP(c, hipMalloc((void **)&c->dPrio, (size_t)c->plane * sizeof(unsigned) * (size_t)planes));
    c->prio_planes = planes;
    c->prio_dirty = true;
    return HSFLOW_OK;
}

// Both launches for the pairs first_pair .. first_pair + cnt - 1 (cnt <= prio_planes), picture i into pics.rgb[i].  The
// caller has checked every argument.
int enqueue_render_chunk(hsflow_ctx *c, int first_pair, int cnt, const hsflow_render_params &rp, const hsk::RenderBatchPics &pics, size_t stride)
{
    const size_t words = (size_t)c->plane;
    if (c->prio_dirty) {
        HS_HIP(c, hipMemsetAsync(c->dPrio, 0, words * sizeof(unsigned) * (size_t)c->prio_planes, c->stream));
        c->prio_dirty = false;
    }
    const int gx = (c->W + rp.step - 1) / rp.step, gy = (c->H + rp.step - 1) / rp.step;
    const unsigned n = (unsigned)((long long)gx * gy);
    const unsigned dot = rp.dot_rgb[0] | (unsigned)rp.dot_rgb[1] << 8 | (unsigned)rp.dot_rgb[2] << 16;
    const unsigned line = rp.line_rgb[0] | (unsigned)rp.line_rgb[1] << 8 | (unsigned)rp.line_rgb[2] << 16;
    c->prio_dirty = true; // until the resolve pass has been enqueued behind the scatter pass
    hipLaunchKernelGGL(hsk::k_render_scatter_batch, dim3((n + 255u) / 256u, (unsigned)cnt), dim3(256), 0, c->stream, c->dU[c->cur] + first_pair * c->plane,
                       c->dV[c->cur] + first_pair * c->plane, c->dPrio, c->plane, c->W, c->H, c->P, c->P, rp.step, gx, n, rp.threshold, rp.scale);
    HS_HIP(c, hipGetLastError());
    const dim3 grid((c->W + 1023) / 1024, c->H < 65535 ? c->H : 65535, (unsigned)cnt);
    hipLaunchKernelGGL(hsk::k_render_resolve_batch, grid, dim3(256), 0, c->stream, c->dPrio, c->plane, pics, (long long)stride, c->W, c->H, c->P, dot, line);
    HS_HIP(c, hipGetLastError());
    c->prio_dirty = false;
    c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
    return HSFLOW_OK;
}

} // namespace

extern "C" {

void hsflow_default_render_params(hsflow_render_params *rp, int preset)
{
    if (!rp) return;
    std::memset(rp, 0, sizeof(*rp));
    rp->struct_size = sizeof(*rp);
    rp->step = 4;                                        // OpticalFlowOpenCV.cpp:35-36, HSOpticalFlowOpenCL.cpp:760-761
    const bool cl = preset == HSFLOW_RENDER_CL;
    rp->threshold = cl ? 0.5f : 1.0f;                    // HSOpticalFlowOpenCL.cpp:764 / OpticalFlowOpenCV.cpp:40
    rp->scale = cl ? 1.0f : 0.5f;                        // HSOpticalFlowOpenCL.cpp:767 / OpticalFlowOpenCV.cpp:44
    rp->dot_rgb[2] = 255;                                // CV_RGB(0, 0, 255)
    rp->line_rgb[0] = 255;                               // CV_RGB(255, 0, 0)
}

int hsflow_render_flow_device(hsflow_ctx *c, int pair, const hsflow_render_params *rp, void *d_rgb, size_t stride)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = check_render_params(c, rp))) return st;
    if (!d_rgb) return fail(c, HSFLOW_E_ARG, "null picture pointer");
    if (stride < (size_t)c->W * 3) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    if ((st = settle_pending(c))) return st; // (hs_postops.hip.h, rule 1)
    return enqueue_render(c, pair, *rp, (uint8_t *)d_rgb, stride);
}

int hsflow_render_flow_batch_device(hsflow_ctx *c, int first_pair, int n, const hsflow_render_params *rp, void *const *d_rgb, size_t stride)
{
    int st = check_ctx(c, 0), maxb = 0;
    if (st) return st;
    if ((st = check_batch_pairs(c, first_pair, n))) return st;
    if ((st = check_render_params(c, rp))) return st;
    if (!d_rgb) return fail(c, HSFLOW_E_ARG, "null picture list");
    for (int i = 0; i < n; i++)
        if (!d_rgb[i]) return fail(c, HSFLOW_E_ARG, "picture " + std::to_string(i) + ": null picture pointer");
    if (stride < (size_t)c->W * 3) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    if ((st = batch_device_begin(c, nullptr, &maxb))) return st;
    if ((st = render_batch_reserve(c, n < maxb ? n : maxb))) return st;
    for (const hsjpeg_plan::Chunk &ch : hsjpeg_plan::chunks(n, maxb)) {
        hsk::RenderBatchPics pics{};
        for (int k = 0; k < ch.count; k++) {
            pics.rgb[k] = (uint8_t *)d_rgb[ch.first + k];
            if (word_aligned(d_rgb[ch.first + k], stride)) pics.wide |= 1u << k;
        }
        if ((st = enqueue_render_chunk(c, first_pair + ch.first, ch.count, *rp, pics, stride))) return st;
    }
    return HSFLOW_OK;
}

int hsflow_render_flow(hsflow_ctx *c, int pair, const hsflow_render_params *rp, uint8_t *rgb, size_t stride)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = check_render_params(c, rp))) return st;
    if (!rgb) return fail(c, HSFLOW_E_ARG, "null picture pointer");
    const size_t rowb = (size_t)c->W * 3;
    if (stride < rowb) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    if ((st = settle_pending(c))) return st;
    if (!c->dRgb) HS_HIP(c, hipMalloc((void **)&c->dRgb, rowb * c->H));
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    if ((st = enqueue_render(c, pair, *rp, c->dRgb, rowb))) return st;
    HS_HIP(c, copy_rows_async(c, rgb, stride, c->dRgb, rowb, rowb, c->H, hipMemcpyDeviceToHost));
    return sync_finish(c, marked);
}

int hsflow_render_line_pixels(int x0, int y0, int x1, int y1, int width, int height, int32_t *xy, int capacity)
{
    if (width <= 0 || height <= 0 || capacity < 0 || (capacity > 0 && !xy)) return -1;
    hsline::Walk w = hsline::clip(x0, y0, x1, y1, width, height);
    const long long n = w.count;
    for (long long i = 0; i < n; i++) {
        if (i < capacity) { xy[2 * i] = w.x; xy[2 * i + 1] = w.y; }
        hsline::advance(w);
    }
    return (int)n;
}

} // extern "C"
