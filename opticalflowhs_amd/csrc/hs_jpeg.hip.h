// hs_jpeg.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_jpeg_*, hsflow_render_flow_jpeg*,
// the file the reference's runFromImg ends in (cvSaveImage, OpticalFlowOpenCV.cpp:47, HSOpticalFlowOpenCL.cpp:771) from a
// picture that never leaves the device.  Seven launches and one memset on the context's stream
// (hs_kernels_jpeg.hip.h); a context that never encodes allocates and launches nothing here.
#pragma once

namespace {

void jpeg_release(hsflow_ctx *c)
{
    hipFree(c->jpeg.base);
    for (auto &kv : c->jpeg.tables) hipFree(kv.second);
    hipFree(c->jpeg.out);
    if (c->jpeg.hSize) hipHostFree(c->jpeg.hSize);
    c->jpeg = hsflow_ctx::JpegScratch();
}

int check_jpeg_args(hsflow_ctx *c, int quality, const void *d_jpeg, const void *d_bytes)
{
    if (quality < 1 || quality > 100) return fail(c, HSFLOW_E_ARG, "jpeg quality must be 1 .. 100");
    if (!d_jpeg || !d_bytes) return fail(c, HSFLOW_E_ARG, "null jpeg or size pointer");
    if (c->W > 65535 || c->H > 65535) return fail(c, HSFLOW_E_SIZE, "a JPEG picture has at most 65535 columns and rows");
    return HSFLOW_OK;
}

// The scratch of every encode of this context, one allocation, and the tables of `quality`.
int jpeg_prepare(hsflow_ctx *c, int quality, hsjpeg::Tables **tab)
{
    hsflow_ctx::JpegScratch &j = c->jpeg;
    if (!j.base) {
        const long long nb = 6ll * hsjpeg::mcus_x(c->W) * hsjpeg::mcus_y(c->H);
        const size_t raw_bytes = ((size_t)nb * hsjpeg::kMaxBlockBytes + hsk::kJpegChunk - 1) / hsk::kJpegChunk * hsk::kJpegChunk;
        const long long nchunks = (long long)(raw_bytes / hsk::kJpegChunk);
        auto up = [](size_t v) { return (v + 255) / 256 * 256; };
        const size_t o_coef = 0, o_raw = o_coef + up((size_t)nb * 128), o_off = o_raw + up(raw_bytes), o_ffoff = o_off + up(((size_t)nb + 1) * 8),
                     o_len = o_ffoff + up(((size_t)nchunks + 1) * 8), o_ff = o_len + up((size_t)nb * 4), o_size = o_ff + up((size_t)nchunks * 4),
                     total = o_size + 256;
        HS_HIP(c, hipMalloc(&j.base, total));
        uint8_t *p = (uint8_t *)j.base;
        j.coef = (int16_t *)(p + o_coef); j.raw = (uint32_t *)(p + o_raw); j.off = (uint64_t *)(p + o_off); j.ffoff = (uint64_t *)(p + o_ffoff);
        j.len = (uint32_t *)(p + o_len); j.ff = (uint32_t *)(p + o_ff); j.size = (uint64_t *)(p + o_size);
        j.nb = nb; j.nchunks = nchunks; j.raw_bytes = raw_bytes;
    }
    auto it = j.tables.find(quality);
    if (it == j.tables.end()) { // filled once per quality (the size is the context's); a blocking copy into memory nothing uses yet
        hsjpeg::Tables host, *dev = nullptr;
        hsjpeg::build_tables(host, c->W, c->H, quality);
        HS_HIP(c, hipMalloc((void **)&dev, sizeof(hsjpeg::Tables)));
        const hipError_t e = hipMemcpy(dev, &host, sizeof(host), hipMemcpyHostToDevice);
        if (e != hipSuccess) { hipFree(dev); HS_HIP(c, e); }
        it = j.tables.emplace(quality, dev).first;
    }
    *tab = it->second;
    return HSFLOW_OK;
}

// All launches of one encode, enqueued on c's stream.  The caller has checked every argument.  d_bytes == nullptr: the
// size goes to the context's own word (jpeg.size, which exists only once jpeg_prepare has run).
int enqueue_jpeg(hsflow_ctx *c, const uint8_t *d_rgb, size_t stride, int quality, uint8_t *d_jpeg, size_t capacity, uint64_t *d_bytes)
{
    hsjpeg::Tables *tab = nullptr;
    int st = jpeg_prepare(c, quality, &tab);
    if (st) return st;
    hsflow_ctx::JpegScratch &j = c->jpeg;
    if (!d_bytes) d_bytes = j.size;
    const int MW = hsjpeg::mcus_x(c->W), MH = hsjpeg::mcus_y(c->H);
    const int wide = (((uintptr_t)d_rgb | stride) & 3u) == 0;
    const unsigned gb = (unsigned)((j.nb + 255) / 256), gc = (unsigned)((j.nchunks + 255) / 256);
    HS_HIP(c, hipMemsetAsync(j.raw, 0, j.raw_bytes, c->stream));
    hipLaunchKernelGGL(hsk::k_jpeg_blocks, dim3((MW + hsk::kJpegStripMcus - 1) / hsk::kJpegStripMcus, MH), dim3(256), 0, c->stream, d_rgb,
                       (long long)stride, c->W, c->H, MW, tab, j.coef, wide);
    hipLaunchKernelGGL(hsk::k_jpeg_lengths, dim3(gb), dim3(256), 0, c->stream, tab, j.coef, c->W, c->H, MW, j.nb, j.len);
    hipLaunchKernelGGL(hsk::k_jpeg_scan, dim3(1), dim3(hsk::kJpegScanLanes), 0, c->stream, j.len, j.off, j.nb, (const uint64_t *)nullptr);
    hipLaunchKernelGGL(hsk::k_jpeg_emit, dim3(gb), dim3(256), 0, c->stream, tab, j.coef, c->W, c->H, MW, j.nb, j.off, j.raw);
    hipLaunchKernelGGL(hsk::k_jpeg_count_ff, dim3(gc), dim3(256), 0, c->stream, j.raw, j.off + j.nb, j.nchunks, j.ff);
    hipLaunchKernelGGL(hsk::k_jpeg_scan, dim3(1), dim3(hsk::kJpegScanLanes), 0, c->stream, j.ff, j.ffoff, j.nchunks, j.off + j.nb);
    hipLaunchKernelGGL(hsk::k_jpeg_stuff, dim3(gc), dim3(256), 0, c->stream, tab, j.raw, j.off + j.nb, j.ffoff, j.nchunks, d_jpeg,
                       (unsigned long long)capacity, d_bytes);
    HS_HIP(c, hipGetLastError());
    return HSFLOW_OK;
}

// The checks the two render-and-encode forms share, the owed ITER|EPS check settled, the context's own picture there.
int render_jpeg_begin(hsflow_ctx *c, int pair, const hsflow_render_params *rp, int quality, const void *jpeg, const void *bytes)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = check_render_params(c, rp))) return st;
    if ((st = check_jpeg_args(c, quality, jpeg, bytes))) return st;
    if ((st = settle_pending(c))) return st;
    if (!c->dRgb) HS_HIP(c, hipMalloc((void **)&c->dRgb, (size_t)c->W * 3 * c->H));
    return HSFLOW_OK;
}

} // namespace

extern "C" {

size_t hsflow_jpeg_bound(int width, int height) { return hsjpeg::bound(width, height); }

int hsflow_jpeg_encode_host(const uint8_t *rgb, size_t stride, int width, int height, int quality, uint8_t *jpeg, size_t capacity, size_t *bytes)
{
    switch (hsjpeg::encode_host(rgb, stride, width, height, quality, jpeg, capacity, bytes)) {
    case 0: return HSFLOW_OK;
    case 1: return fail(nullptr, HSFLOW_E_ARG, "hsflow_jpeg_encode_host: null pointer or quality outside 1 .. 100");
    case 2: return fail(nullptr, HSFLOW_E_SIZE, "hsflow_jpeg_encode_host: size outside 1 .. 65535, stride smaller than 3*width, or capacity smaller than the file");
    default: return fail(nullptr, HSFLOW_E_OOM, "hsflow_jpeg_encode_host: host allocation failed");
    }
}

int hsflow_jpeg_encode_device(hsflow_ctx *c, const void *d_rgb, size_t stride, int quality, void *d_jpeg, size_t capacity, uint64_t *d_bytes)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (!d_rgb) return fail(c, HSFLOW_E_ARG, "null picture pointer");
    if ((st = check_jpeg_args(c, quality, d_jpeg, d_bytes))) return st;
    if ((uintptr_t)d_bytes & 7u) return fail(c, HSFLOW_E_ARG, "the size word must be 8-byte aligned");
    if (stride < (size_t)c->W * 3) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    return enqueue_jpeg(c, (const uint8_t *)d_rgb, stride, quality, (uint8_t *)d_jpeg, capacity, d_bytes);
}

int hsflow_render_flow_jpeg_device(hsflow_ctx *c, int pair, const hsflow_render_params *rp, int quality, void *d_jpeg, size_t capacity,
                                   uint64_t *d_bytes)
{
    int st = render_jpeg_begin(c, pair, rp, quality, d_jpeg, d_bytes);
    if (st) return st;
    if ((uintptr_t)d_bytes & 7u) return fail(c, HSFLOW_E_ARG, "the size word must be 8-byte aligned");
    const size_t rowb = (size_t)c->W * 3;
    if ((st = enqueue_render(c, pair, *rp, c->dRgb, rowb))) return st;
    return enqueue_jpeg(c, c->dRgb, rowb, quality, (uint8_t *)d_jpeg, capacity, d_bytes);
}

int hsflow_render_flow_jpeg(hsflow_ctx *c, int pair, const hsflow_render_params *rp, int quality, uint8_t *jpeg, size_t capacity, size_t *bytes)
{
    int st = render_jpeg_begin(c, pair, rp, quality, jpeg, bytes);
    if (st) return st;
    hsflow_ctx::JpegScratch &j = c->jpeg;
    const size_t bound = hsjpeg::bound(c->W, c->H), want = capacity < bound ? (capacity ? capacity : 1) : bound;
    if (j.out_bytes < want) { // (the synchronous forms leave nothing in flight that reads the old one)
        hipFree(j.out);
        j.out = nullptr; j.out_bytes = 0;
        HS_HIP(c, hipMalloc((void **)&j.out, want));
        j.out_bytes = want;
    }
    if (!j.hSize) HS_HIP(c, hipHostMalloc((void **)&j.hSize, 64, hipHostMallocDefault));
    if (!c->evRender) HS_HIP(c, hipEventCreateWithFlags(&c->evRender, hipEventDisableTiming));
    const bool marked = c->last_marked;
    const size_t rowb = (size_t)c->W * 3, cap = capacity < bound ? capacity : bound;
    if ((st = enqueue_render(c, pair, *rp, c->dRgb, rowb))) return st;
    if ((st = enqueue_jpeg(c, c->dRgb, rowb, quality, j.out, cap, nullptr))) return st;
    // the size word first, then that many bytes: only the file crosses; what THIS context enqueued is all that is waited for
    HS_HIP(c, hipMemcpyAsync(j.hSize, j.size, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HS_HIP(c, hipEventRecord(c->evRender, c->stream));
    HS_HIP(c, hipEventSynchronize(c->evRender));
    const uint64_t size = *j.hSize;
    *bytes = (size_t)size;
    if (size <= capacity) {
        HS_HIP(c, hipMemcpyAsync(jpeg, j.out, (size_t)size, hipMemcpyDeviceToHost, c->stream));
        HS_HIP(c, hipEventRecord(c->evRender, c->stream));
        HS_HIP(c, hipEventSynchronize(c->evRender));
    }
    c->last_marked = marked; // nothing of this call is in flight any more: the solve's marker speaks for the context again
    if (size > capacity) return fail(c, HSFLOW_E_SIZE, "capacity smaller than the file (hsflow_jpeg_bound always suffices)");
    return check_persist(c);
}

} // extern "C"
