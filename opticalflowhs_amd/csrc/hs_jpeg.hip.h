// hs_jpeg.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_jpeg_*, hsflow_render_flow_jpeg*,
// the file the reference's runFromImg ends in (cvSaveImage, OpticalFlowOpenCV.cpp:47, HSOpticalFlowOpenCL.cpp:771) from a
// picture that never leaves the device.  Seven launches and one memset on the context's stream
// (hs_kernels_jpeg.hip.h); a context that never encodes allocates and launches nothing here.
// hsflow_jpeg_encode_batch_device, hsflow_render_flow_jpeg_batch[_device]: many pictures by one memset and one set of
// launches per chunk of at most HSFLOW_JPEG_BATCH_MAX (what cvSaveImage does once per run, OpticalFlowOpenCV.cpp:32-47,
// HSOpticalFlowOpenCL.cpp:759-771, for every pair of the context at once), scratch laid out by hs_jpeg_batch_plan.h.
#pragma once

#include "hs_jpeg_batch_plan.h"

namespace {

void jpeg_release(hsflow_ctx *c)
{
    hipFree(c->jpeg.base);
    for (auto &kv : c->jpeg.tables) hipFree(kv.second);
    hipFree(c->jpeg.out);
    if (c->jpeg.hSize) hipHostFree(c->jpeg.hSize);
    c->jpeg = hsflow_ctx::JpegScratch();
    hipFree(c->jpeg_batch.base);
    hipFree(c->jpeg_batch.rgb);
    hipFree(c->jpeg_batch.out);
    if (c->jpeg_batch.hSize) hipHostFree(c->jpeg_batch.hSize);
    c->jpeg_batch = hsflow_ctx::JpegBatchScratch();
}

int check_jpeg_args(hsflow_ctx *c, int quality, const void *d_jpeg, const void *d_bytes)
{
    if (quality < 1 || quality > 100) return fail(c, HSFLOW_E_ARG, "jpeg quality must be 1 .. 100");
    if (!d_jpeg || !d_bytes) return fail(c, HSFLOW_E_ARG, "null jpeg or size pointer");
    if (c->W > 65535 || c->H > 65535) return fail(c, HSFLOW_E_SIZE, "a JPEG picture has at most 65535 columns and rows");
    return HSFLOW_OK;
}

// The tables and header of `quality` on the device, filled once per quality (the size is the context's): a blocking
// copy into memory nothing uses yet.
int jpeg_tables(hsflow_ctx *c, int quality, hsjpeg::Tables **tab)
{
    hsflow_ctx::JpegScratch &j = c->jpeg;
    auto it = j.tables.find(quality);
    if (it == j.tables.end()) {
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

// The scratch of every single encode of this context, one allocation, and the tables of `quality`.
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
    return jpeg_tables(c, quality, tab);
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
    const int wide = word_aligned(d_rgb, stride);
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

// ---- a batch of pictures ------------------------------------------------------------------------------------------------

static_assert(hsjpeg_plan::kMaxBlockBytes == (size_t)hsjpeg::kMaxBlockBytes && hsjpeg_plan::kChunkBytes == (size_t)hsk::kJpegChunk,
              "hs_jpeg_batch_plan.h restates two constants");
static_assert(sizeof(hsk::JpegBatchPic) == 32, "one picture of a batch is 32 bytes of kernel arguments");

// The batched scratch for a chunk of `pictures`.  Grown behind a wait for the stream: what is in flight still uses the
// old one.
int jpeg_batch_reserve(hsflow_ctx *c, int pictures)
{
    hsflow_ctx::JpegBatchScratch &b = c->jpeg_batch;
    if (b.pictures >= pictures) return HSFLOW_OK;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(b.base);
    b.base = nullptr; b.pictures = 0;
    HS_HIP(c, hipMalloc(&b.base, hsjpeg_plan::layout(c->W, c->H, pictures).total));
    b.pictures = pictures;
    return HSFLOW_OK;
}

// The context's own pictures for a chunk of `pictures`: 3*W x H bytes each, 256-byte multiples apart.
size_t jpeg_batch_rgb_span(const hsflow_ctx *c) { return hsjpeg_plan::up256((size_t)c->W * 3 * c->H); }

int jpeg_batch_reserve_rgb(hsflow_ctx *c, int pictures)
{
    hsflow_ctx::JpegBatchScratch &b = c->jpeg_batch;
    if (b.rgb_pictures >= pictures) return HSFLOW_OK;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(b.rgb);
    b.rgb = nullptr; b.rgb_pictures = 0;
    HS_HIP(c, hipMalloc((void **)&b.rgb, jpeg_batch_rgb_span(c) * (size_t)pictures));
    b.rgb_pictures = pictures;
    return HSFLOW_OK;
}

// The size words of a chunk inside the batched scratch (the synchronous form's; the device forms write the caller's).
uint64_t *jpeg_batch_size_words(hsflow_ctx *c)
{
    return (uint64_t *)((uint8_t *)c->jpeg_batch.base + hsjpeg_plan::layout(c->W, c->H, c->jpeg_batch.pictures).o_size);
}

// One memset and all launches for a chunk of cnt pictures (cnt <= jpeg_batch.pictures), enqueued on c's stream; picture
// i's size goes to d_bytes[i].  The caller has checked every argument.
int enqueue_jpeg_chunk(hsflow_ctx *c, const hsjpeg::Tables *tab, const hsk::JpegBatchPics &pics, int cnt, size_t stride, uint64_t *d_bytes)
{
    const hsjpeg_plan::Layout l = hsjpeg_plan::layout(c->W, c->H, c->jpeg_batch.pictures);
    uint8_t *p = (uint8_t *)c->jpeg_batch.base;
    const hsk::JpegBatchScratch sc{p + l.o_coef, p + l.o_raw, p + l.o_off, p + l.o_ffoff, p + l.o_len, p + l.o_ff,
                                   l.s.s_coef, l.s.s_raw, l.s.s_off, l.s.s_ffoff, l.s.s_len, l.s.s_ff};
    const int MW = hsjpeg::mcus_x(c->W), MH = hsjpeg::mcus_y(c->H);
    const long long nb = l.s.nb, nchunks = l.s.nchunks;
    const unsigned gb = (unsigned)((nb + 255) / 256), gc = (unsigned)((nchunks + 255) / 256), np = (unsigned)cnt;
    HS_HIP(c, hipMemsetAsync(sc.raw, 0, l.s.s_raw * (size_t)cnt, c->stream)); // the chunk's raw streams lie behind each other
    hipLaunchKernelGGL(hsk::k_jpeg_blocks_batch, dim3((MW + hsk::kJpegStripMcus - 1) / hsk::kJpegStripMcus, MH, np), dim3(256), 0, c->stream, pics,
                       (long long)stride, c->W, c->H, MW, tab, sc);
    hipLaunchKernelGGL(hsk::k_jpeg_lengths_batch, dim3(gb, np), dim3(256), 0, c->stream, tab, sc, c->W, c->H, MW, nb);
    hipLaunchKernelGGL(hsk::k_jpeg_scan_batch, dim3(np), dim3(hsk::kJpegScanLanes), 0, c->stream, sc, nb, nchunks, 0);
    hipLaunchKernelGGL(hsk::k_jpeg_emit_batch, dim3(gb, np), dim3(256), 0, c->stream, tab, sc, c->W, c->H, MW, nb);
    hipLaunchKernelGGL(hsk::k_jpeg_count_ff_batch, dim3(gc, np), dim3(256), 0, c->stream, sc, nb, nchunks);
    hipLaunchKernelGGL(hsk::k_jpeg_scan_batch, dim3(np), dim3(hsk::kJpegScanLanes), 0, c->stream, sc, nb, nchunks, 1);
    hipLaunchKernelGGL(hsk::k_jpeg_stuff_batch, dim3(gc, np), dim3(256), 0, c->stream, tab, sc, nb, nchunks, pics, d_bytes);
    HS_HIP(c, hipGetLastError());
    return HSFLOW_OK;
}

hsk::JpegBatchPic jpeg_batch_pic(const void *rgb, size_t stride, void *out, size_t capacity)
{
    return hsk::JpegBatchPic{(const uint8_t *)rgb, (uint8_t *)out, (unsigned long long)capacity, word_aligned(rgb, stride), 0};
}

// What the batched encodes check of the file side: quality, the lists, the context's size.
int check_jpeg_batch_args(hsflow_ctx *c, int n, int quality, const void *const *list, const void *bytes)
{
    if (quality < 1 || quality > 100) return fail(c, HSFLOW_E_ARG, "jpeg quality must be 1 .. 100");
    if (!list || !bytes) return fail(c, HSFLOW_E_ARG, "null jpeg list or size pointer");
    for (int i = 0; i < n; i++)
        if (!list[i]) return fail(c, HSFLOW_E_ARG, "picture " + std::to_string(i) + ": null jpeg pointer");
    if (c->W > 65535 || c->H > 65535) return fail(c, HSFLOW_E_SIZE, "a JPEG picture has at most 65535 columns and rows");
    return HSFLOW_OK;
}

// What a batch draws in front of its encode: the reference's arrows (rp) or the colour picture (cp, hs_color.hip.h).
struct Drawing {
    bool color;
    const hsflow_render_params *rp;
    const hsflow_color_params *cp;
};

// The checks the batched draw-and-encode forms share, then the owed ITER|EPS check settled and everything a chunk
// needs on the device there.  *maxb: the chunk size of this call.
int render_jpeg_batch_begin(hsflow_ctx *c, int first_pair, int n, const Drawing &d, int quality, const void *const *jpeg, const void *bytes,
                            bool aligned8, int *maxb, hsjpeg::Tables **tab)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = check_batch_pairs(c, first_pair, n))) return st;
    if ((st = d.color ? check_color_params(c, d.cp) : check_render_params(c, d.rp))) return st;
    if ((st = check_jpeg_batch_args(c, n, quality, jpeg, bytes))) return st;
    if (aligned8 && ((uintptr_t)bytes & 7u)) return fail(c, HSFLOW_E_ARG, "the size words must be 8-byte aligned");
    if ((st = batch_device_begin(c, nullptr, maxb))) return st;
    const int most = n < *maxb ? n : *maxb;
    if ((st = jpeg_tables(c, quality, tab))) return st;
    if ((st = d.color ? color_reserve(c) : render_batch_reserve(c, most))) return st;
    if ((st = jpeg_batch_reserve_rgb(c, most))) return st;
    return jpeg_batch_reserve(c, most);
}

// The pictures of cnt pairs from first_pair on into the context's own pictures, and their encodes into out[k] /
// d_bytes[k], behind each other on the stream.
int enqueue_render_jpeg_chunk(hsflow_ctx *c, int first_pair, int cnt, const Drawing &d, const hsjpeg::Tables *tab, uint8_t *const *out,
                              size_t capacity, uint64_t *d_bytes)
{
    const size_t rowb = (size_t)c->W * 3, span = jpeg_batch_rgb_span(c);
    hsk::RenderBatchPics rpics{};
    hsk::JpegBatchPics jpics{};
    for (int k = 0; k < cnt; k++) {
        uint8_t *pic = c->jpeg_batch.rgb + span * (size_t)k;
        rpics.rgb[k] = pic;
        jpics.p[k] = jpeg_batch_pic(pic, rowb, out[k], capacity);
        if (jpics.p[k].wide) rpics.wide |= 1u << k;
    }
    int st = d.color ? enqueue_color_chunk(c, first_pair, cnt, *d.cp, rpics, rowb) : enqueue_render_chunk(c, first_pair, cnt, *d.rp, rpics, rowb);
    if (st) return st;
    return enqueue_jpeg_chunk(c, tab, jpics, cnt, rowb, d_bytes);
}

// hsflow_render_flow_jpeg_batch_device and hsflow_color_flow_jpeg_batch_device: the pictures of a batch drawn into the
// context's own and encoded behind each other on the stream, only enqueued.
int draw_jpeg_batch_device(hsflow_ctx *c, int first_pair, int n, const Drawing &d, int quality, void *const *d_jpeg, size_t capacity, uint64_t *d_bytes)
{
    int maxb = 0;
    hsjpeg::Tables *tab = nullptr;
    int st = render_jpeg_batch_begin(c, first_pair, n, d, quality, d_jpeg, d_bytes, true, &maxb, &tab);
    if (st) return st;
    for (const hsjpeg_plan::Chunk &ch : hsjpeg_plan::chunks(n, maxb))
        if ((st = enqueue_render_jpeg_chunk(c, first_pair + ch.first, ch.count, d, tab, (uint8_t *const *)d_jpeg + ch.first, capacity, d_bytes + ch.first)))
            return st;
    return HSFLOW_OK;
}

// hsflow_render_flow_jpeg_batch and hsflow_color_flow_jpeg_batch: the same into host memory, complete on return.
int draw_jpeg_batch(hsflow_ctx *c, int first_pair, int n, const Drawing &d, int quality, uint8_t *const *jpeg, size_t capacity, size_t *bytes)
{
    int maxb = 0;
    hsjpeg::Tables *tab = nullptr;
    int st = render_jpeg_batch_begin(c, first_pair, n, d, quality, (const void *const *)jpeg, bytes, false, &maxb, &tab);
    if (st) return st;
    hsflow_ctx::JpegBatchScratch &b = c->jpeg_batch;
    const int most = n < maxb ? n : maxb;
    const size_t bound = hsjpeg::bound(c->W, c->H), cap = capacity < bound ? capacity : bound, slot = hsjpeg_plan::up256(cap ? cap : 1);
    if (b.slot < slot || b.out_pictures < most) { // (the synchronous form leaves nothing in flight that writes the old ones)
        const size_t s = b.slot > slot ? b.slot : slot;
        const int pictures = b.out_pictures > most ? b.out_pictures : most;
        hipFree(b.out);
        b.out = nullptr; b.slot = 0; b.out_pictures = 0;
        HS_HIP(c, hipMalloc((void **)&b.out, s * (size_t)pictures));
        b.slot = s; b.out_pictures = pictures;
    }
    if (!b.hSize) HS_HIP(c, hipHostMalloc((void **)&b.hSize, sizeof(uint64_t) * hsk::kJpegBatchMax, hipHostMallocDefault));
    bool marked = false, fits = true;
    if ((st = sync_begin(c, &marked))) return st;
    for (const hsjpeg_plan::Chunk &ch : hsjpeg_plan::chunks(n, maxb)) {
        uint8_t *out[hsk::kJpegBatchMax];
        for (int k = 0; k < ch.count; k++) out[k] = b.out + b.slot * (size_t)k;
        uint64_t *words = jpeg_batch_size_words(c);
        if ((st = enqueue_render_jpeg_chunk(c, first_pair + ch.first, ch.count, d, tab, out, cap, words))) return st;
        // the chunk's size words in one copy, then each file's bytes: only the files cross, and what THIS context enqueued
        // is all that is waited for
        HS_HIP(c, hipMemcpyAsync(b.hSize, words, sizeof(uint64_t) * (size_t)ch.count, hipMemcpyDeviceToHost, c->stream));
        if ((st = sync_wait(c))) return st;
        bool any = false;
        for (int k = 0; k < ch.count; k++) {
            const uint64_t size = b.hSize[k];
            bytes[ch.first + k] = (size_t)size;
            if (size > capacity) { fits = false; continue; }
            HS_HIP(c, hipMemcpyAsync(jpeg[ch.first + k], out[k], (size_t)size, hipMemcpyDeviceToHost, c->stream));
            any = true;
        }
        if (any && (st = sync_wait(c))) return st;
    }
    sync_restore(c, marked);
    if (!fits) return fail(c, HSFLOW_E_SIZE, "capacity smaller than a file (hsflow_jpeg_bound always suffices)");
    return check_persist(c);
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
    if ((st = stage_reserve(c, &j.out, &j.out_bytes, want))) return st;
    if (!j.hSize) HS_HIP(c, hipHostMalloc((void **)&j.hSize, 64, hipHostMallocDefault));
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    const size_t rowb = (size_t)c->W * 3, cap = capacity < bound ? capacity : bound;
    if ((st = enqueue_render(c, pair, *rp, c->dRgb, rowb))) return st;
    if ((st = enqueue_jpeg(c, c->dRgb, rowb, quality, j.out, cap, nullptr))) return st;
    // the size word first, then that many bytes: only the file crosses
    HS_HIP(c, hipMemcpyAsync(j.hSize, j.size, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if ((st = sync_wait(c))) return st;
    const uint64_t size = *j.hSize;
    *bytes = (size_t)size;
    if (size > capacity) {
        sync_restore(c, marked);
        return fail(c, HSFLOW_E_SIZE, "capacity smaller than the file (hsflow_jpeg_bound always suffices)");
    }
    HS_HIP(c, hipMemcpyAsync(jpeg, j.out, (size_t)size, hipMemcpyDeviceToHost, c->stream));
    return sync_finish(c, marked);
}

int hsflow_jpeg_encode_batch_device(hsflow_ctx *c, const void *const *d_rgb, int n, size_t stride, int quality, void *const *d_jpeg, size_t capacity,
                                    uint64_t *d_bytes)
{
    int st = check_ctx(c, 0), maxb = 0;
    if (st) return st;
    if (n < 1) return fail(c, HSFLOW_E_ARG, "a batch needs at least one picture");
    if (!d_rgb) return fail(c, HSFLOW_E_ARG, "null picture list");
    for (int i = 0; i < n; i++)
        if (!d_rgb[i]) return fail(c, HSFLOW_E_ARG, "picture " + std::to_string(i) + ": null picture pointer");
    if ((st = check_jpeg_batch_args(c, n, quality, d_jpeg, d_bytes))) return st;
    if ((uintptr_t)d_bytes & 7u) return fail(c, HSFLOW_E_ARG, "the size words must be 8-byte aligned");
    if (stride < (size_t)c->W * 3) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    if ((st = check_batch_max(c, &maxb))) return st;
    hsjpeg::Tables *tab = nullptr;
    if ((st = jpeg_tables(c, quality, &tab))) return st;
    if ((st = jpeg_batch_reserve(c, n < maxb ? n : maxb))) return st;
    for (const hsjpeg_plan::Chunk &ch : hsjpeg_plan::chunks(n, maxb)) {
        hsk::JpegBatchPics pics{};
        for (int k = 0; k < ch.count; k++) pics.p[k] = jpeg_batch_pic(d_rgb[ch.first + k], stride, d_jpeg[ch.first + k], capacity);
        if ((st = enqueue_jpeg_chunk(c, tab, pics, ch.count, stride, d_bytes + ch.first))) return st;
    }
    return HSFLOW_OK;
}

int hsflow_render_flow_jpeg_batch_device(hsflow_ctx *c, int first_pair, int n, const hsflow_render_params *rp, int quality, void *const *d_jpeg,
                                         size_t capacity, uint64_t *d_bytes)
{
    return draw_jpeg_batch_device(c, first_pair, n, Drawing{false, rp, nullptr}, quality, d_jpeg, capacity, d_bytes);
}

int hsflow_render_flow_jpeg_batch(hsflow_ctx *c, int first_pair, int n, const hsflow_render_params *rp, int quality, uint8_t *const *jpeg, size_t capacity,
                                  size_t *bytes)
{
    return draw_jpeg_batch(c, first_pair, n, Drawing{false, rp, nullptr}, quality, jpeg, capacity, bytes);
}

// The colour picture's files (hs_color.hip.h draws, the chain above encodes); the single forms are batches of one.
int hsflow_color_flow_jpeg_batch_device(hsflow_ctx *c, int first_pair, int n, const hsflow_color_params *cp, int quality, void *const *d_jpeg,
                                        size_t capacity, uint64_t *d_bytes)
{
    return draw_jpeg_batch_device(c, first_pair, n, Drawing{true, nullptr, cp}, quality, d_jpeg, capacity, d_bytes);
}

int hsflow_color_flow_jpeg_batch(hsflow_ctx *c, int first_pair, int n, const hsflow_color_params *cp, int quality, uint8_t *const *jpeg, size_t capacity,
                                 size_t *bytes)
{
    return draw_jpeg_batch(c, first_pair, n, Drawing{true, nullptr, cp}, quality, jpeg, capacity, bytes);
}

int hsflow_color_flow_jpeg_device(hsflow_ctx *c, int pair, const hsflow_color_params *cp, int quality, void *d_jpeg, size_t capacity, uint64_t *d_bytes)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    void *const list[1] = {d_jpeg};
    return draw_jpeg_batch_device(c, pair, 1, Drawing{true, nullptr, cp}, quality, d_jpeg ? list : nullptr, capacity, d_bytes);
}

int hsflow_color_flow_jpeg(hsflow_ctx *c, int pair, const hsflow_color_params *cp, int quality, uint8_t *jpeg, size_t capacity, size_t *bytes)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    uint8_t *const list[1] = {jpeg};
    return draw_jpeg_batch(c, pair, 1, Drawing{true, nullptr, cp}, quality, jpeg ? list : nullptr, capacity, bytes);
}

} // extern "C"
