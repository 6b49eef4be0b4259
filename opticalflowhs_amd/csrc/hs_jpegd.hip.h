// hs_jpegd.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_jpeg_read_header,
// hsflow_jpeg_decode[_host|_device|_batch_device], hsflow_set_frames_jpeg[_async], hsflow_push_frame_jpeg,
// hsflow_set_sequence_jpeg[_ex]: the frames the reference's runFromImg starts from (cvLoadImage, OpticalFlowOpenCV.cpp:15,18,
// HSOpticalFlowOpenCL.cpp:721,732), decoded on the device from the files' entropy-coded bytes.  One path: files are
// decoded in chunks of at most HSFLOW_JPEGD_BATCH_MAX, laid out by hs_jpegd_batch_plan.h, each chunk by one copy, three
// memsets and eight or eleven launches on the context's stream (hs_kernels_jpegd.hip.h); a single file is a chunk of
// one.  A context that never decodes allocates and launches nothing here.
#pragma once

#include "hs_jpegd_batch_plan.h"

namespace {

void jpegd_release(hsflow_ctx *c)
{
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    hipFree(j.base);
    hipFree(j.seq);
    if (j.hSeq) hipHostFree(j.hSeq);
    hipFree(j.out);
    for (int i = 0; i < 2; i++) {
        hipFree(j.bgr[i]);
        if (j.stage[i]) hipHostFree(j.stage[i]);
        if (j.evStage[i]) hipEventDestroy(j.evStage[i]);
    }
    if (j.hStatus) hipHostFree(j.hStatus);
    if (j.evDone) hipEventDestroy(j.evDone);
    if (j.evPair) hipEventDestroy(j.evPair);
    c->jpegd = hsflow_ctx::JpegdScratch();
}

// HSFLOW_JPEGD_SUBSEQ_BITS of this call: the environment's, else the header's.  0: the environment's value is unusable.
int jpegd_subseq_bits()
{
    const char *e = getenv("HSFLOW_JPEGD_SUBSEQ_BITS");
    if (!e || !*e) return HSFLOW_JPEGD_SUBSEQ_BITS;
    char *rest = nullptr;
    const long v = strtol(e, &rest, 10);
    if (*rest || v < 32 || v > 4096 || v % 32) return 0;
    return (int)v;
}

// HSFLOW_JPEGD_BATCH_MAX of this call: the environment's (1 .. 32, for measuring the candidates), else the header's.
// 0: the environment's value is unusable.
int jpegd_batch_max()
{
    const char *e = getenv("HSFLOW_JPEGD_BATCH_MAX");
    if (!e || !*e) return HSFLOW_JPEGD_BATCH_MAX;
    char *rest = nullptr;
    const long v = strtol(e, &rest, 10);
    if (*rest || v < 1 || v > 32) return 0;
    return (int)v;
}

void jpegd_fill_info(const hsjpegd::Frame &f, hsflow_jpeg_info *info)
{
    info->width = f.W; info->height = f.H; info->components = f.ncomp; info->h_samp = f.hs; info->v_samp = f.vs;
    info->restart_interval = f.ri;
    info->subseq_bits = f.ri ? 0 : jpegd_subseq_bits();
    info->blocks = f.nblocks; info->scan_offset = f.scan_offset; info->scan_bytes = f.scan_bytes;
}

// Staging: the older of the two page-locked areas, once the copy out of it is done, at least `bytes` large.  The caller
// records evStage[*slot] behind its copy.
int jpegd_stage(hsflow_ctx *c, size_t bytes, int *slot_out)
{
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    const int slot = j.next_slot;
    j.next_slot ^= 1;
    if (j.evStage[slot]) HS_HIP(c, hipEventSynchronize(j.evStage[slot]));
    else HS_HIP(c, hipEventCreateWithFlags(&j.evStage[slot], hipEventDisableTiming));
    if (j.stage_bytes[slot] < bytes) {
        if (j.stage[slot]) hipHostFree(j.stage[slot]);
        j.stage[slot] = nullptr; j.stage_bytes[slot] = 0;
        HS_HIP(c, hipHostMalloc((void **)&j.stage[slot], bytes, hipHostMallocDefault));
        j.stage_bytes[slot] = bytes;
    }
    *slot_out = slot;
    return HSFLOW_OK;
}

// The status words of the decodes enqueued so far into page-locked memory, waited for.
int jpegd_wait_status(hsflow_ctx *c, int words)
{
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    if (!j.evDone) HS_HIP(c, hipEventCreateWithFlags(&j.evDone, hipEventDisableTiming));
    HS_HIP(c, hipMemcpyAsync(j.hStatus, j.dStatus, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HS_HIP(c, hipEventRecord(j.evDone, c->stream));
    HS_HIP(c, hipEventSynchronize(j.evDone));
    for (int i = 0; i < words; i++)
        if (j.hStatus[i]) return fail(c, HSFLOW_E_DATA, j.hStatus[i] == 2 ? "JPEG file: truncated entropy-coded data" : "JPEG file: corrupt entropy-coded data");
    return HSFLOW_OK;
}

// The context's own status words (device and page-locked) and, with pictures != 0, its BGR pictures.
int jpegd_own(hsflow_ctx *c, int pictures)
{
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    if (!j.hStatus) {
        HS_HIP(c, hipHostMalloc((void **)&j.hStatus, 64, hipHostMallocDefault));
        j.hStatus[0] = j.hStatus[1] = 0;
    }
    if (!j.out) { HS_HIP(c, hipMalloc((void **)&j.out, 256)); j.out_bytes = 256; } // its first 256 bytes hold the status words, the picture lies behind them
    for (int i = 0; i < pictures; i++)
        if (!j.bgr[i]) HS_HIP(c, hipMalloc((void **)&j.bgr[i], (size_t)c->W * 3 * c->H));
    return HSFLOW_OK;
}

// ---- chunks of files: the one decode path ------------------------------------------------------------------------------

// The headers of n files of the context's size, before anything is enqueued.  An error names the file's index.
int jpegd_batch_parse(hsflow_ctx *c, const uint8_t *const *files, const size_t *bytes, int n, std::vector<hsjpegd::Frame> &fr,
                      std::vector<hsjpegd::Tables> &tabs)
{
    if (!files || !bytes) return fail(c, HSFLOW_E_ARG, "null file list");
    if (n < 1) return fail(c, HSFLOW_E_ARG, "a batch needs at least one file");
    if (!jpegd_subseq_bits()) return fail(c, HSFLOW_E_ARG, "HSFLOW_JPEGD_SUBSEQ_BITS must be a multiple of 32 in 32 .. 4096");
    if (!jpegd_batch_max()) return fail(c, HSFLOW_E_ARG, "HSFLOW_JPEGD_BATCH_MAX in the environment must be 1 .. 32");
    try { fr.resize((size_t)n); tabs.resize((size_t)n); }
    catch (const std::bad_alloc &) { return fail(c, HSFLOW_E_OOM, "host allocation failed"); }
    for (int i = 0; i < n; i++) {
        const std::string who = "file " + std::to_string(i) + ": ";
        if (!files[i]) return fail(c, HSFLOW_E_ARG, who + "null file pointer");
        const char *why = "";
        if (hsjpegd::parse(files[i], bytes[i], fr[(size_t)i], tabs[(size_t)i], &why)) return fail(c, HSFLOW_E_DATA, who + "JPEG file: " + why);
        if (fr[(size_t)i].W != c->W || fr[(size_t)i].H != c->H) return fail(c, HSFLOW_E_SIZE, who + "the picture does not have the context's size");
    }
    return HSFLOW_OK;
}

// n files' decodes, enqueued on c's stream chunk after chunk of at most max_batch: per chunk one copy, three memsets and
// one set of launches (hs_kernels_jpegd.hip.h).  The caller has checked every argument and parsed every header.
int enqueue_jpegd_batch(hsflow_ctx *c, const uint8_t *const *files, const hsjpegd::Frame *fr, const hsjpegd::Tables *tabs, int n, int max_batch, int order,
                        void *const *d_pix, size_t stride, uint32_t *d_status)
{
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    const int S = jpegd_subseq_bits();
    hsjpegd_plan::Plan plan;
    try {
        std::vector<hsjpegd_plan::FileIn> in((size_t)n);
        for (int i = 0; i < n; i++) in[(size_t)i] = hsjpegd_plan::FileIn{fr[i].scan_bytes, fr[i].nblocks, (int64_t)fr[i].mcux * fr[i].mcuy, fr[i].ri};
        plan = hsjpegd_plan::layout(in.data(), n, hsjpegd_plan::Params{sizeof(hsjpegd::Tables), sizeof(hsk::JpegdBatchRec), (uint32_t)S, max_batch});
    } catch (const std::bad_alloc &) { return fail(c, HSFLOW_E_OOM, "host allocation failed"); }
    if (j.bytes < plan.device_bytes) { // (what is in flight still reads the old one)
        HS_HIP(c, hipStreamSynchronize(c->stream));
        hipFree(j.base);
        j.base = nullptr; j.bytes = 0;
        HS_HIP(c, hipMalloc(&j.base, plan.device_bytes));
        j.bytes = plan.device_bytes;
    }
    uint8_t *p = (uint8_t *)j.base;
    const int rgb = order == HSFLOW_JPEG_ORDER_RGB ? 1 : 0;
    for (const hsjpegd_plan::Chunk &ch : plan.chunks) {
        int slot = 0;
        const int sst = jpegd_stage(c, ch.in_bytes, &slot);
        if (sst) return sst;
        uint8_t *h = j.stage[slot];
        hsk::JpegdBatchRec *recs = (hsk::JpegdBatchRec *)(h + ch.o_recs);
        for (int k = 0; k < ch.count; k++) {
            const int i = ch.first + k;
            const hsjpegd_plan::FileOut &o = plan.files[(size_t)i];
            const hsjpegd::Frame &f = fr[i];
            std::memcpy(h + o.o_tab, &tabs[i], sizeof(hsjpegd::Tables));
            std::memcpy(h + o.o_scan, files[i] + f.scan_offset, o.n);
            std::memset(h + o.o_scan + o.n, 0, o.scan_span - o.n);
            hsk::JpegdBatchRec &r = recs[k];
            hsk::JpegdArgs &a = r.a;
            a.f = f;
            a.tab = (const hsjpegd::Tables *)(p + o.o_tab);
            a.scan = p + o.o_scan;
            a.n = o.n; a.nchunks = o.nchunks; a.S = (uint32_t)S;
            a.cntRem = (uint32_t *)(p + o.o_cr); a.cntRst = (uint32_t *)(p + o.o_cs);
            a.remOff = (uint64_t *)(p + o.o_ro); a.rstOff = (uint64_t *)(p + o.o_so);
            a.clean = (uint32_t *)(p + o.o_clean);
            a.rstPos = (uint32_t *)(p + o.o_rst);
            a.nint = o.nint;
            a.start = (uint64_t *)(p + o.o_start); a.exit = (uint64_t *)(p + o.o_exit);
            a.cnt = (uint32_t *)(p + o.o_cnt); a.base = (uint64_t *)(p + o.o_base);
            a.nsubCap = o.nsubCap;
            a.coef = (int16_t *)(p + o.o_coef); a.diff = (uint32_t *)(p + o.o_diff); a.dcsum = (uint64_t *)(p + o.o_dcsum); a.planes = p + o.o_planes;
            a.status = d_status + i;
            r.pix = (uint8_t *)d_pix[i];
            r.stride = (long long)stride;
            r.rgb = rgb;
            r.wide = word_aligned(d_pix[i], stride);
        }
        HS_HIP(c, hipMemcpyAsync(p, h, ch.in_bytes, hipMemcpyHostToDevice, c->stream));
        HS_HIP(c, hipEventRecord(j.evStage[slot], c->stream));
        HS_HIP(c, hipMemsetAsync(d_status + ch.first, 0, (size_t)ch.count * sizeof(uint32_t), c->stream));
        HS_HIP(c, hipMemsetAsync(p + ch.o_clean, 0, ch.clean_bytes, c->stream));
        HS_HIP(c, hipMemsetAsync(p + ch.o_coef, 0, ch.coef_bytes, c->stream));
        const hsk::JpegdBatchRec *d = (const hsk::JpegdBatchRec *)(p + ch.o_recs);
        const unsigned nf = (unsigned)ch.count;
        hipLaunchKernelGGL(hsk::k_jpegd_clean_batch<0>, dim3(ch.g_clean, nf), dim3(256), 0, c->stream, d);
        hipLaunchKernelGGL(hsk::k_jpegd_scan_batch<0>, dim3(nf, 2), dim3(hsk::kJpegScanLanes), 0, c->stream, d);
        hipLaunchKernelGGL(hsk::k_jpegd_clean_batch<1>, dim3(ch.g_clean, nf), dim3(256), 0, c->stream, d);
        if (ch.g_sub) { // the files without restart intervals
            hipLaunchKernelGGL(hsk::k_jpegd_sync_batch, dim3(ch.g_sub, nf), dim3(hsk::kJpegdGroup), 0, c->stream, d);
            hipLaunchKernelGGL(hsk::k_jpegd_repair_batch, dim3(nf), dim3(hsk::kJpegdRepairLanes), 0, c->stream, d);
            hipLaunchKernelGGL(hsk::k_jpegd_scan_batch<2>, dim3(nf), dim3(hsk::kJpegScanLanes), 0, c->stream, d);
            hipLaunchKernelGGL(hsk::k_jpegd_write_batch, dim3(ch.g_sub, nf), dim3(256), 0, c->stream, d);
        }
        if (ch.g_rst) hipLaunchKernelGGL(hsk::k_jpegd_write_rst_batch, dim3(ch.g_rst, nf), dim3(256), 0, c->stream, d); // those with
        hipLaunchKernelGGL(hsk::k_jpegd_dc_gather_batch, dim3(ch.g_gather, nf), dim3(256), 0, c->stream, d);
        hipLaunchKernelGGL(hsk::k_jpegd_scan_batch<3>, dim3(nf), dim3(hsk::kJpegScanLanes), 0, c->stream, d);
        hipLaunchKernelGGL(hsk::k_jpegd_blocks_batch, dim3(ch.g_blocks, nf), dim3(256), 0, c->stream, d);
        hipLaunchKernelGGL(hsk::k_jpegd_pixels_batch, dim3((c->W + 255) / 256, (c->H + 3) / 4, nf), dim3(64, 4), 0, c->stream, d);
        HS_HIP(c, hipGetLastError());
    }
    return HSFLOW_OK;
}

// The checks of hsflow_jpeg_decode_batch_device that the lists' owners inside the library share with it.
int jpegd_batch(hsflow_ctx *c, const uint8_t *const *files, const size_t *bytes, int n, int order, void *const *d_pix, size_t stride, uint32_t *d_status)
{
    if (order != HSFLOW_JPEG_ORDER_BGR && order != HSFLOW_JPEG_ORDER_RGB) return fail(c, HSFLOW_E_ARG, "unknown pixel order");
    if (!d_pix || !d_status) return fail(c, HSFLOW_E_ARG, "null picture list or status pointer");
    if ((uintptr_t)d_status & 3u) return fail(c, HSFLOW_E_ARG, "the status words must be 4-byte aligned");
    if (stride < (size_t)c->W * 3) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    std::vector<hsjpegd::Frame> fr;
    std::vector<hsjpegd::Tables> tabs;
    int st = jpegd_batch_parse(c, files, bytes, n, fr, tabs);
    if (st) return st;
    for (int i = 0; i < n; i++)
        if (!d_pix[i]) return fail(c, HSFLOW_E_ARG, "file " + std::to_string(i) + ": null picture pointer");
    return enqueue_jpegd_batch(c, files, fr.data(), tabs.data(), n, jpegd_batch_max(), order, d_pix, stride, d_status);
}

// Header, checks and the enqueue for one file of the context's size: a chunk of one, which is never cut -- the batch
// maximum does not enter.  Its messages name no position in a list.
int jpegd_one(hsflow_ctx *c, const uint8_t *file, size_t bytes, int order, uint8_t *d_pix, size_t stride, uint32_t *d_status)
{
    if (!file) return fail(c, HSFLOW_E_ARG, "null file pointer");
    if (order != HSFLOW_JPEG_ORDER_BGR && order != HSFLOW_JPEG_ORDER_RGB) return fail(c, HSFLOW_E_ARG, "unknown pixel order");
    hsjpegd::Frame f;
    std::unique_ptr<hsjpegd::Tables> t(new (std::nothrow) hsjpegd::Tables);
    if (!t) return fail(c, HSFLOW_E_OOM, "host allocation failed");
    const char *why = "";
    if (hsjpegd::parse(file, bytes, f, *t, &why)) return fail(c, HSFLOW_E_DATA, std::string("JPEG file: ") + why);
    if (f.W != c->W || f.H != c->H) return fail(c, HSFLOW_E_SIZE, "the picture does not have the context's size");
    if (stride < (size_t)c->W * 3) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    if (!jpegd_subseq_bits()) return fail(c, HSFLOW_E_ARG, "HSFLOW_JPEGD_SUBSEQ_BITS must be a multiple of 32 in 32 .. 4096");
    void *pix = d_pix;
    return enqueue_jpegd_batch(c, &file, &f, t.get(), 1, 1, order, &pix, stride, d_status);
}

} // namespace

extern "C" {

int hsflow_jpeg_read_header(const uint8_t *file, size_t bytes, hsflow_jpeg_info *info)
{
    if (!file || !info) return fail(nullptr, HSFLOW_E_ARG, "hsflow_jpeg_read_header: null pointer");
    if (info->struct_size != sizeof(hsflow_jpeg_info)) return fail(nullptr, HSFLOW_E_ARG, "hsflow_jpeg_read_header: struct_size mismatch");
    hsjpegd::Frame f;
    std::unique_ptr<hsjpegd::Tables> t(new (std::nothrow) hsjpegd::Tables);
    if (!t) return fail(nullptr, HSFLOW_E_OOM, "hsflow_jpeg_read_header: host allocation failed");
    const char *why = "";
    if (hsjpegd::parse(file, bytes, f, *t, &why)) return fail(nullptr, HSFLOW_E_DATA, std::string("JPEG file: ") + why);
    jpegd_fill_info(f, info);
    return HSFLOW_OK;
}

int hsflow_jpeg_decode_host(const uint8_t *file, size_t bytes, int order, uint8_t *pix, size_t stride, hsflow_jpeg_info *info)
{
    if (!file || !pix) return fail(nullptr, HSFLOW_E_ARG, "hsflow_jpeg_decode_host: null pointer");
    if (order != HSFLOW_JPEG_ORDER_BGR && order != HSFLOW_JPEG_ORDER_RGB) return fail(nullptr, HSFLOW_E_ARG, "hsflow_jpeg_decode_host: unknown pixel order");
    if (info && info->struct_size != sizeof(hsflow_jpeg_info)) return fail(nullptr, HSFLOW_E_ARG, "hsflow_jpeg_decode_host: struct_size mismatch");
    hsjpegd::Frame f;
    const char *why = "";
    int status = 0;
    const int r = hsjpegd::decode_host(file, bytes, order == HSFLOW_JPEG_ORDER_RGB, pix, stride, &f, &status, &why);
    if (info && (r == 0 || r == 2 || (r == 7 && status))) jpegd_fill_info(f, info);
    switch (r) {
    case 0: return HSFLOW_OK;
    case 1: return fail(nullptr, HSFLOW_E_ARG, "hsflow_jpeg_decode_host: null pointer");
    case 2: return fail(nullptr, HSFLOW_E_SIZE, "hsflow_jpeg_decode_host: stride smaller than 3*width");
    case 7: return fail(nullptr, HSFLOW_E_DATA, std::string("JPEG file: ") + why);
    default: return fail(nullptr, HSFLOW_E_OOM, "hsflow_jpeg_decode_host: host allocation failed");
    }
}

int hsflow_jpeg_decode_device(hsflow_ctx *c, const uint8_t *file, size_t bytes, int order, void *d_pix, size_t stride, uint32_t *d_status)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (!d_pix || !d_status) return fail(c, HSFLOW_E_ARG, "null picture or status pointer");
    if ((uintptr_t)d_status & 3u) return fail(c, HSFLOW_E_ARG, "the status word must be 4-byte aligned");
    return jpegd_one(c, file, bytes, order, (uint8_t *)d_pix, stride, d_status);
}

int hsflow_jpeg_decode(hsflow_ctx *c, const uint8_t *file, size_t bytes, int order, uint8_t *pix, size_t stride)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (!pix) return fail(c, HSFLOW_E_ARG, "null picture pointer");
    if ((st = jpegd_own(c, 0))) return st;
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    const size_t rowb = (size_t)c->W * 3;
    if (stride < rowb) return fail(c, HSFLOW_E_SIZE, "picture stride smaller than 3*width");
    // the picture on the device: pix's alignment and row padding modulo 4
    const size_t dstride = rowb + ((stride - rowb) & 3u), off = 256 + ((uintptr_t)pix & 3u), want = off + dstride * (size_t)c->H;
    if (j.out_bytes < want) { // (the synchronous forms leave nothing in flight that uses the old one)
        HS_HIP(c, hipStreamSynchronize(c->stream));
        hipFree(j.out);
        j.out = nullptr; j.out_bytes = 0;
        HS_HIP(c, hipMalloc((void **)&j.out, want));
        j.out_bytes = want;
    }
    j.dStatus = (uint32_t *)j.out;
    if ((st = jpegd_one(c, file, bytes, order, j.out + off, dstride, j.dStatus))) return st;
    st = jpegd_wait_status(c, 1);
    if (!st) {
        HS_HIP(c, hipMemcpy2DAsync(pix, stride, j.out + off, dstride, rowb, c->H, hipMemcpyDeviceToHost, c->stream));
        HS_HIP(c, hipEventRecord(j.evDone, c->stream));
        HS_HIP(c, hipEventSynchronize(j.evDone));
    }
    return st;
}

int hsflow_set_frames_jpeg(hsflow_ctx *c, int pair, const uint8_t *prev, size_t prev_bytes, const uint8_t *curr, size_t curr_bytes, int blur3x3)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!prev || !curr) return fail(c, HSFLOW_E_ARG, "null file pointer");
    if ((st = jpegd_own(c, 2))) return st;
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    j.dStatus = (uint32_t *)j.out;
    const size_t rowb = (size_t)c->W * 3;
    if ((st = jpegd_one(c, prev, prev_bytes, HSFLOW_JPEG_ORDER_BGR, j.bgr[0], rowb, j.dStatus))) return st;
    if ((st = jpegd_one(c, curr, curr_bytes, HSFLOW_JPEG_ORDER_BGR, j.bgr[1], rowb, j.dStatus + 1))) return st;
    if ((st = jpegd_wait_status(c, 2))) return st;
    if ((st = hsflow_set_frames_device_ex(c, pair, blur3x3 ? HSFLOW_FRAMES_BGR8_BLUR : HSFLOW_FRAMES_BGR8, j.bgr[0], rowb, j.bgr[1], rowb))) return st;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    return HSFLOW_OK;
}

int hsflow_push_frame_jpeg(hsflow_ctx *c, int pair, const uint8_t *next, size_t bytes, int blur3x3, int reblur_prev)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!next) return fail(c, HSFLOW_E_ARG, "null file pointer");
    if (reblur_prev != 0 && reblur_prev != 1) return fail(c, HSFLOW_E_ARG, "reblur_prev must be 0 or 1");
    if (!c->frames_set) return fail(c, HSFLOW_E_STATE, "push_frame needs a previous pair");
    if ((st = jpegd_own(c, 1))) return st;
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    j.dStatus = (uint32_t *)j.out;
    const size_t rowb = (size_t)c->W * 3;
    if ((st = jpegd_one(c, next, bytes, HSFLOW_JPEG_ORDER_BGR, j.bgr[0], rowb, j.dStatus))) return st;
    if ((st = jpegd_wait_status(c, 1))) return st;
    return hsflow_push_frame_device_ex(c, pair, blur3x3 ? HSFLOW_FRAMES_BGR8_BLUR : HSFLOW_FRAMES_BGR8, j.bgr[0], rowb, reblur_prev);
}

int hsflow_jpeg_decode_batch_device(hsflow_ctx *c, const uint8_t *const *files, const size_t *bytes, int n, int order, void *const *d_pix, size_t stride,
                                    uint32_t *d_status)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    return jpegd_batch(c, files, bytes, n, order, d_pix, stride, d_status);
}

int hsflow_set_sequence_jpeg(hsflow_ctx *c, int first_pair, const uint8_t *const *files, const size_t *bytes, int n_files, int blur3x3)
{
    return hsflow_set_sequence_jpeg_ex(c, first_pair, files, bytes, n_files, blur3x3, 0);
}

int hsflow_set_sequence_jpeg_ex(hsflow_ctx *c, int first_pair, const uint8_t *const *files, const size_t *bytes, int n_files, int blur3x3, int flags)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (n_files < 2) return fail(c, HSFLOW_E_ARG, "a sequence needs at least two files");
    if (first_pair < 0 || (long long)first_pair + n_files - 1 > c->N) return fail(c, HSFLOW_E_ARG, "the sequence's pairs exceed the context's");
    if (!hspre::seq_flags_known(flags)) return fail(c, HSFLOW_E_ARG, "flags must be 0, HSFLOW_SEQ_REBLUR or HSFLOW_SEQ_REBLUR | HSFLOW_SEQ_REBLUR_FIRST");
    if (!pre_seq_max()) return fail(c, HSFLOW_E_ARG, "HSFLOW_PRE_SEQ_MAX in the environment must be 1 .. " + std::to_string(HSFLOW_PRE_SEQ_MAX));
    if ((st = settle_pending(c))) return st; // (before the all-or-nothing part: an owed check belongs to the frames that are there)
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    const size_t rowb = (size_t)c->W * 3, pic = hsjpegd_plan::up256(rowb * (size_t)c->H), words = hsjpegd_plan::up256((size_t)n_files * 4), want = words + pic * (size_t)n_files;
    if (j.seq_bytes < want) { // (synchronous: nothing in flight uses the old one)
        HS_HIP(c, hipStreamSynchronize(c->stream));
        hipFree(j.seq);
        j.seq = nullptr; j.seq_bytes = 0;
        HS_HIP(c, hipMalloc((void **)&j.seq, want));
        j.seq_bytes = want;
    }
    if (j.hSeq_words < n_files) {
        if (j.hSeq) hipHostFree(j.hSeq);
        j.hSeq = nullptr; j.hSeq_words = 0;
        HS_HIP(c, hipHostMalloc((void **)&j.hSeq, (size_t)n_files * 4, hipHostMallocDefault));
        j.hSeq_words = n_files;
    }
    std::vector<void *> pix((size_t)n_files);
    for (int i = 0; i < n_files; i++) pix[(size_t)i] = j.seq + words + pic * (size_t)i;
    if ((st = jpegd_batch(c, files, bytes, n_files, HSFLOW_JPEG_ORDER_BGR, pix.data(), rowb, (uint32_t *)j.seq))) return st;
    HS_HIP(c, hipMemcpyAsync(j.hSeq, j.seq, (size_t)n_files * 4, hipMemcpyDeviceToHost, c->stream));
    HS_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n_files; i++)
        if (j.hSeq[i])
            return fail(c, HSFLOW_E_DATA, "file " + std::to_string(i) + (j.hSeq[i] == 2 ? ": JPEG file: truncated entropy-coded data" : ": JPEG file: corrupt entropy-coded data"));
    // the pictures into the pairs: one launch per HSFLOW_PRE_SEQ_MAX of them, each read once
    if ((st = hsflow_set_sequence_device_ex(c, first_pair, blur3x3 ? HSFLOW_FRAMES_BGR8_BLUR : HSFLOW_FRAMES_BGR8, pix.data(), n_files, rowb, flags))) return st;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    return HSFLOW_OK;
}

int hsflow_set_frames_jpeg_async(hsflow_ctx *c, int pair, const uint8_t *prev, size_t prev_bytes, const uint8_t *curr, size_t curr_bytes, int blur3x3)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = jpegd_own(c, 2))) return st;
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    uint32_t *dPair = (uint32_t *)j.out + 2; // words of its own, device and host: a synchronous decode in between uses [0, 2)
    const size_t rowb = (size_t)c->W * 3;
    const uint8_t *files[2] = {prev, curr};
    const size_t bytes[2] = {prev_bytes, curr_bytes};
    void *pix[2] = {j.bgr[0], j.bgr[1]};
    if ((st = jpegd_batch(c, files, bytes, 2, HSFLOW_JPEG_ORDER_BGR, pix, rowb, dPair))) return st;
    HS_HIP(c, hipMemcpyAsync(j.hStatus + 2, dPair, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (!j.evPair) HS_HIP(c, hipEventCreateWithFlags(&j.evPair, hipEventDisableTiming));
    HS_HIP(c, hipEventRecord(j.evPair, c->stream));
    j.pair_status_owed = true;
    return hsflow_set_frames_device_ex(c, pair, blur3x3 ? HSFLOW_FRAMES_BGR8_BLUR : HSFLOW_FRAMES_BGR8, j.bgr[0], rowb, j.bgr[1], rowb);
}

int hsflow_jpeg_async_status(hsflow_ctx *c)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    hsflow_ctx::JpegdScratch &j = c->jpegd;
    if (!j.pair_status_owed) return fail(c, HSFLOW_E_STATE, "no hsflow_set_frames_jpeg_async whose status has not been asked for yet");
    HS_HIP(c, hipEventSynchronize(j.evPair));
    j.pair_status_owed = false; // one answer per call
    for (int i = 0; i < 2; i++)
        if (j.hStatus[2 + i])
            return fail(c, HSFLOW_E_DATA, "file " + std::to_string(i) + (j.hStatus[2 + i] == 2 ? ": JPEG file: truncated entropy-coded data" : ": JPEG file: corrupt entropy-coded data"));
    return HSFLOW_OK;
}

} // extern "C"
