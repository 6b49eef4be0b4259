// hsflow.hip -- C ABI (include/hsflow.h) over the HIP kernels in hs_kernels.hip.h.
//
// Host side of the hot path, i.e. what HSOpticalFlowOpenCL::setupCL / runDerivatives /
// runCLKernels / cleanup did with OpenCL (OpticalFlowHS/HSOpticalFlowOpenCL.cpp:67-679,
// :849-892), re-designed for MI355X: device-resident planar buffers, no per-iteration
// host<->device copies (the reference moved u,v over PCIe twice per iteration, :483-501 and
// :655-675), one stream, the whole launch sequence optionally captured as a hipGraph.
#include "../../include/hsflow.h"
#include "hs_kernels.hip.h"
#include "hs_kernels_pre.hip.h"
#include "hs_kernels_classic.hip.h"
#include "hs_kernels_classic_strip.hip.h"
#include "hs_kernels_render.hip.h"
#include "hs_kernels_color.hip.h"
#include "hs_kernels_warp.hip.h"
#include "hs_kernels_fb.hip.h"
#include "hs_kernels_median.hip.h"
#include "hs_kernels_interp.hip.h"
#include "hs_kernels_pyramid.hip.h"
#include "hs_kernels_chain.hip.h"
#include "hs_kernels_gmotion.hip.h"
#include "hs_kernels_regions.hip.h"
#include "hs_kernels_link.hip.h"
#include "hs_kernels_corners.hip.h"
#include "hs_kernels_verify.hip.h"
#include "hs_kernels_jpeg.hip.h"
#include "hs_kernels_jpegd.hip.h"

#include <atomic>
#include <chrono>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "hs_stop_rule.h"
#include "hs_context.hip.h"
#include "hs_plan_launch.hip.h"
#include "hs_runtime.hip.h"
#include "hs_solve.hip.h"


namespace { void jpeg_release(hsflow_ctx *c); void jpegd_release(hsflow_ctx *c); void postops_release(hsflow_ctx *c); void pyramid_release(hsflow_ctx *c); void chain_release(hsflow_ctx *c); void gmotion_release(hsflow_ctx *c); void regions_release(hsflow_ctx *c); void link_release(hsflow_ctx *c); void corners_release(hsflow_ctx *c); } // hs_jpeg.hip.h, hs_jpegd.hip.h, hs_postops.hip.h, hs_pyramid.hip.h, hs_chain.hip.h, hs_gmotion.hip.h, hs_regions.hip.h, hs_link.hip.h, hs_corners.hip.h

extern "C" {

void hsflow_default_params(hsflow_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(*p);
    p->mode = HSFLOW_MODE_CV;
    p->lambda = 1.0f;
    p->alpha = 1.0f;
    p->term_type = HSFLOW_TERM_ITER | HSFLOW_TERM_EPS; // as the reference calls it, OpticalFlowOpenCV.cpp:29
    p->max_iter = 100;                                  // main.cpp:4
    p->epsilon = (double)1e-6f;                         // cvTermCriteria rounds through float, cxtypes.h:912
    p->kernel = HSFLOW_KERNEL_AUTO;
}

int hsflow_device_count(int *count)
{
    if (!count) return HSFLOW_E_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return HSFLOW_E_DEVICE; }
    *count = n;
    return HSFLOW_OK;
}

int hsflow_host_alloc(void **out, size_t bytes)
{
    if (!out || !bytes) return fail(nullptr, HSFLOW_E_ARG, "hsflow_host_alloc: null out or zero size");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) { *out = nullptr; return fail(nullptr, HSFLOW_E_OOM, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
    return HSFLOW_OK;
}

int hsflow_host_free(void *p)
{
    if (!p) return HSFLOW_OK;
    hipError_t e = hipHostFree(p);
    return e == hipSuccess ? HSFLOW_OK : fail(nullptr, HSFLOW_E_ARG, std::string("hipHostFree: ") + hipGetErrorString(e));
}

int hsflow_host_register(void *p, size_t bytes)
{
    if (!p || !bytes) return fail(nullptr, HSFLOW_E_ARG, "hsflow_host_register: null pointer or zero size");
    hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    return e == hipSuccess ? HSFLOW_OK : fail(nullptr, HSFLOW_E_DEVICE, std::string("hipHostRegister: ") + hipGetErrorString(e));
}

int hsflow_host_unregister(void *p)
{
    if (!p) return HSFLOW_OK;
    hipError_t e = hipHostUnregister(p);
    return e == hipSuccess ? HSFLOW_OK : fail(nullptr, HSFLOW_E_ARG, std::string("hipHostUnregister: ") + hipGetErrorString(e));
}

int hsflow_version(void) { return HSFLOW_VERSION_MAJOR * 1000 + HSFLOW_VERSION_MINOR; }

const char *hsflow_status_string(int s)
{
    switch (s) {
    case HSFLOW_OK: return "ok";
    case HSFLOW_E_ARG: return "invalid argument";
    case HSFLOW_E_SIZE: return "invalid size or stride";
    case HSFLOW_E_DEVICE: return "device error";
    case HSFLOW_E_OOM: return "out of memory";
    case HSFLOW_E_STATE: return "invalid call order";
    case HSFLOW_E_NOTERM: return "termination criteria never met";
    case HSFLOW_E_DATA: return "unsupported, corrupt or truncated file";
    default: return "unknown status";
    }
}

const char *hsflow_last_error(hsflow_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int hsflow_create(hsflow_ctx **out, int device, int width, int height, int n_pairs, void *stream, int own_stream)
{
    if (!out) return fail(nullptr, HSFLOW_E_ARG, "out is null");
    *out = nullptr;
    if (width <= 0 || height <= 0 || n_pairs <= 0) return fail(nullptr, HSFLOW_E_SIZE, "width, height, n_pairs must be positive");
    if ((long long)round_up(width, 64) * height > (1LL << 30)) return fail(nullptr, HSFLOW_E_SIZE, "plane too large (pitch*height > 2^30)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, HSFLOW_E_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(nullptr, HSFLOW_E_ARG, "device ordinal out of range");
    hsflow_ctx *c = new (std::nothrow) hsflow_ctx();
    if (!c) return fail(nullptr, HSFLOW_E_OOM, "host allocation failed");
    c->device = device; c->W = width; c->H = height; c->N = n_pairs;
    c->P = round_up(width, 64);
    c->plane = (long long)c->P * height;
    std::memset(&c->info, 0, sizeof(c->info));
    c->info.struct_size = sizeof(hsflow_info);
    c->info.width = width; c->info.height = height; c->info.n_pairs = n_pairs; c->info.pitch = c->P;
    auto bail = [&](int code, const std::string &m) { g_create_error = m; hsflow_destroy(c); return code; };
#define HS_TRY(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return bail(e_ == hipErrorOutOfMemory ? HSFLOW_E_OOM : HSFLOW_E_DEVICE,               \
                        std::string(#call) + ": " + hipGetErrorString(e_));                       \
    } while (0)
    HS_TRY(hipSetDevice(device));
    if (own_stream) {
        HS_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    } else {
        c->stream = (hipStream_t)stream;
    }
    const size_t px = (size_t)c->plane * n_pairs;
    HS_TRY(hipMalloc((void **)&c->dA, px));
    HS_TRY(hipMalloc((void **)&c->dB, px));
    HS_TRY(hipMalloc((void **)&c->dCoef, px * sizeof(uint32_t)));
    for (int i = 0; i < 2; i++) {
        HS_TRY(hipMalloc((void **)&c->dU[i], px * sizeof(float)));
        HS_TRY(hipMalloc((void **)&c->dV[i], px * sizeof(float)));
    }
    HS_TRY(hipMalloc((void **)&c->dEps, kMaxFuse * sizeof(unsigned)));
    HS_TRY(hipMalloc((void **)&c->dZero, ((size_t)c->P + 64) * sizeof(float)));
    {
        int ncu = 0;
        HS_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
        c->num_cu = ncu;
        int gz = 0;
        HS_TRY(hipDeviceGetAttribute(&gz, hipDeviceAttributeMaxGridDimZ, device));
        if (gz > 0) c->max_grid_z = gz;
    }
    if (getenv("HSFLOW_DEBUG_STAMPS")) HS_TRY(hipMalloc((void **)&c->dStamps, (size_t)kStampTiles * 8 * sizeof(unsigned long long)));
    // deterministic contents for padding columns and the initial flow
    HS_TRY(hipMemsetAsync(c->dZero, 0, ((size_t)c->P + 64) * sizeof(float), c->stream));
    HS_TRY(hipMemsetAsync(c->dA, 0, px, c->stream));
    HS_TRY(hipMemsetAsync(c->dB, 0, px, c->stream));
    HS_TRY(hipMemsetAsync(c->dCoef, 0, px * sizeof(uint32_t), c->stream));
    for (int i = 0; i < 2; i++) {
        HS_TRY(hipMemsetAsync(c->dU[i], 0, px * sizeof(float), c->stream));
        HS_TRY(hipMemsetAsync(c->dV[i], 0, px * sizeof(float), c->stream));
    }
    HS_TRY(hipStreamSynchronize(c->stream));
#undef HS_TRY
    g_live_ctx[device & 63]++;
    c->counted = true;
    *out = c;
    return HSFLOW_OK;
}

int hsflow_set_row_origin(hsflow_ctx *c, int first_row)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = settle_pending(c))) return st;
    const int org = first_row & 1;
    if (org != c->org) {
        drop_graphs(c); // captured launches carry the phase (kernel choice and geometry)
        c->plan_cache.clear();
        c->lastl.valid = false;
        c->org = org;
    }
    return HSFLOW_OK;
}

int hsflow_set_cu_share(hsflow_ctx *c, int compute_units)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (compute_units < 0) return fail(c, HSFLOW_E_ARG, "compute_units must be >= 0 (0: the whole chip)");
    const int share = compute_units >= kNumCU ? 0 : compute_units;
    if (share != c->cu_share) {
        if ((st = settle_pending(c))) return st;
        c->cu_share = share; // (graphs are keyed by the launch shape, so cached ones stay valid)
        c->plan_cache.clear();
    }
    return HSFLOW_OK;
}

int hsflow_destroy(hsflow_ctx *c)
{
    if (!c) return HSFLOW_OK;
    hipSetDevice(c->device);
    if (c->stream || !c->own_stream) hipStreamSynchronize(c->stream);
    if (c->shadow) { hsflow_destroy(c->shadow); c->shadow = nullptr; } // hsflow_verify's scratch
    pyramid_release(c);                                                 // hsflow_solve_pyramid's level contexts
    if (c->borrowed) c->dA = c->dB = nullptr;                           // (the owner's frames)
    hipFree(c->dCmp);
    if (c->hCmp) hipHostFree(c->hCmp);
    if (c->evVerify) hipEventDestroy(c->evVerify);
    for (auto &kv : c->graphs) {
        if (kv.second.exec) hipGraphExecDestroy(kv.second.exec);
        if (kv.second.graph) hipGraphDestroy(kv.second.graph);
    }
    for (hipEvent_t e : c->events) hipEventDestroy(e);
    hipFree(c->dA); hipFree(c->dB); hipFree(c->dCoef);
    for (int i = 0; i < 3; i++) hipFree(c->dE[i]);
    for (int i = 0; i < 2; i++) { hipFree(c->dU[i]); hipFree(c->dV[i]); }
    hipFree(c->dEps);
    hipFree(c->dPairs);
    hipFree(c->dEpsTiles); hipFree(c->dUb); hipFree(c->dVb);
    hipFree(c->dFlowMax);
    if (c->hFlowMax) hipHostFree(c->hFlowMax);
    hipFree(c->dUp); hipFree(c->dVp); hipFree(c->dFlags);
    hipFree(c->dSeq);
    hipFree(c->dZero);
    if (c->hMark) hipHostFree(c->hMark);
    if (c->hErr) hipHostFree(c->hErr);
    if (c->counted) g_live_ctx[c->device & 63]--;
    hipFree(c->dStamps);
    hipFree(c->dScratch);
    hipFree(c->dPrio); hipFree(c->dRgb);
    hipFree(c->dColorScale);
    if (c->hColorScale) hipHostFree(c->hColorScale);
    postops_release(c);
    chain_release(c);
    gmotion_release(c);
    regions_release(c);
    link_release(c);
    corners_release(c);
    if (c->evRender) hipEventDestroy(c->evRender);
    jpeg_release(c);
    jpegd_release(c);
    if (c->hEps) hipHostFree(c->hEps);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;
    return HSFLOW_OK;
}

// One transfer of `rows` rows of `rowb` bytes between a pitched device plane and a host buffer on
// ctx's stream.  Dense layouts on both sides take the 1-D path (a single SDMA copy).
static hipError_t copy_rows_async(hsflow_ctx *c, void *dst, size_t dpitch, const void *src, size_t spitch, size_t rowb,
                                  size_t rows, hipMemcpyKind kind)
{
    if (dpitch == rowb && spitch == rowb) return hipMemcpyAsync(dst, src, rowb * rows, kind, c->stream);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, rowb, rows, kind, c->stream);
}

// One call of the frame-input entries below.
struct FramesIn {
    int format = HSFLOW_FRAMES_GRAY8; // HSFLOW_FRAMES_*
    const void *src[2] = {nullptr, nullptr}; // a pair: prev, curr; a push: the next frame alone
    size_t stride[2] = {0, 0};
    bool host = true;   // the sources are host memory, else device memory on ctx's device
    bool async = false; // only enqueued (host buffers belong to the context until hsflow_synchronize), else complete on return
    bool push = false;  // the camera sequence instead of a pair: prev := reblur_prev ? box_blur3(curr) : curr, curr := pre(src[0])
    int reblur_prev = 0;
};

// Host rows of a frame into device memory: blocking (the caller has drained the stream), or enqueued.
static hipError_t upload_rows(hsflow_ctx *c, void *dst, size_t dpitch, const void *src, size_t spitch, size_t rowb, bool async)
{
    if (!async) return hipMemcpy2D(dst, dpitch, src, spitch, rowb, c->H, hipMemcpyHostToDevice);
    return copy_rows_async(c, dst, dpitch, src, spitch, rowb, c->H, hipMemcpyHostToDevice);
}

// The staging of host frames: two areas of dScratch (`slot` 0 / 1, so that both frames of a pair can be in flight), each a
// packed BGR frame followed by two gray planes of pitch P.
static int stage_area(hsflow_ctx *c, int slot, uint8_t **bgr, uint8_t **gray)
{
    const size_t bgr_bytes = (size_t)c->W * 3 * c->H, one = bgr_bytes + 2 * (size_t)c->plane;
    const int st = scratch_reserve(c, 2 * one);
    *bgr = (uint8_t *)c->dScratch + (size_t)slot * one;
    *gray = *bgr + bgr_bytes;
    return st;
}

// Every way frames enter a context.  HSFLOW_FRAMES_GRAY8 is a copy into the planes.  The other formats: frames in device
// memory, and a pushed host frame once it is staged, are ONE k_pre_pair launch (hs_kernels_pre.hip.h).  A host PAIR still
// goes frame by frame through k_bgr2gray / k_box_blur3 and a gray plane of the staging: staging both frames as they are
// and running the one launch on them gave the same bytes but a 1080p BGR host-buffer stream 12 % slower, for a reason
// not found yet, so that route is held back.  A push (OpticalFlowOpenCV.cpp:92-93,118) is two launches
// in stream order -- one could not do both: the second write would race the first read of the same plane -- into the
// planes the cached graphs were captured with.
static int frames_in(hsflow_ctx *c, int pair, const FramesIn &f)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = settle_pending(c))) return st; // an unverified asynchronous solve still needs the old inputs
    const int n = f.push ? 1 : 2;
    if (!f.src[0] || (n == 2 && !f.src[1])) return fail(c, HSFLOW_E_ARG, "null frame pointer");
    if (!hspre::format_known(f.format)) return fail(c, HSFLOW_E_ARG, "unknown frame format");
    if (f.reblur_prev != 0 && f.reblur_prev != 1) return fail(c, HSFLOW_E_ARG, "reblur_prev must be 0 or 1");
    const bool colour = hspre::format_colour(f.format), plain = f.format == HSFLOW_FRAMES_GRAY8;
    const size_t rowb = (size_t)c->W * (colour ? 3 : 1);
    if (f.stride[0] < rowb || (n == 2 && f.stride[1] < rowb))
        return fail(c, HSFLOW_E_SIZE, colour ? "colour frame stride smaller than 3*width" : "frame stride smaller than width");
    if (f.push && !c->frames_set) return fail(c, HSFLOW_E_STATE, "push_frame needs a previous pair");
    uint8_t *dPrev = c->dA + pair * c->plane, *dCurr = c->dB + pair * c->plane;
    uint8_t *dst[2] = {f.push ? dCurr : dPrev, dCurr}; // where source i goes
    const bool wait = f.host && !f.async;              // complete on return: blocking copies on a drained stream
    const bool first_sync = wait && !(plain && f.push); // (a plain gray push waits once, behind its plane copy)
    uint8_t *bgr[2] = {nullptr, nullptr}, *gray[2] = {nullptr, nullptr};
    if (f.host && !plain)
        for (int i = 0; i < 2; i++)
            if ((st = stage_area(c, i, &bgr[i], &gray[i]))) return st;
    if (first_sync) HS_HIP(c, hipStreamSynchronize(c->stream));
    if (f.push && f.reblur_prev) HS_HIP(c, launch_pre_fused(c, HSFLOW_FRAMES_GRAY8_BLUR, 1, dCurr, (size_t)c->P, nullptr, 0, dPrev, nullptr));
    else if (f.push) HS_HIP(c, hipMemcpyAsync(dPrev, dCurr, (size_t)c->plane, hipMemcpyDeviceToDevice, c->stream));
    if (plain && f.host) { // host gray: straight into the planes
        if (wait && f.push) HS_HIP(c, hipStreamSynchronize(c->stream)); // (the plane copy above reads dCurr)
        for (int i = 0; i < n; i++) HS_HIP(c, upload_rows(c, dst[i], c->P, f.src[i], f.stride[i], rowb, f.async));
    } else if (plain && f.push) {
        HS_HIP(c, hipMemcpy2DAsync(dCurr, c->P, f.src[0], f.stride[0], rowb, c->H, hipMemcpyDeviceToDevice, c->stream));
    } else if (plain) {
        HS_HIP(c, launch_frame_copy(c, pair, f.src[0], f.stride[0], f.src[1], f.stride[1]));
    } else if (!f.host) {
        HS_HIP(c, launch_pre_fused(c, f.format, n, f.src[0], f.stride[0], f.src[1], f.stride[1], dst[0], dst[1]));
    } else if (f.push) { // a host frame: staged in area 1 as it is, then the same launch
        uint8_t *s = colour ? bgr[1] : gray[1];
        const size_t sp = colour ? rowb : (size_t)c->P;
        HS_HIP(c, upload_rows(c, s, sp, f.src[0], f.stride[0], rowb, f.async));
        HS_HIP(c, launch_pre_fused(c, f.format, 1, s, sp, nullptr, 0, dCurr, nullptr));
        HS_HIP(c, hipStreamSynchronize(c->stream));
    } else { // a host pair: frame by frame through the two kernels (see above)
        const bool blur = hspre::format_blur(f.format);
        const dim3 grid((c->W + 255) / 256, (c->H + 3) / 4), block(64, 4);
        for (int i = 0; i < 2; i++) {
            uint8_t *mid = blur ? gray[i] : dst[i]; // the gray frame before the blur
            if (colour) {
                HS_HIP(c, upload_rows(c, bgr[i], rowb, f.src[i], f.stride[i], rowb, f.async));
                hipLaunchKernelGGL(hsk::k_bgr2gray, grid, block, 0, c->stream, bgr[i], (long long)rowb, mid, c->W, c->H, c->P);
            } else HS_HIP(c, upload_rows(c, mid, c->P, f.src[i], f.stride[i], rowb, f.async));
            if (blur) hipLaunchKernelGGL(hsk::k_box_blur3, grid, block, 0, c->stream, gray[i], dst[i], c->W, c->H, c->P);
            HS_HIP(c, hipGetLastError());
        }
        if (wait) HS_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (!f.push) c->frames_set = true;
    c->coef_valid = false;
    return HSFLOW_OK;
}

static FramesIn pair_in(int format, const void *prev, size_t ps, const void *curr, size_t cs, bool host, bool async)
{
    FramesIn f;
    f.format = format; f.src[0] = prev; f.src[1] = curr; f.stride[0] = ps; f.stride[1] = cs; f.host = host; f.async = async;
    return f;
}

static FramesIn push_in(int format, const void *next, size_t ns, int reblur_prev, bool host)
{
    FramesIn f;
    f.format = format; f.src[0] = next; f.stride[0] = ns; f.host = host; f.async = !host; f.push = true; f.reblur_prev = reblur_prev;
    return f;
}

int hsflow_set_frames_u8(hsflow_ctx *c, int pair, const uint8_t *prev, size_t ps, const uint8_t *curr, size_t cs)
{
    return frames_in(c, pair, pair_in(HSFLOW_FRAMES_GRAY8, prev, ps, curr, cs, true, false));
}

int hsflow_set_frames_u8_async(hsflow_ctx *c, int pair, const uint8_t *prev, size_t ps, const uint8_t *curr, size_t cs)
{
    return frames_in(c, pair, pair_in(HSFLOW_FRAMES_GRAY8, prev, ps, curr, cs, true, true));
}

int hsflow_set_frames_u8_device(hsflow_ctx *c, int pair, const void *dprev, size_t ps, const void *dcurr, size_t cs)
{
    return frames_in(c, pair, pair_in(HSFLOW_FRAMES_GRAY8, dprev, ps, dcurr, cs, false, true));
}

int hsflow_set_frames_bgr8(hsflow_ctx *c, int pair, const uint8_t *prev, size_t ps, const uint8_t *curr, size_t cs, int blur3x3)
{
    return frames_in(c, pair, pair_in(blur3x3 ? HSFLOW_FRAMES_BGR8_BLUR : HSFLOW_FRAMES_BGR8, prev, ps, curr, cs, true, false));
}

int hsflow_set_frames_gray8_blur(hsflow_ctx *c, int pair, const uint8_t *prev, size_t ps, const uint8_t *curr, size_t cs)
{
    return frames_in(c, pair, pair_in(HSFLOW_FRAMES_GRAY8_BLUR, prev, ps, curr, cs, true, false));
}

int hsflow_set_frames_bgr8_async(hsflow_ctx *c, int pair, const uint8_t *prev, size_t ps, const uint8_t *curr, size_t cs, int blur3x3)
{
    return frames_in(c, pair, pair_in(blur3x3 ? HSFLOW_FRAMES_BGR8_BLUR : HSFLOW_FRAMES_BGR8, prev, ps, curr, cs, true, true));
}

int hsflow_set_frames_gray8_blur_async(hsflow_ctx *c, int pair, const uint8_t *prev, size_t ps, const uint8_t *curr, size_t cs)
{
    return frames_in(c, pair, pair_in(HSFLOW_FRAMES_GRAY8_BLUR, prev, ps, curr, cs, true, true));
}

int hsflow_set_frames_device_ex(hsflow_ctx *c, int pair, int format, const void *dprev, size_t ps, const void *dcurr, size_t cs)
{
    return frames_in(c, pair, pair_in(format, dprev, ps, dcurr, cs, false, true));
}

int hsflow_push_frame_u8(hsflow_ctx *c, int pair, const uint8_t *next, size_t ns)
{
    return frames_in(c, pair, push_in(HSFLOW_FRAMES_GRAY8, next, ns, 0, true));
}

int hsflow_push_frame_ex(hsflow_ctx *c, int pair, int format, const uint8_t *next, size_t stride, int reblur_prev)
{
    return frames_in(c, pair, push_in(format, next, stride, reblur_prev, true));
}

int hsflow_push_frame_device_ex(hsflow_ctx *c, int pair, int format, const void *d_next, size_t stride, int reblur_prev)
{
    return frames_in(c, pair, push_in(format, d_next, stride, reblur_prev, false));
}

int hsflow_preprocess_frame_host(int format, const uint8_t *src, size_t src_stride, int width, int height, uint8_t *dst, size_t dst_stride)
{
    switch (hspre::preprocess_host(format, src, src_stride, width, height, dst, dst_stride)) {
    case 0: return HSFLOW_OK;
    case 1: return fail(nullptr, HSFLOW_E_ARG, "hsflow_preprocess_frame_host: null pointer or unknown frame format");
    case 2: return fail(nullptr, HSFLOW_E_SIZE, "hsflow_preprocess_frame_host: non-positive size or stride smaller than a row");
    default: return fail(nullptr, HSFLOW_E_OOM, "hsflow_preprocess_frame_host: host allocation failed");
    }
}

// The camera loop's frame handling for n_frames frames at once (OpticalFlowOpenCV.cpp:76-93,118): every argument is
// checked, an owed check is settled against the frames that are there, and then the planes of the pairs receive the
// results of one launch per chunk -- the planes the context has always had, so cached graphs stay valid.
int hsflow_set_sequence_device_ex(hsflow_ctx *c, int first_pair, int format, const void *const *d_frames, int n_frames, size_t stride, int flags)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (!d_frames) return fail(c, HSFLOW_E_ARG, "null frame list");
    if (n_frames < 2) return fail(c, HSFLOW_E_ARG, "a sequence needs at least two frames");
    if (first_pair < 0 || (long long)first_pair + n_frames - 1 > c->N) return fail(c, HSFLOW_E_ARG, "the sequence's pairs exceed the context's");
    for (int j = 0; j < n_frames; j++)
        if (!d_frames[j]) return fail(c, HSFLOW_E_ARG, "frame " + std::to_string(j) + ": null frame pointer");
    if (!hspre::format_known(format)) return fail(c, HSFLOW_E_ARG, "unknown frame format");
    if (!hspre::seq_flags_known(flags)) return fail(c, HSFLOW_E_ARG, "flags must be 0, HSFLOW_SEQ_REBLUR or HSFLOW_SEQ_REBLUR | HSFLOW_SEQ_REBLUR_FIRST");
    const int maxf = pre_seq_max();
    if (!maxf) return fail(c, HSFLOW_E_ARG, "HSFLOW_PRE_SEQ_MAX in the environment must be 1 .. " + std::to_string(HSFLOW_PRE_SEQ_MAX));
    if (stride < (size_t)c->W * (hspre::format_colour(format) ? 3 : 1))
        return fail(c, HSFLOW_E_SIZE, hspre::format_colour(format) ? "colour frame stride smaller than 3*width" : "frame stride smaller than width");
    if ((st = settle_pending(c))) return st; // an unverified asynchronous solve still needs the old inputs
    HS_HIP(c, launch_pre_sequence(c, first_pair, format, d_frames, n_frames, stride, flags, maxf));
    c->frames_set = true;
    c->coef_valid = false;
    return HSFLOW_OK;
}

int hsflow_preprocess_sequence_host(int format, int flags, const uint8_t *const *frames, int n_frames, size_t stride, int width, int height,
                                    uint8_t *const *prev, uint8_t *const *curr, size_t dst_stride)
{
    switch (hspre::preprocess_sequence_host(format, flags, frames, n_frames, stride, width, height, prev, curr, dst_stride)) {
    case 0: return HSFLOW_OK;
    case 1: return fail(nullptr, HSFLOW_E_ARG, "hsflow_preprocess_sequence_host: null pointer, unknown frame format or flags, or fewer than two frames");
    default: return fail(nullptr, HSFLOW_E_SIZE, "hsflow_preprocess_sequence_host: non-positive size or stride smaller than a row");
    }
}

int hsflow_set_async_reduce(hsflow_ctx *c, int on)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = settle_pending(c))) return st;
    if (on && !c->hMark) { // the marker word (page-locked, device-visible) and its device-side counter
        HS_HIP(c, hipMalloc((void **)&c->dSeq, 2 * sizeof(unsigned)));
        HS_HIP(c, hipMemsetAsync(c->dSeq, 0, 2 * sizeof(unsigned), c->stream));
        HS_HIP(c, hipHostMalloc((void **)&c->hMark, 64, hipHostMallocMapped | hipHostMallocCoherent));
        HS_HIP(c, hipHostGetDevicePointer((void **)&c->hMarkDev, c->hMark, 0));
        *c->hMark = 0u;
        c->mark_issued = 0;
    }
    c->last_marked = false;
    c->async_reduce = on != 0;
    return HSFLOW_OK;
}

int hsflow_set_eps_rows(hsflow_ctx *c, int first_row, int rows)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (rows > 0 && (first_row < 0 || first_row + rows > c->H)) return fail(c, HSFLOW_E_SIZE, "Eps row window outside the frame");
    if ((st = settle_pending(c))) return st;
    const int r0 = rows > 0 ? first_row : 0, n = rows > 0 ? rows : 0;
    if (r0 != c->eps_row0 || n != c->eps_rows) {
        drop_graphs(c); // captured launches carry the window in their geometry
        c->plan_cache.clear();
        c->lastl.valid = false;
        c->eps_row0 = r0;
        c->eps_rows = n;
    }
    return HSFLOW_OK;
}

// What hsflow_verify re-solves: the parameters of the last solve asked for through the ABI, and how that ended.
static int note_solve(hsflow_ctx *c, const hsflow_params *p, int st)
{
    if (!c) return st;
    c->vstate = st ? 2 : 1;
    c->last_status = st;
    if (!st) {
        c->vparams = *p;
        c->v_org = c->org; c->v_eps_row0 = c->eps_row0; c->v_eps_rows = c->eps_rows;
        c->v_per_pair = c->per_pair;
    }
    return st;
}

// hsflow_solve_probe and hsflow_solve_probe_pairs (pairs: c->sweep_eps_pairs is filled too)
static int probe_impl(hsflow_ctx *c, const hsflow_params *pp, const float *sweep_eps, bool pairs)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (!pp || pp->struct_size != sizeof(hsflow_params)) return fail(c, HSFLOW_E_ARG, "params null or struct_size mismatch");
    if (!sweep_eps) return fail(c, HSFLOW_E_ARG, "sweep_eps is null");
    if (pp->mode != HSFLOW_MODE_CV) return fail(c, HSFLOW_E_ARG, "hsflow_solve_probe: CV mode only");
    if (pp->max_iter <= 0 || pp->max_iter > (1 << 16)) return fail(c, HSFLOW_E_ARG, "hsflow_solve_probe: max_iter must be 1 .. 65536");
    if (pairs && (long long)pp->max_iter * c->N > (1LL << 28))
        return fail(c, HSFLOW_E_SIZE, "hsflow_solve_probe_pairs: max_iter x n_pairs must not exceed 2^28");
    hsflow_params q = *pp;
    q.term_type = HSFLOW_TERM_ITER | HSFLOW_TERM_EPS;
    q.epsilon = 0.0;  // Eps < 0 never holds: every sweep of the budget runs
    q.profile = 0;
    if (q.kernel == HSFLOW_KERNEL_PERSIST) q.kernel = HSFLOW_KERNEL_STRIP;
    c->force_exact = true; // the per-sweep pass, not the witness pass
    c->probe_pairs = pairs;
    c->sweep_eps.clear();
    c->sweep_eps_pairs.clear();
    st = solve_impl(c, &q, false);
    c->force_exact = false;
    c->probe_pairs = false;
    {   // to hsflow_verify a probe is an ITER solve of max_iter sweeps
        hsflow_params v = *pp;
        v.term_type = HSFLOW_TERM_ITER;
        note_solve(c, &v, st);
    }
    if (st) return st;
    if ((int)c->sweep_eps.size() != pp->max_iter) return fail(c, HSFLOW_E_STATE, "hsflow_solve_probe: the per-sweep pass did not run");
    if (!pairs) return HSFLOW_OK;
    const size_t n = (size_t)pp->max_iter, N = (size_t)c->N;
    if (c->N == 1) c->sweep_eps_pairs = c->sweep_eps;
    else if (c->sweep_eps_pairs.size() != n * N) return fail(c, HSFLOW_E_STATE, "hsflow_solve_probe_pairs: the per-pair words were not collected");
    return HSFLOW_OK;
}

int hsflow_solve_probe(hsflow_ctx *c, const hsflow_params *pp, float *sweep_eps)
{
    const int st = probe_impl(c, pp, sweep_eps, false);
    if (st) return st;
    std::memcpy(sweep_eps, c->sweep_eps.data(), c->sweep_eps.size() * sizeof(float));
    return HSFLOW_OK;
}

int hsflow_solve_probe_pairs(hsflow_ctx *c, const hsflow_params *pp, float *sweep_eps)
{
    const int st = probe_impl(c, pp, sweep_eps, true);
    if (st) return st;
    std::memcpy(sweep_eps, c->sweep_eps_pairs.data(), c->sweep_eps_pairs.size() * sizeof(float));
    return HSFLOW_OK;
}

int hsflow_set_pair_termination(hsflow_ctx *c, int per_pair)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = settle_pending(c))) return st; // the owed check belongs to a solve under the old rule
    c->per_pair = per_pair != 0; // (graphs are keyed by it; the plans do not depend on it)
    return HSFLOW_OK;
}

int hsflow_get_pair_result(hsflow_ctx *c, int pair, hsflow_pair_result *out)
{
    if (!c) return fail(nullptr, HSFLOW_E_ARG, "null context");
    if (!out || out->struct_size != sizeof(hsflow_pair_result)) return fail(c, HSFLOW_E_ARG, "hsflow_get_pair_result: out null or struct_size mismatch");
    if (pair < 0 || pair >= c->N) return fail(c, HSFLOW_E_ARG, "pair index out of range");
    if (c->vstate == 0) return fail(c, HSFLOW_E_STATE, "hsflow_get_pair_result: no solve yet on this context");
    int st = settle_pending(c);
    if (st) return st;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, HSFLOW_E_DEVICE, "hipSetDevice failed");
    if ((st = measure_last_eps(c))) return st;
    hsflow_pair_result r;
    std::memset(&r, 0, sizeof(r));
    r.struct_size = sizeof(r);
    r.pair = pair;
    if (c->pair_res_valid) { // the pairs stopped each on its own
        const hsflow_ctx::PairResult &q = c->pair_res[(size_t)pair];
        r.status = q.status; r.iterations_done = q.iterations_done; r.last_eps = q.last_eps; r.eps_rerun = q.eps_rerun;
        r.sweeps_executed = q.sweeps;
    } else { // the batch stopped as one: its values for every pair
        r.status = c->last_status; r.iterations_done = c->info.iterations_done; r.last_eps = c->info.last_eps;
        r.eps_rerun = c->info.eps_rerun; r.sweeps_executed = c->sweeps_run;
    }
    *out = r;
    return HSFLOW_OK;
}

int hsflow_take_verdict(hsflow_ctx *c, int *proven)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (!proven) return fail(c, HSFLOW_E_ARG, "proven is null");
    if (!c->pend.active) return fail(c, HSFLOW_E_STATE, "no asynchronous ITER|EPS solve is waiting for its early-stop check");
    *proven = 0;
    return settle_pending(c, proven);
}

int hsflow_solve(hsflow_ctx *c, const hsflow_params *p) { return note_solve(c, p, solve_impl(c, p, false)); }
int hsflow_solve_async(hsflow_ctx *c, const hsflow_params *p) { return note_solve(c, p, solve_impl(c, p, true)); }

int hsflow_solve_async_frames_device(hsflow_ctx *c, const void *dprev, size_t ps, const void *dcurr, size_t cs, const hsflow_params *p)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (!dprev || !dcurr || !frames_readable_in_place(c, dprev, ps, dcurr, cs)) { // the two calls it stands for
        if ((st = hsflow_set_frames_u8_device(c, 0, dprev, ps, dcurr, cs))) return st;
        return hsflow_solve_async(c, p);
    }
    if ((st = settle_pending(c))) return st; // an unverified asynchronous solve still needs the old inputs
    if (ps < (size_t)c->W || cs < (size_t)c->W) return fail(c, HSFLOW_E_SIZE, "frame stride smaller than width");
    // who copies the frames is the solve's decision (resolve_lazy_frames); a solve that fails before it has decided leaves
    // the copy to this call, so that the context holds the new frames either way, as after hsflow_set_frames_u8_device
    c->lazy.active = true;
    c->lazy.A = (const uint8_t *)dprev; c->lazy.B = (const uint8_t *)dcurr;
    c->lazy.PA = (long long)ps; c->lazy.PB = (long long)cs;
    c->frames_set = true;
    c->coef_valid = false;
    st = note_solve(c, p, solve_impl(c, p, true));
    const int st2 = resolve_lazy_frames(c, false);
    return st ? st : st2;
}

int hsflow_frame_copies_elided(hsflow_ctx *c, uint64_t *count)
{
    if (!c || !count) return HSFLOW_E_ARG;
    *count = c->copies_elided;
    return HSFLOW_OK;
}

int hsflow_wait_solve(hsflow_ctx *c)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    // (with the witness words reduced in-stream the owed check is settled by waiting for the solve's event; otherwise
    // settle_pending enqueues the reduction and waits for the stream)
    if ((st = settle_pending(c))) return st;
    if (c->last_marked) { if ((st = wait_marker(c, c->mark_issued))) return st; }
    else HS_HIP(c, hipStreamSynchronize(c->stream));
    return check_persist(c);
}

int hsflow_synchronize(hsflow_ctx *c)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if ((st = settle_pending(c))) return st;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    return check_persist(c);
}

int hsflow_get_flow(hsflow_ctx *c, int pair, float *u, size_t us, float *v, size_t vs)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!u || !v) return fail(c, HSFLOW_E_ARG, "null flow pointer");
    const size_t rowb = (size_t)c->W * 4;
    if ((us & 3) || (vs & 3) || us < rowb || vs < rowb) return fail(c, HSFLOW_E_SIZE, "flow stride must be a multiple of 4 and >= 4*width");
    if ((st = settle_pending(c))) return st;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    if ((st = check_persist(c))) return st;
    HS_HIP(c, hipMemcpy2D(u, us, c->dU[c->cur] + pair * c->plane, (size_t)c->P * 4, rowb, c->H, hipMemcpyDeviceToHost));
    HS_HIP(c, hipMemcpy2D(v, vs, c->dV[c->cur] + pair * c->plane, (size_t)c->P * 4, rowb, c->H, hipMemcpyDeviceToHost));
    return HSFLOW_OK;
}

int hsflow_get_flow_async(hsflow_ctx *c, int pair, float *u, size_t us, float *v, size_t vs)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!u || !v) return fail(c, HSFLOW_E_ARG, "null flow pointer");
    const size_t rowb = (size_t)c->W * 4;
    if ((us & 3) || (vs & 3) || us < rowb || vs < rowb) return fail(c, HSFLOW_E_SIZE, "flow stride must be a multiple of 4 and >= 4*width");
    HS_HIP(c, copy_rows_async(c, u, us, c->dU[c->cur] + pair * c->plane, (size_t)c->P * 4, rowb, c->H, hipMemcpyDeviceToHost));
    HS_HIP(c, copy_rows_async(c, v, vs, c->dV[c->cur] + pair * c->plane, (size_t)c->P * 4, rowb, c->H, hipMemcpyDeviceToHost));
    c->flow_after_mark = true;
    return HSFLOW_OK;
}

static int flow_rows_args(hsflow_ctx *c, int pair, int row0, int nrows, const void *du, size_t us, const void *dv, size_t vs)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!du || !dv) return fail(c, HSFLOW_E_ARG, "null flow pointer");
    if (row0 < 0 || nrows <= 0 || row0 + nrows > c->H) return fail(c, HSFLOW_E_SIZE, "row range outside the frame");
    const size_t rowb = (size_t)c->W * 4;
    if ((us & 3) || (vs & 3) || us < rowb || vs < rowb) return fail(c, HSFLOW_E_SIZE, "flow stride must be a multiple of 4 and >= 4*width");
    return HSFLOW_OK;
}

int hsflow_flow_view_device(hsflow_ctx *c, int pair, const float **du, const float **dv, size_t *stride_bytes)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!du || !dv || !stride_bytes) return fail(c, HSFLOW_E_ARG, "null out pointer");
    if ((st = settle_pending(c))) return st;
    // the flow is final behind the last solve -- unless copies into or out of the planes were enqueued since: then the stream
    if (c->last_marked && !c->flow_after_mark) { if ((st = wait_marker(c, c->mark_issued))) return st; }
    else {
        HS_HIP(c, hipStreamSynchronize(c->stream));
        c->flow_after_mark = false;
    }
    if ((st = check_persist(c))) return st;
    *du = c->dU[c->cur] + pair * c->plane;
    *dv = c->dV[c->cur] + pair * c->plane;
    *stride_bytes = (size_t)c->P * sizeof(float);
    return HSFLOW_OK;
}

int hsflow_get_flow_device(hsflow_ctx *c, int pair, int row0, int nrows, void *du, size_t us, void *dv, size_t vs)
{
    int st = flow_rows_args(c, pair, row0, nrows, du, us, dv, vs);
    if (st) return st;
    // rows handed to another consumer on the device (halo exchange) must be final: an ITER|EPS check that
    // hsflow_solve_async still owes is settled first (a re-run would change them)
    if ((st = settle_pending(c))) return st;
    const size_t rowb = (size_t)c->W * 4;
    const long long off = pair * c->plane + (long long)row0 * c->P;
    HS_HIP(c, hipMemcpy2DAsync(du, us, c->dU[c->cur] + off, (size_t)c->P * 4, rowb, nrows, hipMemcpyDeviceToDevice, c->stream));
    HS_HIP(c, hipMemcpy2DAsync(dv, vs, c->dV[c->cur] + off, (size_t)c->P * 4, rowb, nrows, hipMemcpyDeviceToDevice, c->stream));
    c->flow_after_mark = true;
    return HSFLOW_OK;
}

int hsflow_set_flow_device(hsflow_ctx *c, int pair, int row0, int nrows, const void *du, size_t us, const void *dv, size_t vs)
{
    return hsflow_set_flow_device_ex(c, pair, row0, nrows, du, us, dv, vs, 0);
}

int hsflow_set_flow_device_ex(hsflow_ctx *c, int pair, int row0, int nrows, const void *du, size_t us, const void *dv, size_t vs, int flags)
{
    int st = flow_rows_args(c, pair, row0, nrows, du, us, dv, vs);
    if (st) return st;
    if (flags & ~HSFLOW_FLOW_SOLVER_MADE) return fail(c, HSFLOW_E_ARG, "hsflow_set_flow_device_ex: unknown flag");
    if ((st = settle_pending(c))) return st; // an unverified asynchronous solve still needs the old inputs
    c->lastl.valid = false;                  // (its last_eps can no longer be measured: the flow is about to change)
    if (!(flags & HSFLOW_FLOW_SOLVER_MADE)) c->flow_tame = false; // (the caller's values: the next warm strip / fold solve measures the planes)
    const size_t rowb = (size_t)c->W * 4;
    const long long off = pair * c->plane + (long long)row0 * c->P;
    HS_HIP(c, hipMemcpy2DAsync(c->dU[c->cur] + off, (size_t)c->P * 4, du, us, rowb, nrows, hipMemcpyDeviceToDevice, c->stream));
    HS_HIP(c, hipMemcpy2DAsync(c->dV[c->cur] + off, (size_t)c->P * 4, dv, vs, rowb, nrows, hipMemcpyDeviceToDevice, c->stream));
    c->flow_after_mark = true;
    return HSFLOW_OK;
}

int hsflow_get_derivatives(hsflow_ctx *c, int pair, float *dx, float *dy, float *dt, size_t stride)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!dx || !dy || !dt) return fail(c, HSFLOW_E_ARG, "null derivative pointer");
    const size_t rowb = (size_t)c->W * 4;
    if ((stride & 3) || stride < rowb) return fail(c, HSFLOW_E_SIZE, "stride must be a multiple of 4 and >= 4*width");
    if (!c->coef_valid) return fail(c, HSFLOW_E_STATE, "no derivatives yet: call hsflow_solve first");
    if ((st = scratch_reserve(c, (size_t)c->W * c->H * 3 * sizeof(float)))) return st;
    float *sx = (float *)c->dScratch, *sy = sx + (size_t)c->W * c->H, *stt = sy + (size_t)c->W * c->H;
    if (c->coef_mode == HSFLOW_MODE_CLASSIC) // (each mode packs its derivatives its own way)
        hipLaunchKernelGGL(hsk::k_unpack_deriv<true>, dim3((c->W + 255) / 256, c->H), dim3(256), 0, c->stream,
                           c->dCoef + pair * c->plane, sx, sy, stt, c->W, c->H, c->P);
    else
        hipLaunchKernelGGL(hsk::k_unpack_deriv<false>, dim3((c->W + 255) / 256, c->H), dim3(256), 0, c->stream,
                           c->dCoef + pair * c->plane, sx, sy, stt, c->W, c->H, c->P);
    HS_HIP(c, hipGetLastError());
    HS_HIP(c, hipStreamSynchronize(c->stream));
    HS_HIP(c, hipMemcpy2D(dx, stride, sx, rowb, rowb, c->H, hipMemcpyDeviceToHost));
    HS_HIP(c, hipMemcpy2D(dy, stride, sy, rowb, rowb, c->H, hipMemcpyDeviceToHost));
    HS_HIP(c, hipMemcpy2D(dt, stride, stt, rowb, rowb, c->H, hipMemcpyDeviceToHost));
    return HSFLOW_OK;
}

int hsflow_get_frames_u8(hsflow_ctx *c, int pair, uint8_t *prev, size_t ps, uint8_t *curr, size_t cs)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!prev || !curr) return fail(c, HSFLOW_E_ARG, "null frame pointer");
    if (ps < (size_t)c->W || cs < (size_t)c->W) return fail(c, HSFLOW_E_SIZE, "frame stride smaller than width");
    HS_HIP(c, hipStreamSynchronize(c->stream));
    HS_HIP(c, hipMemcpy2D(prev, ps, c->dA + pair * c->plane, c->P, c->W, c->H, hipMemcpyDeviceToHost));
    HS_HIP(c, hipMemcpy2D(curr, cs, c->dB + pair * c->plane, c->P, c->W, c->H, hipMemcpyDeviceToHost));
    return HSFLOW_OK;
}

int hsflow_get_info(hsflow_ctx *c, hsflow_info *info) { return hsflow_get_info_ex(c, info, 1); }

int hsflow_get_info_ex(hsflow_ctx *c, hsflow_info *info, int measure_eps)
{
    if (!c) return fail(nullptr, HSFLOW_E_ARG, "null context");
    if (!info || info->struct_size != sizeof(hsflow_info)) return fail(c, HSFLOW_E_ARG, "info null or struct_size mismatch");
    int st = settle_pending(c); // iterations_done of an asynchronous ITER|EPS solve
    if (st) return st;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, HSFLOW_E_DEVICE, "hipSetDevice failed");
    if (measure_eps && (st = measure_last_eps(c))) return st; // ... and its last_eps, measured now that somebody asks
    *info = c->info;
    return HSFLOW_OK;
}

int hsflow_calc_optical_flow_hs_8u32f(const uint8_t *prev, const uint8_t *curr, int img_step, int width, int height,
                                      int use_previous, float *velx, float *vely, int vel_step, float lambda,
                                      int term_type, int max_iter, double epsilon)
{
    // argument checks of the original, cv210.dll VA 0x1012e089-0x1012e0c7
    if (!prev || !curr || !velx || !vely) return fail(nullptr, HSFLOW_E_ARG, "null pointer");
    if (width <= 0 || height <= 0 || width > img_step || (vel_step & 3) || width * 4 > vel_step)
        return fail(nullptr, HSFLOW_E_SIZE, "bad size or step");
    // The reference calls cvCalcOpticalFlowHS once per frame of a stream (OpticalFlowOpenCV.cpp:94):
    // building a context per call (7 device allocations, a stream) would cost several solves, so the
    // one-shot form keeps the last context and reuses it while the frame size stays the same.
    std::lock_guard<std::mutex> lock(g_oneshot_mutex);
    hsflow_ctx *c = g_oneshot;
    int st = HSFLOW_OK;
    if (!c || c->W != width || c->H != height) {
        if (c) hsflow_destroy(c);
        g_oneshot = c = nullptr;
        if ((st = hsflow_create(&c, 0, width, height, 1, nullptr, 1))) return st;
        g_oneshot = c;
    }
    hsflow_params p;
    hsflow_default_params(&p);
    p.lambda = lambda; p.term_type = term_type; p.max_iter = max_iter; p.epsilon = epsilon;
    p.use_previous = use_previous ? 1 : 0;
    st = hsflow_set_frames_u8(c, 0, prev, (size_t)img_step, curr, (size_t)img_step);
    if (!st && use_previous) { // the caller's velx/vely are the starting flow
        const size_t rowb = (size_t)width * 4;
        hipError_t e = hipMemcpy2D(c->dU[c->cur], (size_t)c->P * 4, velx, (size_t)vel_step, rowb, height, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy2D(c->dV[c->cur], (size_t)c->P * 4, vely, (size_t)vel_step, rowb, height, hipMemcpyHostToDevice);
        if (e != hipSuccess) st = HSFLOW_E_DEVICE;
        c->flow_tame = false;
    }
    if (!st) st = hsflow_solve(c, &p);
    if (!st) st = hsflow_get_flow(c, 0, velx, (size_t)vel_step, vely, (size_t)vel_step);
    if (st) { // do not keep a context in an unknown state
        g_create_error = c->err;
        hsflow_destroy(c);
        g_oneshot = nullptr;
    }
    return st;
}

int hsflow_plan_query(int width, int height, int n_pairs, const hsflow_params *pp, hsflow_info *out)
{
    if (!pp || pp->struct_size != sizeof(hsflow_params)) return fail(nullptr, HSFLOW_E_ARG, "params null or struct_size mismatch");
    if (!out || out->struct_size != sizeof(hsflow_info)) return fail(nullptr, HSFLOW_E_ARG, "info null or struct_size mismatch");
    if (width <= 0 || height <= 0 || n_pairs <= 0) return fail(nullptr, HSFLOW_E_SIZE, "width, height, n_pairs must be positive");
    if ((long long)round_up(width, 64) * height > (1LL << 30)) return fail(nullptr, HSFLOW_E_SIZE, "plane too large (pitch*height > 2^30)");
    hsflow_ctx c; // host-side shell only: the planners read sizes, nothing touches a device
    c.W = width; c.H = height; c.N = n_pairs;
    c.P = round_up(width, 64);
    c.plane = (long long)c.P * height;
    std::memset(&c.info, 0, sizeof(c.info));
    c.info.struct_size = sizeof(hsflow_info);
    c.info.width = width; c.info.height = height; c.info.n_pairs = n_pairs; c.info.pitch = c.P;
    const hsflow_params &p = *pp;
    int st = HSFLOW_OK;
    if (p.mode == HSFLOW_MODE_CV) {
        SolveSetup S;
        st = prepare_solve(&c, p, false, S);
        if (!st) {
            const long long b = S.budget > (1LL << 30) ? 0 : S.budget;
            c.info.jacobi_launches = S.persist ? 1 : S.multi ? (int)((b + S.T - 1) / S.T) : (int)b;
        }
    } else if (p.mode == HSFLOW_MODE_CLASSIC || p.mode == HSFLOW_MODE_CLASSIC_AS_SHIPPED) {
        ClassicSetup S;
        st = prepare_classic(&c, p, S);
    } else st = fail(&c, HSFLOW_E_ARG, "unknown mode");
    if (st) { g_create_error = c.err; return st; }
    *out = c.info;
    return HSFLOW_OK;
}

void hsflow_release_cached(void)
{
    std::lock_guard<std::mutex> lock(g_oneshot_mutex);
    if (g_oneshot) hsflow_destroy(g_oneshot);
    g_oneshot = nullptr;
}

} // extern "C"

#include "hs_postops.hip.h" // what the operators on a solved flow share: the synchronous bracket, staging, statistics, batches
#include "hs_render.hip.h" // hsflow_render_flow[_device], hsflow_default_render_params
#include "hs_color.hip.h"  // hsflow_color_flow[_host|_device|_batch_device], hsflow_default_color_params
#include "hs_warp.hip.h"   // hsflow_warp[_host|_device|_batch_device], hsflow_default_warp_params
#include "hs_fb.hip.h"     // hsflow_fb[_host|_device|_batch_device|_planes_device|_planes], hsflow_set_frames_reversed, hsflow_default_fb_params
#include "hs_median.hip.h" // hsflow_median[_host|_device|_batch_device|_planes_device|_apply], hsflow_default_median_params
#include "hs_interp.hip.h" // hsflow_interp[_host|_device|_batch_device], hsflow_project_flow_host / _device, hsflow_default_interp_params
#include "hs_pyramid.hip.h" // hsflow_solve_pyramid, hsflow_pyramid_plan / _down_host / _prolong_host / _get_level, hsflow_get_pyramid_info, hsflow_default_pyramid_params
#include "hs_chain.hip.h"  // hsflow_chain_flow[_host|_device], hsflow_chain_planes_device, hsflow_track_points[_host|_device], hsflow_default_chain_params
#include "hs_gmotion.hip.h" // hsflow_gmotion_fit[_host|_device|_batch_device|_planes_device], hsflow_gmotion_warp[_host|_device], hsflow_gmotion_compose_host / _invert_host, hsflow_default_gmotion_params
#include "hs_regions.hip.h" // hsflow_regions[_host|_device|_batch_device|_planes_device], hsflow_default_regions_params
#include "hs_link.hip.h"    // hsflow_link_regions[_host|_device|_batch_device|_planes_device], hsflow_link_tracks_host, hsflow_default_link_params
#include "hs_corners.hip.h" // hsflow_corners[_host|_device|_batch_device|_planes_device], hsflow_default_corners_params
#include "hs_verify.hip.h" // hsflow_verify, hsflow_compare_flow_device, hsflow_compare_planes_host
#include "hs_jpeg.hip.h"   // hsflow_jpeg_bound, hsflow_jpeg_encode_host / _device, hsflow_render_flow_jpeg[_device]
#include "hs_jpegd.hip.h"  // hsflow_jpeg_read_header, hsflow_jpeg_decode[_host|_device], hsflow_set_frames_jpeg, hsflow_push_frame_jpeg
