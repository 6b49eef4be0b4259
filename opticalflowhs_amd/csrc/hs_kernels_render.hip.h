// hs_kernels_render.hip.h -- the flow picture of the reference, drawn on the GPU:
//   OpticalFlowHS/OpticalFlowOpenCV.cpp:33-46     (threshold 1, half-length lines)
//   OpticalFlowHS/HSOpticalFlowOpenCL.cpp:759-769 (threshold 0.5, full-length lines)
// On a black image, for every grid point (y outer, x inner, multiples of `step`) whose flow passes the threshold: a
// filled dot of radius 2 and a line along the flow, LATER WRITES OVER EARLIER ONES.  That order becomes a maximum:
// write number 2k + 1 is the dot and 2k + 2 the line of grid point k (raster order, 0 = nothing), a pixel shows the
// write with the highest number that reached it, and the number's parity says which colour.  atomicMax is
// independent of the order of execution, so the picture is deterministic and equal to the host's, byte for byte.
//
//   k_render_scatter: one lane per grid point; priorities into a uint32 plane (zero before).
//   k_render_resolve: one pass over the plane: packed RGB out, zero written back -- no clear between renders.
// Each kernel's work for one picture is a __device__ body; the entries above call it with their own arguments, and
//   k_render_scatter_batch, k_render_resolve_batch take the pair from a further grid dimension: pair i reads its own
//   flow planes and owns a priority plane of its own, and its picture's pointer comes from an argument block by value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_render_line.h"

namespace hsk {

constexpr int kRenderBatchMax = 32; // pictures per set of launches (HSFLOW_JPEG_BATCH_MAX is at most this)

// What differs from picture to picture of a batched render, handed to the kernel by value.
struct RenderBatchPics {
    uint8_t *rgb[kRenderBatchMax];
    uint32_t wide; // bit i: picture i's base and the stride are multiples of 4
};

// u, v: the flow planes of one pair (pitch P floats).  prio: width x height words, pitch PP.  n = gx * gy grid points.
__device__ __forceinline__ void render_scatter_body(const float *__restrict__ u, const float *__restrict__ v, unsigned *__restrict__ prio,
                                                    int W, int H, int P, int PP, int step, int gx, unsigned n, float thr, float scale)
{
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const int x = (int)(k % (unsigned)gx) * step, y = (int)(k / (unsigned)gx) * step;
    const float a = u[(long long)y * P + x], b = v[(long long)y * P + x];
    if (!(a > thr || b > thr || a < -thr || b < -thr)) return; // (NaN in both: nothing)
    const unsigned pd = 2u * k + 1u, pl = 2u * k + 2u;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++)
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            if (dx * dx + dy * dy > 4) continue;
            const int xx = x + dx, yy = y + dy;
            if (xx >= 0 && yy >= 0 && xx < W && yy < H) atomicMax(prio + (long long)yy * PP + xx, pd);
        }
    // cvPoint(x + a*scale, y + b*scale): fp32 arithmetic, then truncation toward zero.  Outside the range where the
    // host's conversion is defined (not finite, or |.| >= 2^20) the dot stands alone (include/hsflow.h).
    const float fx = __fadd_rn((float)x, __fmul_rn(a, scale)), fy = __fadd_rn((float)y, __fmul_rn(b, scale));
    if (!(fabsf(fx) < 1048576.f && fabsf(fy) < 1048576.f)) return;
    hsline::Walk w = hsline::clip(x, y, (int)fx, (int)fy, W, H);
    for (long long i = 0; i < w.count; i++) { // at most max(W, H) steps: the in-image part only
        atomicMax(prio + (long long)w.y * PP + w.x, pl);
        hsline::advance(w);
    }
}

__global__ __launch_bounds__(256) void k_render_scatter(const float *__restrict__ u, const float *__restrict__ v, unsigned *__restrict__ prio,
                                                        int W, int H, int P, int PP, int step, int gx, unsigned n, float thr, float scale)
{
    render_scatter_body(u, v, prio, W, H, P, PP, step, gx, n, thr, scale);
}

// Grid: (ceil(n / 256), pairs).  u, v: the planes of the first pair; pair i's lie i * plane floats, its priorities
// i * plane words further.
__global__ __launch_bounds__(256) void k_render_scatter_batch(const float *__restrict__ u, const float *__restrict__ v, unsigned *__restrict__ prio,
                                                              long long plane, int W, int H, int P, int PP, int step, int gx, unsigned n, float thr,
                                                              float scale)
{
    const long long o = (long long)blockIdx.y * plane;
    render_scatter_body(u + o, v + o, prio + o, W, H, P, PP, step, gx, n, thr, scale);
}

__device__ __forceinline__ unsigned render_colour(unsigned p, unsigned dot, unsigned line)
{
    return p == 0u ? 0u : ((p & 1u) ? dot : line);
}

// Each lane takes 4 pixels of a row: one 16-byte load of priorities, 12 bytes of picture.  dot / line: R | G << 8 | B << 16.
// wide != 0: rgb and stride are multiples of 4, so the 12 bytes go out as three aligned words; the last pixels of a
// row whose width is no multiple of 4, and every pixel otherwise, go out byte by byte -- nothing beyond 3*W is touched.
__device__ __forceinline__ void render_resolve_body(unsigned *__restrict__ prio, uint8_t *__restrict__ rgb, long long stride, int W, int H,
                                                    int PP, unsigned dot, unsigned line, int wide)
{
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        uint4 *pp = (uint4 *)(prio + (long long)y * PP + x0); // PP is a multiple of 64 >= W: aligned and in bounds
        const uint4 p = *pp;
        if (p.x | p.y | p.z | p.w) *pp = make_uint4(0u, 0u, 0u, 0u);
        const unsigned c0 = render_colour(p.x, dot, line), c1 = render_colour(p.y, dot, line), c2 = render_colour(p.z, dot, line),
                       c3 = render_colour(p.w, dot, line);
        uint8_t *d = rgb + (long long)y * stride + 3ll * x0;
        if (wide && x0 + 4 <= W) {
            uint32_t *dw = (uint32_t *)d;
            dw[0] = c0 | (c1 << 24);
            dw[1] = (c1 >> 8) | (c2 << 16);
            dw[2] = (c2 >> 16) | (c3 << 8);
        } else {
            const unsigned c[4] = {c0, c1, c2, c3};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x0 + j < W) {
                    d[3 * j] = (uint8_t)c[j];
                    d[3 * j + 1] = (uint8_t)(c[j] >> 8);
                    d[3 * j + 2] = (uint8_t)(c[j] >> 16);
                }
        }
    }
}

__global__ __launch_bounds__(256) void k_render_resolve(unsigned *__restrict__ prio, uint8_t *__restrict__ rgb, long long stride, int W, int H,
                                                        int PP, unsigned dot, unsigned line, int wide)
{
    render_resolve_body(prio, rgb, stride, W, H, PP, dot, line, wide);
}

// Grid: (ceil(W / 1024), rows, pairs): pair i's priority plane into pics.rgb[i].
__global__ __launch_bounds__(256) void k_render_resolve_batch(unsigned *__restrict__ prio, long long plane, const RenderBatchPics pics, long long stride,
                                                              int W, int H, int PP, unsigned dot, unsigned line)
{
    const unsigned i = blockIdx.z;
    render_resolve_body(prio + (long long)i * plane, pics.rgb[i], stride, W, H, PP, dot, line, (int)((pics.wide >> i) & 1u));
}

} // namespace hsk
