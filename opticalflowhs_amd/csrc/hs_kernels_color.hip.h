// hs_kernels_color.hip.h -- the colour picture of the dense flow (hs_color_rule.h: the Middlebury wheel), drawn on the
// GPU from the flow where the solver left it.  Both kernels are batched: the picture is a grid dimension, picture i reads
// the flow planes of pair i (i * plane floats behind the first) and its picture's pointer comes from an argument block by
// value, as k_render_resolve_batch's does.
//   k_color_max_batch: only when the scale is taken from the picture.  The largest raw radius of picture i's known pixels
//     into scale[i] (zero before), as the BIT PATTERN of the non-negative float -- such floats order like unsigned
//     integers, so an integer atomicMax finds it, whatever the order of execution.  The wavefronts reduce by shuffles, the
//     workgroup through LDS, and its one atomic is left out where the word already holds as much (it only ever grows).
//   k_color_batch: the pixels.  The scale comes from scale[i] in device memory; no value goes through the host.  The wheel
//     lies in LDS as the 165 channel levels fl(level / 255) the rule interpolates between.
// A lane takes 4 consecutive pixels of a row: one 16-byte load each of u and v (the context's planes start at 256-byte
// multiples and their pitch is a multiple of 64 floats >= W: aligned and in bounds, the columns beyond W masked), 12 bytes
// of picture out -- three words where the picture's base and stride are multiples of 4 and the group lies inside the
// row, byte by byte otherwise and for the ragged end; nothing beyond 3*W is touched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_color_rule.h"
#include "hs_kernels_render.hip.h"

namespace hsk {

// Grid: (ceil(W / 1024), rows, pictures); 256 lanes.  Every lane stays to the end: the wavefront reduces together.
__global__ __launch_bounds__(256) void k_color_max_batch(const float *__restrict__ u, const float *__restrict__ v, long long plane, int W, int H, int P,
                                                         unsigned *__restrict__ scale)
{
    const long long o = (long long)blockIdx.z * plane;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned best = 0u;
    if (x0 < W)
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            const float4 a = *(const float4 *)(u + o + (long long)y * P + x0), b = *(const float4 *)(v + o + (long long)y * P + x0);
            const float aa[4] = {a.x, a.y, a.z, a.w}, bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x0 + j < W && hscolor::known(aa[j], bb[j])) {
                    const unsigned r = hscolor::float_bits(hscolor::radius(aa[j], bb[j]));
                    best = r > best ? r : best;
                }
        }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)best, d, 64);
        best = other > best ? other : best;
    }
    __shared__ unsigned part[4];
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (int w = 1; w < 4; w++) best = part[w] > best ? part[w] : best;
        unsigned *word = scale + blockIdx.z;
        if (best > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, best);
    }
}

// Grid: (ceil(W / 1024), rows, pictures); 256 lanes.  scale: one word per picture as k_color_max_batch left it, or NULL:
// the scale is fixed_m for every picture.
__global__ __launch_bounds__(256) void k_color_batch(const float *__restrict__ u, const float *__restrict__ v, long long plane, const RenderBatchPics pics,
                                                     long long stride, int W, int H, int P, const unsigned *__restrict__ scale, float fixed_m)
{
    __shared__ float wheel[3 * hscolor::kWheel];
    if (threadIdx.x < 3u * hscolor::kWheel) wheel[threadIdx.x] = hscolor::wheel_level((int)threadIdx.x / 3, (int)threadIdx.x % 3);
    __syncthreads();
    const unsigned i = blockIdx.z;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= W) return;
    const long long o = (long long)i * plane;
    const float m = scale ? hscolor::auto_scale(scale[i]) : fixed_m;
    uint8_t *rgb = pics.rgb[i];
    const bool wide = ((pics.wide >> i) & 1u) && x0 + 4 <= W;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const float4 a = *(const float4 *)(u + o + (long long)y * P + x0), b = *(const float4 *)(v + o + (long long)y * P + x0);
        const unsigned c0 = hscolor::pixel(a.x, b.x, m, wheel), c1 = hscolor::pixel(a.y, b.y, m, wheel), c2 = hscolor::pixel(a.z, b.z, m, wheel),
                       c3 = hscolor::pixel(a.w, b.w, m, wheel);
        uint8_t *d = rgb + (long long)y * stride + 3ll * x0;
        if (wide) {
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

} // namespace hsk
