// hs_kernels_warp.hip.h -- a picture warped backwards by the dense flow (hs_warp_rule.h) where the flow lies, and the
// residual it leaves against a reference picture, in ONE launch.  The kernel is batched like k_color_batch: the picture is
// blockIdx.z, picture i reads the flow planes of pair i (i * plane floats behind the first), and its source, reference,
// destination and statistics pointers come from an argument block by value.
// A lane takes 4 consecutive pixels of a row: one 16-byte load each of u and v (the context's planes start at 256-byte
// multiples and their pitch is a multiple of 64 floats >= W: aligned and in bounds, the columns beyond W masked); its
// taps are gathered from src byte by byte (locate() keeps every tap inside the W x H picture); 4 * C bytes of picture out
// -- C words where the picture's base and stride are multiples of 4 and the group lies inside the row, byte by byte
// otherwise and for the ragged end; nothing beyond C * W bytes of a row is touched.
// With statistics (STATS) the same lanes read ref and src at their own pixels and count in 32-bit registers: a lane sees
// at most ceil(H / gridDim.y) <= 258 rows (pitch * H <= 2^30, pitch >= 64) of 4 pixels of 3 channels of at most 255, so a
// workgroup's sums stay below 2^28.  The wavefronts reduce by shuffles, the workgroup through LDS, and every counter gets
// one 64-bit atomicAdd (the maxima one 32-bit atomicMax) per workgroup into the picture's hsflow_warp_stats, zero before.
// All are integers: the result does not depend on the order of execution.  No workgroup waits for another.
// The atomics of one picture all land in one 64-byte line and the memory side takes them one after the other (measured:
// 3.3 ns each, profiles/warp_time.txt), so with statistics the host gives a workgroup several rows (the y loop) as soon as
// the grid still fills the device twice: 1080p runs 4 rows per workgroup, 600x480 one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_kernels_render.hip.h"
#include "hs_warp_rule.h"

namespace hsk {

// What differs from picture to picture of a batched warp, handed to the kernel by value.
struct WarpBatchPics {
    const uint8_t *src[kRenderBatchMax];
    const uint8_t *ref[kRenderBatchMax]; // or NULL: no sums of differences
    uint8_t *dst[kRenderBatchMax];       // or NULL: statistics only
    uint32_t wide;                       // bit i: dst[i] and the dst stride are multiples of 4
};

// The layout of hsflow_warp_stats (include/hsflow.h) as the kernel writes it.
struct WarpStatsWords {
    unsigned long long inside, outside, unknown, sad_warped, sad_plain;
    unsigned max_warped, max_plain;
    unsigned reserved[4];
};
static_assert(sizeof(WarpStatsWords) == 64, "hsflow_warp_stats is 64 bytes");

__device__ __forceinline__ unsigned warp_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned warp_wave_max(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Grid: (ceil(W / 1024), rows, pictures); 256 lanes.  With STATS every lane stays to the end: the wavefront reduces
// together.  stats: the first picture's record, picture i's 64 bytes behind each other.
template <int C, bool STATS>
__global__ __launch_bounds__(256) void k_warp_batch(const float *__restrict__ u, const float *__restrict__ v, long long plane, const WarpBatchPics pics,
                                                    long long src_stride, long long ref_stride, long long dst_stride, int W, int H, int P, float t,
                                                    int border, unsigned fill, WarpStatsWords *__restrict__ stats)
{
    const unsigned i = blockIdx.z;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    hswarp::Acc acc = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (x0 < W) {
        const long long o = (long long)i * plane;
        const uint8_t *src = pics.src[i], *ref = pics.ref[i];
        uint8_t *dst = pics.dst[i];
        const bool wide = ((pics.wide >> i) & 1u) && x0 + 4 <= W;
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            const float4 a = *(const float4 *)(u + o + (long long)y * P + x0), b = *(const float4 *)(v + o + (long long)y * P + x0);
            const float aa[4] = {a.x, a.y, a.z, a.w}, bb[4] = {b.x, b.y, b.z, b.w};
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                w[j] = 0u;
                if (x0 + j < W) {
                    const hswarp::Tap p = hswarp::locate(aa[j], bb[j], x0 + j, y, t, W, H, border);
                    w[j] = hswarp::pixel<C>(src, src_stride, p, fill);
                    if (STATS) {
                        const unsigned q = hswarp::load_pixel<C>(src + (long long)y * src_stride + (long long)C * (x0 + j));
                        const unsigned r = ref ? hswarp::load_pixel<C>(ref + (long long)y * ref_stride + (long long)C * (x0 + j)) : 0u;
                        hswarp::account<C>(acc, p.cls, w[j], q, r, ref != nullptr);
                    }
                }
            }
            if (!dst) continue;
            uint8_t *d = dst + (long long)y * dst_stride + (long long)C * x0;
            if (wide) {
                uint32_t *dw = (uint32_t *)d;
                if (C == 1) {
                    dw[0] = w[0] | (w[1] << 8) | (w[2] << 16) | (w[3] << 24);
                } else {
                    dw[0] = w[0] | (w[1] << 24);
                    dw[1] = (w[1] >> 8) | (w[2] << 16);
                    dw[2] = (w[2] >> 16) | (w[3] << 8);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (x0 + j < W)
#pragma unroll
                        for (int c = 0; c < C; c++) d[C * j + c] = (uint8_t)(w[j] >> (8 * c));
            }
        }
    }
    if (!STATS) return;
    unsigned part[7] = {warp_wave_sum(acc.inside),     warp_wave_sum(acc.outside),   warp_wave_sum(acc.unknown), warp_wave_sum(acc.sad_warped),
                        warp_wave_sum(acc.sad_plain),  warp_wave_max(acc.max_warped), warp_wave_max(acc.max_plain)};
    __shared__ unsigned lds[4][7];
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (int k = 0; k < 7; k++) lds[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x < 7u) {
        const unsigned k = threadIdx.x;
        unsigned long long *sums = (unsigned long long *)(stats + i); // five sums, then the two maxima
        if (k < 5u) {
            const unsigned long long sum = (unsigned long long)lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k];
            if (sum) atomicAdd(sums + k, sum);
        } else { // (a maximum only ever grows: the atomic is left out where the word already holds as much)
            unsigned m = lds[0][k];
            for (int wv = 1; wv < 4; wv++) m = lds[wv][k] > m ? lds[wv][k] : m;
            unsigned *word = (unsigned *)(sums + 5) + (k - 5u);
            if (m > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, m);
        }
    }
}

} // namespace hsk
