// hs_kernels_fb.hip.h -- the forward-backward consistency of two flow fields (hs_fb_rule.h) where the flows lie: a u8
// mask of the four classes, the squared error as an fp32 plane and exact integer statistics, any of the three, in ONE
// launch.  The kernel is batched like k_warp_batch: the check is blockIdx.z, and an argument block by value carries, per
// check, the forward and the backward planes and the two destinations.  The forward planes are a context's (base at a
// 256-byte multiple, pitch a multiple of 64 floats >= W); the backward planes have a base and a stride in bytes of their
// own (any multiple of 4), so one kernel serves pairs of one context and backward planes from anywhere.
// A lane takes 4 consecutive pixels of a row: one 16-byte load each of uf and vf (aligned and in bounds by the above, the
// columns beyond W masked); the four backward taps of each plane are gathered from global memory (locate() keeps every
// tap inside the W x H plane); the mask goes out as one word where its base and stride are multiples of 4 and the group
// lies inside the row, byte by byte otherwise and for the ragged end; err2 as one 16-byte store where its base and stride
// are multiples of 16 and the group lies inside the row, float by float otherwise.  Nothing beyond W bytes of a mask row
// or W floats of an err2 row is touched.
// With statistics (STATS) every lane counts in 32-bit registers.  A lane sees at most ceil(H / gridDim.y) <= 258 rows
// (pitch * H <= 2^30, pitch >= 64, gridDim.y = min(ceil(H / per), 65535)) of 4 pixels: a class counter stays below 2^11,
// and sum_q, which takes up to 65 535 per pixel, below 258 * 4 * 65 535 < 2^27.  64 such lanes could pass 2^32, so sum_q
// crosses the wavefront in two halves -- the low 16 bits (wave sum < 2^22) and the rest (lane < 2^11, wave sum < 2^17) --
// and is put together as 64 bits; the four waves add up through LDS in 64 bits.  Every counter gets one 64-bit atomicAdd
// per workgroup (none for a zero sum), the maximum one 32-bit atomicMax and only where the word is smaller, into the
// check's hsflow_fb_stats, zero before.  All are integers: the result does not depend on the order of execution.  No
// workgroup waits for another.  The host gives a workgroup several rows as enqueue_warp_chunk does (hs_fb.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_fb_rule.h"
#include "hs_kernels_warp.hip.h"

namespace hsk {

// What differs from check to check of a batch, handed to the kernel by value.
struct FbBatchChecks {
    const float *uf[kRenderBatchMax], *vf[kRenderBatchMax]; // the forward planes, rows `pitch` floats apart
    const float *ub[kRenderBatchMax], *vb[kRenderBatchMax]; // the backward planes, rows `bwd_stride` bytes apart
    uint8_t *mask[kRenderBatchMax];                         // or NULL
    float *err2[kRenderBatchMax];                           // or NULL (always NULL without ERR)
    uint32_t wide_mask;                                     // bit i: mask[i] and the mask stride are multiples of 4
    uint32_t wide_err2;                                     // bit i: err2[i] and the err2 stride are multiples of 16
};
static_assert(sizeof(FbBatchChecks) <= 2048, "the argument block stays well inside the 4 KiB of kernel arguments");

// The layout of hsflow_fb_stats (include/hsflow.h) as the kernel writes it.
struct FbStatsWords {
    unsigned long long cls[4], sum_err2_q;
    unsigned max_err2_bits;
    unsigned reserved[5];
};
static_assert(sizeof(FbStatsWords) == 64, "hsflow_fb_stats is 64 bytes");

// Grid: (ceil(W / 1024), rows, checks); 256 lanes.  With STATS every lane stays to the end: the wavefront reduces
// together.  stats: the first check's record, check i's 64 bytes behind each other.
template <bool ERR, bool STATS>
__global__ __launch_bounds__(256) void k_fb_batch(const FbBatchChecks chk, long long pitch, long long bwd_stride, long long mask_stride, long long err2_stride,
                                                  int W, int H, float alpha, float beta, unsigned value, FbStatsWords *__restrict__ stats)
{
    const unsigned i = blockIdx.z;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    hsfb::Acc acc = {{0u, 0u, 0u, 0u}, 0u, 0u};
    if (x0 < W) {
        const float *uf = chk.uf[i], *vf = chk.vf[i], *ub = chk.ub[i], *vb = chk.vb[i];
        uint8_t *mask = chk.mask[i];
        float *err2 = ERR ? chk.err2[i] : nullptr;
        const bool whole = x0 + 4 <= W;
        const bool wide_mask = ((chk.wide_mask >> i) & 1u) && whole, wide_err2 = ((chk.wide_err2 >> i) & 1u) && whole;
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            const float4 a = *(const float4 *)(uf + (long long)y * pitch + x0), b = *(const float4 *)(vf + (long long)y * pitch + x0);
            const float aa[4] = {a.x, a.y, a.z, a.w}, bb[4] = {b.x, b.y, b.z, b.w};
            unsigned m[4], e[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                m[j] = 0u;
                e[j] = 0u;
                if (x0 + j < W) {
                    const hsfb::Pixel r = hsfb::decide(aa[j], bb[j], x0 + j, y, W, H, ub, bwd_stride, vb, bwd_stride, alpha, beta);
                    m[j] = (value >> (8 * r.cls)) & 255u;
                    if (ERR) e[j] = hsfb::err2_bits(r);
                    if (STATS) hsfb::account(acc, r);
                }
            }
            if (mask) {
                uint8_t *d = mask + (long long)y * mask_stride + x0;
                if (wide_mask) {
                    *(uint32_t *)d = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (x0 + j < W) d[j] = (uint8_t)m[j];
                }
            }
            if (ERR && err2) {
                uint32_t *d = (uint32_t *)((uint8_t *)err2 + (long long)y * err2_stride) + x0;
                if (wide_err2) {
                    *(uint4 *)d = make_uint4(e[0], e[1], e[2], e[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (x0 + j < W) d[j] = e[j];
                }
            }
        }
    }
    if (!STATS) return;
    // (sum_q in two halves: see the head of this file)
    const unsigned lo = warp_wave_sum(acc.sum_q & 0xffffu), hi = warp_wave_sum(acc.sum_q >> 16);
    const unsigned long long part[6] = {warp_wave_sum(acc.cls[0]), warp_wave_sum(acc.cls[1]), warp_wave_sum(acc.cls[2]), warp_wave_sum(acc.cls[3]),
                                        ((unsigned long long)hi << 16) + lo, warp_wave_max(acc.max_bits)};
    __shared__ unsigned long long lds[4][6];
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (int k = 0; k < 6; k++) lds[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x < 6u) {
        const unsigned k = threadIdx.x;
        unsigned long long *sums = (unsigned long long *)(stats + i); // five sums, then the maximum
        if (k < 5u) {
            const unsigned long long sum = lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k];
            if (sum) atomicAdd(sums + k, sum);
        } else { // (a maximum only ever grows: the atomic is left out where the word already holds as much)
            unsigned m = (unsigned)lds[0][k];
            for (int wv = 1; wv < 4; wv++) m = (unsigned)lds[wv][k] > m ? (unsigned)lds[wv][k] : m;
            unsigned *word = (unsigned *)(sums + 5);
            if (m > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, m);
        }
    }
}

} // namespace hsk
