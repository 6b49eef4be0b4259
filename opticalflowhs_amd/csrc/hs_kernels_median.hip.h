// hs_kernels_median.hip.h -- one pass of the median filter / hole filling of a flow field (hs_median_rule.h) where the
// flow lies: the filtered planes, the output state and exact integer statistics, any of the three, in ONE launch.  The
// kernel is batched like k_fb_batch: the field is blockIdx.z, and an argument block by value carries, per field, the two
// input planes, the input state and the destinations.  Every plane has a base and a row stride in BYTES (fp32 planes:
// multiples of 4; byte planes: anything), so one kernel serves the planes of a context (stride 4 * pitch) and caller
// planes from anywhere.
// A workgroup of 256 lanes takes tiles of kMedTileX x kMedTileY = 64 x 16 pixels.  It stages the tile plus a halo of R
// as keys in LDS, two planes of (16 + 2R) x (64 + 2R) words (R = 1: 9 504 bytes, R = 2: 10 880): a slot outside the frame
// or with input state 0 holds hsmed::kLow in both.  Every read of global memory is guarded by the frame, every write by
// x < W and y < H: nothing beyond W elements of a row is touched.  A wavefront then takes one row of the tile at a time
// (rows wave, wave + 4, ...): a lane scans its window from LDS (consecutive lanes, consecutive words), selects both
// medians in registers by hsmed::mid_of and reads its own pixel's bits and state byte once more from global memory (the
// bits of an invalid pixel are not in LDS).  With STATS every lane counts in 32-bit registers -- a workgroup sees at most
// 8 tiles (hs_median.hip.h), a lane 32 pixels -- the wavefront reduces, the four waves add up through LDS and every
// counter gets one 64-bit atomicAdd per workgroup (none for a zero sum) into the field's hsflow_median_stats, zero
// before.  All are integers: the result does not depend on the order of execution.  No workgroup waits for another.
// The eight instantiations live in a translation unit of their own, hs_median_kernels.hip, behind launch_median_batch:
// their code object is then a second one in the library, loaded by the first launch, and the code object of every other
// kernel stays what it was -- a process that never filters does not even load these kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_median_rule.h"

namespace hsk {

constexpr int kMedTileX = 64, kMedTileY = 16;
constexpr int kMedianBatchMax = 32; // fields per launch (= kRenderBatchMax, hs_median.hip.h holds them equal)

__device__ __forceinline__ unsigned median_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

// What differs from field to field of a batch, handed to the kernel by value.
struct MedianBatchFields {
    const float *u[kMedianBatchMax], *v[kMedianBatchMax]; // the input planes, rows `in_stride` bytes apart
    const uint8_t *state[kMedianBatchMax];                // or NULL
    float *u_out[kMedianBatchMax], *v_out[kMedianBatchMax]; // both or neither, rows `out_stride` bytes apart
    uint8_t *state_out[kMedianBatchMax];                  // or NULL
};
static_assert(sizeof(MedianBatchFields) <= 2048, "the argument block stays well inside the 4 KiB of kernel arguments");

// The layout of hsflow_median_stats (include/hsflow.h) as the kernel writes it.
struct MedianStatsWords {
    unsigned long long kept, filled, unfilled, newly_filled, changed;
    unsigned long long reserved[3];
};
static_assert(sizeof(MedianStatsWords) == 64, "hsflow_median_stats is 64 bytes");

// Grid: (ceil(W / 64), tile rows a workgroup strides over, fields); 256 lanes.  stats: the first field's record, field
// i's 64 bytes behind each other.
template <int R, bool FILL, bool STATS>
__global__ __launch_bounds__(256) void k_median_batch(const MedianBatchFields f, long long in_stride, long long state_stride, long long out_stride,
                                                      long long state_out_stride, int W, int H, int min_votes, MedianStatsWords *__restrict__ stats)
{
    constexpr int N = (2 * R + 1) * (2 * R + 1), LW = kMedTileX + 2 * R, LH = kMedTileY + 2 * R;
    __shared__ uint32_t ku[LH][LW], kv[LH][LW];
    const unsigned i = blockIdx.z;
    const uint8_t *u = (const uint8_t *)f.u[i], *v = (const uint8_t *)f.v[i], *state = f.state[i];
    uint8_t *u_out = (uint8_t *)f.u_out[i], *v_out = (uint8_t *)f.v_out[i], *state_out = f.state_out[i];
    const int tx0 = blockIdx.x * kMedTileX, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    hsmed::Acc acc = {0u, 0u, 0u, 0u, 0u};
    for (int ty0 = blockIdx.y * kMedTileY; ty0 < H; ty0 += gridDim.y * kMedTileY) {
        for (int k = threadIdx.x; k < LW * LH; k += 256) {
            const int ly = k / LW, lx = k - ly * LW;
            const int qx = tx0 - R + lx, qy = ty0 - R + ly;
            uint32_t a = hsmed::kLow, b = hsmed::kLow;
            if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                const float fa = *(const float *)(u + (long long)qy * in_stride + 4ll * qx), fb = *(const float *)(v + (long long)qy * in_stride + 4ll * qx);
                const unsigned byte = state ? state[(long long)qy * state_stride + qx] : 255u;
                if (hsmed::state_of(fa, fb, byte) != hsmed::kUnfilled) {
                    a = hsmed::key_of(__float_as_uint(fa));
                    b = hsmed::key_of(__float_as_uint(fb));
                }
            }
            ku[ly][lx] = a;
            kv[ly][lx] = b;
        }
        __syncthreads();
        const int x = tx0 + lane;
        for (int row = wave; row < kMedTileY; row += 4) {
            const int y = ty0 + row;
            if (x < W && y < H) {
                hsmed::Window<N> w;
                w.n = 0;
#pragma unroll
                for (int dy = 0; dy <= 2 * R; dy++)
#pragma unroll
                    for (int dx = 0; dx <= 2 * R; dx++) hsmed::take(w, dy * (2 * R + 1) + dx, ku[row + dy][lane + dx], kv[row + dy][lane + dx]);
                const uint32_t abits = *(const uint32_t *)(u + (long long)y * in_stride + 4ll * x), bbits = *(const uint32_t *)(v + (long long)y * in_stride + 4ll * x);
                const unsigned byte = state ? state[(long long)y * state_stride + x] : 255u;
                const int s = hsmed::state_of(__uint_as_float(abits), __uint_as_float(bbits), byte);
                const hsmed::Out o = hsmed::decide(abits, bbits, s, w.n, hsmed::mid_of(w.ku), hsmed::mid_of(w.kv), FILL ? 1 : 0, min_votes);
                if (u_out) {
                    *(uint32_t *)(u_out + (long long)y * out_stride + 4ll * x) = o.ubits;
                    *(uint32_t *)(v_out + (long long)y * out_stride + 4ll * x) = o.vbits;
                }
                if (state_out) state_out[(long long)y * state_out_stride + x] = (uint8_t)o.s_out;
                if (STATS) hsmed::account(acc, o, abits, bbits, s);
            }
        }
        __syncthreads(); // (the next tile overwrites the keys)
    }
    if (!STATS) return;
    const unsigned part[5] = {median_wave_sum(acc.kept), median_wave_sum(acc.filled), median_wave_sum(acc.unfilled), median_wave_sum(acc.newly_filled),
                              median_wave_sum(acc.changed)};
    __shared__ unsigned lds[4][5];
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 5; k++) lds[wave][k] = part[k];
    __syncthreads();
    if (threadIdx.x < 5u) {
        const unsigned k = threadIdx.x;
        const unsigned long long sum = (unsigned long long)lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k];
        if (sum) atomicAdd((unsigned long long *)(stats + i) + k, sum);
    }
}

// The launch of one pass (hs_median_kernels.hip): grid as above, 256 lanes; the status of the launch.
hipError_t launch_median_batch(int radius, bool fill, const dim3 &grid, hipStream_t stream, const MedianBatchFields &f, long long in_stride, long long state_stride,
                               long long out_stride, long long state_out_stride, int W, int H, int min_votes, MedianStatsWords *stats);

} // namespace hsk
