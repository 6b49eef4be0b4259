// hs_kernels_interp.hip.h -- the frame at time t between the two frames of a pair (hs_interp_rule.h) where the flow lies.
// Three kernels, and between the second and the third the fill's passes, which are launches of k_median_batch in FILL
// mode (hs_kernels_median.hip.h) on the scratch planes:
//   k_interp_splat    P, the scatter: every source pixel computes where it is at time t and the photo-consistency of its
//                     vector, and takes its cell of the key plane by ONE 64-bit atomicMin (cost << 32 | source index).
//                     The key plane is all-ones before (a memset in front).  A minimum does not depend on the order of
//                     arrival: the result is deterministic.  The lane mapping is k_warp_batch's: 4 consecutive pixels of
//                     a row per lane, one 16-byte load each of u and v (the context's planes: 256-byte bases, pitch a
//                     multiple of 64 floats).  The target comes from hsinterp::target(), which tests the floats and then
//                     the integers: no address leaves the W x H cells of the plane.
//   k_interp_resolve  keys become ut, vt and state (a gather of the winner's vector by its index), and the cell (x, y)
//                     classifies the SOURCE (x, y) once more, so that the five counters of P come from one pass.
//   k_interp_blend    B, a gather like k_warp_batch that reads two pictures and two optional visibility planes.
// The batch axis (blockIdx.z) is the TIME: the n intermediate frames of ONE pair.  Time i has its own scratch planes
// (`plane` elements behind each other), its own destinations and its own 64-byte record.
// Statistics are integers counted in 32-bit registers (a lane sees at most 258 rows of 4 pixels of 3 channels, as in
// k_warp_batch), reduced by shuffles in the wavefront, through LDS in the workgroup, then one atomic per counter and
// workgroup (none for a zero sum).  No workgroup waits for another.
// The instantiations live in a translation unit of their own, hs_interp_kernels.hip, behind the launch_interp_*
// functions, as the median's do: a process that never interpolates does not load them, and the code object of every
// other kernel stays what it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_interp_rule.h"

namespace hsk {

constexpr int kInterpBatchMax = hsinterp::kBatchMax; // times per set of launches

// The layout of hsflow_interp_stats (include/hsflow.h) as the kernels write it.
struct InterpStatsWords {
    unsigned long long blended, prev_only, curr_only, clamped, sad;
    unsigned holes, unfilled, collisions, left, unknown, max_diff;
};
static_assert(sizeof(InterpStatsWords) == 64, "hsflow_interp_stats is 64 bytes");

struct InterpTimes {
    float t[kInterpBatchMax];
};

// Where the resolve writes time i: fp32 planes with rows `flow_stride` bytes apart, a byte plane `state_stride` apart.
struct InterpFlowOut {
    float *ut[kInterpBatchMax], *vt[kInterpBatchMax];
    uint8_t *state[kInterpBatchMax];
};

// What differs from time to time of the blend.
struct InterpBlendPics {
    const float *ut[kInterpBatchMax], *vt[kInterpBatchMax]; // the filled flow: 16-byte aligned, rows `flow_stride` bytes apart (a multiple of 16)
    const uint8_t *ref[kInterpBatchMax];                    // or NULL: no sum of differences
    uint8_t *dst[kInterpBatchMax];                          // or NULL
    uint8_t *cls[kInterpBatchMax];                          // or NULL
    float t[kInterpBatchMax];
    uint32_t wide_dst, wide_cls; // bit i: the base and the stride are multiples of 4
};

// The two pictures and the visibility planes, the same for every time.
struct InterpFrames {
    const uint8_t *prev, *curr, *vis_prev, *vis_curr; // vis_*: or NULL
    long long prev_stride, curr_stride, vis_prev_stride, vis_curr_stride;
};

__device__ __forceinline__ unsigned interp_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned interp_wave_max(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Grid: (ceil(W / 1024), rows, times); 256 lanes.  u, v: the pair's planes of pitch P.  keys: time i's plane of P x H
// words `plane` words behind time 0's, all-ones before.
template <int C>
__global__ __launch_bounds__(256) void k_interp_splat(const float *__restrict__ u, const float *__restrict__ v, int P, const InterpFrames fr, int W, int H,
                                                      unsigned long long *__restrict__ keys, long long plane, const InterpTimes times)
{
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= W) return;
    const float t = times.t[blockIdx.z];
    unsigned long long *cell = keys + (long long)blockIdx.z * plane;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const float4 a = *(const float4 *)(u + (long long)y * P + x0), b = *(const float4 *)(v + (long long)y * P + x0);
        const float aa[4] = {a.x, a.y, a.z, a.w}, bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (x0 + j >= W) continue;
            const hsinterp::Splat s = hsinterp::splat<C>(aa[j], bb[j], x0 + j, y, t, W, H, fr.prev, fr.prev_stride, fr.curr, fr.curr_stride);
            if (s.cls == hsinterp::kLanded) atomicMin(cell + (long long)s.qy * P + s.qx, (unsigned long long)s.key); // 0 <= qx < W <= P, 0 <= qy < H
        }
    }
}

// Grid: (ceil(W / 1024), rows, times); 256 lanes; every lane stays to the end when there are statistics.  stats: the
// first time's record, zero before.  unfilled_too: no fill follows, the holes are the unfilled cells.
template <bool STATS>
__global__ __launch_bounds__(256) void k_interp_resolve(const unsigned long long *__restrict__ keys, long long plane, const float *__restrict__ u,
                                                        const float *__restrict__ v, int P, int W, int H, const InterpTimes times, const InterpFlowOut out,
                                                        long long flow_stride, long long state_stride, InterpStatsWords *__restrict__ stats, int unfilled_too)
{
    const unsigned i = blockIdx.z;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    hsinterp::ProjAcc acc = {0u, 0u, 0u};
    if (x0 < W) {
        const float t = times.t[i];
        const unsigned long long *cell = keys + (long long)i * plane;
        uint8_t *ut = (uint8_t *)out.ut[i], *vt = (uint8_t *)out.vt[i], *state = out.state[i];
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int x = x0 + j;
                if (x >= W) continue;
                const unsigned long long key = cell[(long long)y * P + x];
                const bool have = key != hsinterp::kEmpty;
                unsigned abits = 0u, bbits = 0u;
                if (have) {
                    const unsigned src = (unsigned)key; // < W * H: a source index that splat() formed
                    const unsigned sy = src / (unsigned)W, sx = src - sy * (unsigned)W;
                    abits = __float_as_uint(u[(long long)sy * P + sx]);
                    bbits = __float_as_uint(v[(long long)sy * P + sx]);
                }
                if (ut) {
                    *(unsigned *)(ut + (long long)y * flow_stride + 4ll * x) = abits;
                    *(unsigned *)(vt + (long long)y * flow_stride + 4ll * x) = bbits;
                }
                if (state) state[(long long)y * state_stride + x] = have ? 1u : 0u;
                if (STATS) {
                    const hsinterp::Splat s = hsinterp::target(u[(long long)y * P + x], v[(long long)y * P + x], x, y, t, W, H);
                    acc.holes += !have;
                    acc.left += s.cls == hsinterp::kLeft;
                    acc.unknown += s.cls == hsinterp::kUnknown;
                }
            }
        }
    }
    if (!STATS) return;
    const unsigned part[3] = {interp_wave_sum(acc.holes), interp_wave_sum(acc.left), interp_wave_sum(acc.unknown)};
    __shared__ unsigned lds[4][3];
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (int k = 0; k < 3; k++) lds[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x == 0u) {
        const unsigned holes = lds[0][0] + lds[1][0] + lds[2][0] + lds[3][0], left = lds[0][1] + lds[1][1] + lds[2][1] + lds[3][1],
                       unknown = lds[0][2] + lds[1][2] + lds[2][2] + lds[3][2];
        InterpStatsWords *r = stats + i;
        if (holes) atomicAdd(&r->holes, holes);
        if (holes && unfilled_too) atomicAdd(&r->unfilled, holes);
        if (left) atomicAdd(&r->left, left);
        if (unknown) atomicAdd(&r->unknown, unknown);
        // collisions = landed - hit = holes - left - unknown over the plane; a workgroup's share may be negative, the sum
        // modulo 2^32 is the count
        const unsigned coll = holes - left - unknown;
        if (coll) atomicAdd(&r->collisions, coll);
    }
}

// Grid: (ceil(W / 1024), rows, times); 256 lanes.  With STATS every lane stays to the end.  stats: the first time's record.
template <int C, bool STATS>
__global__ __launch_bounds__(256) void k_interp_blend(const InterpBlendPics pics, long long flow_stride, const InterpFrames fr, long long ref_stride,
                                                      long long dst_stride, long long cls_stride, int W, int H, InterpStatsWords *__restrict__ stats)
{
    const unsigned i = blockIdx.z;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    hsinterp::Acc acc = {{0u, 0u, 0u, 0u}, 0u, 0u};
    if (x0 < W) {
        const float t = pics.t[i];
        const uint8_t *ut = (const uint8_t *)pics.ut[i], *vt = (const uint8_t *)pics.vt[i], *ref = pics.ref[i];
        uint8_t *dst = pics.dst[i], *cls = pics.cls[i];
        const bool full = x0 + 4 <= W, wide_dst = ((pics.wide_dst >> i) & 1u) && full, wide_cls = ((pics.wide_cls >> i) & 1u) && full;
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            const float4 a = *(const float4 *)(ut + (long long)y * flow_stride + 4ll * x0), b = *(const float4 *)(vt + (long long)y * flow_stride + 4ll * x0);
            const float aa[4] = {a.x, a.y, a.z, a.w}, bb[4] = {b.x, b.y, b.z, b.w};
            unsigned w[4], k[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                w[j] = 0u;
                k[j] = 0u;
                if (x0 + j < W) {
                    int kk = 0;
                    w[j] = hsinterp::pixel<C>(aa[j], bb[j], x0 + j, y, t, W, H, fr.prev, fr.prev_stride, fr.curr, fr.curr_stride, fr.vis_prev, fr.vis_prev_stride,
                                              fr.vis_curr, fr.vis_curr_stride, &kk);
                    k[j] = (unsigned)kk;
                    if (STATS) {
                        const unsigned r = ref ? hswarp::load_pixel<C>(ref + (long long)y * ref_stride + (long long)C * (x0 + j)) : 0u;
                        hsinterp::account<C>(acc, kk, w[j], r, ref != nullptr);
                    }
                }
            }
            if (cls) {
                uint8_t *d = cls + (long long)y * cls_stride + x0;
                if (wide_cls) {
                    *(uint32_t *)d = k[0] | (k[1] << 8) | (k[2] << 16) | (k[3] << 24);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (x0 + j < W) d[j] = (uint8_t)k[j];
                }
            }
            if (!dst) continue;
            uint8_t *d = dst + (long long)y * dst_stride + (long long)C * x0;
            if (wide_dst) {
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
    const unsigned part[6] = {interp_wave_sum(acc.cls[0]), interp_wave_sum(acc.cls[1]), interp_wave_sum(acc.cls[2]),
                              interp_wave_sum(acc.cls[3]), interp_wave_sum(acc.sad),    interp_wave_max(acc.max_diff)};
    __shared__ unsigned lds[4][6];
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (int k = 0; k < 6; k++) lds[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x < 6u) {
        const unsigned k = threadIdx.x;
        InterpStatsWords *r = stats + i;
        if (k < 5u) { // the four classes and sad: the record's first five words
            const unsigned long long sum = (unsigned long long)lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k];
            if (sum) atomicAdd((unsigned long long *)r + k, sum);
        } else { // (a maximum only ever grows: the atomic is left out where the word already holds as much)
            unsigned m = lds[0][k];
            for (int wv = 1; wv < 4; wv++) m = lds[wv][k] > m ? lds[wv][k] : m;
            if (m > __hip_atomic_load(&r->max_diff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&r->max_diff, m);
        }
    }
}

// The launches (hs_interp_kernels.hip): grids as above, 256 lanes; the status of the launch.
hipError_t launch_interp_splat(int channels, const dim3 &grid, hipStream_t stream, const float *u, const float *v, int P, const InterpFrames &fr, int W, int H,
                               unsigned long long *keys, long long plane, const InterpTimes &times);
hipError_t launch_interp_resolve(const dim3 &grid, hipStream_t stream, const unsigned long long *keys, long long plane, const float *u, const float *v, int P, int W,
                                 int H, const InterpTimes &times, const InterpFlowOut &out, long long flow_stride, long long state_stride, InterpStatsWords *stats,
                                 int unfilled_too);
hipError_t launch_interp_blend(int channels, const dim3 &grid, hipStream_t stream, const InterpBlendPics &pics, long long flow_stride, const InterpFrames &fr,
                               long long ref_stride, long long dst_stride, long long cls_stride, int W, int H, InterpStatsWords *stats);

} // namespace hsk
