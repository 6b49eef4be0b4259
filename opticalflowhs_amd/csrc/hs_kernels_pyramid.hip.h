// hs_kernels_pyramid.hip.h -- the three kernels a coarse-to-fine solve puts around the solver (hs_pyramid_rule.h,
// hs_pyramid.hip.h); a code object of their own (hs_pyramid_kernels.hip).  Every plane they touch is a context's: its base a
// 256-byte multiple, its pitch P a multiple of 64 elements >= W, pair i's plane P * H elements behind pair i-1's.  So a
// lane's 4 consecutive columns from a multiple of 4 are one aligned 16-byte (flow) or 4-byte (frame) access inside the
// row's pitch; the columns beyond W of a context's flow plane keep what they held, those of a base plane and of a frame
// (up to the next multiple of 4) are written as zeros, which is what a frame holds there from the context's creation on.
//   k_pyr_down   both frames of every pair, one level down: blockIdx.z = 2 * pair + frame.  A workgroup makes 64 x 16
//                output bytes: it stages the 131 x 35 source bytes they read (clamped at the plane's edges) in LDS, sums
//                the five taps of every staged row at its 64 output columns (16 bits each), and every lane then sums five of
//                those row sums for each of its 4 output bytes and stores them as one word.
//   k_pyr_step   the start of a step: the base flow u0, v0 -- MODE kProlong: prolonged from the coarser level's total, 3
//                coarse columns of 1 or 2 coarse rows per lane; kSame: the level's own total; kSameAdd: the level's base of
//                the step before plus that step's increment, the addition nowhere else -- stored to the pyramid's base
//                planes, and the second frame warped by it (hswarp::locate / pixel<1>, t = 1, REPLICATE; a pixel whose base
//                flow is not known() keeps the frame's own byte) stored to the plane the solver reads, one word per lane.
//   k_pyr_total  the flow after the step: fl(u0 + du), fl(v0 + dv) over the increment, in place.
// Rows are walked with a grid stride over all pairs' rows; nothing here waits for another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_pyramid_rule.h"
#include "hs_warp_rule.h"

namespace hsk {

constexpr int kPyrTileX = 64, kPyrTileY = 16;                              // output bytes of a k_pyr_down workgroup
constexpr int kPyrInX = 2 * kPyrTileX + 3, kPyrInY = 2 * kPyrTileY + 3;    // source bytes it reads: 131 x 35
constexpr int kPyrInPitch = 132;
constexpr int kPyrProlong = 0, kPyrSame = 1, kPyrSameAdd = 2;

// prev / curr: the finer level's frames (pitch Ps, planes `splane` bytes apart), W x H; prev_out / curr_out: the coarser
// level's (pitch Pd, planes `dplane` apart), ceil(W/2) x ceil(H/2).  Grid: (ceil(Wd / 64), ceil(Hd / 16), 2 * pairs); 256 lanes.
// (Templates, like every kernel of a code object of its own: instantiated where they are launched, hs_pyramid_kernels.hip.)
template <int TX, int TY>
__global__ __launch_bounds__(256) void k_pyr_down(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ curr, long long splane, int Ps, int W, int H,
                                                  uint8_t *__restrict__ prev_out, uint8_t *__restrict__ curr_out, long long dplane, int Pd)
{
    static_assert(TX == kPyrTileX && TY == kPyrTileY && TX * TY == 4 * 256, "a lane makes 4 of the tile's bytes");
    __shared__ uint8_t in[kPyrInY][kPyrInPitch];
    __shared__ uint16_t sums[kPyrInY][kPyrTileX];
    const int Wd = hspyr::half_up(W), Hd = hspyr::half_up(H);
    const unsigned pair = blockIdx.z >> 1;
    const uint8_t *src = ((blockIdx.z & 1u) ? curr : prev) + (long long)pair * splane;
    uint8_t *dst = ((blockIdx.z & 1u) ? curr_out : prev_out) + (long long)pair * dplane;
    const int ox = blockIdx.x * kPyrTileX, oy = blockIdx.y * kPyrTileY;
    const int sx = 2 * ox - 2, sy = 2 * oy - 2;
    for (int i = threadIdx.x; i < kPyrInY * kPyrInX; i += 256) {
        const int r = i / kPyrInX, q = i - r * kPyrInX;
        in[r][q] = src[(long long)hspyr::clampi(sy + r, H - 1) * Ps + hspyr::clampi(sx + q, W - 1)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kPyrInY * kPyrTileX; i += 256) {
        const int r = i / kPyrTileX, x = i - r * kPyrTileX;
        const uint8_t *p = &in[r][2 * x];
        sums[r][x] = (uint16_t)hspyr::taps5(p[0], p[1], p[2], p[3], p[4]);
    }
    __syncthreads();
    const int lx = (threadIdx.x & 15) * 4, ly = threadIdx.x >> 4;
    const int x0 = ox + lx, y = oy + ly;
    if (x0 >= Wd || y >= Hd) return;
    uint32_t word = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint16_t *p = &sums[2 * ly][lx + j];
        const uint32_t b = hspyr::down_finish(hspyr::taps5(p[0], p[kPyrTileX], p[2 * kPyrTileX], p[3 * kPyrTileX], p[4 * kPyrTileX]));
        if (x0 + j < Wd) word |= b << (8 * j);
    }
    *(uint32_t *)(dst + (long long)y * Pd + x0) = word;
}

// bu, bv: kProlong -- the coarser level's total (pitch Pc, planes cplane elements apart, Wc x Hc); kSame -- this level's
// total; kSameAdd -- this level's base planes, and iu, iv the increment of the step before (both pitch P, planes `plane`).
// u0, v0: this level's base planes (kSameAdd: they are bu, bv -- a lane reads its own 4 elements before it writes them).
// curr: the level's second frame; warped: where the solver reads it.  rows = pairs * H.  Grid: (ceil(W / 1024), rows up to
// 65535); 256 lanes.
template <int MODE>
__global__ __launch_bounds__(256) void k_pyr_step(const float *bu, const float *bv, const float *__restrict__ iu, const float *__restrict__ iv, long long cplane,
                                                  int Pc, int Wc, int Hc, float *u0, float *v0, const uint8_t *__restrict__ curr,
                                                  uint8_t *__restrict__ warped, long long plane, int P, int W, int H, long long rows)
{
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= W) return;
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        const long long pair = row / H;
        const int y = (int)(row - pair * H);
        const long long o = pair * plane + (long long)y * P + x0;
        float a[4], b[4];
        if (MODE == kPyrProlong) {
            const int k = x0 >> 1, r = y >> 1, r1 = r + 1 < Hc - 1 ? r + 1 : Hc - 1;
            const long long c0 = pair * cplane + (long long)r * Pc, c1 = pair * cplane + (long long)r1 * Pc;
            int kk[3];
#pragma unroll
            for (int j = 0; j < 3; j++) kk[j] = k + j < Wc - 1 ? k + j : Wc - 1;
            float ua[3], va[3], ub[3], vb[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                ua[j] = bu[c0 + kk[j]]; va[j] = bv[c0 + kk[j]];
                ub[j] = ua[j]; vb[j] = va[j];
            }
            if (y & 1) {
#pragma unroll
                for (int j = 0; j < 3; j++) { ub[j] = bu[c1 + kk[j]]; vb[j] = bv[c1 + kk[j]]; }
            }
            // columns x0 .. x0+3 lie between coarse columns (k, k+1), (k, k+1), (k+1, k+2), (k+1, k+2)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int q = j >> 1;
                a[j] = hspyr::prolong_value(ua[q], ua[q + 1], ub[q], ub[q + 1], x0 + j, y);
                b[j] = hspyr::prolong_value(va[q], va[q + 1], vb[q], vb[q + 1], x0 + j, y);
            }
        } else {
            const float4 p = *(const float4 *)(bu + o), q = *(const float4 *)(bv + o);
            a[0] = p.x; a[1] = p.y; a[2] = p.z; a[3] = p.w;
            b[0] = q.x; b[1] = q.y; b[2] = q.z; b[3] = q.w;
            if (MODE == kPyrSameAdd) {
                const float4 d = *(const float4 *)(iu + o), e = *(const float4 *)(iv + o);
                a[0] = a[0] + d.x; a[1] = a[1] + d.y; a[2] = a[2] + d.z; a[3] = a[3] + d.w;
                b[0] = b[0] + e.x; b[1] = b[1] + e.y; b[2] = b[2] + e.z; b[3] = b[3] + e.w;
            }
        }
        const uint8_t *src = curr + pair * plane;
        uint32_t word = 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (x0 + j < W) {
                const hswarp::Tap t = hswarp::locate(a[j], b[j], x0 + j, y, 1.0f, W, H, hswarp::kBorderReplicate);
                const uint32_t own = src[(long long)y * P + x0 + j];
                word |= hswarp::pixel<1>(src, (long long)P, t, own) << (8 * j);
            } else {
                a[j] = 0.0f; b[j] = 0.0f;
            }
        }
        *(float4 *)(u0 + o) = make_float4(a[0], a[1], a[2], a[3]);
        *(float4 *)(v0 + o) = make_float4(b[0], b[1], b[2], b[3]);
        *(uint32_t *)(warped + pair * plane + (long long)y * P + x0) = word;
    }
}

// u, v (the increment, then the total): pitch P, planes `plane` apart; u0, v0 alike.  Grid as k_pyr_step.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_pyr_total(const float *__restrict__ u0, const float *__restrict__ v0, float *u, float *v, long long plane, int P, int W,
                                                   int H, long long rows)
{
    const int x0 = (blockIdx.x * BLOCK + threadIdx.x) * 4;
    if (x0 >= W) return;
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        const long long pair = row / H;
        const long long o = pair * plane + (row - pair * H) * P + x0;
        const float4 a = *(const float4 *)(u0 + o), b = *(const float4 *)(v0 + o);
        float4 d = *(const float4 *)(u + o), e = *(const float4 *)(v + o);
        d.x = a.x + d.x; e.x = b.x + e.x;
        if (x0 + 1 < W) { d.y = a.y + d.y; e.y = b.y + e.y; }
        if (x0 + 2 < W) { d.z = a.z + d.z; e.z = b.z + e.z; }
        if (x0 + 3 < W) { d.w = a.w + d.w; e.w = b.w + e.w; }
        *(float4 *)(u + o) = d;
        *(float4 *)(v + o) = e;
    }
}

// What hs_pyramid.hip.h launches (hs_pyramid_kernels.hip); each returns hipGetLastError().
hipError_t launch_pyr_down(hipStream_t stream, int pairs, const uint8_t *prev, const uint8_t *curr, long long splane, int Ps, int W, int H, uint8_t *prev_out,
                           uint8_t *curr_out, long long dplane, int Pd);
hipError_t launch_pyr_step(hipStream_t stream, int mode, int pairs, const float *bu, const float *bv, const float *iu, const float *iv, long long cplane, int Pc,
                           int Wc, int Hc, float *u0, float *v0, const uint8_t *curr, uint8_t *warped, long long plane, int P, int W, int H);
hipError_t launch_pyr_total(hipStream_t stream, int pairs, const float *u0, const float *v0, float *u, float *v, long long plane, int P, int W, int H);

} // namespace hsk
