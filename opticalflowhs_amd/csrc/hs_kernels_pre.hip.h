// hs_kernels_pre.hip.h -- pre-processing of the reference's CPU route, on the GPU:
//   cvCvtColor(img, gray, CV_BGR2GRAY)        OpticalFlowHS/OpticalFlowOpenCV.cpp:17,20
//   cvSmooth(img, img, CV_BLUR, 3, 3, 0, 0)   OpticalFlowHS/OpticalFlowOpenCV.cpp:27-28
// Byte work, HBM-bound: each lane handles 4 consecutive pixels (one 32-bit store); the 3x3
// neighbourhood of the blur comes from L1/L2.  Arithmetic = oracle/hs_preproc_oracle.c, bit exact.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_pre_rule.h"

namespace hsk {

// gray = (1868 B + 9617 G + 4899 R + 8192) >> 14 on interleaved BGR bytes (row stride in bytes)
__global__ __launch_bounds__(256) void k_bgr2gray(const uint8_t *__restrict__ bgr, long long bgr_stride,
                                                  uint8_t *__restrict__ gray, int W, int H, int P)
{
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= W || y >= H) return;
    const uint8_t *s = bgr + (long long)y * bgr_stride + 3 * x0;
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (x0 + k < W) {
            const uint32_t g = (1868u * s[3 * k] + 9617u * s[3 * k + 1] + 4899u * s[3 * k + 2] + 8192u) >> 14;
            out |= g << (8 * k);
        }
    }
    *(uint32_t *)(gray + (long long)y * P + x0) = out; // row pitch P is a multiple of 64: in bounds
}

// 3x3 box blur, replicate border, round(sum / 9): (2 s + 9) / 18 is exact because s / 9 is never
// half-way between two integers.  src and dst are distinct planes of pitch P.
__global__ __launch_bounds__(256) void k_box_blur3(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                   int W, int H, int P)
{
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= W || y >= H) return;
    const uint8_t *r0 = src + (long long)(y > 0 ? y - 1 : 0) * P;
    const uint8_t *r1 = src + (long long)y * P;
    const uint8_t *r2 = src + (long long)(y < H - 1 ? y + 1 : H - 1) * P;
    int col[6]; // column sums of columns x0-1 .. x0+4 (clamped)
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int xc = x0 + k - 1;
        xc = xc < 0 ? 0 : (xc > W - 1 ? W - 1 : xc);
        col[k] = r0[xc] + r1[xc] + r2[xc];
    }
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = col[k] + col[k + 1] + col[k + 2];
        out |= (uint32_t)((2 * s + 9) / 18) << (8 * k);
    }
    *(uint32_t *)(dst + (long long)y * P + x0) = out;
}

// Both frames of a pair from device memory into the context's planes in ONE launch (hsflow_set_frames_u8_device: a
// stream of resident pairs pays one copy launch per pair instead of two 2-D copies).  One lane = 16 bytes of one row
// of either frame (blockIdx.z: which frame); ALIGNED: both sources are 16-byte aligned with strides that are multiples
// of 16, so whole groups move as one 128-bit access; the ragged end of a row (W % 16) goes byte by byte.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_copy_pair_u8(const uint8_t *__restrict__ srcA, long long strideA,
                                                      const uint8_t *__restrict__ srcB, long long strideB,
                                                      uint8_t *__restrict__ dstA, uint8_t *__restrict__ dstB, int W, int H, int P)
{
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 16;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= W || y >= H) return;
    const uint8_t *s = (blockIdx.z ? srcB + (long long)y * strideB : srcA + (long long)y * strideA) + x0;
    uint8_t *d = (blockIdx.z ? dstB : dstA) + (long long)y * P + x0;
    if (ALIGNED && x0 + 16 <= W) {
        *(uint4 *)d = *(const uint4 *)s;
    } else {
        const int n = W - x0 < 16 ? W - x0 : 16;
        for (int k = 0; k < n; k++) d[k] = s[k];
    }
}

// Both frames of a pair from device memory through the whole pre-processing into the context's planes in ONE launch
// (hsflow_set_frames_device_ex; the two kernels above cost a pair four launches and a round trip of the gray plane
// through HBM).  COLOUR: the source is interleaved BGR, else gray; BLUR: 3x3 box blur behind it.  The arithmetic is
// hs_pre_rule.h's, so the bytes are those of k_bgr2gray / k_box_blur3.
// One lane = 4 consecutive columns (one 32-bit store per row) of a strip of HSFLOW_PRE_STRIP_ROWS rows; a wavefront = 256
// columns of one strip; blockIdx.z: which frame, as in k_copy_pair_u8 (a launch with gridDim.z = 1 handles source A alone).
// The lane walks down its strip: per source row it loads the gray of its four columns (or converts them) and of the two
// columns beside them, x0 - 1 and x0 + 4 clamped to the frame -- two byte loads of its own, which measured faster than
// taking them from the neighbour lanes by DPP wave shifts with a reload in lanes 0 and 63 -- forms the
// four horizontal 3-sums and keeps those of the last three rows; an output row is the sum of the three through
// round_div9.  A source row is read once per strip, plus one halo row above and below the strip; no gray plane exists
// outside registers.
// word_loads bit z: source z's base and stride are multiples of 4, so a lane's four gray pixels are one dword and its four
// BGR pixels three; otherwise, and for the group that straddles column W - 1, byte by byte.
template <bool COLOUR, bool BLUR>
__global__ __launch_bounds__(256) void k_pre_pair(const uint8_t *__restrict__ srcA, long long strideA, const uint8_t *__restrict__ srcB,
                                                  long long strideB, uint8_t *__restrict__ dstA, uint8_t *__restrict__ dstB, int W, int H,
                                                  int P, unsigned word_loads)
{
    constexpr int S = HSFLOW_PRE_STRIP_ROWS;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4; // blockDim.x = 64: threadIdx.y is the wavefront
    const int y0 = (blockIdx.y * blockDim.y + threadIdx.y) * S;
    if (x0 >= W || y0 >= H) return;
    const uint8_t *src = blockIdx.z ? srcB : srcA;
    const long long stride = blockIdx.z ? strideB : strideA;
    uint8_t *dst = blockIdx.z ? dstB : dstA;
    const bool word = ((word_loads >> blockIdx.z) & 1u) != 0 && x0 + 4 <= W;
    int xc[4];
#pragma unroll
    for (int k = 0; k < 4; k++) xc[k] = hspre::clamp_index(x0 + k, W);
    const int xl = hspre::clamp_index(x0 - 1, W), xr = hspre::clamp_index(x0 + 4, W);

    auto gray4 = [&](const uint8_t *row) -> uint32_t { // gray of columns x0 .. x0 + 3 (clamped), one byte each
        if (word) {
            if (!COLOUR) return *(const uint32_t *)(row + x0);
            const uint32_t *p = (const uint32_t *)(row + 3 * x0);
            const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
            return hspre::gray_bgr(w0 & 0xFFu, (w0 >> 8) & 0xFFu, (w0 >> 16) & 0xFFu) |
                   hspre::gray_bgr(w0 >> 24, w1 & 0xFFu, (w1 >> 8) & 0xFFu) << 8 |
                   hspre::gray_bgr((w1 >> 16) & 0xFFu, w1 >> 24, w2 & 0xFFu) << 16 |
                   hspre::gray_bgr((w2 >> 8) & 0xFFu, (w2 >> 16) & 0xFFu, w2 >> 24) << 24;
        }
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) w |= hspre::gray_at<COLOUR>(row, xc[k]) << (8 * k);
        return w;
    };

    if (!BLUR) {
#pragma unroll
        for (int r = 0; r < S; r++) {
            const int y = y0 + r;
            if (y < H) {
                const uint32_t w = gray4(src + (long long)y * stride);
                *(uint32_t *)(dst + (long long)y * P + x0) = w; // row pitch P is a multiple of 64: in bounds
            }
        }
        return;
    }

    uint32_t h[3][4]; // horizontal 3-sums of the last three source rows (slot j % 3; the loop is unrolled: registers)
#pragma unroll
    for (int j = 0; j < S + 2; j++) { // source rows y0 - 1 .. y0 + S
        const int ys = y0 + j - 1;
        if (j >= 2 && ys - 1 >= H) break; // nothing below the frame is stored
        const uint8_t *row = src + (long long)hspre::clamp_index(ys, H) * stride;
        const uint32_t w = gray4(row);
        uint32_t g[6]; // columns x0 - 1 .. x0 + 4
#pragma unroll
        for (int k = 0; k < 4; k++) g[k + 1] = (w >> (8 * k)) & 0xFFu;
        g[0] = hspre::gray_at<COLOUR>(row, xl);
        g[5] = hspre::gray_at<COLOUR>(row, xr);
#pragma unroll
        for (int k = 0; k < 4; k++) h[j % 3][k] = g[k] + g[k + 1] + g[k + 2];
        if (j >= 2) { // output row y0 + j - 2
            const int y = ys - 1;
            uint32_t out = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) out |= hspre::round_div9(h[0][k] + h[1][k] + h[2][k]) << (8 * k);
            *(uint32_t *)(dst + (long long)y * P + x0) = out;
        }
    }
}

// A SEQUENCE of frames from device memory into consecutive pairs of the context in ONE launch per chunk of at most
// kPreSeqMax frames (hsflow_set_sequence_device_ex; the reference's camera loop, OpticalFlowOpenCV.cpp:76-93,118, in a
// context of N pairs).  blockIdx.z: the frame, as in the batched JPEG kernels; x, y and the lane shape are k_pre_pair's.
// Frame j is read ONCE and leaves up to two results in up to two planes: p_j = pre(format, f_j) in curr of pair j - 1
// and / or prev of pair j, and, where the loop's double blur is asked for, B(p_j) -- the blur of the rounded plane p_j
// with p_j's own border repeated -- in prev of pair j.  The walk is hs_pre_rule.h's seq_strip, the host's too; no gray
// or once-blurred plane exists outside registers.  The double blur keeps three rows of six sums and three rows of four
// (30 words) and reads two halo rows and two halo columns on each side of a lane's strip.
constexpr int kPreSeqMax = 32; // frames per launch: four pointers each, 1 KiB of the kernel's argument block

struct PreSeqFrames { // what differs from frame to frame, handed to the kernel by value
    const uint8_t *src[kPreSeqMax];
    uint8_t *p0[kPreSeqMax], *p1[kPreSeqMax], *b[kPreSeqMax]; // hspre::SeqDst; null: not wanted
    uint32_t words;                                           // bit i: frame i's base and the stride are multiples of 4
};

template <bool COLOUR, bool BLUR>
__global__ __launch_bounds__(256) void k_pre_sequence(PreSeqFrames f, long long stride, int W, int H, int P)
{
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4; // blockDim.x = 64: threadIdx.y is the wavefront
    const int y0 = (blockIdx.y * blockDim.y + threadIdx.y) * HSFLOW_PRE_STRIP_ROWS;
    if (x0 >= W || y0 >= H) return;
    const unsigned z = blockIdx.z;
    const bool word = ((f.words >> z) & 1u) != 0 && x0 + 4 <= W;
    hspre::seq_strip_any<COLOUR, BLUR, false>(f.src[z], (size_t)stride, W, H, x0, y0, word, f.p0[z], f.p1[z], f.b[z], (size_t)P);
}

} // namespace hsk
