// hs_pre_rule.h -- the row rule of the reference CPU route's pre-processing, ONE definition for the device kernel
// (hs_kernels_pre.hip.h, k_pre_pair) and its host twin (hsflow_preprocess_frame_host), the way hs_verify_rule.h serves
// both sides of the comparison:
//   cvCvtColor(img, gray, CV_BGR2GRAY)        OpticalFlowHS/OpticalFlowOpenCV.cpp:17,20,78,85
//   cvSmooth(img, img, CV_BLUR, 3, 3, 0, 0)   OpticalFlowHS/OpticalFlowOpenCV.cpp:27-28,92-93
// Three pieces, all integer arithmetic, so any order of summation gives the same bytes:
//   clamp_index   replicate border: a column or row index outside the frame is the nearest one inside
//   gray_bgr      (1868 B + 9617 G + 4899 R + 8192) >> 14: 0.114, 0.587, 0.299 in 14 fractional bits, rounded
//   round_div9    round(s / 9) as (2 s + 9) / 18 -- exact because s / 9 is never half-way between two integers
// A blurred pixel is round_div9 of the sum of three horizontal 3-sums (rows y-1, y, y+1 clamped; columns x-1, x, x+1
// clamped), which is how both sides walk a frame: one horizontal sum per source row, three of them per output row.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#ifndef HSFLOW_PRE_STRIP_ROWS
#define HSFLOW_PRE_STRIP_ROWS 8 /* include/hsflow.h */
#endif

#if defined(__HIPCC__)
#define HSP_FN __host__ __device__ inline
#else
#define HSP_FN inline
#endif

namespace hspre {

// HSFLOW_FRAMES_* of include/hsflow.h, as the two switches the rule has
HSP_FN bool format_known(int format) { return format >= 0 && format <= 3; }
HSP_FN bool format_colour(int format) { return format >= 2; }
HSP_FN bool format_blur(int format) { return (format & 1) != 0; }

HSP_FN int clamp_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

HSP_FN uint32_t gray_bgr(uint32_t b, uint32_t g, uint32_t r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

HSP_FN uint32_t round_div9(uint32_t s) { return (2u * s + 9u) / 18u; }

// gray of column x (inside the frame) of one source row
template <bool COLOUR>
HSP_FN uint32_t gray_at(const uint8_t *row, int x)
{
    if (COLOUR) return gray_bgr(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
    return row[x];
}

// horizontal 3-sum of column x of one source row, columns clamped to the frame
template <bool COLOUR>
HSP_FN uint32_t hsum_at(const uint8_t *row, int x, int W)
{
    return gray_at<COLOUR>(row, clamp_index(x - 1, W)) + gray_at<COLOUR>(row, x) + gray_at<COLOUR>(row, clamp_index(x + 1, W));
}

// One frame in host memory, walked as the kernel walks a strip: every source row's horizontal sums are formed once and
// kept for the three output rows that need them.  sums: room for three rows of them (3 * W entries; unused without blur).
template <bool COLOUR, bool BLUR>
inline void preprocess_rows(const uint8_t *src, size_t ss, int W, int H, uint8_t *dst, size_t ds, uint16_t *sums)
{
    if (!BLUR) {
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) dst[(size_t)y * ds + x] = (uint8_t)gray_at<COLOUR>(src + (size_t)y * ss, x);
        return;
    }
    auto hrow = [&](int y) { // row y's sums live in slot y % 3 until row y + 3 takes it
        uint16_t *h = sums + (size_t)(y % 3) * W;
        for (int x = 0; x < W; x++) h[x] = (uint16_t)hsum_at<COLOUR>(src + (size_t)y * ss, x, W);
    };
    hrow(0);
    for (int y = 0; y < H; y++) {
        if (y + 1 < H) hrow(y + 1);
        const uint16_t *h0 = sums + (size_t)(clamp_index(y - 1, H) % 3) * W, *h1 = sums + (size_t)(y % 3) * W,
                       *h2 = sums + (size_t)(clamp_index(y + 1, H) % 3) * W;
        for (int x = 0; x < W; x++) dst[(size_t)y * ds + x] = (uint8_t)round_div9((uint32_t)h0[x] + h1[x] + h2[x]);
    }
}

// The rule over one frame in host memory: dst = pre(format, src).  Returns 0, 1 (null pointer, unknown format), 2
// (non-positive size, stride below the row's bytes) or 4 (no memory for three rows of sums): HSFLOW_OK / HSFLOW_E_ARG /
// HSFLOW_E_SIZE / HSFLOW_E_OOM.  Reads exactly the width x height pixels of src and writes exactly width x height bytes
// of dst; src and dst must not overlap.
inline int preprocess_host(int format, const uint8_t *src, size_t src_stride, int width, int height, uint8_t *dst, size_t dst_stride)
{
    if (!src || !dst || !format_known(format)) return 1;
    if (width <= 0 || height <= 0) return 2;
    if (src_stride < (size_t)width * (format_colour(format) ? 3u : 1u) || dst_stride < (size_t)width) return 2;
    uint16_t *sums = format_blur(format) ? (uint16_t *)malloc((size_t)width * 3 * sizeof(uint16_t)) : nullptr;
    if (format_blur(format) && !sums) return 4;
    switch (format) {
    case 0: preprocess_rows<false, false>(src, src_stride, width, height, dst, dst_stride, sums); break;
    case 1: preprocess_rows<false, true>(src, src_stride, width, height, dst, dst_stride, sums); break;
    case 2: preprocess_rows<true, false>(src, src_stride, width, height, dst, dst_stride, sums); break;
    default: preprocess_rows<true, true>(src, src_stride, width, height, dst, dst_stride, sums); break;
    }
    free(sums);
    return 0;
}

} // namespace hspre
