// hs_pre_rule.h -- the row rule of the reference CPU route's pre-processing, ONE definition for the device kernel
// (hs_kernels_pre.hip.h, k_pre_pair, k_pre_sequence) and its host twins (hsflow_preprocess_frame_host, _sequence_host), the way hs_verify_rule.h serves
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

// ---- a SEQUENCE of frames into consecutive pairs (hsflow_set_sequence_device_ex; the camera loop, OpticalFlowOpenCV.cpp:
// 76-93,118) ---------------------------------------------------------------------------------------------------------
// Frames f_0 .. f_{n-1}, p_j = pre(format, f_j), B(x) = HSFLOW_FRAMES_GRAY8_BLUR of the BYTES of x.  Pair k of the call:
//   curr_k = p_{k+1};   prev_k = seq_reblurs(flags, k) ? B(p_k) : p_k
// B(p) is the blur of the rounded, stored plane p with p's OWN edge pixels repeated: row 0 of B(p) needs p rows 0, 0, 1,
// and p row 0 needs source rows 0, 0, 1.  It is not a 5x5 filter over f, and not the blur evaluated at a virtual row -1
// of clamped source rows -- so seq_strip below clamps PLANE coordinates first and only then forms p there.
// One definition walks a lane's share (4 columns x a strip of HSFLOW_PRE_STRIP_ROWS rows) of one frame: the kernel
// (hs_kernels_pre.hip.h, k_pre_sequence) runs it per lane, the host (preprocess_sequence_host) for every share in turn.

HSP_FN bool seq_flags_known(int flags) { return flags == 0 || flags == 1 || flags == 3; } // HSFLOW_SEQ_REBLUR[_FIRST]
HSP_FN bool seq_reblurs(int flags, int k) { return (flags & 1) != 0 && (k > 0 || (flags & 2) != 0); }

// gray of columns x0 .. x0 + 3 (clamped to the frame), one byte each.  word: the row's base and x0's bytes are 4-byte
// aligned and all four columns lie inside the frame (device only; the host reads byte by byte).
template <bool COLOUR>
HSP_FN uint32_t seq_gray4(const uint8_t *row, int x0, int W, bool word)
{
    if (word) {
        if (!COLOUR) return *(const uint32_t *)(row + x0);
        const uint32_t *p = (const uint32_t *)(row + 3 * x0);
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
        return gray_bgr(w0 & 0xFFu, (w0 >> 8) & 0xFFu, (w0 >> 16) & 0xFFu) | gray_bgr(w0 >> 24, w1 & 0xFFu, (w1 >> 8) & 0xFFu) << 8 |
               gray_bgr((w1 >> 16) & 0xFFu, w1 >> 24, w2 & 0xFFu) << 16 | gray_bgr((w2 >> 8) & 0xFFu, (w2 >> 16) & 0xFFu, w2 >> 24) << 24;
    }
    uint32_t w = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) w |= gray_at<COLOUR>(row, clamp_index(x0 + k, W)) << (8 * k);
    return w;
}

// Four result bytes of columns x0 .. x0 + 3 of one plane row.  EXACT: only the columns inside the frame, byte by byte (the
// host); otherwise one 32-bit store (the device's planes have a pitch that is a multiple of 64: in bounds).
template <bool EXACT>
HSP_FN void seq_store4(uint8_t *row, int x0, int W, uint32_t w)
{
    if (!row) return;
    if (!EXACT) {
        *(uint32_t *)(row + x0) = w;
        return;
    }
    for (int k = 0; k < 4 && x0 + k < W; k++) row[x0 + k] = (uint8_t)(w >> (8 * k));
}

HSP_FN uint8_t *seq_row(uint8_t *plane, int y, size_t pitch) { return plane ? plane + (size_t)y * pitch : nullptr; }

// Columns x0 .. x0 + 3, rows y0 .. y0 + HSFLOW_PRE_STRIP_ROWS - 1 of one frame: p = pre(src) into p0 and p1 (either may
// be null), and with REBLUR also B(p) into b.  Every source row is loaded once per strip (plus the halo rows: one above
// and below for a blur, two for the double blur); nothing but the results is stored.
template <bool COLOUR, bool BLUR, bool REBLUR, bool EXACT>
HSP_FN void seq_strip(const uint8_t *src, size_t ss, int W, int H, int x0, int y0, bool word, uint8_t *p0, uint8_t *p1, uint8_t *b, size_t ds)
{
    constexpr int S = HSFLOW_PRE_STRIP_ROWS;
    if (!REBLUR && !BLUR) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int r = 0; r < S; r++) {
            const int y = y0 + r;
            if (y < H) {
                const uint32_t w = seq_gray4<COLOUR>(src + (size_t)y * ss, x0, W, word);
                seq_store4<EXACT>(seq_row(p0, y, ds), x0, W, w);
                seq_store4<EXACT>(seq_row(p1, y, ds), x0, W, w);
            }
        }
        return;
    }
    const int xl = clamp_index(x0 - 1, W), xr = clamp_index(x0 + 4, W);
    if (!REBLUR) { // k_pre_pair's walk, two destinations
        uint32_t h[3][4]; // horizontal 3-sums of the last three source rows (slot j % 3)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < S + 2; j++) { // source rows y0 - 1 .. y0 + S
            const int ys = y0 + j - 1;
            if (j >= 2 && ys - 1 >= H) break; // nothing below the frame is stored
            const uint8_t *row = src + (size_t)clamp_index(ys, H) * ss;
            const uint32_t w = seq_gray4<COLOUR>(row, x0, W, word);
            uint32_t g[6]; // columns x0 - 1 .. x0 + 4
            for (int k = 0; k < 4; k++) g[k + 1] = (w >> (8 * k)) & 0xFFu;
            g[0] = gray_at<COLOUR>(row, xl);
            g[5] = gray_at<COLOUR>(row, xr);
            for (int k = 0; k < 4; k++) h[j % 3][k] = g[k] + g[k + 1] + g[k + 2];
            if (j >= 2) { // output row y0 + j - 2
                uint32_t out = 0;
                for (int k = 0; k < 4; k++) out |= round_div9(h[0][k] + h[1][k] + h[2][k]) << (8 * k);
                seq_store4<EXACT>(seq_row(p0, ys - 1, ds), x0, W, out);
                seq_store4<EXACT>(seq_row(p1, ys - 1, ds), x0, W, out);
            }
        }
        return;
    }
    // p on plane columns x0 - 1 .. x0 + 4 and plane rows y0 - 1 .. y0 + S, both CLAMPED TO THE PLANE: a column or row of p
    // outside the frame is p's nearest one inside, whatever the source holds around it.  Row i of that window
    // (yp = y0 - 1 + i) comes from source rows yp - 1 .. yp + 1 when BLUR (three rows of six horizontal sums, from gray
    // columns x0 - 2 .. x0 + 5), else it is the gray row itself; its four horizontal 3-sums go into hp[i % 3], and an
    // output row of B(p) is round_div9 of the three slots.
    constexpr int LEAD = BLUR ? 2 : 0; // source rows walked before the first row of p is complete
    const int xll = clamp_index(x0 - 2, W), xrr = clamp_index(x0 + 5, W);
    uint32_t h[3][6];
    uint32_t hp[3][4];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int t = 0; t < S + 2 + LEAD; t++) {
        const int i = t - LEAD, yp = y0 - 1 + i; // (i < 0: the first two source rows of a double blur)
        if (i >= 2 && yp - 1 >= H) break;        // nothing below the frame is stored
        const uint8_t *row = src + (size_t)clamp_index(BLUR ? yp + 1 : yp, H) * ss;
        const uint32_t w = seq_gray4<COLOUR>(row, x0, W, word);
        uint32_t p[6]; // p of row yp on columns x0 - 1 .. x0 + 4
        if (BLUR) {
            uint32_t g[8]; // gray of columns x0 - 2 .. x0 + 5, clamped
            for (int k = 0; k < 4; k++) g[k + 2] = (w >> (8 * k)) & 0xFFu;
            g[0] = gray_at<COLOUR>(row, xll);
            g[1] = gray_at<COLOUR>(row, xl);
            g[6] = gray_at<COLOUR>(row, xr);
            g[7] = gray_at<COLOUR>(row, xrr);
            for (int k = 0; k < 6; k++) h[t % 3][k] = g[k] + g[k + 1] + g[k + 2];
            if (i < 0) continue;
            for (int k = 0; k < 6; k++) p[k] = round_div9(h[0][k] + h[1][k] + h[2][k]);
            // what was formed on a column outside the frame is not p there: p's own edge column is
            if (x0 == 0) p[0] = p[1];
            for (int k = 1; k < 6; k++)
                if (x0 - 1 + k > W - 1) p[k] = p[k - 1];
        } else {
            for (int k = 0; k < 4; k++) p[k + 1] = (w >> (8 * k)) & 0xFFu;
            p[0] = gray_at<COLOUR>(row, xl);
            p[5] = gray_at<COLOUR>(row, xr);
        }
        if (i >= 1 && i <= S && yp < H) {
            const uint32_t out = p[1] | p[2] << 8 | p[3] << 16 | p[4] << 24;
            seq_store4<EXACT>(seq_row(p0, yp, ds), x0, W, out);
            seq_store4<EXACT>(seq_row(p1, yp, ds), x0, W, out);
        }
        for (int k = 0; k < 4; k++) hp[i % 3][k] = p[k] + p[k + 1] + p[k + 2];
        // the same for rows: below the frame p's last row again, above it (i == 0 in the top strip) p's row 0, which
        // is complete only now
        if (yp > H - 1)
            for (int k = 0; k < 4; k++) hp[i % 3][k] = hp[(i + 2) % 3][k];
        if (i == 1 && y0 == 0)
            for (int k = 0; k < 4; k++) hp[0][k] = hp[1][k];
        if (i >= 2) { // output row y0 + i - 2 (inside the frame: see the break above)
            uint32_t out = 0;
            for (int k = 0; k < 4; k++) out |= round_div9(hp[0][k] + hp[1][k] + hp[2][k]) << (8 * k);
            seq_store4<EXACT>(seq_row(b, yp - 1, ds), x0, W, out);
        }
    }
}

// The same with the double blur decided by whether there is a plane for it.
template <bool COLOUR, bool BLUR, bool EXACT>
HSP_FN void seq_strip_any(const uint8_t *src, size_t ss, int W, int H, int x0, int y0, bool word, uint8_t *p0, uint8_t *p1, uint8_t *b, size_t ds)
{
    if (b) seq_strip<COLOUR, BLUR, true, EXACT>(src, ss, W, H, x0, y0, word, p0, p1, b, ds);
    else seq_strip<COLOUR, BLUR, false, EXACT>(src, ss, W, H, x0, y0, word, p0, p1, nullptr, ds);
}

// Where frame j of n goes: p_j into curr of pair j - 1 and, unless that pair is reblurred, prev of pair j; B(p_j) into
// prev of a reblurred pair j.  prev / curr: the planes of the call's pairs 0 .. n - 2.
struct SeqDst {
    uint8_t *p0, *p1, *b;
};
HSP_FN SeqDst seq_dst(int flags, int j, int n, uint8_t *prev_j, uint8_t *curr_jm1)
{
    SeqDst d;
    const bool has_pair = j <= n - 2, reblur = has_pair && seq_reblurs(flags, j);
    d.p0 = j >= 1 ? curr_jm1 : nullptr;
    d.p1 = has_pair && !reblur ? prev_j : nullptr;
    d.b = reblur ? prev_j : nullptr;
    return d;
}

// The sequence rule over frames in host memory.  frames: n; prev, curr: n - 1 planes each of width x height bytes, rows
// dst_stride apart.  Returns 0, 1 (null pointer, unknown format or flags, n < 2) or 2 (non-positive size, a stride below
// the row's bytes).  Reads exactly the width x height pixels of every frame, writes exactly width x height bytes of
// every plane, allocates nothing; sources and planes must not overlap.
inline int preprocess_sequence_host(int format, int flags, const uint8_t *const *frames, int n, size_t stride, int width, int height,
                                    uint8_t *const *prev, uint8_t *const *curr, size_t dst_stride)
{
    if (!frames || !prev || !curr || !format_known(format) || !seq_flags_known(flags) || n < 2) return 1;
    for (int j = 0; j < n; j++)
        if (!frames[j] || (j < n - 1 && (!prev[j] || !curr[j]))) return 1;
    if (width <= 0 || height <= 0) return 2;
    if (stride < (size_t)width * (format_colour(format) ? 3u : 1u) || dst_stride < (size_t)width) return 2;
    for (int j = 0; j < n; j++) {
        const SeqDst d = seq_dst(flags, j, n, j <= n - 2 ? prev[j] : nullptr, j >= 1 ? curr[j - 1] : nullptr);
        for (int y0 = 0; y0 < height; y0 += HSFLOW_PRE_STRIP_ROWS)
            for (int x0 = 0; x0 < width; x0 += 4) switch (format) {
                case 0: seq_strip_any<false, false, true>(frames[j], stride, width, height, x0, y0, false, d.p0, d.p1, d.b, dst_stride); break;
                case 1: seq_strip_any<false, true, true>(frames[j], stride, width, height, x0, y0, false, d.p0, d.p1, d.b, dst_stride); break;
                case 2: seq_strip_any<true, false, true>(frames[j], stride, width, height, x0, y0, false, d.p0, d.p1, d.b, dst_stride); break;
                default: seq_strip_any<true, true, true>(frames[j], stride, width, height, x0, y0, false, d.p0, d.p1, d.b, dst_stride); break;
                }
    }
    return 0;
}

} // namespace hspre
