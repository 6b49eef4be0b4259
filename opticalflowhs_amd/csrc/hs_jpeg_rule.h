// hs_jpeg_rule.h -- the baseline-JPEG rule of the flow picture's file, ONE definition for the device encoder
// (hs_kernels_jpeg.hip.h) and its host twin (hsflow_jpeg_encode_host), the way hs_pre_rule.h serves both sides of the
// pre-processing.  What the reference's cvSaveImage("x.jpg") writes (OpticalFlowOpenCV.cpp:47,
// HSOpticalFlowOpenCL.cpp:771): JFIF 1.01, the Annex K tables scaled by the quality, 4:2:0, libjpeg's "islow" forward
// DCT, the standard Huffman tables, no restart markers.  The normative statement is jpegw::encode of
// host/jpeg_encode.hpp with three channels; that header stays as it is, pinned on its own to libjpeg-turbo and to the
// reference's files, and this one is a SECOND statement of the same arithmetic, checked against it byte for byte.
//
// The file as independent pieces:
//   samples       ycc_* of a pixel clamped to the picture; chroma: 2x2 box average with bias 1 + (cx & 1), chroma rows
//                 at or beyond (H + 1) / 2 repeat row (H + 1) / 2 - 1 of the DOWNSAMPLED plane (chroma_rows)
//   coefficients  fdct_1d over the rows, then over the columns, of the level-shifted 8x8 samples; quantise; zigzag
//   blocks        MCU m = my * MW + mx, block b = 6 m + k: k = 0..3 luma at (bx, by) = (k & 1, k >> 1), 4 Cb, 5 Cr.  A
//                 luma block outside the component's own block grid is a DUMMY: no AC, the DC of the block before it
//                 (block_dc follows that chain down to a real block).  Predictors: block_pred.
//   bits          block_bits: a block's bit string from its 64 zigzag coefficients, its DC and its predictor, into any
//                 sink -- one that counts, one that writes.  At most kMaxBlockBits.
//   stream        the strings in order of b, 1-bits up to a whole byte, 0x00 behind every 0xFF, FF D9.
// Integer arithmetic throughout, so any order of evaluation gives the same bytes.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#if defined(__HIPCC__)
#define HSJ_FN __host__ __device__ inline
#else
#define HSJ_FN inline
#endif

namespace hsjpeg {

constexpr int kHeaderBytes = 623;  // HSFLOW_JPEG_HEADER_BYTES of include/hsflow.h
// a DC code of up to 11 bits (category 11 of the chroma table) and 11 value bits, 63 AC coefficients of a 16-bit code
// and 10 value bits each
constexpr int kMaxBlockBits = 1660;
constexpr int kMaxBlockBytes = 208; // ceil(1660 / 8)

// What an encode of one (quality) needs besides the picture; the host fills it (build_tables), the device reads it.
struct Tables {
    uint16_t q[2][64];        // quantisers 1..255 in natural order: luma, chroma
    uint8_t zpos[64];         // natural index -> zigzag position
    uint16_t dc_code[2][12];
    uint8_t dc_size[2][12];
    uint16_t ac_code[2][256]; // by (run << 4) | size
    uint8_t ac_size[2][256];
    uint8_t header[kHeaderBytes + 1];
};

// ---- sizes ---------------------------------------------------------------------------------------------------------

HSJ_FN int mcus_x(int W) { return (W + 15) / 16; }
HSJ_FN int mcus_y(int H) { return (H + 15) / 16; }
HSJ_FN int chroma_rows(int H) { return (H + 1) / 2; } // rows of the downsampled plane that are averaged, not repeated

// Bytes that always suffice: header, EOI, and every block at its longest with every byte stuffed.
inline size_t bound(int W, int H)
{
    if (W <= 0 || H <= 0) return 0;
    return (size_t)(kHeaderBytes + 2) + (size_t)(2 * kMaxBlockBytes) * 6u * (size_t)mcus_x(W) * (size_t)mcus_y(H);
}

// ---- samples -------------------------------------------------------------------------------------------------------

// libjpeg's rgb_ycc_convert: 16 fractional bits, the constants rounded as FIX() rounds them
constexpr int32_t kYR = (int32_t)(0.29900 * 65536.0 + 0.5), kYG = (int32_t)(0.58700 * 65536.0 + 0.5), kYB = (int32_t)(0.11400 * 65536.0 + 0.5);
constexpr int32_t kCbR = (int32_t)(0.16874 * 65536.0 + 0.5), kCbG = (int32_t)(0.33126 * 65536.0 + 0.5), kCbB = (int32_t)(0.50000 * 65536.0 + 0.5);
constexpr int32_t kCrR = (int32_t)(0.50000 * 65536.0 + 0.5), kCrG = (int32_t)(0.41869 * 65536.0 + 0.5), kCrB = (int32_t)(0.08131 * 65536.0 + 0.5);
constexpr int32_t kHalf = 32768, kOff = 128 << 16;

// (every sum below is positive and below 2^24 + 2^16)
HSJ_FN int32_t ycc_y(int32_t r, int32_t g, int32_t b) { return (kYR * r + kYG * g + kYB * b + kHalf) >> 16; }
HSJ_FN int32_t ycc_cb(int32_t r, int32_t g, int32_t b) { return (-kCbR * r - kCbG * g + kCbB * b + kOff + kHalf - 1) >> 16; }
HSJ_FN int32_t ycc_cr(int32_t r, int32_t g, int32_t b) { return (kCrR * r - kCrG * g - kCrB * b + kOff + kHalf - 1) >> 16; }

// h2v2 box average of four full-resolution chroma samples: the bias alternates 1, 2, 1, 2 along a chroma row
HSJ_FN int32_t chroma_avg(int32_t sum4, int cx) { return (sum4 + 1 + (cx & 1)) >> 2; }

HSJ_FN int clamp_hi(int i, int n) { return i > n - 1 ? n - 1 : i; }

// Luma sample (x, y) of the plane padded to whole MCUs by edge replication.
HSJ_FN int32_t luma_at(const uint8_t *rgb, size_t stride, int W, int H, int x, int y)
{
    const uint8_t *p = rgb + (size_t)clamp_hi(y, H) * stride + (size_t)clamp_hi(x, W) * 3u;
    return ycc_y(p[0], p[1], p[2]);
}

// Chroma samples (cx, cy) of the downsampled planes padded to whole MCUs: the full-resolution planes are padded by edge
// replication to a whole row pair and to the MCU width, averaged, and the DOWNSAMPLED plane's last row is repeated.
HSJ_FN void chroma_at(const uint8_t *rgb, size_t stride, int W, int H, int cx, int cy, int32_t *cb, int32_t *cr)
{
    const int ry = clamp_hi(cy, chroma_rows(H));
    int32_t sb = 0, sr = 0;
    for (int dy = 0; dy < 2; dy++)
        for (int dx = 0; dx < 2; dx++) {
            const uint8_t *p = rgb + (size_t)clamp_hi(2 * ry + dy, H) * stride + (size_t)clamp_hi(2 * cx + dx, W) * 3u;
            sb += ycc_cb(p[0], p[1], p[2]);
            sr += ycc_cr(p[0], p[1], p[2]);
        }
    *cb = chroma_avg(sb, cx);
    *cr = chroma_avg(sr, cx);
}

// ---- coefficients --------------------------------------------------------------------------------------------------

// One 1-D pass of libjpeg's jpeg_fdct_islow over p[0], p[s], ... p[7 s]: the row pass (second = false; results scaled
// up by 4) or the column pass (second = true; with the row pass the results are 8 x the DCT).
// 32-bit intermediates suffice for 8-bit samples.  Row pass: |sample| <= 128, sums of four <= 512, the largest product
// 512 * 25172 < 2^24.  Its results are 4 sqrt(8) x an orthonormal 1-D DCT of 8 values of magnitude <= 128, so <= 4096 in
// magnitude.  Column pass: differences of two <= 8192 (tmp4..7), sums of four <= 16384 (z1..z4 and z3 + z4); the
// largest sum before a descale is tmp6 * 25172 + z2 * 20995 + z3 * 16069 + z5 <= 206 M + 344 M + 263 M + 158 M < 2^30.
HSJ_FN void fdct_1d(int32_t *p, int s, bool second)
{
    constexpr int32_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
                      F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
    int32_t tmp0 = p[0] + p[7 * s], tmp7 = p[0] - p[7 * s], tmp1 = p[s] + p[6 * s], tmp6 = p[s] - p[6 * s];
    int32_t tmp2 = p[2 * s] + p[5 * s], tmp5 = p[2 * s] - p[5 * s], tmp3 = p[3 * s] + p[4 * s], tmp4 = p[3 * s] - p[4 * s];
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int sh = second ? 15 : 11;              // CONST_BITS + PASS1_BITS : CONST_BITS - PASS1_BITS
    const int32_t rnd = (int32_t)1 << (sh - 1);
    if (!second) {
        p[0] = (tmp10 + tmp11) * 4;
        p[4 * s] = (tmp10 - tmp11) * 4;
    } else {
        p[0] = (tmp10 + tmp11 + 2) >> 2;
        p[4 * s] = (tmp10 - tmp11 + 2) >> 2;
    }
    int32_t z1 = (tmp12 + tmp13) * F_0_541;
    p[2 * s] = (z1 + tmp13 * F_0_765 + rnd) >> sh;
    p[6 * s] = (z1 - tmp12 * F_1_847 + rnd) >> sh;
    z1 = tmp4 + tmp7;
    int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int32_t z5 = (z3 + z4) * F_1_175;
    tmp4 *= F_0_298; tmp5 *= F_2_053; tmp6 *= F_3_072; tmp7 *= F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562; z3 *= -F_1_961; z4 *= -F_0_390;
    z3 += z5; z4 += z5;
    p[7 * s] = (tmp4 + z1 + z3 + rnd) >> sh;
    p[5 * s] = (tmp5 + z2 + z4 + rnd) >> sh;
    p[3 * s] = (tmp6 + z2 + z3 + rnd) >> sh;
    p[s] = (tmp7 + z1 + z4 + rnd) >> sh;
}

// The rounded division of the 8x-scaled coefficient by the quantiser, on the magnitude, as libjpeg's forward_DCT.
HSJ_FN int32_t quantise(int32_t t, int32_t q)
{
    const int32_t qv = q << 3;
    int32_t a = (t < 0 ? -t : t) + (qv >> 1);
    a = a >= qv ? a / qv : 0;
    return t < 0 ? -a : a;
}

// ---- blocks --------------------------------------------------------------------------------------------------------

// Is luma block k (0..3) of MCU (mx, my) outside the luma component's own block grid?  (k = 0 never is.)
HSJ_FN bool luma_dummy(int W, int H, int mx, int my, int k)
{
    return 2 * mx + (k & 1) >= (W + 7) / 8 || 2 * my + (k >> 1) >= (H + 7) / 8;
}

// The quantised DC of block b: its own, or for a dummy block that of the nearest block before it that is none.
// zz: the coefficient plane, 64 per block; only real blocks' entries are read.
HSJ_FN int32_t block_dc(const int16_t *zz, int W, int H, int MW, long long b)
{
    const long long m = b / 6;
    int k = (int)(b - 6 * m);
    if (k < 4) {
        const int mx = (int)(m % MW), my = (int)(m / MW);
        while (k > 0 && luma_dummy(W, H, mx, my, k)) k--;
    }
    return zz[(size_t)(6 * m + k) * 64u];
}

// The DC predictor of block b: the DC of the component's previous block in the stream, 0 for the first.
HSJ_FN int32_t block_pred(const int16_t *zz, int W, int H, int MW, long long b)
{
    const long long m = b / 6;
    const int k = (int)(b - 6 * m);
    if (k > 0 && k < 4) return block_dc(zz, W, H, MW, b - 1);
    if (m == 0) return 0;
    return block_dc(zz, W, H, MW, 6 * (m - 1) + (k == 0 ? 3 : k));
}

HSJ_FN int nbits(int32_t v)
{
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// Eight consecutive coefficients of a block (16-byte aligned) as four words.
HSJ_FN void load8(const int16_t *p, uint32_t w[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 t = *(const uint4 *)p;
    w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
#else
    memcpy(w, p, 16);
#endif
}

// The bit string of one block: DC category code and the bits of diff (diff - 1 when negative), then run/size codes
// with 0xF0 for every 16 zeros before a coefficient, and EOB (0x00) when zeros are left at the end.  zz: the block's 64
// zigzag coefficients (zz[0] is not read: dc stands for it; a dummy block's are not read at all).  sink.put(code, size):
// `size` (1..16) bits, the low bits of code.
template <class Sink>
HSJ_FN void block_bits(const Tables &t, int tbl, const int16_t *zz, int32_t dc, int32_t pred, bool dummy, Sink &sink)
{
    const int32_t diff = dc - pred;
    int n = nbits(diff);
    sink.put(t.dc_code[tbl][n], t.dc_size[tbl][n]);
    if (n) sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
    int run = dummy ? 63 : 0;
    for (int c = 0; c < 8 && !dummy; c++) {
        uint32_t w[4];
        load8(zz + 8 * c, w);
        if (c == 0) w[0] &= 0xFFFF0000u;
        if (!(w[0] | w[1] | w[2] | w[3])) { run += c == 0 ? 7 : 8; continue; }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 8; j++) {
            if (c == 0 && j == 0) continue;
            const int32_t v = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
            if (!v) { run++; continue; }
            while (run > 15) { sink.put(t.ac_code[tbl][0xF0], t.ac_size[tbl][0xF0]); run -= 16; }
            n = nbits(v);
            sink.put(t.ac_code[tbl][(run << 4) | n], t.ac_size[tbl][(run << 4) | n]);
            sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
            run = 0;
        }
    }
    if (run) sink.put(t.ac_code[tbl][0], t.ac_size[tbl][0]);
}

struct CountSink {
    uint32_t bits = 0;
    HSJ_FN void put(uint32_t, int size) { bits += (uint32_t)size; }
};

// ---- host only from here: the tables, the header, and the rule over a picture in host memory --------------------------

inline void build_huff(const uint8_t *bits, const uint8_t *vals, uint16_t *code, uint8_t *size)
{
    int c = 0, k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < bits[len - 1]; i++) { code[vals[k]] = (uint16_t)c; size[vals[k]] = (uint8_t)len; c++; k++; }
        c <<= 1;
    }
}

// quality 1..100 (the caller has checked), W and H 1..65535.
inline void build_tables(Tables &t, int W, int H, int quality)
{
    // ITU-T T.81 Annex K: tables K.1, K.2 (quantisation, natural order) and K.3 - K.6 (Huffman)
    static const uint8_t quant[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    static const uint8_t zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    static const uint8_t dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
    static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
    static const uint8_t ac_vals[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
         0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
         0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
         0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
         0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
         0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
         0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
         0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
         0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
         0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
         0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
         0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa}};
    memset(&t, 0, sizeof t);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < 64; i++) {
            const int v = (quant[c][i] * scale + 50) / 100;
            t.q[c][i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    for (int i = 0; i < 64; i++) t.zpos[zigzag[i]] = (uint8_t)i;
    for (int c = 0; c < 2; c++) {
        build_huff(dc_bits[c], dc_vals, t.dc_code[c], t.dc_size[c]);
        build_huff(ac_bits[c], ac_vals[c], t.ac_code[c], t.ac_size[c]);
    }
    // SOI, JFIF APP0 (1.01, no units, 1:1, no thumbnail), two DQT, SOF0 (4:2:0), four DHT, SOS
    uint8_t *o = t.header;
    auto put = [&](int v) { *o++ = (uint8_t)v; };
    auto put16 = [&](int v) { put(v >> 8); put(v); };
    static const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    static const uint8_t sof_comps[9] = {1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}, sos_tail[9] = {1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (int v : app0) put(v);
    for (int c = 0; c < 2; c++) {
        put(0xFF); put(0xDB); put16(67); put(c);
        for (int i = 0; i < 64; i++) put(t.q[c][zigzag[i]]);
    }
    put(0xFF); put(0xC0); put16(17); put(8); put16(H); put16(W); put(3);
    for (int v : sof_comps) put(v);
    for (int c = 0; c < 2; c++) {
        put(0xFF); put(0xC4); put16(2 + 1 + 16 + 12); put(c);
        for (int i = 0; i < 16; i++) put(dc_bits[c][i]);
        for (int i = 0; i < 12; i++) put(dc_vals[i]);
        put(0xFF); put(0xC4); put16(2 + 1 + 16 + 162); put(0x10 | c);
        for (int i = 0; i < 16; i++) put(ac_bits[c][i]);
        for (int i = 0; i < 162; i++) put(ac_vals[c][i]);
    }
    put(0xFF); put(0xDA); put16(12); put(3);
    for (int v : sos_tail) put(v);
    // (o == t.header + kHeaderBytes)
}

// The 64 zigzag coefficients of real block k of MCU (mx, my), from the picture.
inline void block_coefs(const Tables &t, const uint8_t *rgb, size_t stride, int W, int H, int mx, int my, int k, int16_t *zz)
{
    int32_t d[64];
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++) {
            if (k < 4) d[8 * y + x] = luma_at(rgb, stride, W, H, 16 * mx + 8 * (k & 1) + x, 16 * my + 8 * (k >> 1) + y) - 128;
            else {
                int32_t cb, cr;
                chroma_at(rgb, stride, W, H, 8 * mx + x, 8 * my + y, &cb, &cr);
                d[8 * y + x] = (k == 4 ? cb : cr) - 128;
            }
        }
    for (int i = 0; i < 8; i++) fdct_1d(d + 8 * i, 1, false);
    for (int i = 0; i < 8; i++) fdct_1d(d + i, 8, true);
    for (int i = 0; i < 64; i++) zz[t.zpos[i]] = (int16_t)quantise(d[i], t.q[k < 4 ? 0 : 1][i]);
}

// The stream's bytes into out[0 .. cap): stuffed, counted beyond cap but not written.
struct ByteSink {
    uint8_t *out;
    size_t cap, n = 0;
    uint32_t acc = 0;
    int fill = 0;
    ByteSink(uint8_t *o, size_t c) : out(o), cap(c) {}
    void byte(uint8_t b) { if (n < cap) out[n] = b; n++; }
    void put(uint32_t code, int size)
    {
        acc = (acc << size) | code;
        fill += size;
        while (fill >= 8) {
            const uint8_t b = (uint8_t)(acc >> (fill - 8));
            byte(b);
            if (b == 0xFF) byte(0);
            fill -= 8;
        }
        acc &= (1u << fill) - 1u;
    }
};

// The rule over one picture in host memory.  Returns 0, 1 (null pointer, quality outside 1..100), 2 (size outside
// 1..65535, stride below 3 * width, or capacity below the file's size: *bytes holds the size either way once the
// arguments are sound), 4 (no memory for the coefficients): HSFLOW_OK / HSFLOW_E_ARG / HSFLOW_E_SIZE / HSFLOW_E_OOM.
// Reads exactly the width x height pixels of rgb and writes nothing at or beyond jpeg + capacity.
inline int encode_host(const uint8_t *rgb, size_t stride, int W, int H, int quality, uint8_t *jpeg, size_t capacity, size_t *bytes)
{
    if (!rgb || !bytes || (!jpeg && capacity) || quality < 1 || quality > 100) return 1;
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || stride < (size_t)W * 3u) return 2;
    const int MW = mcus_x(W), MH = mcus_y(H);
    const long long nb = 6ll * MW * MH;
    Tables *t = (Tables *)malloc(sizeof(Tables));
    int16_t *zz = (int16_t *)malloc((size_t)nb * 64u * sizeof(int16_t));
    if (!t || !zz) { free(t); free(zz); return 4; }
    build_tables(*t, W, H, quality);
    for (long long b = 0; b < nb; b++) {
        const long long m = b / 6;
        const int k = (int)(b - 6 * m), mx = (int)(m % MW), my = (int)(m / MW);
        if (k < 4 && luma_dummy(W, H, mx, my, k)) memset(zz + (size_t)b * 64u, 0, 64 * sizeof(int16_t));
        else block_coefs(*t, rgb, stride, W, H, mx, my, k, zz + (size_t)b * 64u);
    }
    ByteSink s(jpeg, capacity);
    for (int i = 0; i < kHeaderBytes; i++) s.byte(t->header[i]);
    for (long long b = 0; b < nb; b++) {
        const long long m = b / 6;
        const int k = (int)(b - 6 * m);
        const bool dummy = k < 4 && luma_dummy(W, H, (int)(m % MW), (int)(m / MW), k);
        block_bits(*t, k < 4 ? 0 : 1, zz + (size_t)b * 64u, block_dc(zz, W, H, MW, b), block_pred(zz, W, H, MW, b), dummy, s);
    }
    if (s.fill) s.put((1u << (8 - s.fill)) - 1u, 8 - s.fill); // 1-bits up to a whole byte
    s.byte(0xFF);
    s.byte(0xD9);
    free(t);
    free(zz);
    *bytes = s.n;
    return s.n <= capacity ? 0 : 2;
}

} // namespace hsjpeg
