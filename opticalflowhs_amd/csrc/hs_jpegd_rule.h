// hs_jpegd_rule.h -- the baseline-JPEG DECODING rule of the input frames, ONE definition for the device decoder
// (hs_kernels_jpegd.hip.h) and its host twin (hsflow_jpeg_decode_host), the counterpart of hs_jpeg_rule.h.  What the
// reference's cvLoadImage(path, 1) computes (OpticalFlowOpenCV.cpp:15,18, HSOpticalFlowOpenCL.cpp:721,732): libjpeg
// with its defaults -- the "islow" inverse DCT, "fancy" triangle upsampling of the chroma planes, the 16-bit YCbCr ->
// RGB conversion.  The normative statement is jpegb::decode of host/jpeg_baseline.hpp (held to libjpeg-turbo by
// tests/test_jpeg.py); that header stays as it is, and this one is a SECOND statement of the same process, cut into
// pieces that do not depend on each other's order, checked against it pixel for pixel.
//
// The decode as independent pieces:
//   header        parse (host only): SOI, DQT, DHT, SOF0/SOF1 8-bit, DRI, one interleaved SOS -> Frame (sizes, sampling),
//                 Tables (Huffman look-ups, quantisers, zigzag) and the byte range of the entropy-coded segment
//   clean stream  byte_class of every byte of the segment from its two neighbours: kept, dropped (the 0x00 behind a
//                 0xFF, fill bytes, RSTn markers), and "an interval starts behind me" for the second byte of an RSTn
//   symbols       huff_step: ONE symbol from a state (bit position p, block in the MCU b, zigzag position k) to the next
//                 state; never stops, marks what is wrong, can hand the coefficient to a sink.  Bits at or beyond the end
//                 of the clean stream read as 0.
//   blocks        stream block B = MCU * bpm + b; b < hs * vs: luma block (b % hs, b / hs) of the MCU, then Cb, Cr.  DC:
//                 the running sum of the differences of a component, from the last restart on (wrapping 32-bit sums)
//   samples       dequantise (dequant: refuses what the 32-bit IDCT could not carry), idct_1d over the columns, then over
//                 the rows, + 128, clamp
//   pixels        pixel(): the three samples of an output pixel -- chroma_h2v1 / chroma_h2v2 with the edge rules, plain
//                 replication when the chroma plane is at most 2 samples wide -- and ycc_rgb
// Integer arithmetic throughout, so any order of evaluation gives the same bytes.
//
// Stricter than jpegb in two places, both refusals (for every file both accept, the pixels are identical): a decode
// that consumes a bit at or beyond the end of the clean stream is an error (jpegb pads with zeros), and so is a
// coefficient outside the range below (jpegb carries it in 64 bits).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#if defined(__HIPCC__)
#define HSD_FN __host__ __device__ inline
#else
#define HSD_FN inline
#endif

namespace hsjpegd {

constexpr int kSubseqBits = 1024;    // HSFLOW_JPEGD_SUBSEQ_BITS of include/hsflow.h
constexpr int kChunk = 128;          // bytes of the stuffed segment per lane of the cleaning kernels
constexpr uint32_t kMaxScanBytes = 1u << 28; // bit positions are 32-bit words
constexpr int kStatusCorrupt = 1, kStatusTruncated = 2; // the status word; the larger one wins

// One canonical Huffman table in look-up form.  maxcode / valoff as T.81 F.2.2.3 (valoff = valptr - mincode), and for
// the codes of at most 8 bits a table by the next 8 bits: (length << 8) | symbol, 0 = longer than 8 bits or no code.
struct Huff {
    int32_t maxcode[17]; // [k]: the largest code of k bits, -1: none ([0] unused)
    int32_t valoff[17];
    uint16_t lut[256];
    uint8_t vals[256];
};

// What the kernels read besides the stream: filled by parse(), 6 KB, copied into LDS by the kernels that decode symbols.
struct Tables {
    Huff dc[3], ac[3];  // by component
    uint16_t q[3][64];  // quantisers by component, natural order
    uint8_t zpos[64];   // natural index -> zigzag position
};

struct Frame {
    int32_t W, H, ncomp, hs, vs; // hs x vs luma blocks per MCU (1x1, 2x1, 2x2); chroma 1x1
    int32_t ri;                  // MCUs per restart interval, 0: none
    int32_t mcux, mcuy, bpm;     // MCUs across and down, blocks per MCU
    int32_t cw, ch;              // real chroma samples across and down
    int64_t nblocks;             // mcux * mcuy * bpm
    uint64_t scan_offset, scan_bytes; // the entropy-coded segment within the file, up to the marker that ends it
};

HSD_FN int luma_blocks(const Frame &f) { return f.hs * f.vs; }
HSD_FN int comp_of_block(const Frame &f, int b) { const int nl = f.hs * f.vs; return b < nl ? 0 : b - nl + 1; }
// plane of component c: blocks across / down, and its offset in blocks within the planes laid behind each other
HSD_FN int plane_wb(const Frame &f, int c) { return f.mcux * (c ? 1 : f.hs); }
HSD_FN int plane_hb(const Frame &f, int c) { return f.mcuy * (c ? 1 : f.vs); }
HSD_FN int64_t plane_block0(const Frame &f, int c)
{
    const int64_t m = (int64_t)f.mcux * f.mcuy;
    return c == 0 ? 0 : m * f.hs * f.vs + (c - 1) * m;
}

// ---- clean stream --------------------------------------------------------------------------------------------------

// What becomes of byte `cur` of the entropy-coded segment, from its neighbours (0 beyond either end):
// 0 kept, 1 dropped, 2 dropped and a restart interval starts with the next kept byte.
HSD_FN int byte_class(int prev, int cur, int next)
{
    if (prev == 0xFF && cur == 0x00) return 1;                 // the stuffing behind a data 0xFF
    if (prev == 0xFF && cur >= 0xD0 && cur <= 0xD7) return 2;  // RSTn, second byte
    if (cur == 0xFF && next != 0x00) return 1;                 // RSTn's first byte, a fill byte, a lone 0xFF at the end
    return 0;
}

// ---- symbols -------------------------------------------------------------------------------------------------------

struct State {
    uint32_t p; // bit position in the clean stream
    int32_t b;  // block within the MCU
    int32_t k;  // zigzag position of the next coefficient; 0: the DC symbol comes next
};
HSD_FN uint64_t pack(const State &s) { return (uint64_t)s.p << 16 | (uint64_t)s.b << 8 | (uint64_t)s.k; }
HSD_FN State unpack(uint64_t v) { return State{(uint32_t)(v >> 16), (int32_t)((v >> 8) & 255u), (int32_t)(v & 255u)}; }

constexpr int kBad = 1, kBlockDone = 2; // huff_step's result bits

// The 32 bits from bit p on.  words: the clean stream, 4-byte aligned, with at least 8 bytes of anything behind `end`
// bits (they are masked off here: bits at or beyond the end read as 0).
HSD_FN uint32_t peek32(const uint32_t *words, uint32_t p, uint32_t end)
{
    if (p >= end) return 0;
    const uint32_t hi = __builtin_bswap32(words[p >> 5]), lo = __builtin_bswap32(words[(p >> 5) + 1]);
    const int s = (int)(p & 31u);
    uint32_t v = s ? (hi << s) | (lo >> (32 - s)) : hi;
    const uint32_t avail = end - p;
    if (avail < 32u) v &= ~(0xFFFFFFFFu >> avail);
    return v;
}

// One code of table h from the top of v: the symbol, and its length into *len.  No code of at most 16 bits matches:
// 16 bits, symbol 0, *bad set.
HSD_FN int huff_symbol(const Huff &h, uint32_t v, int *len, bool *bad)
{
    const uint32_t e = h.lut[v >> 24];
    if (e) { *len = (int)(e >> 8); return (int)(e & 255u); }
    for (int k = 9; k <= 16; k++) {
        const int32_t code = (int32_t)(v >> (32 - k));
        if (h.maxcode[k] >= 0 && code <= h.maxcode[k]) {
            *len = k;
            return h.vals[(h.valoff[k] + code) & 255];
        }
    }
    *len = 16;
    *bad = true;
    return 0;
}

// T.81 F.2.2.1 EXTEND of the t-bit value v (t >= 1)
HSD_FN int32_t extend(int32_t v, int t) { return v < (1 << (t - 1)) ? v - (1 << t) + 1 : v; }

// ONE symbol.  A DC symbol (k == 0) consumes its code and min(t, 11) value bits and hands sink.coef(0, difference);
// an AC symbol consumes its code and, unless it is EOB or ZRL, its value bits, and hands sink.coef(k, value).  What is
// wrong -- a code of no table, t > 11, a run past 63 -- does not stop it: the result has kBad, the block ends where a
// run left it, and the state goes on.  Every step consumes at least one bit and at most 31.  kBlockDone: the block
// ended with this symbol (s.b is the next block's, s.k is 0).
template <class Sink>
HSD_FN int huff_step(const Tables &t, const Frame &f, const uint32_t *words, uint32_t end, State &s, Sink &sink)
{
    const uint32_t v = peek32(words, s.p, end);
    const int c = comp_of_block(f, s.b);
    bool bad = false;
    int len, done = 0;
    if (s.k == 0) {
        int cat = huff_symbol(t.dc[c], v, &len, &bad);
        if (cat > 11) { cat = 11; bad = true; }
        const int32_t diff = cat ? extend((int32_t)((v << len) >> (32 - cat)), cat) : 0;
        sink.coef(0, diff);
        s.p += (uint32_t)(len + cat);
        s.k = 1;
    } else {
        const int rs = huff_symbol(t.ac[c], v, &len, &bad), run = rs >> 4, sz = rs & 15;
        s.p += (uint32_t)(len + sz);
        if (sz == 0) {
            if (run == 15) s.k += 16;
            else done = 1; // EOB
        } else {
            s.k += run;
            if (s.k > 63) bad = true;
            else sink.coef(s.k, extend((int32_t)((v << len) >> (32 - sz)), sz));
            s.k++;
        }
    }
    if (done || s.k > 63) {
        s.k = 0;
        s.b = s.b + 1 == f.bpm ? 0 : s.b + 1;
        return (bad ? kBad : 0) | kBlockDone;
    }
    return bad ? kBad : 0;
}

struct NullSink {
    HSD_FN void coef(int, int32_t) {}
};

// Stores into the zigzag coefficients of one block after the other (64 int16 each, zero before); the DC slot receives
// the difference.  Blocks at or beyond `limit` are dropped.
struct CoefSink {
    int16_t *zz;
    int64_t block, limit;
    HSD_FN void coef(int k, int32_t v) { if (block < limit) zz[block * 64 + k] = (int16_t)v; }
};

// Symbols from s on until one would start at or beyond bit `stop`: the speculative decode of one subsequence.
// Returns the blocks that ended.
HSD_FN uint32_t run_subsequence(const Tables &t, const Frame &f, const uint32_t *words, uint32_t end, State &s, uint32_t stop)
{
    NullSink sink;
    uint32_t blocks = 0;
    while (s.p < stop) blocks += (uint32_t)(huff_step(t, f, words, end, s, sink) >> 1);
    return blocks;
}

// The pass that counts: symbols from the TRUE state s on, coefficients into sink, until a symbol would start at or beyond
// `stop` or beyond the stream's end, or `nblocks` blocks have ended.  Returns the status this stretch raises: a symbol
// of a block the frame has that is bad (1) or that consumed a bit at or beyond the end (2).
HSD_FN int decode_stretch(const Tables &t, const Frame &f, const uint32_t *words, uint32_t end, State &s, uint32_t stop, int64_t nblocks,
                          CoefSink &sink)
{
    int status = 0;
    while (s.p < stop && s.p < end && sink.block < nblocks) {
        const int r = huff_step(t, f, words, end, s, sink);
        if (r & kBad) status = status > kStatusCorrupt ? status : kStatusCorrupt;
        if (s.p > end) status = kStatusTruncated;
        sink.block += r >> 1;
    }
    return status;
}

// ---- samples -------------------------------------------------------------------------------------------------------

// The quantised coefficient v times its quantiser, *bad set when the product leaves what a baseline file of 8-bit
// samples can hold and idct_1d can carry in 32 bits: |v * q| <= kCoefMax.  An 8x8 block of samples in -128 .. 127 has
// DCT coefficients of magnitude <= 1024, and rounding to a multiple of an 8-bit quantiser adds at most 127.
constexpr int32_t kCoefMax = 1151;
HSD_FN int32_t dequant(int32_t v, int32_t q, bool *bad)
{
    if (v < -2047 || v > 2047) { *bad = true; return 0; } // (beyond the 11-bit categories of a baseline file; the product below fits)
    const int32_t x = v * q;
    if (x < -kCoefMax || x > kCoefMax) { *bad = true; return 0; }
    return x;
}

// One 1-D pass of libjpeg's jpeg_idct_islow over p[0], p[s], ... p[7 s]: the column pass (second = false; results
// scaled up by 4) or the row pass (second = true; descaled to samples, the level shift and the clamp are the caller's).
// 32-bit intermediates suffice for |input| <= kCoefMax.  Every intermediate is a linear form of the eight inputs, so its
// magnitude is at most max|input| times the sum of the magnitudes of its coefficients.  The largest such sums: the
// even part's tmp10 .. tmp13, 16384 + 15137 = 31521; the odd part before its last additions, z2 + z3 with 54862; and
// the values that are descaled, an even sum plus an odd result: 61214.  Column pass: 61214 * 1151 + 2^10 < 2^27, results
// (descaled by 11 bits) of magnitude <= 34403.  Row pass: 61214 * 34403 + 2^17 = 2 106 076 314 < 2^31.
HSD_FN void idct_1d(int32_t *p, int s, bool second)
{
    constexpr int32_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
                      F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
    const int sh = second ? 18 : 11; // CONST_BITS + PASS1_BITS + 3 : CONST_BITS - PASS1_BITS
    const int32_t rnd = (int32_t)1 << (sh - 1);
    int32_t z2 = p[2 * s], z3 = p[6 * s];
    int32_t z1 = (z2 + z3) * F_0_541;
    int32_t tmp2 = z1 + z3 * (-F_1_847), tmp3 = z1 + z2 * F_0_765;
    int32_t tmp0 = (p[0] + p[4 * s]) * 8192, tmp1 = (p[0] - p[4 * s]) * 8192;
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = p[7 * s]; tmp1 = p[5 * s]; tmp2 = p[3 * s]; tmp3 = p[s];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int32_t z4 = tmp1 + tmp3;
    const int32_t z5 = (z3 + z4) * F_1_175;
    tmp0 *= F_0_298; tmp1 *= F_2_053; tmp2 *= F_3_072; tmp3 *= F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562; z3 *= -F_1_961; z4 *= -F_0_390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    p[0] = (tmp10 + tmp3 + rnd) >> sh; p[7 * s] = (tmp10 - tmp3 + rnd) >> sh;
    p[s] = (tmp11 + tmp2 + rnd) >> sh; p[6 * s] = (tmp11 - tmp2 + rnd) >> sh;
    p[2 * s] = (tmp12 + tmp1 + rnd) >> sh; p[5 * s] = (tmp12 - tmp1 + rnd) >> sh;
    p[3 * s] = (tmp13 + tmp0 + rnd) >> sh; p[4 * s] = (tmp13 - tmp0 + rnd) >> sh;
}

HSD_FN int32_t clamp255(int32_t x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// ---- pixels --------------------------------------------------------------------------------------------------------

// libjpeg's fancy h2v1 upsampling as a function of the output column x: 3/4 of the nearer sample, 1/4 of the farther,
// rounding alternating (+1, +2); the first and the last output column are the edge samples themselves.  row: sw (> 2)
// real samples.
HSD_FN int32_t chroma_h2v1(const uint8_t *row, int sw, int x)
{
    const int i = x >> 1;
    if (!(x & 1)) return i == 0 ? row[0] : (row[i] * 3 + row[i - 1] + 1) >> 2;
    return i == sw - 1 ? row[sw - 1] : (row[i] * 3 + row[i + 1] + 2) >> 2;
}

// ... and h2v2 for output pixel (x, y): vertically 3/4 of the nearer row and 1/4 of the farther (the edge row when there
// is none), then the same across, rounding (+8, +7) >> 4.  plane: sw (> 2) x sh real samples, rows `ss` apart.
HSD_FN int32_t chroma_h2v2(const uint8_t *plane, int ss, int sw, int sh, int x, int y)
{
    const int sy = y >> 1;
    int ny = (y & 1) ? sy + 1 : sy - 1;
    ny = ny < 0 ? 0 : (ny > sh - 1 ? sh - 1 : ny);
    const uint8_t *in0 = plane + (size_t)sy * (size_t)ss, *in1 = plane + (size_t)ny * (size_t)ss;
    const int i = x >> 1;
    const int32_t cur = in0[i] * 3 + in1[i];
    if (!(x & 1)) return i == 0 ? (cur * 4 + 8) >> 4 : (cur * 3 + in0[i - 1] * 3 + in1[i - 1] + 8) >> 4;
    return i == sw - 1 ? (cur * 4 + 7) >> 4 : (cur * 3 + in0[i + 1] * 3 + in1[i + 1] + 7) >> 4;
}

// Sample of the chroma plane `plane` (rows `ss` apart) for output pixel (x, y).
HSD_FN int32_t chroma_at(const Frame &f, const uint8_t *plane, int ss, int x, int y)
{
    if (f.hs == 1) return plane[(size_t)y * (size_t)ss + (size_t)x];
    const bool v2 = f.vs == 2;
    if (f.cw <= 2) return plane[(size_t)(v2 ? y >> 1 : y) * (size_t)ss + (size_t)(x >> 1)]; // libjpeg replicates planes this narrow
    return v2 ? chroma_h2v2(plane, ss, f.cw, f.ch, x, y) : chroma_h2v1(plane + (size_t)y * (size_t)ss, f.cw, x);
}

// libjpeg's ycc_rgb_convert: 16 fractional bits, the constants rounded as FIX() rounds them
constexpr int32_t kCrR = (int32_t)(1.40200 * 65536.0 + 0.5), kCbB = (int32_t)(1.77200 * 65536.0 + 0.5),
                  kCrG = (int32_t)(0.71414 * 65536.0 + 0.5), kCbG = (int32_t)(0.34414 * 65536.0 + 0.5);
HSD_FN void ycc_rgb(int32_t y, int32_t cb, int32_t cr, int32_t *r, int32_t *g, int32_t *b)
{
    cb -= 128; cr -= 128;
    *r = clamp255(y + ((kCrR * cr + 32768) >> 16));
    *b = clamp255(y + ((kCbB * cb + 32768) >> 16));
    *g = clamp255(y + ((-kCbG * cb + 32768 - kCrG * cr) >> 16));
}

// Output pixel (x, y) from the component planes (planes[c]: rows strides[c] apart): R, G, B.
HSD_FN void pixel(const Frame &f, const uint8_t *const planes[3], const int strides[3], int x, int y, int32_t *r, int32_t *g, int32_t *b)
{
    const int32_t yy = planes[0][(size_t)y * (size_t)strides[0] + (size_t)x];
    if (f.ncomp == 1) { *r = *g = *b = yy; return; }
    ycc_rgb(yy, chroma_at(f, planes[1], strides[1], x, y), chroma_at(f, planes[2], strides[2], x, y), r, g, b);
}

// ---- host only from here: the header, and the rule over a file in host memory -----------------------------------------

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline void build_huff(Huff &h, const uint8_t *counts /* [1..16] */, const uint8_t *vals, int total)
{
    memset(&h, 0, sizeof h);
    memcpy(h.vals, vals, (size_t)total);
    int32_t code = 0, idx = 0;
    for (int k = 1; k <= 16; k++) {
        h.valoff[k] = idx - code;
        h.maxcode[k] = counts[k] ? code + counts[k] - 1 : -1;
        code = (code + counts[k]) << 1;
        idx += counts[k];
    }
    h.maxcode[0] = -1;
    for (int v = 0; v < 256; v++)
        for (int k = 1; k <= 8; k++) {
            const int32_t c = v >> (8 - k);
            if (h.maxcode[k] >= 0 && c <= h.maxcode[k]) {
                h.lut[v] = (uint16_t)(k << 8 | h.vals[(h.valoff[k] + c) & 255]);
                break;
            }
        }
}

// The header of `file`.  Returns 0, or 7 (HSFLOW_E_DATA) for everything jpegb::decode refuses from the header alone --
// not a JPEG file, a truncated or malformed segment, progressive / lossless / arithmetic / 12-bit, 2 or more than 3
// components, other sampling factors, a second frame header, a missing table, an empty scan header -- and for a segment
// of kMaxScanBytes or more.  *why (may be null): a static text.
inline int parse(const uint8_t *file, size_t bytes, Frame &f, Tables &t, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    auto fail = [&](const char *m) { *why = m; return 7; };
    const uint8_t *p = file, *end = file + bytes;
    if (bytes < 4 || p[0] != 0xFF || p[1] != 0xD8) return fail("not a JPEG file");
    p += 2;
    Huff *dc = (Huff *)malloc(8 * sizeof(Huff));
    if (!dc) return fail("no memory");
    Huff *ac = dc + 4;
    uint16_t qt[4][64];
    bool qt_ok[4] = {false, false, false, false}, dc_ok[4] = {false, false, false, false}, ac_ok[4] = {false, false, false, false};
    int cid[3] = {0, 0, 0}, ch_[3] = {1, 1, 1}, cv[3] = {1, 1, 1}, ctq[3] = {0, 0, 0}, ncomp = 0;
    int W = 0, H = 0, ri = 0;
    bool have_sof = false;
    auto done = [&](int r) { free(dc); return r; };
    while (p + 4 <= end) {
        if (p[0] != 0xFF) { p++; continue; }
        const int m = p[1];
        if (m == 0xFF) { p++; continue; }
        p += 2;
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (m == 0xD9) break;
        if (p + 2 > end) return done(fail("truncated marker"));
        const int len = (p[0] << 8) | p[1];
        if (len < 2 || p + len > end) return done(fail("bad segment length"));
        const uint8_t *s = p + 2, *se = p + len;
        if (m == 0xDB) {
            while (s < se) {
                const int pq = s[0] >> 4, tq = s[0] & 15;
                s++;
                if (tq > 3 || s + (pq ? 128 : 64) > se) return done(fail("bad DQT"));
                for (int i = 0; i < 64; i++) {
                    qt[tq][kZigzag[i]] = pq ? (uint16_t)((s[0] << 8) | s[1]) : s[0];
                    s += pq ? 2 : 1;
                }
                qt_ok[tq] = true;
            }
        } else if (m == 0xC4) {
            while (s < se) {
                const int tc = s[0] >> 4, th = s[0] & 15;
                if (tc > 1 || th > 3 || s + 17 > se) return done(fail("bad DHT"));
                int total = 0;
                for (int k = 1; k <= 16; k++) total += s[k];
                if (total > 256 || s + 17 + total > se) return done(fail("bad DHT"));
                build_huff(tc ? ac[th] : dc[th], s, s + 17, total);
                (tc ? ac_ok : dc_ok)[th] = true;
                s += 17 + total;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            if (have_sof) return done(fail("more than one frame header"));
            if (se - s < 6 || s[0] != 8) return done(fail("only 8-bit samples are supported"));
            H = (s[1] << 8) | s[2]; W = (s[3] << 8) | s[4];
            const int n = s[5];
            if (W <= 0 || H <= 0 || (n != 1 && n != 3) || se - s < 6 + 3 * n) return done(fail("unsupported frame header"));
            ncomp = n;
            for (int i = 0; i < n; i++) {
                cid[i] = s[6 + 3 * i];
                ch_[i] = s[7 + 3 * i] >> 4; cv[i] = s[7 + 3 * i] & 15;
                ctq[i] = s[8 + 3 * i];
                if (ctq[i] > 3) return done(fail("bad quantisation table index"));
                if (ch_[i] < 1 || ch_[i] > 4 || cv[i] < 1 || cv[i] > 4) return done(fail("bad sampling factor"));
            }
            have_sof = true;
        } else if (m == 0xC2 || (m >= 0xC3 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC)) {
            return done(fail("progressive / lossless / arithmetic JPEG is not supported"));
        } else if (m == 0xDD) {
            if (se - s < 2) return done(fail("bad DRI"));
            ri = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!have_sof) return done(fail("scan before frame header"));
            if (se - s < 1) return done(fail("truncated scan header"));
            const int n = s[0];
            if (n != ncomp || se - s < 1 + 2 * n + 3) return done(fail("unsupported scan layout"));
            memset(&t, 0, sizeof t);
            for (int i = 0; i < n; i++) {
                int c = -1;
                for (int j = 0; j < ncomp; j++) if (cid[j] == s[1 + 2 * i]) c = j;
                if (c < 0) return done(fail("scan names an unknown component"));
                const int td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
                if (td > 3 || ta > 3 || !dc_ok[td] || !ac_ok[ta] || !qt_ok[ctq[c]]) return done(fail("missing table"));
                t.dc[c] = dc[td];
                t.ac[c] = ac[ta];
                memcpy(t.q[c], qt[ctq[c]], sizeof t.q[c]);
            }
            // (as jpegb: a component the scan header names twice leaves another without tables -- refuse that too)
            for (int c = 0; c < ncomp; c++) {
                bool named = false;
                for (int i = 0; i < n; i++) named = named || cid[c] == s[1 + 2 * i];
                if (!named) return done(fail("scan leaves a component out"));
            }
            if (ncomp == 3) {
                if (ch_[1] != 1 || cv[1] != 1 || ch_[2] != 1 || cv[2] != 1 || ch_[0] > 2 || cv[0] > 2 || (ch_[0] == 1 && cv[0] == 2))
                    return done(fail("unsupported chroma sampling"));
            } else ch_[0] = cv[0] = 1;
            for (int i = 0; i < 64; i++) t.zpos[kZigzag[i]] = (uint8_t)i;
            memset(&f, 0, sizeof f);
            f.W = W; f.H = H; f.ncomp = ncomp; f.hs = ch_[0]; f.vs = cv[0]; f.ri = ri;
            f.mcux = (W + 8 * f.hs - 1) / (8 * f.hs); f.mcuy = (H + 8 * f.vs - 1) / (8 * f.vs);
            f.bpm = ncomp == 3 ? f.hs * f.vs + 2 : 1;
            f.cw = (W + f.hs - 1) / f.hs; f.ch = (H + f.vs - 1) / f.vs;
            f.nblocks = (int64_t)f.mcux * f.mcuy * f.bpm;
            // the segment ends in front of the first marker that is neither stuffing, fill nor RSTn
            const uint8_t *q = se;
            while (q < end) {
                q = (const uint8_t *)memchr(q, 0xFF, (size_t)(end - q));
                if (!q) { q = end; break; }
                if (q + 1 >= end) { q = end; break; } // a lone 0xFF ends the file: part of the segment (dropped by byte_class)
                const int n2 = q[1];
                if (n2 == 0x00 || n2 == 0xFF || (n2 >= 0xD0 && n2 <= 0xD7)) { q += n2 == 0xFF ? 1 : 2; continue; }
                break;
            }
            f.scan_offset = (uint64_t)(se - file);
            f.scan_bytes = (uint64_t)(q - se);
            if (f.scan_bytes >= kMaxScanBytes) return done(fail("entropy-coded segment too long"));
            return done(0);
        }
        p += len;
    }
    return done(fail("no scan found"));
}

// The clean stream of scan[0 .. n): into clean (n + 8 bytes, the 8 behind the stream zero), the byte positions where
// restart intervals 1, 2, ... start into rst (at most max_rst).  Returns the clean bytes; *nrst the markers met.
inline size_t clean_host(const uint8_t *scan, size_t n, uint8_t *clean, uint32_t *rst, size_t max_rst, size_t *nrst)
{
    size_t o = 0, r = 0;
    for (size_t i = 0; i < n; i++) {
        const int cls = byte_class(i ? scan[i - 1] : 0, scan[i], i + 1 < n ? scan[i + 1] : 0);
        if (cls == 0) clean[o++] = scan[i];
        else if (cls == 2) { if (r < max_rst) rst[r] = (uint32_t)o; r++; }
    }
    memset(clean + o, 0, n + 8 - o);
    *nrst = r;
    return o;
}

// The symbols of the whole stream in order: coefficients into zz (nblocks * 64, zero before).  Returns the status word.
// Without restart intervals ONE stretch from (0, 0, 0); with them one stretch per interval from the byte its marker
// ends at to the next marker, a missing interval being a truncated stream.
inline int entropy_host(const Tables &t, const Frame &f, const uint32_t *words, size_t clean_bytes, const uint32_t *rst, size_t nrst, int16_t *zz)
{
    int status = 0;
    const uint32_t end = (uint32_t)clean_bytes * 8u;
    if (!f.ri) {
        State s{0u, 0, 0};
        CoefSink sink{zz, 0, f.nblocks};
        status = decode_stretch(t, f, words, end, s, end, f.nblocks, sink);
        if (sink.block < f.nblocks) status = kStatusTruncated;
        return status;
    }
    const int64_t nmcu = (int64_t)f.mcux * f.mcuy, nint = (nmcu + f.ri - 1) / f.ri;
    for (int64_t j = 0; j < nint; j++) {
        if (j > 0 && (size_t)(j - 1) >= nrst) { status = kStatusTruncated; break; }
        const uint32_t p0 = j ? rst[j - 1] * 8u : 0u, p1 = (size_t)j < nrst ? rst[j] * 8u : end;
        const int64_t b0 = j * f.ri * f.bpm, b1 = (j + 1) * f.ri < nmcu ? (j + 1) * f.ri * f.bpm : f.nblocks;
        State s{p0, 0, 0};
        CoefSink sink{zz, b0, b1};
        const int st = decode_stretch(t, f, words, p1, s, p1, b1, sink);
        status = st > status ? st : status;
        if (sink.block < b1) status = kStatusTruncated;
    }
    return status;
}

// Where block (bx, by) of component c's plane lies in the stream, and the MCU it belongs to.
HSD_FN int64_t stream_block(const Frame &f, int c, int bx, int by, int64_t *mcu)
{
    const int h = c ? 1 : f.hs, v = c ? 1 : f.vs;
    const int64_t m = (int64_t)(by / v) * f.mcux + bx / h;
    *mcu = m;
    return m * f.bpm + (c ? f.hs * f.vs + c - 1 : (by % v) * h + bx % h);
}

// The rule over one file in host memory: pix receives W x H pixels of 3 bytes, rows `stride` apart, R first (rgb != 0)
// or B first.  Returns 0, 1 (null pointer), 2 (stride below 3 * width), 4 (no memory), 7 (the file: header or stream).
// *status (may be null): the status word, 0 when the header was refused.  Writes exactly the picture's pixels, and none
// unless it returns 0.
inline int decode_host(const uint8_t *file, size_t bytes, int rgb, uint8_t *pix, size_t stride, Frame *frame, int *status, const char **why)
{
    if (status) *status = 0;
    if (!file || !pix) return 1;
    Frame f;
    Tables *t = (Tables *)malloc(sizeof(Tables));
    if (!t) return 4;
    int r = parse(file, bytes, f, *t, why);
    if (r) { free(t); return r; }
    if (frame) *frame = f;
    if (stride < (size_t)f.W * 3u) { free(t); return 2; }
    const size_t n = (size_t)f.scan_bytes;
    const int64_t nmcu = (int64_t)f.mcux * f.mcuy;
    const size_t max_rst = f.ri ? (size_t)((nmcu + f.ri - 1) / f.ri) : 0;
    uint32_t *words = (uint32_t *)malloc((n + 8 + 3) / 4 * 4);
    uint32_t *rst = (uint32_t *)malloc((max_rst + 1) * sizeof(uint32_t));
    int16_t *zz = (int16_t *)calloc((size_t)f.nblocks * 64u, sizeof(int16_t));
    uint8_t *planes = (uint8_t *)malloc((size_t)f.nblocks * 64u);
    auto done = [&](int rr) { free(t); free(words); free(rst); free(zz); free(planes); return rr; };
    if (!words || !rst || !zz || !planes) return done(4);
    size_t nrst = 0;
    const size_t clean_bytes = clean_host(file + f.scan_offset, n, (uint8_t *)words, rst, max_rst, &nrst);
    int st = entropy_host(*t, f, words, clean_bytes, rst, nrst, zz);
    // blocks: DC sums per component in stream order, dequantise, columns, rows, + 128, clamp
    const uint8_t *pl[3] = {nullptr, nullptr, nullptr};
    int strides[3] = {0, 0, 0};
    for (int c = 0; c < f.ncomp; c++) {
        pl[c] = planes + plane_block0(f, c) * 64;
        strides[c] = plane_wb(f, c) * 8;
    }
    uint32_t pred[3] = {0u, 0u, 0u};
    for (int64_t B = 0; B < f.nblocks; B++) {
        const int64_t m = B / f.bpm;
        const int b = (int)(B - m * f.bpm), c = comp_of_block(f, b);
        if (f.ri && b == 0 && m % f.ri == 0) pred[0] = pred[1] = pred[2] = 0u;
        pred[c] += (uint32_t)(int32_t)zz[B * 64];
        bool bad = false;
        int32_t d[64];
        for (int i = 0; i < 64; i++) d[i] = dequant(i ? (int32_t)zz[B * 64 + t->zpos[i]] : (int32_t)pred[c], t->q[c][i], &bad);
        if (bad) st = st > kStatusCorrupt ? st : kStatusCorrupt;
        for (int i = 0; i < 8; i++) idct_1d(d + i, 8, false);
        for (int i = 0; i < 8; i++) idct_1d(d + 8 * i, 1, true);
        const int h = c ? 1 : f.hs, v = c ? 1 : f.vs, s = c ? 0 : b;
        const int bx = (int)(m % f.mcux) * h + s % h, by = (int)(m / f.mcux) * v + s / h;
        uint8_t *o = planes + plane_block0(f, c) * 64 + (size_t)by * 8u * (size_t)strides[c] + (size_t)bx * 8u;
        for (int y = 0; y < 8; y++)
            for (int x = 0; x < 8; x++) o[(size_t)y * (size_t)strides[c] + (size_t)x] = (uint8_t)clamp255(d[8 * y + x] + 128);
    }
    if (status) *status = st;
    if (st) { if (why) *why = st == kStatusTruncated ? "truncated entropy-coded data" : "corrupt entropy-coded data"; return done(7); }
    for (int y = 0; y < f.H; y++) {
        uint8_t *o = pix + (size_t)y * stride;
        for (int x = 0; x < f.W; x++) {
            int32_t rr, gg, bb;
            pixel(f, pl, strides, x, y, &rr, &gg, &bb);
            o[3 * x] = (uint8_t)(rgb ? rr : bb); o[3 * x + 1] = (uint8_t)gg; o[3 * x + 2] = (uint8_t)(rgb ? bb : rr);
        }
    }
    return done(0);
}

} // namespace hsjpegd
