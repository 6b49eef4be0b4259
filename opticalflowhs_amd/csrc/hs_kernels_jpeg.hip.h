// hs_kernels_jpeg.hip.h -- the baseline-JPEG file of an RGB picture in device memory, encoded where the picture lies:
// what cvSaveImage does at the end of the reference's runFromImg (OpticalFlowOpenCV.cpp:47, HSOpticalFlowOpenCL.cpp:771).
// The arithmetic is hs_jpeg_rule.h's, shared with the host twin; this file is the data movement around it.  Nothing
// crosses to the host between the first and the last launch, every grid is sized from W, H and the bound, and the bytes
// do not depend on the order of execution:
//   k_jpeg_blocks    one workgroup per strip of 8 MCUs: the 128 x 16 pixels read once (plus the replicated edge), Y and
//                    the averaged Cb, Cr into LDS, then eight lanes per 8x8 block: row pass in registers, transpose
//                    through LDS, column pass, quantise, zigzag; 128 B of int16 per block out with 16-byte stores
//   k_jpeg_lengths   one lane per block: its bit length (block_bits into a counting sink)
//   k_jpeg_scan      exclusive prefix sums, one workgroup: the blocks' bit offsets, later the chunks' stuffing offsets
//   k_jpeg_emit      one lane per block: its bits into the zeroed raw stream at its offset -- whole words stored, the
//                    two words it may share with its neighbours merged with atomicOr (OR commutes: deterministic);
//                    the last block's lane adds the 1-bits up to a whole byte
//   k_jpeg_count_ff  one lane per 128-byte chunk of the raw stream: its 0xFF bytes
//   k_jpeg_stuff     header + stuffed bytes + FF D9 + the total; nothing at or beyond `capacity` is written
// Each kernel's work for one picture is a __device__ body.  The entries above call it with their by-value arguments;
// the k_jpeg_*_batch entries take the picture from a further grid dimension and call the same body: picture i's scratch
// is slice i of one allocation (JpegBatchScratch, laid out by hs_jpeg_batch_plan.h), and what differs from picture to
// picture -- source, `wide`, output, capacity -- comes from an argument block by value (JpegBatchPics).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_jpeg_rule.h"

namespace hsk {

constexpr int kJpegStripMcus = 8;   // MCUs per workgroup of k_jpeg_blocks
constexpr int kJpegScanLanes = 1024;
constexpr int kJpegScanPer = 4;     // consecutive entries per lane and tile of k_jpeg_scan
constexpr int kJpegChunk = 128;     // bytes of raw stream per lane of the two stuffing kernels
constexpr int kJpegBatchMax = 32;   // pictures per set of launches (HSFLOW_JPEG_BATCH_MAX is at most this)

// One picture of a batch: 32 bytes.
struct JpegBatchPic {
    const uint8_t *rgb;          // the picture, rows `stride` bytes apart
    uint8_t *out;                // its file
    unsigned long long capacity; // bytes of `out`
    int wide, pad;               // rgb and the stride are multiples of 4
};
struct JpegBatchPics {
    JpegBatchPic p[kJpegBatchMax];
};

// The scratch of a chunk: the ranges' first slices and the bytes from one picture's slice to the next one's.
struct JpegBatchScratch {
    uint8_t *coef, *raw, *off, *ffoff, *len, *ff;
    unsigned long long s_coef, s_raw, s_off, s_ffoff, s_len, s_ff;
    __device__ __forceinline__ int16_t *coef_of(unsigned i) const { return (int16_t *)(coef + i * s_coef); }
    __device__ __forceinline__ uint32_t *raw_of(unsigned i) const { return (uint32_t *)(raw + i * s_raw); }
    __device__ __forceinline__ uint64_t *off_of(unsigned i) const { return (uint64_t *)(off + i * s_off); }
    __device__ __forceinline__ uint64_t *ffoff_of(unsigned i) const { return (uint64_t *)(ffoff + i * s_ffoff); }
    __device__ __forceinline__ uint32_t *len_of(unsigned i) const { return (uint32_t *)(len + i * s_len); }
    __device__ __forceinline__ uint32_t *ff_of(unsigned i) const { return (uint32_t *)(ff + i * s_ff); }
};

// Four pixels x .. x + 3 of row `row` (already clamped to the picture); columns clamped to the picture.  wide: the row's
// base and 3 * x are multiples of 4 and x + 4 <= W -- three aligned words.
__device__ __forceinline__ void jpeg_load4(const uint8_t *__restrict__ row, int x, int W, bool wide, int32_t r[4], int32_t g[4], int32_t b[4])
{
    if (wide) {
        const uint32_t *p = (const uint32_t *)(row + 3ll * x);
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
        r[0] = w0 & 255u; g[0] = (w0 >> 8) & 255u; b[0] = (w0 >> 16) & 255u;
        r[1] = w0 >> 24; g[1] = w1 & 255u; b[1] = (w1 >> 8) & 255u;
        r[2] = (w1 >> 16) & 255u; g[2] = w1 >> 24; b[2] = w2 & 255u;
        r[3] = (w2 >> 8) & 255u; g[3] = (w2 >> 16) & 255u; b[3] = w2 >> 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint8_t *p = row + 3ll * hsjpeg::clamp_hi(x + j, W);
            r[j] = p[0]; g[j] = p[1]; b[j] = p[2];
        }
    }
}

// rgb: W x H pixels, rows `stride` bytes apart.  coef: 64 int16 per block, block b = 6 * (my * MW + mx) + k.
// Grid: (ceil(MW / 8), MH), 256 lanes.  wide != 0: rgb and stride are multiples of 4.
__device__ __forceinline__ void jpeg_blocks_body(const uint8_t *__restrict__ rgb, long long stride, int W, int H, int MW,
                                                 const hsjpeg::Tables *__restrict__ tab, int16_t *__restrict__ coef, int wide)
{
    constexpr int S = kJpegStripMcus;
    __shared__ uint32_t sY[16][4 * S + 1];      // 16 rows of 128 luma samples, 4 to a word; the odd stride spreads the rows over the banks
    __shared__ uint16_t sC[2][8][4 * S + 2];    // Cb, Cr: 8 rows of 64 samples, 2 to a halfword, rows 68 bytes apart
    __shared__ int32_t sT[32][72];              // per block in flight: 8 rows of 8 behind the row pass, row stride 9
    __shared__ __attribute__((aligned(16))) int16_t sZ[32][64]; // ... and its zigzag coefficients
    const int t = threadIdx.x, my = blockIdx.y, mx0 = blockIdx.x * S;

    {   // phase 1: lane = a patch of 4 x 2 pixels; 32 patches across, 8 down
        const int px = t & 31, py = t >> 5;
        if (mx0 + (px >> 2) < MW) {
            const int x = 16 * mx0 + 4 * px, y = 16 * my + 2 * py;
            const bool w4 = wide && x + 4 <= W;
            int32_t r[2][4], g[2][4], b[2][4];
#pragma unroll
            for (int dy = 0; dy < 2; dy++) {
                jpeg_load4(rgb + (long long)hsjpeg::clamp_hi(y + dy, H) * stride, x, W, w4, r[dy], g[dy], b[dy]);
                uint32_t yw = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) yw |= (uint32_t)hsjpeg::ycc_y(r[dy][j], g[dy][j], b[dy][j]) << (8 * j);
                sY[2 * py + dy][px] = yw;
            }
            const int cy = 8 * my + py, rr = hsjpeg::chroma_rows(H);
            if (cy >= rr) { // below the downsampled plane's last averaged row: that row again, from its own two picture rows
#pragma unroll
                for (int dy = 0; dy < 2; dy++)
                    jpeg_load4(rgb + (long long)hsjpeg::clamp_hi(2 * (rr - 1) + dy, H) * stride, x, W, w4, r[dy], g[dy], b[dy]);
            }
            uint32_t cbw = 0, crw = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                int32_t sb = 0, sr = 0;
#pragma unroll
                for (int dy = 0; dy < 2; dy++)
#pragma unroll
                    for (int dx = 0; dx < 2; dx++) {
                        sb += hsjpeg::ycc_cb(r[dy][2 * h + dx], g[dy][2 * h + dx], b[dy][2 * h + dx]);
                        sr += hsjpeg::ycc_cr(r[dy][2 * h + dx], g[dy][2 * h + dx], b[dy][2 * h + dx]);
                    }
                cbw |= (uint32_t)hsjpeg::chroma_avg(sb, h) << (8 * h); // (the chroma column 8 * mx0 + 2 * px + h has h's parity)
                crw |= (uint32_t)hsjpeg::chroma_avg(sr, h) << (8 * h);
            }
            sC[0][py][px] = (uint16_t)cbw;
            sC[1][py][px] = (uint16_t)crw;
        }
    }
    __syncthreads();

    // phase 2: eight lanes per block, lane r holds row r, then column r; 32 blocks in flight, 48 in the strip
    const int lb = t >> 3, r = t & 7;
    for (int it = 0; it < 2; it++) {
        const int blk = 32 * it + lb, s = blk / 6, k = blk - 6 * s, mx = mx0 + s;
        const bool live = blk < 6 * S && mx < MW;
        const bool real = live && !(k < 4 && hsjpeg::luma_dummy(W, H, mx, my, k));
        int32_t d[8];
        if (real) {
            uint32_t w0, w1;
            if (k < 4) {
                const uint32_t *p = &sY[8 * (k >> 1) + r][4 * s + 2 * (k & 1)];
                w0 = p[0]; w1 = p[1];
            } else {
                const uint16_t *p = &sC[k - 4][r][4 * s];
                w0 = p[0] | (uint32_t)p[1] << 16; w1 = p[2] | (uint32_t)p[3] << 16;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                d[j] = (int32_t)((w0 >> (8 * j)) & 255u) - 128;
                d[4 + j] = (int32_t)((w1 >> (8 * j)) & 255u) - 128;
            }
            hsjpeg::fdct_1d(d, 1, false);
#pragma unroll
            for (int j = 0; j < 8; j++) sT[lb][9 * r + j] = d[j];
        }
        __syncthreads();
        if (real) {
#pragma unroll
            for (int i = 0; i < 8; i++) d[i] = sT[lb][9 * i + r];
            hsjpeg::fdct_1d(d, 1, true);
            const int tbl = k < 4 ? 0 : 1;
#pragma unroll
            for (int i = 0; i < 8; i++) sZ[lb][tab->zpos[8 * i + r]] = (int16_t)hsjpeg::quantise(d[i], tab->q[tbl][8 * i + r]);
        }
        __syncthreads();
        if (live) {
            const long long b = 6ll * ((long long)my * MW + mx) + k;
            const uint4 z = real ? *(const uint4 *)&sZ[lb][8 * r] : make_uint4(0u, 0u, 0u, 0u); // a dummy block: no AC (its DC: block_dc)
            *(uint4 *)(coef + b * 64 + 8 * r) = z;
        }
    }
}

__global__ __launch_bounds__(256) void k_jpeg_blocks(const uint8_t *__restrict__ rgb, long long stride, int W, int H, int MW,
                                                     const hsjpeg::Tables *__restrict__ tab, int16_t *__restrict__ coef, int wide)
{
    jpeg_blocks_body(rgb, stride, W, H, MW, tab, coef, wide);
}

// Grid: (ceil(MW / 8), MH, pictures).
__global__ __launch_bounds__(256) void k_jpeg_blocks_batch(const JpegBatchPics pics, long long stride, int W, int H, int MW,
                                                           const hsjpeg::Tables *__restrict__ tab, const JpegBatchScratch sc)
{
    const unsigned i = blockIdx.z;
    jpeg_blocks_body(pics.p[i].rgb, stride, W, H, MW, tab, sc.coef_of(i), pics.p[i].wide);
}

// len[b]: the bits of block b, at most hsjpeg::kMaxBlockBits.
__device__ __forceinline__ void jpeg_lengths_body(const hsjpeg::Tables *__restrict__ tab, const int16_t *__restrict__ coef, int W, int H, int MW,
                                                  long long nb, uint32_t *__restrict__ len)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const long long m = b / 6;
    const int k = (int)(b - 6 * m);
    const bool dummy = k < 4 && hsjpeg::luma_dummy(W, H, (int)(m % MW), (int)(m / MW), k);
    hsjpeg::CountSink sink;
    hsjpeg::block_bits(*tab, k < 4 ? 0 : 1, coef + b * 64, hsjpeg::block_dc(coef, W, H, MW, b), hsjpeg::block_pred(coef, W, H, MW, b), dummy, sink);
    len[b] = sink.bits;
}

__global__ __launch_bounds__(256) void k_jpeg_lengths(const hsjpeg::Tables *__restrict__ tab, const int16_t *__restrict__ coef, int W, int H, int MW,
                                                      long long nb, uint32_t *__restrict__ len)
{
    jpeg_lengths_body(tab, coef, W, H, MW, nb, len);
}

// Grid: (ceil(nb / 256), pictures).
__global__ __launch_bounds__(256) void k_jpeg_lengths_batch(const hsjpeg::Tables *__restrict__ tab, const JpegBatchScratch sc, int W, int H, int MW,
                                                            long long nb)
{
    const unsigned i = blockIdx.y;
    jpeg_lengths_body(tab, sc.coef_of(i), W, H, MW, nb, sc.len_of(i));
}

// out[i] = in[0] + ... + in[i - 1] for i = 0 .. n (n + 1 entries: out[n] is the total).  One workgroup of 1024 lanes:
// tiles of 4096 entries behind each other, wave shuffles inside a wave, LDS across the 16 waves, a running carry.
// raw_bits != nullptr: in[] are per-chunk counts over a raw stream of *raw_bits bits, and n shrinks to the chunks that
// stream reaches (jpeg_chunks_used).
__device__ __forceinline__ long long jpeg_chunks_used(uint64_t raw_bits, long long nchunks)
{
    const uint64_t used = ((raw_bits + 7u) / 8u + (uint64_t)kJpegChunk - 1u) / (uint64_t)kJpegChunk;
    return used < (uint64_t)nchunks ? (long long)used : nchunks;
}

// (the body: k_jpeg_scan's and, one workgroup per file, k_jpegd_scan_batch's in hs_kernels_jpegd.hip.h)
__device__ __forceinline__ void jpeg_scan_body(const uint32_t *__restrict__ in, uint64_t *__restrict__ out, long long n,
                                               const uint64_t *__restrict__ raw_bits)
{
    __shared__ uint32_t sWave[16], sExcl[17];
    if (raw_bits) n = jpeg_chunks_used(*raw_bits, n);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint64_t carry = 0;
    for (long long base = 0; base < n; base += kJpegScanLanes * kJpegScanPer) {
        const long long i0 = base + (long long)t * kJpegScanPer;
        uint32_t v[kJpegScanPer], s = 0;
#pragma unroll
        for (int j = 0; j < kJpegScanPer; j++) { v[j] = i0 + j < n ? in[i0 + j] : 0u; s += v[j]; }
        uint32_t incl = s; // (a tile's total is below 4096 * 1660 < 2^23)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        if (t == 0) {
            uint32_t a = 0;
            for (int w = 0; w < 16; w++) { sExcl[w] = a; a += sWave[w]; }
            sExcl[16] = a;
        }
        __syncthreads();
        uint64_t e = carry + sExcl[wave] + (incl - s);
#pragma unroll
        for (int j = 0; j < kJpegScanPer; j++) {
            if (i0 + j < n) out[i0 + j] = e;
            e += v[j];
        }
        carry += sExcl[16];
        __syncthreads(); // sWave and sExcl are free again
    }
    if (t == 0) out[n] = carry;
}

__global__ __launch_bounds__(kJpegScanLanes) void k_jpeg_scan(const uint32_t *__restrict__ in, uint64_t *__restrict__ out, long long n,
                                                             const uint64_t *__restrict__ raw_bits)
{
    jpeg_scan_body(in, out, n, raw_bits);
}

// One workgroup per picture (grid = pictures).  second == 0: the nb blocks' bit lengths into their offsets; otherwise
// the nchunks chunks' 0xFF counts into their stuffing offsets, over the chunks the picture's raw stream reaches.
__global__ __launch_bounds__(kJpegScanLanes) void k_jpeg_scan_batch(const JpegBatchScratch sc, long long nb, long long nchunks, int second)
{
    const unsigned i = blockIdx.x;
    if (!second) jpeg_scan_body(sc.len_of(i), sc.off_of(i), nb, (const uint64_t *)nullptr);
    else jpeg_scan_body(sc.ff_of(i), sc.ffoff_of(i), nchunks, sc.off_of(i) + nb);
}

// A block's bits into the raw stream from bit `pos` on.  Stream bit i is bit 7 - i % 8 of byte i / 8; a word is
// assembled with its first stream bit on top and byte-swapped into memory order.  Words that hold bits of this block
// alone are stored; the first word when the block starts inside it, and the last when it ends inside it, are OR-ed
// into the zeroed stream.
struct JpegEmitSink {
    uint32_t *words;
    uint64_t widx;
    uint32_t cur = 0;
    int fill;
    bool shared; // the word in hand began with a neighbour's bits
    __device__ JpegEmitSink(uint32_t *w, uint64_t pos) : words(w), widx(pos >> 5), fill((int)(pos & 31u)), shared((pos & 31u) != 0) {}
    __device__ __forceinline__ void flush_full()
    {
        const uint32_t m = __builtin_bswap32(cur);
        if (shared) atomicOr(words + widx, m);
        else words[widx] = m;
        widx++; cur = 0; fill = 0; shared = false;
    }
    __device__ __forceinline__ void put(uint32_t code, int size)
    {
        const int room = 32 - fill;
        if (size <= room) {
            cur |= code << (room - size);
            fill += size;
            if (fill == 32) flush_full();
        } else {
            const int rest = size - room;
            cur |= code >> rest;
            flush_full();
            cur = code << (32 - rest);
            fill = rest;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (fill) atomicOr(words + widx, __builtin_bswap32(cur));
    }
};

// raw: the raw stream, zero before; off[b]: block b's bit offset, off[nb] the total.
__device__ __forceinline__ void jpeg_emit_body(const hsjpeg::Tables *__restrict__ tab, const int16_t *__restrict__ coef, int W, int H, int MW,
                                               long long nb, const uint64_t *__restrict__ off, uint32_t *__restrict__ raw)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const long long m = b / 6;
    const int k = (int)(b - 6 * m);
    const bool dummy = k < 4 && hsjpeg::luma_dummy(W, H, (int)(m % MW), (int)(m / MW), k);
    JpegEmitSink sink(raw, off[b]);
    hsjpeg::block_bits(*tab, k < 4 ? 0 : 1, coef + b * 64, hsjpeg::block_dc(coef, W, H, MW, b), hsjpeg::block_pred(coef, W, H, MW, b), dummy, sink);
    if (b == nb - 1) { // 1-bits up to a whole byte
        const int pad = (int)((0u - (uint32_t)off[nb]) & 7u);
        if (pad) sink.put((1u << pad) - 1u, pad);
    }
    sink.finish();
}

__global__ __launch_bounds__(256) void k_jpeg_emit(const hsjpeg::Tables *__restrict__ tab, const int16_t *__restrict__ coef, int W, int H, int MW,
                                                   long long nb, const uint64_t *__restrict__ off, uint32_t *__restrict__ raw)
{
    jpeg_emit_body(tab, coef, W, H, MW, nb, off, raw);
}

// Grid: (ceil(nb / 256), pictures).
__global__ __launch_bounds__(256) void k_jpeg_emit_batch(const hsjpeg::Tables *__restrict__ tab, const JpegBatchScratch sc, int W, int H, int MW,
                                                         long long nb)
{
    const unsigned i = blockIdx.y;
    jpeg_emit_body(tab, sc.coef_of(i), W, H, MW, nb, sc.off_of(i), sc.raw_of(i));
}

__device__ __forceinline__ uint32_t jpeg_ff_in_word(uint32_t w)
{
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) n += ((w >> (8 * j)) & 255u) == 255u;
    return n;
}

// cnt[c]: the 0xFF bytes of chunk c of the raw stream, for the chunks the stream reaches (it is zero behind its end).
__device__ __forceinline__ void jpeg_count_ff_body(const uint32_t *__restrict__ raw, const uint64_t *__restrict__ raw_bits, long long nchunks,
                                                   uint32_t *__restrict__ cnt)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= jpeg_chunks_used(*raw_bits, nchunks)) return;
    const uint4 *p = (const uint4 *)(raw + c * (kJpegChunk / 4));
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < kJpegChunk / 16; i++) {
        const uint4 w = p[i];
        n += jpeg_ff_in_word(w.x) + jpeg_ff_in_word(w.y) + jpeg_ff_in_word(w.z) + jpeg_ff_in_word(w.w);
    }
    cnt[c] = n;
}

__global__ __launch_bounds__(256) void k_jpeg_count_ff(const uint32_t *__restrict__ raw, const uint64_t *__restrict__ raw_bits, long long nchunks,
                                                       uint32_t *__restrict__ cnt)
{
    jpeg_count_ff_body(raw, raw_bits, nchunks, cnt);
}

// Grid: (ceil(nchunks / 256), pictures).
__global__ __launch_bounds__(256) void k_jpeg_count_ff_batch(const JpegBatchScratch sc, long long nb, long long nchunks)
{
    const unsigned i = blockIdx.y;
    jpeg_count_ff_body(sc.raw_of(i), sc.off_of(i) + nb, nchunks, sc.ff_of(i));
}

// The file: header, the raw stream with 0x00 behind every 0xFF (chunk c's bytes start ffoff[c] later than unstuffed),
// FF D9.  *total: the file's size, whatever `capacity`; bytes at or beyond capacity are not written.
__device__ __forceinline__ void jpeg_stuff_body(const hsjpeg::Tables *__restrict__ tab, const uint32_t *__restrict__ raw, const uint64_t *__restrict__ raw_bits,
                                                const uint64_t *__restrict__ ffoff, long long nchunks, uint8_t *__restrict__ out,
                                                unsigned long long capacity, uint64_t *__restrict__ total)
{
    const unsigned long long raw_bytes = (*raw_bits + 7u) / 8u;
    const long long used = jpeg_chunks_used(*raw_bits, nchunks);
    if (blockIdx.x == 0) {
        for (unsigned i = threadIdx.x; i < (unsigned)hsjpeg::kHeaderBytes; i += 256u)
            if (i < capacity) out[i] = tab->header[i];
        if (threadIdx.x == 0) {
            const unsigned long long end = (unsigned long long)hsjpeg::kHeaderBytes + raw_bytes + ffoff[used];
            if (end < capacity) out[end] = 0xFF;
            if (end + 1 < capacity) out[end + 1] = 0xD9;
            *total = end + 2;
        }
    }
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= used) return;
    unsigned long long src = (unsigned long long)c * kJpegChunk, pos = (unsigned long long)hsjpeg::kHeaderBytes + src + ffoff[c];
    const uint4 *p = (const uint4 *)(raw + c * (kJpegChunk / 4));
    for (int i = 0; i < kJpegChunk / 16; i++) {
        const uint4 q = p[i];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t v = (w[j >> 2] >> (8 * (j & 3))) & 255u;
            if (src < raw_bytes) {
                if (pos < capacity) out[pos] = (uint8_t)v;
                pos++;
                if (v == 255u) {
                    if (pos < capacity) out[pos] = 0;
                    pos++;
                }
            }
            src++;
        }
    }
}

__global__ __launch_bounds__(256) void k_jpeg_stuff(const hsjpeg::Tables *__restrict__ tab, const uint32_t *__restrict__ raw, const uint64_t *__restrict__ raw_bits,
                                                    const uint64_t *__restrict__ ffoff, long long nchunks, uint8_t *__restrict__ out,
                                                    unsigned long long capacity, uint64_t *__restrict__ total)
{
    jpeg_stuff_body(tab, raw, raw_bits, ffoff, nchunks, out, capacity, total);
}

// Grid: (ceil(nchunks / 256), pictures).  total: the chunk's size words, picture i's is total[i].
__global__ __launch_bounds__(256) void k_jpeg_stuff_batch(const hsjpeg::Tables *__restrict__ tab, const JpegBatchScratch sc, long long nb, long long nchunks,
                                                          const JpegBatchPics pics, uint64_t *__restrict__ total)
{
    const unsigned i = blockIdx.y;
    jpeg_stuff_body(tab, sc.raw_of(i), sc.off_of(i) + nb, sc.ffoff_of(i), nchunks, pics.p[i].out, pics.p[i].capacity, total + i);
}

} // namespace hsk
