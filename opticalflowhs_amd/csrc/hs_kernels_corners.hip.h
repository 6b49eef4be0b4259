// hs_kernels_corners.hip.h -- corner detection on a u8 gray plane (hs_corners_rule.h) where the frames lie.  Six kernels
// behind one memset of the accumulators, launched one behind the other on one stream; the field is blockIdx.z, field i reads
// its own planes from an argument block by value and owns slice i of the scratch: a score plane of W * H int64, per 256
// pixels of a row (a SEGMENT) four ballot words and one offset word, kCnMaxCandidates candidates of 16 bytes, and the
// CnAcc record.  Every word of the scratch that a call reads it has written itself first, or the memset has.
//   k_cn_score     grid (ceil(W / 64), ceil(H / 16), fields), 256 lanes: a tile of the gray plane in LDS with a halo of
//                  block_r + 1, Sobel once per LDS pixel of the inner halo block_r, the window sums separable (rows, then
//                  columns), the score to the plane; the allowed pixels and their maximum reduced per wavefront, then per
//                  workgroup: ONE 64-bit atomicMax and ONE atomicAdd.
//   k_cn_suppress  grid (ceil(W / 256), ceil(H / 8), fields), 256 lanes: 256 x 8 scores in LDS with a halo of nms_r; a
//                  lane owns a column, a wavefront 64 pixels of a row; the survivors of a row are the wavefront's ballot
//                  word -- bit b of word 4 * segment + w is pixel 64 w + b of the segment: ascending index is the order of
//                  the bits.  The strong pixels are counted per workgroup, one atomicAdd.
//   k_cn_scan      ONE workgroup per field: the exclusive prefix sum of the segments' survivor counts (the population of
//                  their four words) in raster order; the total goes to CnAcc.
//   k_cn_compact   grid (ceil(W / 256), H, fields): survivor number k < max_candidates writes (score, index) as candidate k.
//   k_cn_rank      grid (kCnMaxCandidates / 256, 1, fields): one lane per candidate counts the candidates that rank in
//                  front of it, streaming the list through LDS kCnChunk at a time; that count IS its rank -- exact, whatever
//                  the order of execution -- and a rank below capacity writes its own record and xy slot.
//   k_cn_finish    the NaN tail of xy and the result header.
// No workgroup waits for another anywhere.  All quantities are integers: the outputs do not depend on the order of execution.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_corners_rule.h"

namespace hsk {

constexpr int kCnBatchMax = 8; // fields per launch: the scratch is a score plane per field
constexpr int kCnTileW = 64, kCnTileH = 16;  // k_cn_score
constexpr int kCnSegW = 256, kCnSupH = 8;    // k_cn_suppress: a segment wide, this many rows
constexpr int kCnScanRound = 1024;           // segments per round of k_cn_scan
constexpr int kCnChunk = 1024;               // candidates per LDS chunk of k_cn_rank
constexpr int kCnRankLanes = 256;            // candidates per workgroup of k_cn_rank
constexpr unsigned kCnMaxCandidates = hscn::kMaxCandidates;

// What the kernels of a field share between launches; zeroed by the memset in front of k_cn_score.
struct CnAcc {
    long long smax;
    unsigned long long allowed_px, strong_px;
    unsigned n_survivors, pad;
};
static_assert(sizeof(CnAcc) == 32, "CnAcc: 8-byte words for the 64-bit atomics");

struct CnCand {
    long long score;
    uint32_t index, pad;
};
static_assert(sizeof(CnCand) == 16, "a candidate is 16 bytes");

// The planes of a batch, handed to the kernels by value.
struct CnPlanes {
    const uint8_t *gray[kCnBatchMax];
    const uint8_t *mask[kCnBatchMax];   // or NULL: every pixel passes
    hscn::Record *records[kCnBatchMax]; // or NULL
    float *xy[kCnBatchMax];             // or NULL
    hscn::Result *results[kCnBatchMax]; // or NULL
    long long gs, ms;                   // strides in bytes: gray, mask
    int W, H;
    unsigned capacity;
    hscn::Rule rule;
    // the scratch: field i at score + i * plane, bits + i * 4 * n_segs, offsets + i * n_segs, cand + i * kCnMaxCandidates, acc + i
    long long *score;
    unsigned long long *bits;
    uint32_t *offsets;
    CnCand *cand;
    CnAcc *acc;
    long long plane, n_segs;
};
static_assert(sizeof(CnPlanes) + 64 <= 1024, "the argument block stays well inside the 4 KiB of kernel arguments");

#if defined(HS_CORNERS_KERNELS) // the kernels themselves: hs_corners_kernels.hip alone defines it

__device__ __forceinline__ long long cn_wave_max64(long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Grid: (ceil(W / 64), ceil(H / 16), fields); 256 lanes.
__global__ __launch_bounds__(256) void k_cn_score(const CnPlanes pl)
{
    constexpr int TW = kCnTileW, TH = kCnTileH, R = hscn::kMaxBlockR;
    constexpr int GW = TW + 2 * R + 2, GH = TH + 2 * R + 2; // the gray tile: halo block_r + 1
    constexpr int DW = TW + 2 * R, DH = TH + 2 * R;         // the gradients: halo block_r
    __shared__ uint8_t G[GH * GW];
    __shared__ int32_t D[DH * DW];     // Ix in the low half, Iy in the high half
    __shared__ int32_t RS[3][DH * TW]; // the row sums of Ix^2, Ix Iy, Iy^2
    __shared__ long long wmax[4];
    __shared__ unsigned wcnt[4];
    const unsigned i = blockIdx.z;
    const int W = pl.W, H = pl.H, r = pl.rule.block_r;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int gw = TW + 2 * r + 2, gh = TH + 2 * r + 2, dw = TW + 2 * r, dh = TH + 2 * r;
    const int gx0 = tx0 - r - 1, gy0 = ty0 - r - 1; // the frame coordinate of G's first byte (before clamping)
    const uint8_t *gray = pl.gray[i];
    for (int k = threadIdx.x; k < gw * gh; k += 256) {
        const int ly = k / gw, lx = k - ly * gw;
        G[ly * GW + lx] = gray[(long long)hscn::clampi(gy0 + ly, H - 1) * pl.gs + hscn::clampi(gx0 + lx, W - 1)];
    }
    __syncthreads();
    // the gradient at window place (xu, yu) is the gradient at the CLAMPED pixel, whose own neighbours are clamped again:
    // all of them lie inside G (the tile starts inside the frame, so a clamped pixel is at most block_r outside the tile)
    for (int k = threadIdx.x; k < dw * dh; k += 256) {
        const int ly = k / dw, lx = k - ly * dw;
        const int xc = hscn::clampi(tx0 - r + lx, W - 1), yc = hscn::clampi(ty0 - r + ly, H - 1);
        int nb[3][3];
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
            for (int a = 0; a < 3; a++) nb[b][a] = G[(hscn::clampi(yc + b - 1, H - 1) - gy0) * GW + hscn::clampi(xc + a - 1, W - 1) - gx0];
        int ix, iy;
        hscn::sobel(nb, &ix, &iy);
        D[ly * DW + lx] = (ix & 0xffff) | (int)((unsigned)iy << 16);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < TW * dh; k += 256) {
        const int ly = k / TW, lx = k - ly * TW;
        int a = 0, b = 0, c = 0;
        for (int d = 0; d <= 2 * r; d++) {
            const int w = D[ly * DW + lx + d];
            const int ix = (int)(short)(w & 0xffff), iy = w >> 16;
            a += ix * ix; b += ix * iy; c += iy * iy;
        }
        RS[0][k] = a; RS[1][k] = b; RS[2][k] = c;
    }
    __syncthreads();
    long long best = 0;
    unsigned cnt = 0;
    const uint8_t *mask = pl.mask[i];
    long long *score = pl.score + (long long)i * pl.plane;
#pragma unroll
    for (int k = 0; k < TW * TH / 256; k++) {
        const int ly = (int)(threadIdx.x >> 6) + 4 * k, lx = threadIdx.x & 63;
        const int x = tx0 + lx, y = ty0 + ly;
        if (x >= W || y >= H) continue;
        int a = 0, b = 0, c = 0;
        for (int d = 0; d <= 2 * r; d++) {
            a += RS[0][(ly + d) * TW + lx]; b += RS[1][(ly + d) * TW + lx]; c += RS[2][(ly + d) * TW + lx];
        }
        const long long s = hscn::score(pl.rule.kind, a, b, c);
        score[(long long)y * W + x] = s;
        const bool m = !mask || hscn::in_mask(mask[(long long)y * pl.ms + x], pl.rule.lo, pl.rule.hi);
        if (hscn::allowed(m, x, y, W, H, pl.rule.border)) {
            cnt++;
            best = s > best ? s : best;
        }
    }
    best = cn_wave_max64(best);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, d, 64);
    if ((threadIdx.x & 63u) == 0u) {
        wmax[threadIdx.x >> 6] = best;
        wcnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        long long m = wmax[0];
        unsigned n = wcnt[0];
        for (int q = 1; q < 4; q++) {
            m = wmax[q] > m ? wmax[q] : m;
            n += wcnt[q];
        }
        CnAcc &acc = pl.acc[i];
        if (m > 0) atomicMax(&acc.smax, m);
        if (n) atomicAdd(&acc.allowed_px, (unsigned long long)n);
    }
}

// Grid: (ceil(W / 256), ceil(H / 8), fields); 256 lanes, lane t owns column t of the segment.
__global__ __launch_bounds__(256) void k_cn_suppress(const CnPlanes pl)
{
    constexpr int SW = kCnSegW, SH = kCnSupH, R = hscn::kMaxNmsR;
    constexpr int LW = SW + 2 * R, LH = SH + 2 * R;
    __shared__ long long S[LH * LW];
    __shared__ unsigned wstrong[4];
    const unsigned i = blockIdx.z;
    const int W = pl.W, H = pl.H, r = pl.rule.nms_r;
    const int x0 = blockIdx.x * SW, y0 = blockIdx.y * SH;
    const int lw = SW + 2 * r, lh = SH + 2 * r;
    const long long *score = pl.score + (long long)i * pl.plane;
    for (int k = threadIdx.x; k < lw * lh; k += 256) {
        const int ly = k / lw, lx = k - ly * lw;
        const int x = x0 - r + lx, y = y0 - r + ly;
        S[ly * LW + lx] = x >= 0 && x < W && y >= 0 && y < H ? score[(long long)y * W + x] : hscn::kNoScore;
    }
    __syncthreads();
    const CnAcc &acc = pl.acc[i];
    const long long T = hscn::threshold(acc.smax, pl.rule.min_score, pl.rule.quality_q16);
    const uint8_t *mask = pl.mask[i];
    const int x = x0 + (int)threadIdx.x;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long *bits = pl.bits + (long long)i * 4 * pl.n_segs;
    unsigned strong = 0;
    for (int ry = 0; ry < SH; ry++) {
        const int y = y0 + ry;
        if (y >= H) break; // (uniform)
        bool alive = false;
        if (x < W) {
            const long long sp = S[(ry + r) * LW + (int)threadIdx.x + r];
            const bool m = !mask || hscn::in_mask(mask[(long long)y * pl.ms + x], pl.rule.lo, pl.rule.hi);
            if (sp >= T && hscn::allowed(m, x, y, W, H, pl.rule.border)) {
                strong++;
                alive = true;
                for (int dy = -r; dy <= r && alive; dy++)
                    for (int dx = -r; dx <= r; dx++) {
                        if (dx == 0 && dy == 0) continue;
                        if (hscn::loses_to(sp, S[(ry + r + dy) * LW + (int)threadIdx.x + r + dx], dy < 0 || (dy == 0 && dx < 0))) {
                            alive = false;
                            break;
                        }
                    }
            }
        }
        const unsigned long long votes = __ballot(alive);
        if (lane == 0u) bits[((long long)y * gridDim.x + blockIdx.x) * 4 + wave] = votes;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) strong += (unsigned)__shfl_xor((int)strong, d, 64);
    if (lane == 0u) wstrong[wave] = strong;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const unsigned n = wstrong[0] + wstrong[1] + wstrong[2] + wstrong[3];
        if (n) atomicAdd(&pl.acc[i].strong_px, (unsigned long long)n);
    }
}

// Grid: (1, 1, fields); 1024 lanes, kCnScanRound segments per round.  offsets[k] = the survivors in front of segment k.
__global__ __launch_bounds__(1024) void k_cn_scan(const CnPlanes pl)
{
    const unsigned i = blockIdx.z;
    const unsigned long long *bits = pl.bits + (long long)i * 4 * pl.n_segs;
    uint32_t *offsets = pl.offsets + (long long)i * pl.n_segs;
    __shared__ unsigned wsum[16];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned carry = 0u;
    for (long long base = 0; base < pl.n_segs; base += kCnScanRound) {
        const long long k = base + threadIdx.x;
        unsigned mine = 0u;
        if (k < pl.n_segs) mine = (unsigned)(__popcll(bits[4 * k]) + __popcll(bits[4 * k + 1]) + __popcll(bits[4 * k + 2]) + __popcll(bits[4 * k + 3]));
        unsigned incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = (unsigned)__shfl_up((int)incl, d, 64);
            if (lane >= (unsigned)d) incl += o;
        }
        __syncthreads(); // (the last round's wsum has been read)
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        unsigned before = 0u, total = 0u;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            before += (unsigned)q < wave ? wsum[q] : 0u;
            total += wsum[q];
        }
        if (k < pl.n_segs) offsets[k] = carry + before + incl - mine;
        carry += total;
    }
    if (threadIdx.x == 0u) pl.acc[i].n_survivors = carry;
}

// Grid: (ceil(W / 256), H, fields); 256 lanes, one pixel each.
__global__ __launch_bounds__(256) void k_cn_compact(const CnPlanes pl)
{
    const unsigned i = blockIdx.z;
    const long long seg = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned long long *b = pl.bits + ((long long)i * pl.n_segs + seg) * 4;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long mine = b[wave];
    if (!((mine >> lane) & 1ull)) return;
    unsigned k = pl.offsets[(long long)i * pl.n_segs + seg] + (unsigned)__popcll(mine & ((1ull << lane) - 1ull));
    for (unsigned q = 0; q < wave; q++) k += (unsigned)__popcll(b[q]);
    if (k >= pl.rule.max_candidates) return;
    const uint32_t index = (uint32_t)((long long)blockIdx.y * pl.W + blockIdx.x * kCnSegW + threadIdx.x);
    CnCand c;
    c.score = pl.score[(long long)i * pl.plane + index];
    c.index = index;
    c.pad = 0u;
    pl.cand[(long long)i * kCnMaxCandidates + k] = c;
}

// Grid: (kCnMaxCandidates / 256, 1, fields); 256 lanes, one candidate each.  The list is in ascending index, so "the smaller
// index" is "the earlier place".
__global__ __launch_bounds__(kCnRankLanes) void k_cn_rank(const CnPlanes pl)
{
    __shared__ long long Ls[kCnChunk];
    const unsigned i = blockIdx.z;
    const CnAcc &acc = pl.acc[i];
    const unsigned n = acc.n_survivors < pl.rule.max_candidates ? acc.n_survivors : pl.rule.max_candidates;
    if (blockIdx.x * kCnRankLanes >= n) return; // (uniform)
    const CnCand *cand = pl.cand + (long long)i * kCnMaxCandidates;
    const unsigned me = blockIdx.x * kCnRankLanes + threadIdx.x;
    const bool live = me < n;
    const long long s = live ? cand[me].score : 0;
    unsigned rank = 0u;
    for (unsigned base = 0; base < n; base += kCnChunk) {
        const unsigned len = n - base < (unsigned)kCnChunk ? n - base : (unsigned)kCnChunk;
        __syncthreads(); // (the last chunk has been read)
        for (unsigned k = threadIdx.x; k < len; k += kCnRankLanes) Ls[k] = cand[base + k].score;
        __syncthreads();
        // in front of me: a larger score anywhere, an equal one at an earlier place
        const unsigned eq_end = me > base ? (me - base < len ? me - base : len) : 0u;
        for (unsigned k = 0; k < len; k++) rank += (unsigned)(Ls[k] > s) + (unsigned)(k < eq_end && Ls[k] == s);
    }
    if (!live || rank >= pl.capacity) return;
    const uint32_t index = cand[me].index;
    hscn::Record rec;
    hscn::write_record(&rec, index, pl.W, s);
    if (pl.records[i]) pl.records[i][rank] = rec;
    if (pl.xy[i]) {
        pl.xy[i][2 * (long long)rank] = (float)rec.x;
        pl.xy[i][2 * (long long)rank + 1] = (float)rec.y;
    }
}

// Grid: (ceil(max(capacity, 1) / 256), 1, fields); 256 lanes, one xy slot each; lane 0 of block 0 writes the result.
__global__ __launch_bounds__(256) void k_cn_finish(const CnPlanes pl)
{
    const unsigned i = blockIdx.z;
    const CnAcc &acc = pl.acc[i];
    hscn::Result r;
    hscn::finish_result(&r, acc.n_survivors, pl.rule.max_candidates, pl.capacity, acc.smax, hscn::threshold(acc.smax, pl.rule.min_score, pl.rule.quality_q16),
                        acc.allowed_px, acc.strong_px);
    const unsigned k = blockIdx.x * 256 + threadIdx.x;
    if (pl.xy[i] && k >= r.n_written && k < pl.capacity) {
        uint32_t *w = (uint32_t *)pl.xy[i] + 2 * (long long)k;
        w[0] = hscn::kNanBits;
        w[1] = hscn::kNanBits;
    }
    if (k == 0u && pl.results[i]) *pl.results[i] = r;
}

#endif // HS_CORNERS_KERNELS

// hs_corners_kernels.hip: the memset, the kernels and their launches, in the order of a call.
hipError_t launch_corners(hipStream_t stream, const CnPlanes &pl, int fields);

} // namespace hsk
