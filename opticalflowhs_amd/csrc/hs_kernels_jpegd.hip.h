// hs_kernels_jpegd.hip.h -- a baseline-JPEG file's entropy-coded segment in device memory, decoded where the frame is
// wanted: what cvLoadImage does in front of the reference's runFromImg (OpticalFlowOpenCV.cpp:15,18,
// HSOpticalFlowOpenCL.cpp:721,732).  The arithmetic is hs_jpegd_rule.h's, shared with the host twin; this file is the
// data movement around it.  Nothing crosses to the host between the first and the last launch, every grid is sized from
// the header, no kernel waits on another workgroup, and the pixels do not depend on the order of execution:
//   k_jpegd_clean_batch<0> one lane per 128-byte chunk of the segment: the bytes byte_class drops, the RSTn markers
//   k_jpegd_scan_batch<0>  (jpeg_scan_body, hs_kernels_jpeg.hip.h) where a chunk's kept bytes go, which marker is its first
//   k_jpegd_clean_batch<1> the clean stream (zero behind its end), and the byte each restart interval starts at
// without restart intervals, the stream cut into subsequences of S bits, one lane each:
//   k_jpegd_sync_batch     256 subsequences per workgroup.  Round 0: every lane decodes from (its first bit, block 0, DC) to
//                    the first symbol at or beyond its last bit and keeps its exit state in LDS; later rounds: a lane whose
//                    predecessor's exit state is not what it started from starts again from that; until a round changes
//                    nothing.  Afterwards a group is right if its first lane's start is.
//   k_jpegd_repair_batch   ONE workgroup per file, lane g for group g: from group g - 1's last exit state through its own
//                    subsequences until it meets a stored start state it agrees with; rounds over __syncthreads until
//                    nothing changes.  Subsequence 0 starts from the true state, so round r leaves at least r + 1 groups right.
//   k_jpegd_scan_batch<2>  the blocks that end in a subsequence -> the first block of each
//   k_jpegd_write_batch    one lane per subsequence from its now-true start state: coefficients into the zeroed int16
//                    buffer, DC as the difference; the only entropy pass that raises the status word
// with them:
//   k_jpegd_write_rst_batch one lane per interval: start bit, first block and DC reset are known
// then for both:
//   k_jpegd_dc_gather_batch + k_jpegd_scan_batch<3>  the DC differences by component in stream order, their prefix sums
//                    (mod 2^32)
//   k_jpegd_blocks_batch   eight lanes per block: dequantise, column pass in registers, transpose through LDS (row stride 9),
//                    row pass, + 128, clamp, 8 bytes per lane into the component planes padded to whole MCUs
//   k_jpegd_pixels_batch   one lane per four pixels: upsample, convert, three words (or twelve bytes) out
// Huffman look-ups: the file's tables in look-up form (5.9 KB) are copied into LDS by every kernel that decodes symbols.
// Every kernel's work for one file is a __device__ body; the __global__ entries at the end of this file hand it a record
// read from device memory, the file picked by the grid's y or z: the files of a chunk by one set of launches, each
// workgroup with its own file's tables in LDS.  A single decode is a chunk of one file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_jpegd_rule.h"

namespace hsk {

constexpr int kJpegdGroup = 256;      // subsequences per workgroup of k_jpegd_sync_batch
constexpr int kJpegdRepairLanes = 1024;

// What every kernel body is handed of one file.
struct JpegdArgs {
    hsjpegd::Frame f;
    const hsjpegd::Tables *tab;
    const uint8_t *scan;      // the stuffed segment, f.scan_bytes of it
    uint32_t n, nchunks;      // its bytes, its chunks
    uint32_t S;               // bits per subsequence
    uint32_t *cntRem, *cntRst;
    uint64_t *remOff, *rstOff; // nchunks + 1 each; the last entry is the total
    uint32_t *clean;          // the clean stream (as words), zero before
    uint32_t *rstPos;         // clean byte at which interval j + 1 starts
    uint32_t nint;            // restart intervals of the frame (0: none)
    uint64_t *start, *exit;   // per subsequence: packed states
    uint32_t *cnt;            // ... blocks that end in it
    uint64_t *base;           // ... its first block
    uint32_t nsubCap;         // subsequences the grids cover (a multiple of kJpegdGroup)
    int16_t *coef;            // 64 zigzag coefficients per stream block, zero before
    uint32_t *diff;           // DC differences, component after component
    uint64_t *dcsum;          // their exclusive prefix sums, nblocks + 1
    uint8_t *planes;          // component planes behind each other
    uint32_t *status;
};

__device__ __forceinline__ void jpegd_tables_to_lds(hsjpegd::Tables *dst, const hsjpegd::Tables *src)
{
    for (unsigned i = threadIdx.x; i < sizeof(hsjpegd::Tables) / 4; i += blockDim.x) ((uint32_t *)dst)[i] = ((const uint32_t *)src)[i];
    __syncthreads();
}

__device__ __forceinline__ uint32_t jpegd_end_bits(const JpegdArgs &a) { return (a.n - (uint32_t)a.remOff[a.nchunks]) * 8u; }

// MODE 0: count what a chunk drops and the markers in it.  MODE 1: write its kept bytes and its intervals' starts.
template <int MODE>
__device__ __forceinline__ void jpegd_clean_body(const JpegdArgs &a, const uint32_t bx)
{
    const uint32_t c = bx * 256u + threadIdx.x;
    if (c >= a.nchunks) return;
    const uint32_t i0 = c * (uint32_t)hsjpegd::kChunk;
    const uint8_t *scan = a.scan;
    uint32_t dropped = 0, markers = 0, o = 0, ord = 0;
    uint8_t *out = (uint8_t *)a.clean;
    if (MODE == 1) { o = i0 - (uint32_t)a.remOff[c]; ord = (uint32_t)a.rstOff[c]; }
    int prev = i0 ? scan[i0 - 1] : 0, cur = scan[i0];
    for (uint32_t j = 0; j < (uint32_t)hsjpegd::kChunk && i0 + j < a.n; j++) {
        const int next = i0 + j + 1 < a.n ? scan[i0 + j + 1] : 0;
        const int cls = hsjpegd::byte_class(prev, cur, next);
        if (MODE == 0) { dropped += cls != 0; markers += cls == 2; }
        else if (cls == 0) out[o++] = (uint8_t)cur;
        else if (cls == 2) { if (ord < a.nint) a.rstPos[ord] = o; ord++; }
        prev = cur; cur = next;
    }
    if (MODE == 0) { a.cntRem[c] = dropped; a.cntRst[c] = markers; }
}

// Grid: nsubCap / 256 workgroups of 256.
__device__ __forceinline__ void jpegd_sync_body(const JpegdArgs &a, const uint32_t bx)
{
    __shared__ hsjpegd::Tables sTab;
    __shared__ uint64_t sExit[kJpegdGroup];
    jpegd_tables_to_lds(&sTab, a.tab);
    const uint32_t end = jpegd_end_bits(a), nsub = (end + a.S - 1u) / a.S;
    const int t = threadIdx.x;
    const uint32_t i = bx * (uint32_t)kJpegdGroup + t;
    const bool active = i < nsub;
    uint64_t st0 = hsjpegd::pack(hsjpegd::State{i * a.S, 0, 0}), ex = 0;
    uint32_t nb = 0;
    if (active) {
        hsjpegd::State s = hsjpegd::unpack(st0);
        nb = hsjpegd::run_subsequence(sTab, a.f, a.clean, end, s, (i + 1u) * a.S);
        ex = hsjpegd::pack(s);
    }
    sExit[t] = ex;
    for (;;) {
        __syncthreads();
        bool changed = false;
        if (active && t > 0 && sExit[t - 1] != st0) { st0 = sExit[t - 1]; changed = true; }
        if (!__syncthreads_or(changed)) break; // (every read of this round lies in front of this barrier, every write behind it)
        if (changed) {
            hsjpegd::State s = hsjpegd::unpack(st0);
            nb = hsjpegd::run_subsequence(sTab, a.f, a.clean, end, s, (i + 1u) * a.S);
            sExit[t] = hsjpegd::pack(s);
            ex = sExit[t];
        }
    }
    a.start[i] = st0;
    a.exit[i] = ex;
    a.cnt[i] = active ? nb : 0u;
}

// Grid: ONE workgroup of kJpegdRepairLanes.
__device__ __forceinline__ void jpegd_repair_body(const JpegdArgs &a)
{
    __shared__ hsjpegd::Tables sTab;
    jpegd_tables_to_lds(&sTab, a.tab);
    const uint32_t end = jpegd_end_bits(a), nsub = (end + a.S - 1u) / a.S, ngroups = (nsub + kJpegdGroup - 1u) / kJpegdGroup;
    for (;;) {
        bool changed = false;
        for (uint32_t g = threadIdx.x + 1u; g < ngroups; g += kJpegdRepairLanes) {
            const uint32_t first = g * (uint32_t)kJpegdGroup, last = first + kJpegdGroup < nsub ? first + kJpegdGroup : nsub;
            // (a neighbour may be storing this word in the same round: either value is a state it held, and a round in
            // which anything was stored is followed by another)
            uint64_t s = __hip_atomic_load(a.exit + first - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            for (uint32_t i = first; i < last; i++) {
                if (a.start[i] == s) break;
                a.start[i] = s;
                hsjpegd::State st = hsjpegd::unpack(s);
                a.cnt[i] = hsjpegd::run_subsequence(sTab, a.f, a.clean, end, st, (i + 1u) * a.S);
                s = hsjpegd::pack(st);
                __hip_atomic_store(a.exit + i, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                changed = true;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
}

// Grid: nsubCap / 256 workgroups of 256.
__device__ __forceinline__ void jpegd_write_body(const JpegdArgs &a, const uint32_t bx)
{
    __shared__ hsjpegd::Tables sTab;
    jpegd_tables_to_lds(&sTab, a.tab);
    const uint32_t end = jpegd_end_bits(a), nsub = (end + a.S - 1u) / a.S;
    const uint32_t i = bx * 256u + threadIdx.x;
    if (i == 0 && nsub == 0) atomicMax(a.status, (uint32_t)hsjpegd::kStatusTruncated);
    if (i >= nsub) return;
    hsjpegd::State s = hsjpegd::unpack(a.start[i]);
    hsjpegd::CoefSink sink{a.coef, (int64_t)a.base[i], a.f.nblocks};
    int st = hsjpegd::decode_stretch(sTab, a.f, a.clean, end, s, (i + 1u) * a.S, a.f.nblocks, sink);
    if (i == nsub - 1u && sink.block < a.f.nblocks) st = hsjpegd::kStatusTruncated;
    if (st) atomicMax(a.status, (uint32_t)st);
}

// Grid: ceil(nint / 256) workgroups of 256.  (hsjpegd::entropy_host's loop body, one interval per lane.)
__device__ __forceinline__ void jpegd_write_rst_body(const JpegdArgs &a, const uint32_t bx)
{
    __shared__ hsjpegd::Tables sTab;
    jpegd_tables_to_lds(&sTab, a.tab);
    const uint32_t j = bx * 256u + threadIdx.x;
    if (j >= a.nint) return;
    const uint32_t end = jpegd_end_bits(a), nrst = (uint32_t)a.rstOff[a.nchunks];
    int st = 0;
    if (j > 0 && j - 1u >= nrst) st = hsjpegd::kStatusTruncated;
    else {
        const uint32_t p0 = j ? a.rstPos[j - 1] * 8u : 0u, p1 = j < nrst ? a.rstPos[j] * 8u : end;
        const int64_t nmcu = (int64_t)a.f.mcux * a.f.mcuy;
        const int64_t b0 = (int64_t)j * a.f.ri * a.f.bpm, b1 = ((int64_t)j + 1) * a.f.ri < nmcu ? ((int64_t)j + 1) * a.f.ri * a.f.bpm : a.f.nblocks;
        hsjpegd::State s{p0, 0, 0};
        hsjpegd::CoefSink sink{a.coef, b0, b1};
        st = hsjpegd::decode_stretch(sTab, a.f, a.clean, p1, s, p1, b1, sink);
        if (sink.block < b1) st = hsjpegd::kStatusTruncated;
    }
    if (st) atomicMax(a.status, (uint32_t)st);
}

// Block j of the component-after-component order: its component, MCU, place in the MCU and stream block.
struct JpegdBlockAt {
    int c, s, h, v;
    int64_t m, B;
};
__device__ __forceinline__ JpegdBlockAt jpegd_block_at(const hsjpegd::Frame &f, int64_t j)
{
    JpegdBlockAt r;
    const int64_t nmcu = (int64_t)f.mcux * f.mcuy, nl = f.hs * f.vs;
    if (j < nmcu * nl) { r.c = 0; r.m = j / nl; r.s = (int)(j - r.m * nl); r.h = f.hs; r.v = f.vs; }
    else { const int64_t k = j - nmcu * nl; r.c = 1 + (int)(k / nmcu); r.m = k - (r.c - 1) * nmcu; r.s = 0; r.h = r.v = 1; }
    r.B = r.m * f.bpm + (r.c ? nl + r.c - 1 : r.s);
    return r;
}

__device__ __forceinline__ void jpegd_dc_gather_body(const JpegdArgs &a, const uint32_t bx)
{
    const int64_t j = (int64_t)bx * 256 + threadIdx.x;
    if (j >= a.f.nblocks) return;
    a.diff[j] = (uint32_t)(int32_t)a.coef[jpegd_block_at(a.f, j).B * 64];
}

// Grid: ceil(nblocks / 32) workgroups of 256: eight lanes per block.
__device__ __forceinline__ void jpegd_blocks_body(const JpegdArgs &a, const uint32_t wg)
{
    __shared__ int32_t sT[32][72];
    const int t = threadIdx.x, lb = t >> 3, r = t & 7;
    const int64_t j = (int64_t)wg * 32 + lb;
    const bool live = j < a.f.nblocks;
    JpegdBlockAt at{};
    int32_t d[8];
    bool bad = false;
    if (live) {
        at = jpegd_block_at(a.f, j);
        const int nbc = at.h * at.v; // the component's blocks per MCU
        const int64_t seg = j - at.s - (a.f.ri ? (at.m % a.f.ri) * nbc : at.m * nbc); // its first block since the last restart
        const int32_t dc = (int32_t)((uint32_t)a.dcsum[j + 1] - (uint32_t)a.dcsum[seg]);
        const int16_t *zz = a.coef + at.B * 64;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int n = 8 * i + r;
            d[i] = hsjpegd::dequant(n ? (int32_t)zz[a.tab->zpos[n]] : dc, a.tab->q[at.c][n], &bad);
        }
        hsjpegd::idct_1d(d, 1, false);
#pragma unroll
        for (int i = 0; i < 8; i++) sT[lb][9 * i + r] = d[i];
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = sT[lb][9 * r + i];
    hsjpegd::idct_1d(d, 1, true);
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        w0 |= (uint32_t)hsjpegd::clamp255(d[i] + 128) << (8 * i);
        w1 |= (uint32_t)hsjpegd::clamp255(d[4 + i] + 128) << (8 * i);
    }
    const int bx = (int)(at.m % a.f.mcux) * at.h + at.s % at.h, by = (int)(at.m / a.f.mcux) * at.v + at.s / at.h;
    const size_t stride = (size_t)hsjpegd::plane_wb(a.f, at.c) * 8u;
    uint8_t *o = a.planes + hsjpegd::plane_block0(a.f, at.c) * 64 + ((size_t)by * 8u + (size_t)r) * stride + (size_t)bx * 8u;
    *(uint2 *)o = make_uint2(w0, w1);
    if (bad) atomicMax(a.status, (uint32_t)hsjpegd::kStatusCorrupt);
}

// pix: W x H pixels of 3 bytes, rows `stride` apart; rgb != 0: R first, else B first.  wide != 0: pix and stride are
// multiples of 4.  Grid: (ceil(W / 256), ceil(H / 4)), block (64, 4).
__device__ __forceinline__ void jpegd_pixels_body(const JpegdArgs &a, uint8_t *__restrict__ pix, long long stride, int rgb, int wide)
{
    const int x0 = 4 * (int)(blockIdx.x * 64 + threadIdx.x), y = (int)(blockIdx.y * 4 + threadIdx.y);
    if (x0 >= a.f.W || y >= a.f.H) return;
    const uint8_t *planes[3];
    int strides[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        planes[c] = a.planes + hsjpegd::plane_block0(a.f, c < a.f.ncomp ? c : 0) * 64;
        strides[c] = hsjpegd::plane_wb(a.f, c < a.f.ncomp ? c : 0) * 8;
    }
    uint32_t v[12];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int32_t r = 0, g = 0, b = 0;
        if (x0 + i < a.f.W) hsjpegd::pixel(a.f, planes, strides, x0 + i, y, &r, &g, &b);
        v[3 * i] = (uint32_t)(rgb ? r : b); v[3 * i + 1] = (uint32_t)g; v[3 * i + 2] = (uint32_t)(rgb ? b : r);
    }
    uint8_t *o = pix + (long long)y * stride + 3ll * x0;
    if (wide && x0 + 4 <= a.f.W) {
        uint32_t *w = (uint32_t *)o;
#pragma unroll
        for (int i = 0; i < 3; i++) w[i] = v[4 * i] | v[4 * i + 1] << 8 | v[4 * i + 2] << 16 | v[4 * i + 3] << 24;
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++)
            if (x0 + i / 3 < a.f.W) o[i] = (uint8_t)v[i];
    }
}

// ---- the entries: a chunk of files by the same launches ---------------------------------------------------------------
// One record per file in device memory; the file is the grid's y (pixels: z).  Every grid is sized for the chunk's
// largest file: a workgroup beyond its own file's extent, or of a file that takes the other route between clean and
// dc_gather (restart intervals or not), reads its record and returns -- before any LDS, barrier or store.  A body sees
// its own file's record alone, so a file's pixels are the same whatever lies beside it.
struct JpegdBatchRec {
    JpegdArgs a;
    uint8_t *pix;      // where k_jpegd_pixels_batch puts this file's picture
    long long stride;
    int32_t rgb, wide;
};

template <int MODE>
__global__ __launch_bounds__(256) void k_jpegd_clean_batch(const JpegdBatchRec *__restrict__ recs)
{
    const JpegdArgs a = recs[blockIdx.y].a;
    if (blockIdx.x * 256u >= a.nchunks) return;
    jpegd_clean_body<MODE>(a, blockIdx.x);
}

// Grid: (files, WHICH == 0 ? 2 : 1) workgroups of kJpegScanLanes.  WHICH 0: cntRem -> remOff (y = 0) and cntRst -> rstOff
// (y = 1); 2: cnt -> base, files without restart intervals; 3: diff -> dcsum.
template <int WHICH>
__global__ __launch_bounds__(kJpegScanLanes) void k_jpegd_scan_batch(const JpegdBatchRec *__restrict__ recs)
{
    const JpegdArgs a = recs[blockIdx.x].a;
    const uint32_t *in;
    uint64_t *out;
    long long n;
    if (WHICH == 0) { in = blockIdx.y ? a.cntRst : a.cntRem; out = blockIdx.y ? a.rstOff : a.remOff; n = a.nchunks; }
    else if (WHICH == 2) { if (a.f.ri) return; in = a.cnt; out = a.base; n = a.nsubCap; }
    else { in = a.diff; out = a.dcsum; n = a.f.nblocks; }
    jpeg_scan_body(in, out, n, nullptr);
}

__global__ __launch_bounds__(kJpegdGroup) void k_jpegd_sync_batch(const JpegdBatchRec *__restrict__ recs)
{
    const JpegdArgs a = recs[blockIdx.y].a;
    if (a.f.ri || blockIdx.x * (uint32_t)kJpegdGroup >= a.nsubCap) return;
    jpegd_sync_body(a, blockIdx.x);
}

// Grid: one workgroup of kJpegdRepairLanes per file.
__global__ __launch_bounds__(kJpegdRepairLanes) void k_jpegd_repair_batch(const JpegdBatchRec *__restrict__ recs)
{
    const JpegdArgs a = recs[blockIdx.x].a;
    if (a.f.ri) return;
    jpegd_repair_body(a);
}

__global__ __launch_bounds__(256) void k_jpegd_write_batch(const JpegdBatchRec *__restrict__ recs)
{
    const JpegdArgs a = recs[blockIdx.y].a;
    if (a.f.ri || blockIdx.x * 256u >= a.nsubCap) return;
    jpegd_write_body(a, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_jpegd_write_rst_batch(const JpegdBatchRec *__restrict__ recs)
{
    const JpegdArgs a = recs[blockIdx.y].a;
    if (!a.f.ri || blockIdx.x * 256u >= a.nint) return;
    jpegd_write_rst_body(a, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_jpegd_dc_gather_batch(const JpegdBatchRec *__restrict__ recs)
{
    const JpegdArgs a = recs[blockIdx.y].a;
    if ((int64_t)blockIdx.x * 256 >= a.f.nblocks) return;
    jpegd_dc_gather_body(a, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_jpegd_blocks_batch(const JpegdBatchRec *__restrict__ recs)
{
    const JpegdArgs a = recs[blockIdx.y].a;
    if ((int64_t)blockIdx.x * 32 >= a.f.nblocks) return;
    jpegd_blocks_body(a, blockIdx.x);
}

// Grid: (ceil(W / 256), ceil(H / 4), files), block (64, 4).
__global__ __launch_bounds__(256) void k_jpegd_pixels_batch(const JpegdBatchRec *__restrict__ recs)
{
    const JpegdBatchRec r = recs[blockIdx.z];
    if ((int)(blockIdx.x * 256u) >= r.a.f.W || (int)(blockIdx.y * 4u) >= r.a.f.H) return;
    jpegd_pixels_body(r.a, r.pix, r.stride, r.rgb, r.wide);
}

} // namespace hsk
