// hs_kernels_regions.hip.h -- connected regions of a foreground mask (hs_regions_rule.h) labelled where the mask lies.
// Eight kernels, launched one behind the other on one stream; the field is blockIdx.z, field i reads its own planes from an
// argument block by value and owns slice i of the scratch: a parent plane and an area plane of W * H words each, one count
// word per 256 pixels of a row, and the RgAcc record.  Every word of the scratch that a call reads it has written itself
// first: there is no memset and nothing is carried from one call to the next.
//   k_rg_tile     grid (ceil(W / 64), ceil(H / 16), fields), 256 lanes: a tile of 64 x 16 pixels in LDS.  The foreground
//                 test and, under thr > 0, the flow go to LDS once; every edge inside the tile is evaluated once, by its
//                 later pixel, and united by the lock-free union below on LDS words; then every pixel walks to its root and
//                 writes it as a GLOBAL linear index (kBackground for background), and zeroes its word of the area plane.
//   k_rg_seam     one lane per edge that crosses a tile border (the diagonals across corners included): the same union on
//                 the global parent plane, every access an agent-scope atomic.
//   k_rg_flatten  one lane per pixel: walks to the root, writes it, counts the pixel into area[root] -- lanes of a
//                 wavefront that share a root issue ONE atomic.
//   k_rg_count    per 256 pixels of a row: the roots and the roots that are kept (area >= min_area), one word.
//   k_rg_scan     ONE workgroup per field: the exclusive prefix sum of the kept counts in raster order, in place; the
//                 totals go to RgAcc, whose sums it zeroes.
//   k_rg_number   per 256 pixels of a row again: the dense number of every kept root, written INTO the root's parent word
//                 (bit 31 set, the number below it; 0 for a dropped root), the record of the root initialised, the sums of
//                 the result (foreground and dropped pixels, largest region) reduced per wavefront.
//   k_rg_relabel  one lane per pixel: the label plane and the records' sums and boxes, reduced per wavefront for up to
//                 kRgGroups labels per wavefront, lane by lane beyond.
//   k_rg_finish   packs the boxes of the records into their 16-bit fields and writes the result header.
// The union (Playne and Hawick's lock-free form): walk both ends to their roots; if they differ, atomicMin the smaller
// into the larger root's word; if the word no longer held that root -- somebody else hung it elsewhere meanwhile -- go on
// from what it held.  Parents only ever decrease, so every walk ends, nothing is lost, and ONE pass over the edges followed
// by one flatten gives the components whatever the order of execution: no kernel iterates "until nothing changes" and the
// host launches a fixed sequence.  No workgroup waits for another anywhere: the scan is three launches.
// All sums are integers: the outputs do not depend on the order of execution.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_regions_rule.h"

namespace hsk {

constexpr int kRgBatchMax = 8; // fields per launch: the scratch is two planes per field
constexpr int kRgTileW = 64, kRgTileH = 16;
constexpr int kRgGroups = 4;   // labels of a wavefront that are reduced together before the rest goes lane by lane
constexpr uint32_t kRgNumbered = 0x80000000u; // a root's parent word once k_rg_number has run: this bit | its number

// What the kernels of a field share between launches.
struct RgAcc {
    unsigned n_regions, n_roots;
    unsigned long long fg_px, dropped_px, unknown_px, largest;
};
static_assert(sizeof(RgAcc) == 40, "RgAcc: 8-byte words for the 64-bit atomics");

// The planes of a batch, handed to the kernels by value.
struct RgPlanes {
    const uint8_t *mask[kRgBatchMax];         // or NULL: every pixel is foreground
    const float *u[kRgBatchMax], *v[kRgBatchMax]; // or NULL (both)
    int32_t *labels[kRgBatchMax];             // or NULL
    hsrg::Record *records[kRgBatchMax];       // or NULL
    hsrg::Result *results[kRgBatchMax];       // or NULL
    long long ms, fs, ls;                     // strides in BYTES: mask, flow, labels
    int W, H;
    unsigned capacity;
    unsigned lo, hi, min_area;
    int conn;
    float thr;
    // the scratch: field i at parent + i * plane, area + i * plane, counts + i * n_counts, acc + i
    uint32_t *parent, *area, *counts;
    RgAcc *acc;
    long long plane, n_counts;
};
static_assert(sizeof(RgPlanes) + 64 <= 1024, "the argument block stays well inside the 4 KiB of kernel arguments");

#if defined(HS_REGIONS_KERNELS) // the kernels themselves: hs_regions_kernels.hip alone defines it

__device__ __forceinline__ uint32_t rg_load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t rg_find(uint32_t *parent, uint32_t a)
{
    uint32_t p = rg_load(parent + a);
    while (p != a) {
        a = p;
        p = rg_load(parent + a);
    }
    return a;
}

// The lock-free union on global words.
__device__ __forceinline__ void rg_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = rg_find(parent, a);
        b = rg_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a; a = b; b = t;
        }
        // a > b: hang a below b, if a is still a root
        const uint32_t old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ uint32_t rg_lds_find(volatile uint32_t *L, uint32_t a)
{
    uint32_t p = L[a];
    while (p != a) {
        a = p;
        p = L[a];
    }
    return a;
}

__device__ __forceinline__ void rg_lds_unite(uint32_t *L, uint32_t a, uint32_t b)
{
    for (;;) {
        a = rg_lds_find(L, a);
        b = rg_lds_find(L, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a; a = b; b = t;
        }
        const uint32_t old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ unsigned rg_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ int rg_wave_sumi(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long rg_wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long rg_wave_max64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned rg_wave_min(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned rg_wave_max(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ const float *rg_frow(const float *p, long long stride, int y) { return (const float *)((const uint8_t *)p + (long long)y * stride); }

// Grid: (ceil(W / 64), ceil(H / 16), fields); 256 lanes, lane t takes the local pixels t, t + 256, t + 512, t + 768 (rows
// (t >> 6) + 4 k of the tile, column t & 63).
__global__ __launch_bounds__(256) void k_rg_tile(const RgPlanes pl)
{
    constexpr int TW = kRgTileW, TH = kRgTileH, N = TW * TH;
    __shared__ uint32_t L[N];
    __shared__ float fu[N], fv[N];
    const unsigned i = blockIdx.z;
    const int W = pl.W, H = pl.H;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int lx = threadIdx.x & 63;
    const int x = tx0 + lx;
    const bool join = pl.thr > 0.0f;
    const uint8_t *mask = pl.mask[i];
    uint32_t *parent = pl.parent + (long long)i * pl.plane, *area = pl.area + (long long)i * pl.plane;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = (int)(threadIdx.x >> 6) + 4 * k, y = ty0 + ly, li = ly * TW + lx;
        const bool in = x < W && y < H;
        bool fg = in;
        if (in && mask) fg = hsrg::foreground(mask[(long long)y * pl.ms + x], pl.lo, pl.hi);
        L[li] = fg ? (uint32_t)li : hsrg::kBackground;
        if (join) {
            fu[li] = fg ? rg_frow(pl.u[i], pl.fs, y)[x] : 0.0f;
            fv[li] = fg ? rg_frow(pl.v[i], pl.fs, y)[x] : 0.0f;
        }
        if (in) area[(long long)y * W + x] = 0u;
    }
    __syncthreads();
    // every edge once, by its later pixel: left, up, and under 8 up-left and up-right
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = (int)(threadIdx.x >> 6) + 4 * k, li = ly * TW + lx;
        if (((volatile uint32_t *)L)[li] == hsrg::kBackground) continue;
        const int ndir = pl.conn == 8 ? 4 : 2;
        for (int d = 0; d < ndir; d++) {
            const int bx = lx + (d == 0 || d == 2 ? -1 : d == 3 ? 1 : 0), by = ly - (d == 0 ? 0 : 1);
            if (bx < 0 || bx >= TW || by < 0) continue;
            const int lj = by * TW + bx;
            if (((volatile uint32_t *)L)[lj] == hsrg::kBackground) continue;
            if (join && !hsrg::joined(fu[li], fv[li], fu[lj], fv[lj], pl.thr)) continue;
            rg_lds_unite(L, (uint32_t)li, (uint32_t)lj);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = (int)(threadIdx.x >> 6) + 4 * k, y = ty0 + ly, li = ly * TW + lx;
        if (x >= W || y >= H) continue;
        uint32_t g = hsrg::kBackground;
        if (((volatile uint32_t *)L)[li] != hsrg::kBackground) {
            const uint32_t r = rg_lds_find(L, (uint32_t)li);
            g = (uint32_t)((ty0 + (int)(r / TW)) * W + tx0 + (int)(r % TW));
        }
        parent[(long long)y * W + x] = g;
    }
}

// Grid: (ceil(edges / 256), 1, fields), edges = (nv * H + nh * W) * ndir with nv = (W - 1) / 64 vertical and
// nh = (H - 1) / 16 horizontal seams and ndir = 1 (4-connectivity) or 3.  Lane e: direction e % ndir of seam pixel e / ndir.
// A pixel (x, y) of a vertical seam has x = 64 k and looks left to (x - 1, y + {0, -1, +1}); one of a horizontal seam has
// y = 16 k and looks up to (x + {0, -1, +1}, y - 1).  Corner diagonals come up twice; a union done twice is done once.
__global__ __launch_bounds__(256) void k_rg_seam(const RgPlanes pl, long long edges, int ndir)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= edges) return;
    const unsigned i = blockIdx.z;
    const int W = pl.W, H = pl.H;
    const int d = (int)(e % ndir);
    long long s = e / ndir;
    const int off = d == 0 ? 0 : d == 1 ? -1 : 1;
    const long long nvH = (long long)((W - 1) / kRgTileW) * H;
    int x, y, xb, yb;
    if (s < nvH) {
        x = ((int)(s / H) + 1) * kRgTileW; y = (int)(s % H);
        xb = x - 1; yb = y + off;
    } else {
        s -= nvH;
        y = ((int)(s / W) + 1) * kRgTileH; x = (int)(s % W);
        xb = x + off; yb = y - 1;
    }
    if (xb < 0 || xb >= W || yb < 0 || yb >= H) return;
    uint32_t *parent = pl.parent + (long long)i * pl.plane;
    const uint32_t a = (uint32_t)(y * W + x), b = (uint32_t)(yb * W + xb);
    if (rg_load(parent + a) == hsrg::kBackground || rg_load(parent + b) == hsrg::kBackground) return;
    if (pl.thr > 0.0f) {
        const float *u = pl.u[i], *v = pl.v[i];
        if (!hsrg::joined(rg_frow(u, pl.fs, y)[x], rg_frow(v, pl.fs, y)[x], rg_frow(u, pl.fs, yb)[xb], rg_frow(v, pl.fs, yb)[xb], pl.thr)) return;
    }
    rg_unite(parent, a, b);
}

// Grid: (ceil(W / 256), H, fields); 256 lanes, one pixel each; every lane stays to the end: the wavefront votes together.
__global__ __launch_bounds__(256) void k_rg_flatten(const RgPlanes pl)
{
    const unsigned i = blockIdx.z;
    const int W = pl.W;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    uint32_t *parent = pl.parent + (long long)i * pl.plane, *area = pl.area + (long long)i * pl.plane;
    uint32_t r = hsrg::kBackground;
    if (x < W) {
        const uint32_t self = (uint32_t)(y * W + x);
        if (parent[self] != hsrg::kBackground) {
            // (other lanes shorten paths meanwhile: whatever a word holds is an ancestor, and a root's word stays)
            r = rg_find(parent, self);
            if (r != self) parent[self] = r;
        }
    }
    unsigned long long todo = __ballot(r != hsrg::kBackground);
    const unsigned lane = threadIdx.x & 63u;
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const uint32_t lr = (uint32_t)__shfl((int)r, lead, 64);
        const unsigned long long same = __ballot(r == lr);
        if (lane == (unsigned)lead) atomicAdd(area + lr, (unsigned)__popcll(same));
        todo &= ~same;
    }
}

// Is pixel `self` a root, and is it kept?  (Before k_rg_number: a root's word holds itself.)
__device__ __forceinline__ void rg_root_flags(const RgPlanes &pl, const uint32_t *parent, const uint32_t *area, int x, uint32_t self, bool *root, bool *kept)
{
    *root = x < pl.W && parent[self] == self;
    *kept = *root && area[self] >= pl.min_area;
}

// Grid as k_rg_flatten.  counts[y * gridDim.x + blockIdx.x] = kept | roots << 16.
__global__ __launch_bounds__(256) void k_rg_count(const RgPlanes pl)
{
    const unsigned i = blockIdx.z;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const uint32_t *parent = pl.parent + (long long)i * pl.plane, *area = pl.area + (long long)i * pl.plane;
    bool root, kept;
    rg_root_flags(pl, parent, area, x, (uint32_t)(y * pl.W + x), &root, &kept);
    __shared__ unsigned part[4];
    const unsigned w = (unsigned)__popcll(__ballot(kept)) | (unsigned)__popcll(__ballot(root)) << 16;
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0u) pl.counts[(long long)i * pl.n_counts + (long long)y * gridDim.x + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// Grid: (1, 1, fields); 1024 lanes.  In place: counts[k] becomes the number of kept roots in front of block k.
__global__ __launch_bounds__(1024) void k_rg_scan(const RgPlanes pl)
{
    const unsigned i = blockIdx.z;
    uint32_t *counts = pl.counts + (long long)i * pl.n_counts;
    __shared__ unsigned wsum[16], wroots[16];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned carry = 0u, roots = 0u;
    for (long long base = 0; base < pl.n_counts; base += 1024) {
        const long long k = base + threadIdx.x;
        const unsigned w = k < pl.n_counts ? counts[k] : 0u;
        const unsigned mine = w & 0xffffu;
        unsigned incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = (unsigned)__shfl_up((int)incl, d, 64);
            if (lane >= (unsigned)d) incl += o;
        }
        const unsigned r = rg_wave_sum(w >> 16);
        __syncthreads(); // (the last round's wsum has been read)
        if (lane == 63u) {
            wsum[wave] = incl;
            wroots[wave] = r;
        }
        __syncthreads();
        unsigned before = 0u, total = 0u, rtotal = 0u;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            before += (unsigned)q < wave ? wsum[q] : 0u;
            total += wsum[q];
            rtotal += wroots[q];
        }
        if (k < pl.n_counts) counts[k] = carry + before + incl - mine;
        carry += total;
        roots += rtotal;
    }
    if (threadIdx.x == 0u) {
        RgAcc &a = pl.acc[i];
        a.n_regions = carry;
        a.n_roots = roots;
        a.fg_px = 0ull; a.dropped_px = 0ull; a.unknown_px = 0ull; a.largest = 0ull;
    }
}

// Grid as k_rg_flatten.
__global__ __launch_bounds__(256) void k_rg_number(const RgPlanes pl)
{
    const unsigned i = blockIdx.z;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    uint32_t *parent = pl.parent + (long long)i * pl.plane;
    const uint32_t *area = pl.area + (long long)i * pl.plane;
    const uint32_t self = (uint32_t)(y * pl.W + x);
    bool root, kept;
    rg_root_flags(pl, parent, area, x, self, &root, &kept);
    __shared__ unsigned part[4];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long votes = __ballot(kept);
    if (lane == 0u) part[wave] = (unsigned)__popcll(votes);
    __syncthreads();
    unsigned before = pl.counts[(long long)i * pl.n_counts + (long long)y * gridDim.x + blockIdx.x];
    for (unsigned q = 0; q < wave; q++) before += part[q];
    const unsigned label = before + (unsigned)__popcll(votes & ((1ull << lane) - 1ull)) + 1u;
    unsigned long long all = 0ull, dropped = 0ull, key = 0ull;
    if (root) {
        const uint32_t a = area[self];
        all = a; // (every foreground pixel is counted at its root)
        parent[self] = kRgNumbered | (kept ? label : 0u);
        if (kept) {
            key = hsrg::largest_key(a, label);
            hsrg::Record *rec = pl.records[i];
            if (rec && label <= pl.capacity) {
                // the box in four whole words until k_rg_finish packs it: x0 in (x0, y0), y0 in (x1, y1), x1 in reserved0, y1 in reserved1
                uint32_t *w = (uint32_t *)(rec + (label - 1u));
                w[0] = self; w[1] = a; w[2] = 0xffffffffu; w[3] = 0xffffffffu;
                w[4] = 0u; w[5] = 0u; w[6] = 0u; w[7] = 0u;
                w[8] = 0u; w[9] = 0u; w[10] = 0u; w[11] = 0u; w[12] = 0u; w[13] = 0u; w[14] = 0u; w[15] = 0u;
            }
        } else {
            dropped = a;
        }
    }
    all = rg_wave_sum64(all);
    dropped = rg_wave_sum64(dropped);
    key = rg_wave_max64(key);
    if (lane == 0u) {
        RgAcc &acc = pl.acc[i];
        if (all) atomicAdd(&acc.fg_px, all);
        if (dropped) atomicAdd(&acc.dropped_px, dropped);
        if (key) atomicMax(&acc.largest, key);
    }
}

// Grid as k_rg_flatten; every lane stays to the end.
__global__ __launch_bounds__(256) void k_rg_relabel(const RgPlanes pl)
{
    const unsigned i = blockIdx.z;
    const int W = pl.W;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const uint32_t *parent = pl.parent + (long long)i * pl.plane;
    const unsigned lane = threadIdx.x & 63u;
    unsigned label = 0u;
    bool fg = false, known = false;
    int qu = 0, qv = 0;
    if (x < W) {
        uint32_t p = parent[y * W + x];
        fg = p != hsrg::kBackground;
        if (fg) {
            if (!(p & kRgNumbered)) p = parent[p];
            label = p & ~kRgNumbered;
            if (pl.u[i]) {
                const float a = rg_frow(pl.u[i], pl.fs, y)[x], b = rg_frow(pl.v[i], pl.fs, y)[x];
                known = hsrg::flow_known(a, b);
                if (known) {
                    qu = hsgm::quant(a);
                    qv = hsgm::quant(b);
                }
            }
        }
        if (pl.labels[i]) ((int32_t *)((uint8_t *)pl.labels[i] + (long long)y * pl.ls))[x] = (int32_t)label;
    }
    if (pl.u[i]) {
        const unsigned unknown = (unsigned)__popcll(__ballot(fg && !known));
        if (lane == 0u && unknown) atomicAdd(&pl.acc[i].unknown_px, (unsigned long long)unknown);
    }
    hsrg::Record *rec = pl.records[i];
    if (!rec) return; // (uniform: an argument)
    const bool mine = label != 0u && label <= pl.capacity;
    unsigned long long todo = __ballot(mine);
    for (int g = 0; g < kRgGroups && todo; g++) {
        const int lead = __ffsll((long long)todo) - 1;
        const unsigned ll = (unsigned)__shfl((int)label, lead, 64);
        const bool in = mine && label == ll;
        const unsigned long long same = __ballot(in);
        // a wavefront lies in one row: 64 columns at most, so every sum fits 32 bits (64 * 2^14, 64 * 2^19)
        const unsigned cnt = (unsigned)__popcll(same);
        const unsigned sx = rg_wave_sum(in ? (unsigned)x : 0u);
        const unsigned nf = (unsigned)__popcll(__ballot(in && known));
        const int su = rg_wave_sumi(in ? qu : 0), sv = rg_wave_sumi(in ? qv : 0);
        const unsigned mn = rg_wave_min(in ? (unsigned)x : 0xffffffffu), mx = rg_wave_max(in ? (unsigned)x : 0u);
        if (lane == (unsigned)lead) {
            uint32_t *w = (uint32_t *)(rec + (ll - 1u));
            unsigned long long *d = (unsigned long long *)w;
            atomicMin(w + 2, mn); atomicMin(w + 3, (unsigned)y); atomicMax(w + 9, mx); atomicMax(w + 14, (unsigned)y);
            atomicAdd(d + 2, (unsigned long long)sx);
            atomicAdd(d + 3, (unsigned long long)cnt * (unsigned)y);
            if (nf) {
                atomicAdd(w + 8, nf);
                atomicAdd(d + 5, (unsigned long long)(long long)su); // (two's complement: the sum of the shares)
                atomicAdd(d + 6, (unsigned long long)(long long)sv);
            }
        }
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) {
        uint32_t *w = (uint32_t *)(rec + (label - 1u));
        unsigned long long *d = (unsigned long long *)w;
        atomicMin(w + 2, (unsigned)x); atomicMin(w + 3, (unsigned)y); atomicMax(w + 9, (unsigned)x); atomicMax(w + 14, (unsigned)y);
        atomicAdd(d + 2, (unsigned long long)x);
        atomicAdd(d + 3, (unsigned long long)y);
        if (known) {
            atomicAdd(w + 8, 1u);
            atomicAdd(d + 5, (unsigned long long)(long long)qu);
            atomicAdd(d + 6, (unsigned long long)(long long)qv);
        }
    }
}

// Grid: (ceil(max(capacity, 1) / 256), 1, fields); 256 lanes, one record each; lane 0 of block 0 writes the result.
__global__ __launch_bounds__(256) void k_rg_finish(const RgPlanes pl)
{
    const unsigned i = blockIdx.z;
    const RgAcc &acc = pl.acc[i];
    const unsigned k = blockIdx.x * 256 + threadIdx.x;
    const unsigned written = acc.n_regions < pl.capacity ? acc.n_regions : pl.capacity;
    hsrg::Record *rec = pl.records[i];
    if (rec && k < written) {
        uint32_t *w = (uint32_t *)(rec + k);
        const uint32_t x0 = w[2], y0 = w[3], x1 = w[9], y1 = w[14];
        w[2] = (x0 & 0xffffu) | y0 << 16;
        w[3] = (x1 & 0xffffu) | y1 << 16;
        w[9] = 0u;
        w[14] = 0u;
    }
    if (k == 0u && pl.results[i]) {
        hsrg::Result r;
        hsrg::finish_result(&r, acc.n_regions, acc.n_roots, pl.capacity, acc.fg_px, acc.dropped_px, acc.unknown_px, acc.largest);
        *pl.results[i] = r;
    }
}

#endif // HS_REGIONS_KERNELS

// hs_regions_kernels.hip: the kernels and their launches, in the order of a call.
hipError_t launch_regions(hipStream_t stream, const RgPlanes &pl, int fields);

} // namespace hsk
