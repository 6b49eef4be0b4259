// hs_regions_rule.h -- the moving objects of a scene: the connected regions of a foreground mask, optionally cut where the
// flow of two neighbours differs (motion segmentation), with each region's size, box, centroid sums and motion sums.  ONE
// definition for the device kernels (hs_kernels_regions.hip.h) and the host form (hsflow_regions_host), the way
// hs_gmotion_rule.h serves both sides of the fit.
//   Foreground.  A pixel whose mask byte lies in fg_lo .. fg_hi (inclusive); with no mask plane every pixel.
//   Graph.  Foreground pixels a, b that are neighbours (connectivity 4: left / right / up / down; 8: the diagonals too) are
//   joined when thr == 0 (join_px == 0), else when both flows are KNOWN -- gmotion's test, hsgm::usable_class -- and
//     fl(fl(du * du) + fl(dv * dv)) <= thr,  du = fl(ua - ub), dv = fl(va - vb),  thr = fl(join_px * join_px);
//   equality joins.  fl(ua - ub) and fl(ub - ua) differ in the sign alone and the squares drop it: the predicate gives the
//   same bits from either end.  Under thr > 0 a foreground pixel with unknown flow joins nobody: a region of its own.
//   Regions.  The connected components; a region's root is the smallest y * W + x among its pixels.  Regions of fewer
//   than min_area pixels are dropped (label 0, as background); the kept ones are numbered 1, 2, ... by ascending root.
//   Sums.  Exact integers, so the order of accumulation cannot matter and device and host agree bit for bit: area,
//   sum_x, sum_y of plain coordinates, n_flow (pixels whose flow is known, 0 without flow planes), and the flow of those
//   pixels quantised as gmotion does, q = (int)rintf(fl(a * 256)), ties to even (hsgm::quant).  The overflow proof is the
//   static_asserts below.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "hs_gmotion_rule.h"

#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace hsrg {

constexpr int kMaxSide = hsgm::kMaxSide;           // the largest width and height the entry points accept
constexpr long long kMaxPixels = hsgm::kMaxPixels; // ... and the largest W * H
constexpr unsigned kFlagOverflow = 1u;             // more regions than records
constexpr uint32_t kBackground = 0xffffffffu;      // a parent that is no pixel

// ---- no sum overflows -------------------------------------------------------------------------------------------------------
static_assert(kMaxPixels <= 0x3fffffffLL + 1, "a linear index, an area and a label fit 30 bits: bit 31 of a parent word is free");
static_assert(kMaxSide - 1 <= 0xffff, "a box coordinate fits 16 bits");
static_assert(kMaxPixels <= hsgm::kInt64Max / (kMaxSide - 1), "sum_x, sum_y over every pixel stay inside 64 bits");
static_assert(kMaxPixels <= hsgm::kInt64Max / hsgm::kMaxQ, "sum_qu, sum_qv over every pixel stay inside int64");

// hsflow_regions_record (include/hsflow.h) as both sides write it.
struct Record {
    uint32_t root, area;
    uint16_t x0, y0, x1, y1;
    uint64_t sum_x, sum_y;
    uint32_t n_flow, reserved0;
    int64_t sum_qu, sum_qv;
    uint64_t reserved1;
};
static_assert(sizeof(Record) == 64, "hsflow_regions_record is 64 bytes");

// hsflow_regions_result.
struct Result {
    uint32_t n_regions, n_written, n_dropped, flags;
    uint64_t fg_px, dropped_px, unknown_flow_px;
    uint32_t largest_area, largest_label;
    uint64_t reserved[2];
};
static_assert(sizeof(Result) == 64, "hsflow_regions_result is 64 bytes");

struct Rule {
    int conn;      // 4 or 8
    unsigned lo, hi; // the foreground bytes
    unsigned min_area;
    float thr;     // fl(join_px * join_px); 0: neighbours always join
};

HSW_FN bool foreground(unsigned byte, unsigned lo, unsigned hi) { return byte >= lo && byte <= hi; }

HSW_FN bool flow_known(float a, float b) { return hsgm::usable_class(a, b, 1u) != hsgm::kUnknown; }

// Two adjacent foreground pixels under thr > 0.
HSW_FN bool joined(float ua, float va, float ub, float vb, float thr)
{
    if (!flow_known(ua, va) || !flow_known(ub, vb)) return false;
    const float du = ua - ub, dv = va - vb;
    const float uu = du * du, vv = dv * dv;
    return uu + vv <= thr;
}

// The larger area wins, then the smaller label: one 64-bit key whose maximum is the answer (0: no region).
HSW_FN uint64_t largest_key(uint32_t area, uint32_t label) { return (uint64_t)area << 32 | (uint32_t)~label; }

HSW_FN void finish_result(Result *r, uint32_t n_regions, uint32_t n_roots, uint32_t capacity, uint64_t fg_px, uint64_t dropped_px, uint64_t unknown_px, uint64_t key)
{
    r->n_regions = n_regions;
    r->n_written = n_regions < capacity ? n_regions : capacity;
    r->n_dropped = n_roots - n_regions;
    r->flags = n_regions > capacity ? kFlagOverflow : 0u;
    r->fg_px = fg_px;
    r->dropped_px = dropped_px;
    r->unknown_flow_px = unknown_px;
    r->largest_area = (uint32_t)(key >> 32);
    r->largest_label = key ? ~(uint32_t)key : 0u;
    r->reserved[0] = r->reserved[1] = 0;
}

// ---- a whole field in host memory: the specification, a plain two-pass union-find ------------------------------------------

struct Field {
    const uint8_t *mask; // or NULL
    size_t ms;
    const float *u, *v; // both or neither
    size_t fs;          // rows of u and v fs BYTES apart
    int W, H;
};

inline uint32_t find(std::vector<uint32_t> &parent, uint32_t a)
{
    uint32_t r = a;
    while (parent[r] != r) r = parent[r];
    while (parent[a] != r) {
        const uint32_t next = parent[a];
        parent[a] = r;
        a = next;
    }
    return r;
}

// The smaller root becomes the parent: a set's root is its smallest index.
inline void unite(std::vector<uint32_t> &parent, uint32_t a, uint32_t b)
{
    a = find(parent, a);
    b = find(parent, b);
    if (a < b) parent[b] = a;
    else if (b < a) parent[a] = b;
}

// labels (rows ls BYTES apart), records (capacity of them) and result may each be NULL.  Writes W labels of every row, the
// records of the regions 1 .. min(n_regions, capacity), the result, and nothing else.
inline void label_rows(const Field &f, const Rule &rule, int32_t *labels, size_t ls, Record *records, uint32_t capacity, Result *result)
{
    const int W = f.W, H = f.H;
    const size_t n = (size_t)W * H;
    std::vector<uint32_t> parent(n);
    auto fg = [&](int x, int y) { return !f.mask || foreground(f.mask[(size_t)y * f.ms + x], rule.lo, rule.hi); };
    auto link = [&](int x, int y, int xb, int yb) {
        if (xb < 0 || xb >= W || yb < 0 || parent[(size_t)yb * W + xb] == kBackground) return;
        if (rule.thr > 0.0f) {
            const float *ua = hsgm::frow(f.u, f.fs, y), *va = hsgm::frow(f.v, f.fs, y), *ub = hsgm::frow(f.u, f.fs, yb), *vb = hsgm::frow(f.v, f.fs, yb);
            if (!joined(ua[x], va[x], ub[xb], vb[xb], rule.thr)) return;
        }
        unite(parent, (uint32_t)((size_t)y * W + x), (uint32_t)((size_t)yb * W + xb));
    };
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            parent[i] = fg(x, y) ? (uint32_t)i : kBackground;
            if (parent[i] == kBackground) continue;
            link(x, y, x - 1, y);
            link(x, y, x, y - 1);
            if (rule.conn == 8) {
                link(x, y, x - 1, y - 1);
                link(x, y, x + 1, y - 1);
            }
        }
    std::vector<uint32_t> area(n, 0u);
    uint64_t fg_px = 0;
    for (size_t i = 0; i < n; i++)
        if (parent[i] != kBackground) {
            parent[i] = find(parent, (uint32_t)i);
            area[parent[i]]++;
            fg_px++;
        }
    // roots in ascending order: the area word of a root becomes its number (0: dropped)
    uint32_t n_regions = 0, n_roots = 0;
    uint64_t dropped_px = 0, key = 0;
    for (size_t i = 0; i < n; i++) {
        if (parent[i] != i) continue;
        n_roots++;
        const uint32_t a = area[i];
        if (a < rule.min_area) {
            dropped_px += a;
            area[i] = 0;
            continue;
        }
        const uint32_t k = ++n_regions;
        area[i] = k;
        const uint64_t cand = largest_key(a, k);
        key = cand > key ? cand : key;
        if (records && k <= capacity) {
            Record &r = records[k - 1];
            r.root = (uint32_t)i; r.area = a;
            r.x0 = r.y0 = 0xffff; r.x1 = r.y1 = 0;
            r.sum_x = r.sum_y = 0; r.n_flow = 0; r.reserved0 = 0; r.sum_qu = r.sum_qv = 0; r.reserved1 = 0;
        }
    }
    uint64_t unknown_px = 0;
    for (int y = 0; y < H; y++) {
        int32_t *row = labels ? (int32_t *)((uint8_t *)labels + (size_t)y * ls) : nullptr;
        const float *ru = f.u ? hsgm::frow(f.u, f.fs, y) : nullptr, *rv = f.u ? hsgm::frow(f.v, f.fs, y) : nullptr;
        for (int x = 0; x < W; x++) {
            const uint32_t p = parent[(size_t)y * W + x];
            const uint32_t k = p == kBackground ? 0u : area[p];
            if (row) row[x] = (int32_t)k;
            if (p == kBackground) continue;
            const bool known = f.u && flow_known(ru[x], rv[x]);
            if (f.u && !known) unknown_px++;
            if (!records || k == 0 || k > capacity) continue;
            Record &r = records[k - 1];
            r.x0 = x < r.x0 ? (uint16_t)x : r.x0; r.x1 = x > r.x1 ? (uint16_t)x : r.x1;
            r.y0 = y < r.y0 ? (uint16_t)y : r.y0; r.y1 = y > r.y1 ? (uint16_t)y : r.y1;
            r.sum_x += (uint64_t)x; r.sum_y += (uint64_t)y;
            if (known) {
                r.n_flow++;
                r.sum_qu += hsgm::quant(ru[x]);
                r.sum_qv += hsgm::quant(rv[x]);
            }
        }
    }
    if (result) finish_result(result, n_regions, n_roots, capacity, fg_px, dropped_px, unknown_px, key);
}

} // namespace hsrg
