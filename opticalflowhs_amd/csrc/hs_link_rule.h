// hs_link_rule.h -- the moving objects of a SEQUENCE: the regions of frame k (a label plane A, hs_regions_rule.h's or any
// other) linked to the regions of frame k + 1 (a label plane B) by the flow of the pair k -> k + 1.  ONE definition for the
// device kernels (hs_kernels_link.hip.h) and the host form (hsflow_link_regions_host), the way hs_regions_rule.h serves both
// sides of the labelling.
//   Pixel.  (x, y) with a = A[y][x] > 0 (a value <= 0 is background and does nothing):
//     a > cap_a                                  counts into over_a_px, nothing else;
//     s = hsinterp::target(u, v, x, y, 1, W, H)  the landing rule of the interpolation operator, bit for bit;
//     s unknown or left                          counts into gone_px of a;
//     b = B[s.qy][s.qx] <= 0 or > cap_b          counts into unmatched_px of a;
//     else                                       ONE VOTE for the cell (a, b).
//   Every labelled pixel therefore adds 1 to exactly one word of ONE table of cap_a * cap_b + 2 * cap_a + 1 words (word_of):
//   the cell matrix in raster order of (a, b), the gone tallies, the unmatched tallies, over_a.  All outputs are functions
//   of that table:
//     links    the non-zero cells in raster order, which is ascending (a, b);
//     side_a   per row a: px = gone + unmatched + the row's votes, n_links = its non-zero cells, best = the b of the largest
//              cell -- a tie to the smaller b: the maximum of px << 32 | ~b (best_key), as hsrg::largest_key -- 0 with no vote;
//     side_b   the same over the columns; px = the arrivals, gone = unmatched = 0;
//     result   the totals and n_mutual, the pairs with best(a) == b and best(b) == a.
//   Every quantity is an exact integer count: the order of arrival cannot matter, device and host agree byte for byte.
//   Tracks (host only, link_tracks): the ids of a chain of steps from the side records alone.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "hs_interp_rule.h"
#include "hs_regions_rule.h"

#include <vector>

namespace hsln {

constexpr uint32_t kMaxCells = 1u << 24;  // HSFLOW_LINK_MAX_CELLS: cap_a * cap_b, and link_capacity, at most
constexpr uint32_t kMaxCap = 1u << 30;    // a cap above it is refused before the product is formed
constexpr unsigned kFlagOverflow = 1u;    // more links than records
constexpr uint32_t kNoWord = 0xffffffffu; // a background pixel adds nothing

// ---- no count overflows -------------------------------------------------------------------------------------------------------
static_assert(hsrg::kMaxPixels < (1LL << 32), "a cell, a tally and a side's px count pixels of one frame: 32 bits hold them");
static_assert(hsrg::kMaxPixels <= hsgm::kInt64Max, "the header's sums count pixels of one frame: 64 bits hold them");
static_assert(kMaxCells == (1u << 24), "a cell index is below 2^24");
static_assert((uint64_t)kMaxCells * 3u + 1u < (1ull << 32), "the table's words -- cells, 2 * cap_a <= 2 * cells tallies, over_a -- index in 32 bits");
static_assert(hsrg::kMaxSide == 16384 && hsrg::kMaxPixels == (1LL << 30), "the bounds the asserts above are taken from");

// hsflow_link_record (include/hsflow.h) as both sides write it.
struct Link {
    uint32_t a, b, px, reserved;
};
static_assert(sizeof(Link) == 16, "hsflow_link_record is 16 bytes");

// hsflow_link_side.
struct Side {
    uint32_t px, n_links, best, best_px, gone_px, unmatched_px, reserved[2];
};
static_assert(sizeof(Side) == 32, "hsflow_link_side is 32 bytes");

// hsflow_link_result.
struct Result {
    uint32_t n_links, n_written, flags, n_mutual;
    uint64_t voted_px, gone_px, unmatched_px, over_a_px;
    uint64_t reserved[2];
};
static_assert(sizeof(Result) == 64, "hsflow_link_result is 64 bytes");

// The table of one step: cells | gone | unmatched | over_a.
struct Table {
    uint32_t cap_a, cap_b, cells;
    HSW_FN uint32_t gone(uint32_t a) const { return cells + (a - 1u); }
    HSW_FN uint32_t unmatched(uint32_t a) const { return cells + cap_a + (a - 1u); }
    HSW_FN uint32_t over_a() const { return cells + 2u * cap_a; }
    HSW_FN uint32_t words() const { return cells + 2u * cap_a + 1u; }
};

HSW_FN Table table_of(uint32_t cap_a, uint32_t cap_b) { return Table{cap_a, cap_b, cap_a * cap_b}; }

HSW_FN const int32_t *lrow(const int32_t *p, long long stride, int y) { return (const int32_t *)((const uint8_t *)p + (long long)y * stride); }

// The word of the table that the pixel (x, y) with label a and flow (u, v) adds 1 to; kNoWord for background.  B: the label
// plane of the next frame, rows bs BYTES apart.
HSW_FN uint32_t word_of(const Table &t, int32_t a, float u, float v, int x, int y, int W, int H, const int32_t *B, long long bs)
{
    if (a <= 0) return kNoWord;
    if ((uint32_t)a > t.cap_a) return t.over_a();
    const hsinterp::Splat s = hsinterp::target(u, v, x, y, 1.0f, W, H);
    if (s.cls != hsinterp::kLanded) return t.gone((uint32_t)a);
    const int32_t b = lrow(B, bs, s.qy)[s.qx];
    if (b <= 0 || (uint32_t)b > t.cap_b) return t.unmatched((uint32_t)a);
    return ((uint32_t)a - 1u) * t.cap_b + ((uint32_t)b - 1u);
}

// The larger cell wins, then the smaller label of the other side: one 64-bit key whose maximum is the answer (0: no vote).
HSW_FN uint64_t best_key(uint32_t px, uint32_t other) { return px ? (uint64_t)px << 32 | (uint32_t)~other : 0ull; }
HSW_FN uint32_t best_of(uint64_t key) { return key ? ~(uint32_t)key : 0u; }

HSW_FN void fill_side(Side *s, uint32_t votes, uint32_t n_links, uint64_t key, uint32_t gone, uint32_t unmatched)
{
    s->px = votes + gone + unmatched;
    s->n_links = n_links;
    s->best = best_of(key);
    s->best_px = (uint32_t)(key >> 32);
    s->gone_px = gone;
    s->unmatched_px = unmatched;
    s->reserved[0] = s->reserved[1] = 0u;
}

HSW_FN void finish_result(Result *r, uint32_t n_links, uint32_t link_capacity, uint32_t n_mutual, uint64_t voted, uint64_t gone, uint64_t unmatched, uint64_t over_a)
{
    r->n_links = n_links;
    r->n_written = n_links < link_capacity ? n_links : link_capacity;
    r->flags = n_links > link_capacity ? kFlagOverflow : 0u;
    r->n_mutual = n_mutual;
    r->voted_px = voted;
    r->gone_px = gone;
    r->unmatched_px = unmatched;
    r->over_a_px = over_a;
    r->reserved[0] = r->reserved[1] = 0;
}

// ---- a whole step in host memory: the specification --------------------------------------------------------------------------

struct Step {
    const int32_t *A;
    size_t as;
    const int32_t *B;
    size_t bs;
    const float *u, *v;
    size_t fs; // rows of u and v fs BYTES apart
    int W, H;
};

// links (link_capacity of them), side_a (cap_a), side_b (cap_b) and result may each be NULL.  Writes the first
// min(n_links, link_capacity) links, every side record, the result, and nothing else.
inline void link_rows(const Step &f, uint32_t cap_a, uint32_t cap_b, Link *links, uint32_t link_capacity, Side *side_a, Side *side_b, Result *result)
{
    const Table t = table_of(cap_a, cap_b);
    std::vector<uint32_t> tab(t.words(), 0u);
    for (int y = 0; y < f.H; y++) {
        const int32_t *ra = lrow(f.A, (long long)f.as, y);
        const float *ru = hsgm::frow(f.u, f.fs, y), *rv = hsgm::frow(f.v, f.fs, y);
        for (int x = 0; x < f.W; x++) {
            const uint32_t w = word_of(t, ra[x], ru[x], rv[x], x, y, f.W, f.H, f.B, (long long)f.bs);
            if (w != kNoWord) tab[w]++;
        }
    }
    std::vector<uint64_t> col_key(cap_b, 0ull);
    std::vector<uint32_t> col_px(cap_b, 0u), col_n(cap_b, 0u), row_best(cap_a, 0u);
    uint32_t n_links = 0;
    uint64_t voted = 0, gone = 0, unmatched = 0;
    for (uint32_t a = 1; a <= cap_a; a++) {
        uint32_t votes = 0, n = 0;
        uint64_t key = 0;
        for (uint32_t b = 1; b <= cap_b; b++) {
            const uint32_t px = tab[(a - 1u) * cap_b + (b - 1u)];
            if (!px) continue;
            if (links && n_links < link_capacity) links[n_links] = Link{a, b, px, 0u};
            n_links++;
            votes += px;
            n++;
            const uint64_t ka = best_key(px, b), kb = best_key(px, a);
            key = ka > key ? ka : key;
            col_key[b - 1u] = kb > col_key[b - 1u] ? kb : col_key[b - 1u];
            col_px[b - 1u] += px;
            col_n[b - 1u]++;
        }
        row_best[a - 1u] = best_of(key);
        voted += votes;
        gone += tab[t.gone(a)];
        unmatched += tab[t.unmatched(a)];
        if (side_a) fill_side(side_a + (a - 1u), votes, n, key, tab[t.gone(a)], tab[t.unmatched(a)]);
    }
    uint32_t n_mutual = 0;
    for (uint32_t b = 1; b <= cap_b; b++) {
        const uint32_t a = best_of(col_key[b - 1u]);
        if (a && row_best[a - 1u] == b) n_mutual++;
        if (side_b) fill_side(side_b + (b - 1u), col_px[b - 1u], col_n[b - 1u], col_key[b - 1u], 0u, 0u);
    }
    if (result) finish_result(result, n_links, link_capacity, n_mutual, voted, gone, unmatched, tab[t.over_a()]);
}

// ---- tracks: ids over a chain of steps, from the side records alone ----------------------------------------------------------
// side_a[i], side_b[i]: the cap records of step i (frame i -> i + 1); n_regions[k]: the regions of frame k, k = 0 .. n_steps.
// ids: (n_steps + 1) * cap words, ids[k * cap + (label - 1)].  Frame 0's regions get 1 .. min(n_regions[0], cap).  In step i
// region b of frame i + 1, b ascending, continues the id of a = side_b[i][b].best iff a != 0, side_a[i][a].best == b and
// best_px * 256 >= min_share_256 * px of a; otherwise it gets the next fresh id.  Slots above min(n_regions, cap) get 0.
// Returns the number of ids handed out.
inline uint32_t link_tracks(const Side *const *side_a, const Side *const *side_b, const uint32_t *n_regions, int n_steps, uint32_t cap, uint32_t min_share_256,
                            uint32_t *ids)
{
    uint32_t next = 0;
    for (int k = 0; k <= n_steps; k++) {
        const uint32_t n = n_regions[k] < cap ? n_regions[k] : cap;
        uint32_t *row = ids + (size_t)k * cap;
        for (uint32_t b = 1; b <= cap; b++) {
            uint32_t id = 0;
            if (b <= n) {
                if (k > 0) {
                    const uint32_t a = side_b[k - 1][b - 1u].best;
                    if (a != 0u && a <= cap) {
                        const Side &sa = side_a[k - 1][a - 1u];
                        if (sa.best == b && (uint64_t)sa.best_px * 256u >= (uint64_t)min_share_256 * sa.px) id = ids[(size_t)(k - 1) * cap + (a - 1u)];
                    }
                }
                if (!id) id = ++next;
            }
            row[b - 1u] = id;
        }
    }
    return next;
}

} // namespace hsln
