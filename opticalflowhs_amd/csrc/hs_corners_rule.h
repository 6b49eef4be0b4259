// hs_corners_rule.h -- which points of a frame are worth following: corner detection on a u8 gray plane, in integers alone.
// ONE definition for the device kernels (hs_kernels_corners.hip.h) and the host form (hsflow_corners_host), the way
// hs_regions_rule.h serves both sides of the labelling.  A pixel's index is y * W + x.
//   Gradients.  The 3 x 3 Sobel pair, coordinates clamped to the frame (the replicate border):
//     Ix = (g[y-1][x+1] + 2 g[y][x+1] + g[y+1][x+1]) - (the same at x-1), Iy the same along y; both in -1020 .. 1020.
//   Structure tensor.  A = sum Ix^2, B = sum Ix Iy, C = sum Iy^2 over the (2 block_r + 1)^2 window, block_r in 1 .. 3; the
//   window's coordinates are clamped to the frame too, so a border pixel's window counts the edge gradients more than once.
//   Score, an int64.  MIN_EIGEN: S = (A + C) - ceil(sqrt(D)), D = (A - C)^2 + 4 B^2: twice the smaller eigenvalue, rounded
//   down; the root is the exact integer one (ceil_sqrt), so S does not depend on how either side rounds sqrt; S >= 0
//   because (A + C)^2 - D = 4 (A C - B^2) >= 0 (Cauchy-Schwarz).  HARRIS: S = 25 (A C - B^2) - (A + C)^2, k = 1 / 25.
//   Allowed.  A pixel whose mask byte lies in fg_lo .. fg_hi (no mask: every pixel) and that lies at least `border` pixels
//   from every frame edge.  A pixel that is not allowed is no corner and does not count towards the maximum, yet it still
//   competes in the suppression: a mask never creates corners.
//   Threshold.  smax = max(0, max S over allowed pixels); T = max(min_score, (smax >> 16) * quality_q16).
//   Strong.  Allowed and S >= T.
//   Survivors.  A strong pixel p that beats every other pixel q of the frame with max(|dx|, |dy|) <= nms_r; p beats q iff
//   S_p > S_q, or S_p == S_q and index_p < index_q.  No two survivors are closer than nms_r + 1 in either axis.
//   Candidates.  The first max_candidates survivors in ascending index (more: TRUNCATED).
//   Corners.  The candidates by descending S, ties by ascending index; the first `capacity` are the output (more
//   candidates than that: OVERFLOW).
// The overflow proof is the static_asserts below.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define HSCN_FN __host__ __device__ inline
#else
#define HSCN_FN inline
#endif

namespace hscn {

constexpr int kMaxSide = 16384;           // the largest width and height the entry points accept
constexpr int kMinEigen = 0, kHarris = 1; // the kinds
constexpr int kMaxBlockR = 3, kMaxNmsR = 8;
constexpr unsigned kMaxCandidates = 65536u;
constexpr unsigned kMaxCapacity = 1u << 24; // hsflow_track_points' largest m
constexpr unsigned kFlagOverflow = 1u, kFlagTruncated = 2u;
constexpr uint32_t kNanBits = 0x7fc00000u;  // both floats of an empty xy slot
constexpr int64_t kNoScore = INT64_MIN;     // what a place outside the frame holds in the suppression: it loses to everyone

// ---- no sum overflows -------------------------------------------------------------------------------------------------------
constexpr int64_t kMaxGrad = 4 * 255;                                                      // |Ix|, |Iy|
constexpr int64_t kMaxSum = (2 * kMaxBlockR + 1) * (2 * kMaxBlockR + 1) * kMaxGrad * kMaxGrad; // A, C, |B|
static_assert(kMaxSum < (1ll << 26), "A, B, C fit int32 with room");
static_assert((2 * kMaxBlockR + 1) * kMaxGrad * kMaxGrad < (1ll << 23), "a row of the window fits int32");
static_assert(kMaxSum * kMaxSum + 4 * kMaxSum * kMaxSum < (1ll << 55), "D = (A - C)^2 + 4 B^2 fits 64 bits, and a double holds its root to within 1");
static_assert(25 * kMaxSum * kMaxSum < 70000000000000000ll, "0 <= A C - B^2 <= A C, so -(A + C)^2 <= Harris <= 25 A C: |Harris| < 7e16 fits int64");
static_assert((INT64_MAX >> 16) * 65535ll > 0, "(smax >> 16) * quality_q16 cannot overflow: the shift comes first");
static_assert((long long)kMaxSide * kMaxSide <= 0x10000000ll, "a pixel index fits uint32");
static_assert(kMaxSide - 1 <= 0xffff, "a coordinate fits 16 bits");

// hsflow_corners_record (include/hsflow.h) as both sides write it.
struct Record {
    uint16_t x, y;
    uint32_t index;
    int64_t score;
};
static_assert(sizeof(Record) == 16, "hsflow_corners_record is 16 bytes");

// hsflow_corners_result.
struct Result {
    uint32_t n_survivors, n_candidates, n_written, flags;
    int64_t smax, threshold;
    uint64_t allowed_px, strong_px;
    uint64_t reserved[2];
};
static_assert(sizeof(Result) == 64, "hsflow_corners_result is 64 bytes");

struct Rule {
    int kind, block_r, nms_r;
    unsigned quality_q16;
    int border;
    unsigned lo, hi; // the allowed mask bytes
    unsigned max_candidates;
    int64_t min_score;
};

HSCN_FN int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// The Sobel pair from the nine bytes around a pixel: g[j][i], j the row.
HSCN_FN void sobel(const int g[3][3], int *ix, int *iy)
{
    *ix = (g[0][2] + 2 * g[1][2] + g[2][2]) - (g[0][0] + 2 * g[1][0] + g[2][0]);
    *iy = (g[2][0] + 2 * g[2][1] + g[2][2]) - (g[0][0] + 2 * g[0][1] + g[0][2]);
}

// The smallest r with r * r >= D, exactly: the double root is a first guess, 64-bit comparisons settle it.
HSCN_FN uint64_t ceil_sqrt(uint64_t D)
{
    uint64_t r = (uint64_t)sqrt((double)D);
    while (r * r < D) r++;
    while (r > 0 && (r - 1) * (r - 1) >= D) r--;
    return r;
}

HSCN_FN int64_t score(int kind, int32_t A, int32_t B, int32_t C)
{
    const int64_t a = A, b = B, c = C;
    if (kind == kHarris) return 25 * (a * c - b * b) - (a + c) * (a + c);
    const uint64_t D = (uint64_t)((a - c) * (a - c)) + 4u * (uint64_t)(b * b);
    return (a + c) - (int64_t)ceil_sqrt(D);
}

HSCN_FN bool allowed(bool in_mask, int x, int y, int W, int H, int border) { return in_mask && x >= border && y >= border && x < W - border && y < H - border; }

HSCN_FN bool in_mask(unsigned byte, unsigned lo, unsigned hi) { return byte >= lo && byte <= hi; }

HSCN_FN int64_t threshold(int64_t smax, int64_t min_score, unsigned quality_q16)
{
    const int64_t t = (smax >> 16) * (int64_t)quality_q16;
    return t > min_score ? t : min_score;
}

// Does the pixel with score sq, `earlier` in index order or not, keep p (score sp) from surviving?
HSCN_FN bool loses_to(int64_t sp, int64_t sq, bool earlier) { return sq > sp || (sq == sp && earlier); }

// Among candidates: does (sa, ia) rank in front of (sb, ib)?
HSCN_FN bool ranks_before(int64_t sa, uint32_t ia, int64_t sb, uint32_t ib) { return sa > sb || (sa == sb && ia < ib); }

HSCN_FN void finish_result(Result *r, uint32_t n_survivors, unsigned max_candidates, uint32_t capacity, int64_t smax, int64_t thr, uint64_t allowed_px,
                           uint64_t strong_px)
{
    const uint32_t n_cand = n_survivors < max_candidates ? n_survivors : max_candidates;
    r->n_survivors = n_survivors;
    r->n_candidates = n_cand;
    r->n_written = n_cand < capacity ? n_cand : capacity;
    r->flags = (n_cand > capacity ? kFlagOverflow : 0u) | (n_survivors > max_candidates ? kFlagTruncated : 0u);
    r->smax = smax;
    r->threshold = thr;
    r->allowed_px = allowed_px;
    r->strong_px = strong_px;
    r->reserved[0] = r->reserved[1] = 0;
}

HSCN_FN void write_record(Record *rec, uint32_t index, int W, int64_t s)
{
    rec->x = (uint16_t)(index % (uint32_t)W);
    rec->y = (uint16_t)(index / (uint32_t)W);
    rec->index = index;
    rec->score = s;
}

// ---- a whole frame in host memory: the specification, written plainly ----------------------------------------------------------

// The score of every pixel into S (W * H of them).
inline void score_plane(const uint8_t *g, size_t gs, int W, int H, const Rule &rule, int64_t *S)
{
    const size_t n = (size_t)W * H;
    std::vector<int32_t> xx(n), xy(n), yy(n);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int nb[3][3];
            for (int j = 0; j < 3; j++)
                for (int i = 0; i < 3; i++) nb[j][i] = g[(size_t)clampi(y + j - 1, H - 1) * gs + clampi(x + i - 1, W - 1)];
            int ix, iy;
            sobel(nb, &ix, &iy);
            xx[(size_t)y * W + x] = ix * ix;
            xy[(size_t)y * W + x] = ix * iy;
            yy[(size_t)y * W + x] = iy * iy;
        }
    const int r = rule.block_r;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int32_t A = 0, B = 0, C = 0;
            for (int dy = -r; dy <= r; dy++)
                for (int dx = -r; dx <= r; dx++) {
                    const size_t q = (size_t)clampi(y + dy, H - 1) * W + clampi(x + dx, W - 1);
                    A += xx[q]; B += xy[q]; C += yy[q];
                }
            S[(size_t)y * W + x] = score(rule.kind, A, B, C);
        }
}

// records (capacity of them), xy (capacity pairs) and result may each be NULL.  Writes the records of the ranks below
// n_written, every pair of xy, the result, and nothing else.
inline void corners_rows(const uint8_t *g, size_t gs, int W, int H, const uint8_t *mask, size_t ms, const Rule &rule, Record *records, uint32_t capacity, float *xy,
                         Result *result)
{
    const size_t n = (size_t)W * H;
    std::vector<int64_t> S(n);
    score_plane(g, gs, W, H, rule, S.data());
    auto ok = [&](int x, int y) { return allowed(!mask || in_mask(mask[(size_t)y * ms + x], rule.lo, rule.hi), x, y, W, H, rule.border); };
    int64_t smax = 0;
    uint64_t allowed_px = 0, strong_px = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            if (ok(x, y)) {
                allowed_px++;
                smax = S[(size_t)y * W + x] > smax ? S[(size_t)y * W + x] : smax;
            }
    const int64_t T = threshold(smax, rule.min_score, rule.quality_q16);
    std::vector<Record> cand;
    uint32_t n_survivors = 0;
    const int r = rule.nms_r;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const int64_t sp = S[(size_t)y * W + x];
            if (!ok(x, y) || sp < T) continue;
            strong_px++;
            bool alive = true;
            for (int dy = -r; dy <= r && alive; dy++)
                for (int dx = -r; dx <= r; dx++) {
                    const int xq = x + dx, yq = y + dy;
                    if ((dx == 0 && dy == 0) || xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
                    if (loses_to(sp, S[(size_t)yq * W + xq], dy < 0 || (dy == 0 && dx < 0))) {
                        alive = false;
                        break;
                    }
                }
            if (!alive) continue;
            if (n_survivors++ < rule.max_candidates) {
                Record rec;
                write_record(&rec, (uint32_t)((size_t)y * W + x), W, sp);
                cand.push_back(rec);
            }
        }
    std::sort(cand.begin(), cand.end(), [](const Record &a, const Record &b) { return ranks_before(a.score, a.index, b.score, b.index); });
    Result res;
    finish_result(&res, n_survivors, rule.max_candidates, capacity, smax, T, allowed_px, strong_px);
    for (uint32_t k = 0; k < res.n_written; k++) {
        if (records) records[k] = cand[k];
        if (xy) {
            xy[2 * (size_t)k] = (float)cand[k].x;
            xy[2 * (size_t)k + 1] = (float)cand[k].y;
        }
    }
    if (xy)
        for (size_t k = res.n_written; k < capacity; k++) {
            memcpy(xy + 2 * k, &kNanBits, 4);
            memcpy(xy + 2 * k + 1, &kNanBits, 4);
        }
    if (result) *result = res;
}

} // namespace hscn
