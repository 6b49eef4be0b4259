// corners_host_san.cpp -- the corner rule (csrc/hs_corners_rule.h, included alone) under -fsanitize=address,undefined: both
// kinds on extreme planes -- all 0, all 255, 1-pixel stripes, the 1-pixel checker that maximises A * C -- in heap buffers
// that are exactly as large as the rule may touch, so a read or a write one byte outside is reported, as is any signed
// overflow in the sums and the scores.  Built and run by tests/test_corners_host.py; prints "corners rule: ok".
#include "hs_corners_rule.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

int failures = 0;

void check(bool ok, const char *what, int a, int b, int c)
{
    if (ok) return;
    std::printf("FAILED: %s (%d, %d, %d)\n", what, a, b, c);
    failures++;
}

// pattern 0: all 0; 1: all 255; 2: vertical stripes; 3: horizontal stripes; 4: the 1-pixel checker
uint8_t pixel(int pattern, int x, int y)
{
    switch (pattern) {
    case 0: return 0;
    case 1: return 255;
    case 2: return x & 1 ? 255 : 0;
    case 3: return y & 1 ? 255 : 0;
    default: return (x + y) & 1 ? 255 : 0;
    }
}

void run(int pattern, int W, int H, int kind, int block_r, int nms_r, uint32_t capacity, bool with_mask)
{
    // rows packed: the last row ends where the buffer ends
    uint8_t *g = (uint8_t *)std::malloc((size_t)W * H), *m = with_mask ? (uint8_t *)std::malloc((size_t)W * H) : nullptr;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            g[(size_t)y * W + x] = pixel(pattern, x, y);
            if (m) m[(size_t)y * W + x] = (uint8_t)((x * 7 + y * 3) % 5);
        }
    hscn::Record *rec = capacity ? (hscn::Record *)std::malloc(sizeof(hscn::Record) * capacity) : nullptr;
    float *xy = capacity ? (float *)std::malloc(8 * (size_t)capacity) : nullptr;
    hscn::Result *res = (hscn::Result *)std::malloc(sizeof(hscn::Result));
    const hscn::Rule rule = {kind, block_r, nms_r, 655u, 0, 1u, 255u, 7u, 1};
    hscn::corners_rows(g, (size_t)W, W, H, m, (size_t)W, rule, rec, capacity, xy, res);
    check(res->n_candidates <= 7u && res->n_written <= capacity && res->n_written <= res->n_candidates, "counts", pattern, W, H);
    check(res->smax >= 0 && res->threshold >= 1 && res->strong_px <= res->allowed_px && res->allowed_px <= (uint64_t)W * H, "header", pattern, W, H);
    if (pattern < 2) check(res->smax == 0 && res->n_survivors == 0, "a constant plane has no corners", pattern, W, H);
    if (kind == hscn::kMinEigen && (pattern == 2 || pattern == 3)) check(res->smax == 0, "stripes have one eigenvalue only", pattern, W, H);
    for (uint32_t k = 0; k < res->n_written; k++) {
        check(rec[k].index == (uint32_t)rec[k].y * (uint32_t)W + rec[k].x && rec[k].x < W && rec[k].y < H, "record", pattern, (int)k, kind);
        check(rec[k].score >= res->threshold && rec[k].score <= res->smax, "score", pattern, (int)k, kind);
        if (k) check(hscn::ranks_before(rec[k - 1].score, rec[k - 1].index, rec[k].score, rec[k].index), "rank order", pattern, (int)k, kind);
        check(xy[2 * k] == (float)rec[k].x && xy[2 * k + 1] == (float)rec[k].y, "xy", pattern, (int)k, kind);
    }
    for (uint32_t k = res->n_written; k < capacity; k++) {
        uint32_t bits[2];
        memcpy(bits, xy + 2 * (size_t)k, 8);
        check(bits[0] == hscn::kNanBits && bits[1] == hscn::kNanBits, "NaN tail", pattern, (int)k, kind);
    }
    std::free(g); std::free(m); std::free(rec); std::free(xy); std::free(res);
}

} // namespace

int main()
{
    // no plane reaches the largest sums a window can hold in A and C at once (in the 1-pixel checker's interior the Sobel
    // pair cancels; its gradients live at the frame's edge), so the scores of the bounds themselves are formed here
    const int32_t top = (int32_t)hscn::kMaxSum;
    check(hscn::score(hscn::kHarris, top, 0, top) == 25ll * top * top - 4ll * top * top, "Harris at the bound", 0, 0, 0);
    check(hscn::score(hscn::kHarris, top, top, top) == -4ll * top * top, "Harris at the lower bound", 0, 0, 0);
    check(hscn::score(hscn::kHarris, top, -top, top) == -4ll * top * top, "Harris at the lower bound, B negative", 0, 0, 0);
    check(hscn::score(hscn::kMinEigen, top, 0, top) == 2ll * top, "MIN_EIGEN at the bound", 0, 0, 0);
    check(hscn::score(hscn::kMinEigen, top, top, top) == 0 && hscn::score(hscn::kMinEigen, top, -top, top) == 0, "MIN_EIGEN, 4 B^2 at its largest", 0, 0, 0);
    check(hscn::score(hscn::kMinEigen, top, 0, 0) == 0 && hscn::score(hscn::kMinEigen, 0, 0, top) == 0, "MIN_EIGEN, (A - C)^2 at its largest", 0, 0, 0);
    check(hscn::ceil_sqrt(0) == 0 && hscn::ceil_sqrt(1) == 1 && hscn::ceil_sqrt(2) == 2 && hscn::ceil_sqrt(4) == 2 && hscn::ceil_sqrt(5) == 3, "small roots", 0, 0, 0);
    for (uint64_t r = (1ull << 27) - 3; r < (1ull << 27) + 3; r++) {
        check(hscn::ceil_sqrt(r * r) == r && hscn::ceil_sqrt(r * r + 1) == r + 1 && hscn::ceil_sqrt(r * r - 1) == r, "roots around 2^27", (int)(r & 7), 0, 0);
    }
    check(hscn::threshold(INT64_MAX, 1, 65535u) > 0, "the threshold of the largest int64", 0, 0, 0);
    const int sizes[][2] = {{1, 1}, {1, 7}, {5, 1}, {2, 2}, {9, 6}, {33, 17}};
    for (int pattern = 0; pattern < 5; pattern++)
        for (const auto &s : sizes)
            for (int kind = 0; kind < 2; kind++)
                for (int block_r = 1; block_r <= 3; block_r += 2)
                    for (int nms_r = 1; nms_r <= 8; nms_r += 7) {
                        run(pattern, s[0], s[1], kind, block_r, nms_r, 4u, false);
                        run(pattern, s[0], s[1], kind, block_r, nms_r, 0u, true);
                    }
    if (failures) return 1;
    std::printf("corners rule: ok\n");
    return 0;
}
