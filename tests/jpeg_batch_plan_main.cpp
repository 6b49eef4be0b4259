// The batch layout of the device JPEG encoder (opticalflowhs_amd/csrc/hs_jpeg_batch_plan.h) alone, no HIP: a program of
// its own, built with AddressSanitizer and UBSan by tests/test_jpeg_batch_host.py.  argv[1]: the batch maximum
// (HSFLOW_JPEG_BATCH_MAX of include/hsflow.h).  For W x H over every residue modulo 16 in 1..80 x 1..60 plus 600 x 480 and
// 1920 x 1080, and n in 1 .. 3 * maximum:
//   every picture's part of every range is 256-aligned, inside the total and disjoint from every other;
//   a slice holds 6 * MW * MH blocks x 128 B of coefficients, and its raw stream is nb * 208 bytes rounded up to whole
//   128-byte chunks (what jpeg_prepare of hs_jpeg.hip.h computes for the single encode), written out here once more;
//   the raw streams of a chunk lie behind each other (one memset), the size words are 8 bytes apart;
//   chunks cover 0 .. n exactly once, in order, none above the maximum; the total equals the sum of the ranges.
#include "hs_jpeg_batch_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

using namespace hsjpeg_plan;

static int g_w = 0, g_h = 0, g_n = 0;

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s (%d x %d, n = %d)\n", __LINE__, #cond, g_w, g_h, g_n); return 1; }      \
    } while (0)

struct Range { size_t lo, hi; };

static size_t up(size_t v) { return (v + 255) / 256 * 256; }

static int check_layout(int W, int H, int pictures)
{
    g_w = W; g_h = H; g_n = pictures;
    const Layout l = layout(W, H, pictures);
    const size_t mw = ((size_t)W + 15) / 16, mh = ((size_t)H + 15) / 16, nb = 6 * mw * mh;
    const size_t raw = (nb * 208 + 127) / 128 * 128, nch = raw / 128;
    CHECK(l.pictures == pictures && (size_t)l.s.nb == nb && l.s.raw_bytes == raw && (size_t)l.s.nchunks == nch);
    CHECK(raw % 128 == 0 && raw >= nb * 208 && raw < nb * 208 + 128);
    CHECK(l.s.s_coef == up(nb * 128) && l.s.s_raw == up(raw) && l.s.s_off == up((nb + 1) * 8) && l.s.s_ffoff == up((nch + 1) * 8) &&
          l.s.s_len == up(nb * 4) && l.s.s_ff == up(nch * 4));
    std::vector<Range> r;
    size_t sum = 0;
    const std::pair<size_t, std::pair<size_t, size_t>> ranges[] = { // start, (stride, bytes used per picture)
        {l.o_coef, {l.s.s_coef, nb * 128}}, {l.o_raw, {l.s.s_raw, raw}}, {l.o_off, {l.s.s_off, (nb + 1) * 8}},
        {l.o_ffoff, {l.s.s_ffoff, (nch + 1) * 8}}, {l.o_len, {l.s.s_len, nb * 4}}, {l.o_ff, {l.s.s_ff, nch * 4}}};
    for (const auto &g : ranges) {
        CHECK(g.first % 256 == 0 && g.second.first % 256 == 0 && g.second.second <= g.second.first);
        for (int i = 0; i < pictures; i++) {
            const size_t lo = g.first + (size_t)i * g.second.first;
            CHECK(lo % 256 == 0 && lo + g.second.second <= l.total);
            r.push_back(Range{lo, lo + g.second.second});
        }
        sum += g.second.first * (size_t)pictures;
    }
    CHECK(l.o_size % 256 == 0 && l.o_size + (size_t)pictures * 8 <= l.total);
    r.push_back(Range{l.o_size, l.o_size + (size_t)pictures * 8}); // the size words: 8 bytes apart, one copy
    sum += up((size_t)pictures * 8);
    CHECK(l.total == sum);
    std::sort(r.begin(), r.end(), [](const Range &a, const Range &b) { return a.lo < b.lo; });
    for (size_t i = 1; i < r.size(); i++) CHECK(r[i - 1].hi <= r[i].lo);
    // one memset over the raw streams of the first k pictures touches nothing else
    CHECK(l.o_raw + (size_t)pictures * l.s.s_raw == l.o_off);
    if (pictures == 1) { // the single encode's own allocation (jpeg_prepare): the same ranges in the same order
        const size_t total1 = up(nb * 128) + up(raw) + up((nb + 1) * 8) + up((nch + 1) * 8) + up(nb * 4) + up(nch * 4) + 256;
        CHECK(l.total == total1 && l.o_raw == up(nb * 128));
    }
    return 0;
}

static int check_chunks(int n, int maxb)
{
    g_w = g_h = 0; g_n = n;
    const std::vector<Chunk> cs = chunks(n, maxb);
    CHECK((int)cs.size() == (n + maxb - 1) / maxb);
    int next = 0;
    for (const Chunk &c : cs) {
        CHECK(c.first == next && c.count >= 1 && c.count <= maxb);
        CHECK(c.count == maxb || c.first + c.count == n); // only the last chunk is short
        next += c.count;
    }
    CHECK(next == n);
    return 0;
}

int main(int argc, char **argv)
{
    const int maxb = argc > 1 ? std::atoi(argv[1]) : 8;
    if (maxb < 1) { std::printf("usage: %s <batch maximum>\n", argv[0]); return 2; }
    std::vector<std::pair<int, int>> sizes;
    for (int rw = 0; rw < 16; rw++)
        for (int rh = 0; rh < 16; rh++) {
            // every residue of W with every residue of H; the multiples of 16 added walk through 1..80 x 1..60
            const int W = rw + 1 + 16 * ((rw + 3 * rh) % 4), H = rh + 1 + 16 * ((2 * rw + rh) % 3);
            sizes.push_back({W > 80 ? 80 : W, H > 60 ? 60 : H});
        }
    sizes.push_back({80, 60});
    sizes.push_back({600, 480});
    sizes.push_back({1920, 1080});
    long layouts = 0;
    for (const auto &wh : sizes)
        for (int n = 1; n <= 3 * maxb; n++) {
            if (check_layout(wh.first, wh.second, n < maxb ? n : maxb)) return 1; // (the allocation holds one chunk)
            if (check_layout(wh.first, wh.second, n)) return 1;                   // ... and the layout is sound for any count
            layouts += 2;
        }
    for (const auto &wh : sizes) { // a batch of one with a maximum of 1: one slice, the one chunk (0, 1)
        if (check_layout(wh.first, wh.second, 1)) return 1;
        layouts++;
    }
    {
        if (check_chunks(1, 1)) return 1;
        const std::vector<Chunk> one = chunks(1, 1);
        if (one.size() != 1 || one[0].first != 0 || one[0].count != 1) { std::printf("FAILED: chunks(1, 1)\n"); return 1; }
    }
    for (int n = 1; n <= 3 * maxb; n++)
        for (int m = 1; m <= maxb; m++)
            if (check_chunks(n, m)) return 1;
    std::printf("batch plan ok: %ld layouts, %d sizes, maximum %d\n", layouts, (int)sizes.size(), maxb);
    return 0;
}
