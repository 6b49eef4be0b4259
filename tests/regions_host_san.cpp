// regions_host_san.cpp -- the labelling rule (csrc/hs_regions_rule.h) alone, on the host, for a build with
// -fsanitize=address,undefined (tests/test_regions_host.py builds and runs it): the masks a labelling gets wrong and flow
// fields with the extreme values the rule knows, at (260, 37) and (1, 40), with ragged strides.  Every buffer is exactly as
// large as the rule may touch, so a step beyond a row's width or a record too many is the sanitizer's to report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "hs_regions_rule.h"

static unsigned long long lcg = 88172645463325252ull;
static float rnd()
{
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((lcg >> 40) & 0xffff) / 65536.0f;
}

// pattern: 0 empty, 1 full, 2 checkerboard, 3 comb with its spine in the last row, 4 serpentine, 5 .. 7 random at 0.3, 0.59, 0.8
static uint8_t pattern(int kind, int x, int y, int W, int H)
{
    switch (kind) {
    case 0: return 0;
    case 1: return 255;
    case 2: return ((x + y) & 1) ? 0 : 200;
    case 3: return (x % 2 == 0 || y == H - 1) ? 255 : 0;
    case 4: return (y % 2 == 0 || x == ((y / 2) % 2 ? 0 : W - 1)) ? 9 : 0;
    default: return rnd() < (kind == 5 ? 0.3f : kind == 6 ? 0.59f : 0.8f) ? (uint8_t)(1 + (int)(rnd() * 254.0f)) : 0;
    }
}

static int run(int W, int H, int pad)
{
    const size_t bs = (size_t)W + (size_t)pad, fs = (size_t)(W + pad) * 4;
    // the last row ends at its width: no padding behind it
    std::vector<uint8_t> mask(bs * (H - 1) + W);
    std::vector<float> u((size_t)(W + pad) * (H - 1) + W), v(u.size());
    std::vector<int32_t> labels(u.size());
    const float special[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                             1.0000001e9f, 2048.0f, -2048.0f, std::nextafterf(2048.0f, 4096.0f), -0.0f, 0.5f / 256.0f, 1.5f / 256.0f, 3e38f, 1e-42f};
    int bad = 0;
    for (int kind = 0; kind < 8; kind++) {
        uint64_t fg = 0;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t i = (size_t)y * (W + pad) + x;
                mask[(size_t)y * bs + x] = pattern(kind, x, y, W, H);
                fg += mask[(size_t)y * bs + x] != 0;
                u[i] = 0.4f * (float)x + 0.3f * rnd();
                v[i] = -0.2f * (float)y + 0.3f * rnd();
                if (rnd() < 0.05f) u[i] = special[(int)(rnd() * 11.99f)];
                if (rnd() < 0.05f) v[i] = special[(int)(rnd() * 11.99f)];
            }
        for (int conn = 4; conn <= 8; conn += 4)
            for (int flow = 0; flow < 3; flow++)
                for (unsigned min_area = 1; min_area <= 5; min_area += 4)
                    for (uint32_t capacity = 0; capacity <= 6; capacity += 3) {
                        const hsrg::Field f = {mask.data(), bs, flow ? u.data() : nullptr, flow ? v.data() : nullptr, fs, W, H};
                        const hsrg::Rule rule = {conn, 1u, 255u, min_area, flow == 2 ? 0.25f : 0.0f};
                        std::vector<hsrg::Record> records(capacity);
                        hsrg::Result r;
                        hsrg::label_rows(f, rule, labels.data(), fs, capacity ? records.data() : nullptr, capacity, &r);
                        if (r.fg_px != fg || r.n_written != (r.n_regions < capacity ? r.n_regions : capacity)) bad++;
                        uint64_t kept = 0;
                        for (int y = 0; y < H; y++)
                            for (int x = 0; x < W; x++) {
                                const int32_t k = labels[(size_t)y * (W + pad) + x];
                                if (k < 0 || (uint32_t)k > r.n_regions || ((k != 0) && !mask[(size_t)y * bs + x])) bad++;
                                kept += k != 0;
                            }
                        if (kept + r.dropped_px != fg) bad++;
                        uint64_t in_records = 0;
                        for (uint32_t k = 0; k < r.n_written; k++) {
                            const hsrg::Record &q = records[k];
                            in_records += q.area;
                            if (q.area < min_area || q.x0 > q.x1 || q.y0 > q.y1 || q.x1 >= W || q.y1 >= H || q.root / (uint32_t)W != q.y0) bad++;
                            if (q.n_flow > q.area || (!flow && (q.n_flow || q.sum_qu || q.sum_qv))) bad++;
                        }
                        if (r.n_written == r.n_regions && in_records != kept) bad++;
                        if (kind == 1 && !flow && (r.n_regions != 1 || r.largest_area != (uint32_t)(W * H))) bad++;
                    }
    }
    // no mask at all: every pixel is foreground
    {
        const hsrg::Field f = {nullptr, 0, nullptr, nullptr, 0, W, H};
        const hsrg::Rule rule = {4, 1u, 255u, 1u, 0.0f};
        hsrg::Result r;
        hsrg::label_rows(f, rule, nullptr, 0, nullptr, 0, &r);
        if (r.n_regions != 1 || r.fg_px != (uint64_t)W * H || !(r.flags & hsrg::kFlagOverflow)) bad++;
    }
    return bad;
}

int main()
{
    const int shapes[][2] = {{260, 37}, {1, 40}};
    int bad = 0;
    for (const auto &s : shapes)
        for (int pad = 0; pad < 4; pad += 3) bad += run(s[0], s[1], pad);
    if (bad) {
        std::printf("regions rule: %d failures\n", bad);
        return 1;
    }
    std::printf("regions rule: ok\n");
    return 0;
}
