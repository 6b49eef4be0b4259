// The pyramid's two host rules (csrc/hs_pyramid_rule.h) as a stand-alone program for AddressSanitizer and UBSan: every
// shape of tests/test_pyramid_host.py with exact-size heap blocks, so a byte read or written beyond a plane is caught.
// Prints one line per shape: "W H <FNV-1a of the down plane> <FNV-1a of the two prolonged planes>"; the test computes the
// same from the library.  Input: the LCG x <- 1664525 x + 1013904223 (mod 2^32) from the seed 12345 + 1000 W + H, a byte is
// x >> 24, a float is ((x >> 16) - 32768) / 64.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "hs_pyramid_rule.h"

namespace {

struct Lcg {
    uint32_t x;
    uint32_t next() { return x = x * 1664525u + 1013904223u; }
};

uint32_t fnv(uint32_t h, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 16777619u;
    return h;
}

void run(int W, int H)
{
    Lcg g{12345u + 1000u * (uint32_t)W + (uint32_t)H};
    const int Wd = hspyr::half_up(W), Hd = hspyr::half_up(H);
    std::unique_ptr<uint8_t[]> src(new uint8_t[(size_t)W * H]), dst(new uint8_t[(size_t)Wd * Hd]);
    for (int i = 0; i < W * H; i++) src[i] = (uint8_t)(g.next() >> 24);
    hspyr::down_rows(src.get(), (size_t)W, W, H, dst.get(), (size_t)Wd);
    const uint32_t hd = fnv(2166136261u, dst.get(), (size_t)Wd * Hd);
    // the coarse plane W x H prolonged to both fine sizes it can come from: 2W x 2H and (2W-1) x (2H-1)
    std::unique_ptr<float[]> c(new float[(size_t)W * H]);
    for (int i = 0; i < W * H; i++) c[i] = (float)((int)(g.next() >> 16) - 32768) / 64.0f;
    uint32_t hp = 2166136261u;
    for (int odd = 0; odd < 2; odd++) {
        const int Wf = 2 * W - odd, Hf = 2 * H - odd;
        std::unique_ptr<float[]> f(new float[(size_t)Wf * Hf]);
        hspyr::prolong_rows(c.get(), (size_t)W * 4, Wf, Hf, f.get(), (size_t)Wf * 4);
        hp = fnv(hp, f.get(), (size_t)Wf * Hf * 4);
    }
    std::printf("%d %d %08x %08x\n", W, H, hd, hp);
}

} // namespace

int main()
{
    const int shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {5, 3}, {67, 45}, {160, 128}};
    for (const auto &s : shapes) run(s[0], s[1]);
    // the plan: auto, explicit, and the refusal beyond 1 x 1
    int w[hspyr::kMaxLevels], h[hspyr::kMaxLevels];
    std::printf("plan %d %d %d %d\n", hspyr::plan(160, 128, 0, 32, w, h), hspyr::plan(1920, 1080, 0, 32, w, h), hspyr::plan(1, 1, 0, 32, w, h),
                hspyr::plan(3, 2, 4, 32, w, h));
    return 0;
}
