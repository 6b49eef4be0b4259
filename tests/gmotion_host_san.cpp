// gmotion_host_san.cpp -- the global-motion rule (csrc/hs_gmotion_rule.h) alone, on the host, for a build with
// -fsanitize=address,undefined (tests/test_gmotion_host.py builds and runs it): the fit and the warp by a model on odd
// shapes with ragged strides, on fields of the extreme values the rule knows, and on the largest sums.  Every buffer is
// exactly as large as the rule may touch, so a step beyond a row's width is the sanitizer's to report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "hs_gmotion_rule.h"

static unsigned long long lcg = 88172645463325252ull;
static float rnd()
{
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((lcg >> 40) & 0xffff) / 65536.0f;
}

static int run(int W, int H, int pad, bool extreme)
{
    const size_t fs = (size_t)(W + pad) * 4, bs = (size_t)W + (size_t)pad;
    // the last row ends at its width: no padding behind it
    std::vector<float> u((size_t)(W + pad) * (H - 1) + W), v(u.size()), ru(u.size()), rv(u.size());
    std::vector<uint8_t> state(bs * (H - 1) + W), mask(state.size());
    const float special[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                             1.0000001e9f, 2048.0f, -2048.0f, std::nextafterf(2048.0f, 4096.0f), -0.0f, 0.5f / 256.0f, 1.5f / 256.0f, 3e38f, 1e-42f};
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * (W + pad) + x;
            u[i] = extreme ? (rnd() < 0.5f ? 2048.0f : -2048.0f) : 1.5f + 0.03f * (float)x - 0.02f * (float)y + rnd();
            v[i] = extreme ? (rnd() < 0.5f ? 2048.0f : -2048.0f) : -0.7f + 0.01f * (float)x + 0.02f * (float)y + rnd();
            if (!extreme && rnd() < 0.05f) u[i] = special[(int)(rnd() * 11.99f)];
            if (!extreme && rnd() < 0.05f) v[i] = special[(int)(rnd() * 11.99f)];
            state[(size_t)y * bs + x] = rnd() < 0.1f ? 0 : 200;
        }
    const uint8_t value[4] = {255, 1, 2, 3};
    int bad = 0;
    for (int kind = 0; kind < 3; kind++)
        for (int mode = 0; mode < 2; mode++)
            for (int passes = 1; passes <= 3; passes += 2) {
                const hsgm::Field f = {u.data(), v.data(), fs, (kind & 1) ? nullptr : state.data(), bs, W, H};
                const hsgm::Fit fit = {kind, passes, mode, 1.0f, 6.0f, 0.0625f};
                hsgm::Result r;
                hsgm::fit_rows(f, fit, value, mask.data(), bs, ru.data(), rv.data(), fs, &r);
                if (r.cls[0] + r.cls[1] + r.cls[2] + r.cls[3] != (uint64_t)W * H) bad++;
                for (int k = 0; k < 6; k++)
                    if (!std::isfinite(r.m.p[k])) bad++;
                hsgm::Model inv, back;
                if (hsgm::invert(r.m, &inv)) hsgm::compose(r.m, inv, &back);
            }
    // the warp by a model, every tap inside the picture
    std::vector<uint8_t> src((size_t)(3 * W + pad) * (H - 1) + 3 * W), dst(src.size());
    for (uint8_t &b : src) b = (uint8_t)(rnd() * 255.0f);
    const hsgm::Model models[] = {{{3.25f, 0.05f, -0.08f, -2.5f, 0.08f, 0.05f}}, {{-1e8f, 0, 0, 1e8f, 0, 0}}, {{0.3f, 0.9f, 0.2f, 0.1f, -0.3f, 1.4f}}};
    for (const hsgm::Model &m : models)
        for (int border = 0; border < 2; border++) {
            hswarp::Sums s;
            hsgm::warp_rows<3>(m, W, H, 1.0f, border, 0x030201u, src.data(), (size_t)3 * W + pad, src.data(), (size_t)3 * W + pad, dst.data(), (size_t)3 * W + pad, &s);
            hsgm::warp_rows<1>(m, W, H, -0.5f, border, 7u, src.data(), (size_t)3 * W + pad, nullptr, 0, dst.data(), (size_t)3 * W + pad, &s);
            if (s.inside + s.outside + s.unknown != (uint64_t)W * H) bad++;
        }
    return bad;
}

int main()
{
    const int shapes[][2] = {{13, 7}, {260, 37}, {1027, 9}, {96, 64}, {1, 1}, {1, 40}, {40, 1}};
    int bad = 0;
    for (const auto &s : shapes)
        for (int pad = 0; pad < 4; pad += 3) bad += run(s[0], s[1], pad, false);
    bad += run(16384, 4, 0, true);
    bad += run(4, 16384, 1, true);
    // the largest sums: one sign everywhere
    {
        const int W = 16384, H = 4;
        std::vector<float> u((size_t)W * H, 2048.0f), v((size_t)W * H, -2048.0f);
        const hsgm::Field f = {u.data(), v.data(), (size_t)W * 4, nullptr, 0, W, H};
        hsgm::Sums s = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        hsgm::pass_rows(f, true, hsgm::Model{{0, 0, 0, 0, 0, 0}}, 0.0f, &s, nullptr);
        if (s.u != (long long)W * H * (1 << 19) || s.v != -s.u) bad++;
    }
    if (bad) {
        std::printf("gmotion rule: %d failures\n", bad);
        return 1;
    }
    std::printf("gmotion rule: ok\n");
    return 0;
}
