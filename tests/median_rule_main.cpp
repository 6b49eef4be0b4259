// csrc/hs_median_rule.h and nothing else as a program of its own (tests/test_median_host.py builds it with
// AddressSanitizer and UBSan):
//   1. the selection network on every zero-one input (the zero-one principle: a sequence of min/max exchanges that
//      finds the middle element of every zero-one input finds it for every input), 64 inputs at a time;
//   2. the sentinel identity: with the k-th non-voter replaced by the low sentinel for even k and the high one for odd k,
//      the middle element of all N slots is the voter of rank (n - 1) >> 1, for every n and random voter positions;
//   3. whole fields whose last row ends where the allocation ends, special values included; one line per field with the
//      record and a checksum of the outputs, which the test compares with the library's.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "hs_median_rule.h"

namespace slices {
struct Bits {
    uint64_t w;
};
inline void exchange(Bits &lo, Bits &hi)
{
    const uint64_t a = lo.w & hi.w, b = lo.w | hi.w;
    lo.w = a;
    hi.w = b;
}
} // namespace slices

template <int N>
static bool zero_one()
{
    static const uint64_t lane_bit[6] = {0xaaaaaaaaaaaaaaaaull, 0xccccccccccccccccull, 0xf0f0f0f0f0f0f0f0ull, 0xff00ff00ff00ff00ull, 0xffff0000ffff0000ull,
                                         0xffffffff00000000ull};
    constexpr int mid = (N - 1) / 2;
    for (uint32_t group = 0; group < (1u << (N - 6)); group++) {
        slices::Bits a[N];
        int ones_high = 0;
        for (int k = 0; k < N; k++) {
            if (k < 6) a[k].w = lane_bit[k];
            else {
                const bool one = (group >> (k - 6)) & 1u;
                a[k].w = one ? ~0ull : 0ull;
                ones_high += one;
            }
        }
        uint64_t want = 0; // the element of rank mid is 1 iff at most mid elements are 0
        for (int lane = 0; lane < 64; lane++) {
            int ones = ones_high;
            for (int b = 0; b < 6; b++) ones += (lane >> b) & 1;
            if (N - ones <= mid) want |= 1ull << lane;
        }
        if (hsmed::mid_of(a).w != want) return false;
    }
    return true;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

template <int N>
static bool sentinels()
{
    for (int trial = 0; trial < 4000; trial++) {
        const int n = trial % (N + 1);
        bool voter[N] = {};
        for (int placed = 0; placed < n;) {
            const int k = (int)(rnd() % N);
            if (!voter[k]) { voter[k] = true; placed++; }
        }
        hsmed::Window<N> w;
        w.n = 0;
        std::vector<uint32_t> ku, kv;
        for (int j = 0; j < N; j++) {
            // few distinct values, so ties are common; never a sentinel
            const uint32_t a = voter[j] ? 1u + rnd() % 7u : hsmed::kLow, b = voter[j] ? 0xfffffff0u + rnd() % 15u : hsmed::kLow;
            if (voter[j]) { ku.push_back(a); kv.push_back(b); }
            hsmed::take(w, j, a, b);
        }
        if (w.n != n) return false;
        if (!n) continue;
        std::sort(ku.begin(), ku.end());
        std::sort(kv.begin(), kv.end());
        if (hsmed::mid_of(w.ku) != ku[(size_t)((n - 1) >> 1)] || hsmed::mid_of(w.kv) != kv[(size_t)((n - 1) >> 1)]) return false;
    }
    return true;
}

// W x H planes whose rows are `pad` elements longer than W, in exact-size heap blocks: a read beyond the plane is a finding.
static void run(int W, int H, int pad, int radius, int fill, int min_votes)
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = std::nextafterf(1e9f, inf);
    const float sa[14] = {nan, 1.f, inf, 0.f, big, 0.f, 1e9f, 0.f, 0.f, -0.f, 1e-42f, 2.f, 0.5f, -1e9f};
    const float sb[14] = {1.f, nan, 0.f, -inf, 0.f, -big, 0.f, -1e9f, 0.f, -0.f, -1e-42f, -0.f, 0.5f, 1e9f};
    const uint8_t states[5] = {255, 0, 1, 2, 7};
    const size_t P = (size_t)W + pad, n = P * (H - 1) + W;
    std::vector<float> u(n), v(n), uo(n, -7.f), vo(n, -7.f);
    std::vector<uint8_t> s(n), so(n, 0xA5);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t k = (size_t)y * P + x, j = (size_t)y * W + x;
            u[k] = (float)((int)(j * 7 % 11) - 5) * 0.5f;
            v[k] = (float)((int)(j * 5 % 13) - 6) * 0.25f;
            if (j % 7 == 3) { u[k] = sa[j / 7 % 14]; v[k] = sb[j / 7 % 14]; }
            s[k] = states[j % 5];
        }
    hsmed::Sums sums;
    hsmed::median_rows(radius, u.data(), P * 4, v.data(), P * 4, s.data(), P, W, H, fill, min_votes, uo.data(), vo.data(), P * 4, so.data(), P, &sums);
    unsigned long long sum = 0;
    for (size_t k = 0; k < n; k++) sum = sum * 31 + hscolor::float_bits(uo[k]) + 3ull * hscolor::float_bits(vo[k]) + so[k];
    std::printf("%d %d %d %d %d %d | %llu %llu %llu %llu %llu | %llu\n", W, H, pad, radius, fill, min_votes, (unsigned long long)sums.kept,
                (unsigned long long)sums.filled, (unsigned long long)sums.unfilled, (unsigned long long)sums.newly_filled, (unsigned long long)sums.changed, sum);
}

int main()
{
    if (!zero_one<9>()) { std::printf("the 3x3 network misses a zero-one input\n"); return 1; }
    if (!zero_one<25>()) { std::printf("the 5x5 network misses a zero-one input\n"); return 1; }
    if (!sentinels<9>() || !sentinels<25>()) { std::printf("the sentinel identity does not hold\n"); return 1; }
    const int shapes[5][3] = {{5, 3, 0}, {1, 9, 0}, {9, 1, 0}, {7, 5, 3}, {1, 1, 2}};
    for (const auto &sh : shapes)
        for (int radius = 1; radius <= 2; radius++)
            for (int fill = 0; fill <= 1; fill++) run(sh[0], sh[1], sh[2], radius, fill, fill ? 1 : 2);
    return 0;
}
