// link_host_san.cpp -- the linking rule and its host form (csrc/hs_link_rule.h) alone, for a build with
// -fsanitize=address,undefined (tests/test_link_host.py builds and runs it): label planes with background, negative labels and
// labels above the caps, flow fields with the extreme values the landing rule knows, at (260, 37), (1, 40) and (67, 19), with
// ragged strides.  Every buffer is exactly as large as the rule may touch, so a gather outside B, a step beyond a row's
// width or a record too many is the sanitizer's to report.  The counts are checked against their identities.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "hs_link_rule.h"

static unsigned long long lcg = 88172645463325252ull;
static unsigned rnd(unsigned n)
{
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)((lcg >> 33) % n);
}

static int fail(const char *what, int W, int H)
{
    std::printf("link rule: %s at %d x %d\n", what, W, H);
    return 1;
}

static int run(int W, int H, int pad, uint32_t cap_a, uint32_t cap_b, int max_label)
{
    const size_t row = (size_t)(W + pad), n = row * (H - 1) + W; // the last row ends at its width
    std::vector<int32_t> A(n), B(n);
    std::vector<float> u(n), v(n);
    const float inf = std::numeric_limits<float>::infinity();
    const float special[] = {std::numeric_limits<float>::quiet_NaN(), inf, -inf, 1e10f, -1e10f, 1e9f, -1e9f, 3e38f, -3e38f, 2147483648.0f, -2147483648.0f,
                             4294967296.0f, 0.5f, -0.5f, 0.49999997f, -0.50000006f, (float)W, (float)-W, (float)H, -0.0f, 1e-40f};
    const int n_special = (int)(sizeof(special) / sizeof(special[0]));
    for (size_t i = 0; i < n; i++) {
        A[i] = (int32_t)rnd((unsigned)max_label + 3) - 2;
        B[i] = (int32_t)rnd((unsigned)max_label + 3) - 2;
        u[i] = rnd(5) == 0 ? special[rnd((unsigned)n_special)] : (float)rnd(2000) / 64.0f - 15.0f;
        v[i] = rnd(5) == 0 ? special[rnd((unsigned)n_special)] : (float)rnd(2000) / 64.0f - 15.0f;
    }
    A[0] = std::numeric_limits<int32_t>::max();
    B[n - 1] = std::numeric_limits<int32_t>::min();
    const hsln::Step step = {A.data(), row * 4, B.data(), row * 4, u.data(), v.data(), row * 4, W, H};
    hsln::Result full;
    hsln::link_rows(step, cap_a, cap_b, nullptr, 0, nullptr, nullptr, &full);
    const uint32_t caps[] = {0u, full.n_links ? full.n_links - 1u : 0u, full.n_links + 2u};
    for (const uint32_t capacity : caps) {
        std::vector<hsln::Link> links(capacity);
        std::vector<hsln::Side> sa(cap_a), sb(cap_b);
        hsln::Result r;
        hsln::link_rows(step, cap_a, cap_b, capacity ? links.data() : nullptr, capacity, sa.data(), sb.data(), &r);
        if (r.n_links != full.n_links || r.n_written != (r.n_links < capacity ? r.n_links : capacity)) return fail("n_links / n_written", W, H);
        if ((r.flags != 0u) != (r.n_links > capacity)) return fail("overflow flag", W, H);
        uint64_t labelled = 0, px_a = 0, px_b = 0, votes = 0;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) labelled += A[(size_t)y * row + x] > 0;
        for (const hsln::Side &s : sa) px_a += s.px;
        for (const hsln::Side &s : sb) px_b += s.px;
        for (uint32_t k = 0; k < r.n_written; k++) {
            votes += links[k].px;
            if (k && !(links[k - 1].a < links[k].a || (links[k - 1].a == links[k].a && links[k - 1].b < links[k].b))) return fail("order of the links", W, H);
            if (!links[k].px || links[k].a < 1 || links[k].a > cap_a || links[k].b < 1 || links[k].b > cap_b) return fail("a link's fields", W, H);
        }
        if (r.voted_px + r.gone_px + r.unmatched_px + r.over_a_px != labelled) return fail("the totals do not add up to the labelled pixels", W, H);
        if (px_a != r.voted_px + r.gone_px + r.unmatched_px || px_b != r.voted_px) return fail("the sides' px", W, H);
        if (r.n_written == r.n_links && votes != r.voted_px) return fail("the links' px", W, H);
    }
    // tracks on the sides of two steps of this field
    std::vector<hsln::Side> sa(cap_a > cap_b ? cap_a : cap_b), sb(sa.size());
    const uint32_t cap = cap_a < cap_b ? cap_a : cap_b;
    hsln::link_rows(step, cap, cap, nullptr, 0, sa.data(), sb.data(), nullptr);
    const hsln::Side *pa[2] = {sa.data(), sa.data()}, *pb[2] = {sb.data(), sb.data()};
    const uint32_t counts[3] = {cap, cap + 5u, cap > 1u ? cap - 1u : 1u};
    std::vector<uint32_t> ids((size_t)3 * cap);
    const uint32_t n_tracks = hsln::link_tracks(pa, pb, counts, 2, cap, 128u, ids.data());
    uint32_t top = 0;
    for (const uint32_t id : ids) top = id > top ? id : top;
    if (top != n_tracks || n_tracks < cap) return fail("tracks", W, H);
    return 0;
}

int main()
{
    if (run(260, 37, 3, 64, 64, 70)) return 1;
    if (run(1, 40, 0, 1, 1, 1)) return 1;
    if (run(67, 19, 1, 300, 7, 400)) return 1;
    if (run(64, 16, 0, 5, 4096, 5000)) return 1;
    std::printf("link rule: ok\n");
    return 0;
}
