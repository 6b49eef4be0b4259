// A stand-alone program over csrc/hs_chain_rule.h for AddressSanitizer and UBSan (tests/test_chain_host.py builds and runs
// it): hschain's host loops over the degenerate frame sizes and over a field whose vectors end on the last row and column
// exactly, every plane in a heap block of exactly its size, so a tap outside a plane is a report.  Prints one line per
// case: the four class counts and the sum of the ages.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hs_chain_rule.h"

namespace {

struct Field {
    std::vector<float> u, v;
    std::vector<uint8_t> s;
};

// n planes of W x H, packed; fill(k, x, y, &a, &b) names the vector.
template <class Fill>
int run(int W, int H, int n, bool with_state, bool with_start, Fill fill)
{
    std::vector<Field> f((size_t)n);
    std::vector<hschain::Plane> planes((size_t)n);
    for (int k = 0; k < n; k++) {
        f[k].u.resize((size_t)W * H);
        f[k].v.resize((size_t)W * H);
        f[k].s.assign((size_t)W * H, 1);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) fill(k, x, y, &f[k].u[(size_t)y * W + x], &f[k].v[(size_t)y * W + x]);
        if (with_state) f[k].s[((size_t)k * 7) % ((size_t)W * H)] = 0;
        planes[k] = hschain::Plane{f[k].u.data(), f[k].v.data(), with_state ? f[k].s.data() : nullptr, (long long)W * 4, (long long)W};
    }
    std::vector<float> U0((size_t)W * H, 0.0f), V0((size_t)W * H, 0.0f), U((size_t)W * H), V((size_t)W * H);
    std::vector<uint8_t> status((size_t)W * H), age((size_t)W * H);
    const uint8_t value[4] = {255, 1, 2, 3};
    hschain::Sums sums;
    hschain::chain_rows(planes.data(), n, W, H, with_start ? U0.data() : nullptr, with_start ? V0.data() : nullptr, (size_t)W * 4, value, U.data(), V.data(),
                        (size_t)W * 4, status.data(), (size_t)W, age.data(), (size_t)W, &sums);
    printf("dense %dx%d n=%d state=%d start=%d: %llu %llu %llu %llu age %llu\n", W, H, n, (int)with_state, (int)with_start, (unsigned long long)sums.cls[0],
           (unsigned long long)sums.cls[1], (unsigned long long)sums.cls[2], (unsigned long long)sums.cls[3], (unsigned long long)sums.sum_age);
    if (sums.cls[0] + sums.cls[1] + sums.cls[2] + sums.cls[3] != (uint64_t)W * H) return 1;
    // the same planes for points: the pixel centres, the far corner exactly, and points outside, huge and NaN
    std::vector<float> xy;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) { xy.push_back((float)x); xy.push_back((float)y); }
    const float extra[][2] = {{(float)(W - 1), (float)(H - 1)}, {-0.5f, 0.0f}, {(float)W, 0.0f}, {3e9f, 0.0f}, {NAN, 0.0f}, {(float)(W - 1) * 0.5f, (float)(H - 1) * 0.5f}};
    for (const auto &e : extra) { xy.push_back(e[0]); xy.push_back(e[1]); }
    const int m = (int)(xy.size() / 2);
    std::vector<float> track((size_t)(n + 1) * m * 2), last((size_t)m * 2);
    std::vector<uint8_t> pst((size_t)m), pag((size_t)m);
    hschain::track_rows(planes.data(), n, W, H, xy.data(), m, value, track.data(), last.data(), pst.data(), pag.data(), &sums);
    printf("points %dx%d n=%d m=%d: %llu %llu %llu %llu age %llu\n", W, H, n, m, (unsigned long long)sums.cls[0], (unsigned long long)sums.cls[1],
           (unsigned long long)sums.cls[2], (unsigned long long)sums.cls[3], (unsigned long long)sums.sum_age);
    return sums.cls[0] + sums.cls[1] + sums.cls[2] + sums.cls[3] != (uint64_t)m;
}

} // namespace

int main()
{
    int bad = 0;
    const int sizes[][2] = {{1, 1}, {5, 1}, {1, 6}, {13, 7}};
    for (const auto &wh : sizes)
        for (int n : {1, 2, 5})
            for (int mode = 0; mode < 4; mode++) {
                // zero flow, -0.0, and a flow that leaves
                bad |= run(wh[0], wh[1], n, mode & 1, mode & 2, [](int, int, int, float *a, float *b) { *a = 0.0f; *b = -0.0f; });
                bad |= run(wh[0], wh[1], n, mode & 1, mode & 2, [](int k, int, int, float *a, float *b) { *a = k & 1 ? -0.75f : 0.75f; *b = 0.25f; });
            }
    // every vector of plane 0 ends on the last column and the last row exactly; plane 1 then points back inside
    for (int mode = 0; mode < 4; mode++)
        bad |= run(13, 7, 3, mode & 1, mode & 2, [](int k, int x, int y, float *a, float *b) {
            *a = k == 0 ? (float)(12 - x) : k == 1 ? -0.5f : 0.0f;
            *b = k == 0 ? (float)(6 - y) : k == 1 ? -0.5f : 0.0f;
        });
    return bad;
}
