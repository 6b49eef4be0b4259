// Stand-alone check of the sequence rule of csrc/hs_pre_rule.h (built by tests/test_sequence_host.py with
// -fsanitize=address,undefined; host code only): hspre::preprocess_sequence_host over every shape, format, flag set and
// frame count of the test list.  Every source frame is allocated EXACTLY to size -- a clamp that reads one byte outside
// its frame aborts the program -- every output plane lies between guard bytes that must survive, and the planes are
// compared with a direct evaluation of the definition: p = pre(format, f) pixel by pixel, and B(p) as the 3x3 box blur of
// the stored plane p with p's own border repeated.
#include "hs_pre_rule.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint32_t rng_state = 2463534242u;
static uint8_t next_byte()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}

static int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// the definition, pixel by pixel: gray, then round(sum of the clamped 3x3 neighbourhood / 9)
static uint8_t direct(int format, const uint8_t *src, size_t stride, int W, int H, int x, int y)
{
    const bool colour = format >= 2, blur = (format & 1) != 0;
    auto gray = [&](int xx, int yy) -> int {
        const uint8_t *p = src + (size_t)yy * stride + (colour ? 3 * xx : xx);
        return colour ? (1868 * p[0] + 9617 * p[1] + 4899 * p[2] + 8192) >> 14 : p[0];
    };
    if (!blur) return (uint8_t)gray(x, y);
    int s = 0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) s += gray(clampi(x + dx, W), clampi(y + dy, H));
    return (uint8_t)((2 * s + 9) / 18);
}

constexpr size_t GUARD = 32;

struct Plane { // width x height bytes with rows `ds` apart, exactly sized, between two guards
    std::vector<uint8_t> mem;
    size_t bytes;
    Plane(int W, int H, size_t ds) : mem(2 * GUARD + (size_t)(H - 1) * ds + (size_t)W, 0xA5), bytes((size_t)(H - 1) * ds + (size_t)W) {}
    uint8_t *data() { return mem.data() + GUARD; }
    bool guards_intact() const
    {
        for (size_t i = 0; i < GUARD; i++)
            if (mem[i] != 0xA5 || mem[GUARD + bytes + i] != 0xA5) return false;
        return true;
    }
};

int main(int argc, char **argv)
{
    const int S = argc > 1 ? atoi(argv[1]) : HSFLOW_PRE_STRIP_ROWS;
    const int shapes[][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 3}, {5, 2}, {4, 7}, {7, 9}, {8, 8}, {9, 16}, {13, 17}, {255, 8}, {257, 10}, {6, S - 1}, {6, S + 1}, {5, 2 * S + 1}};
    const int flag_sets[] = {0, 1, 3};
    const int counts[] = {2, 3, 5};
    long cases = 0;
    for (int format = 0; format <= 3; format++)
        for (const auto &shape : shapes)
            for (int flags : flag_sets)
                for (int n : counts) {
                    const int W = shape[0], H = shape[1];
                    if (H < 1) continue;
                    const size_t pad = (size_t)(cases % 3) * 3;
                    const size_t rowb = (size_t)W * (format >= 2 ? 3 : 1), stride = rowb + pad, ds = (size_t)W + pad;
                    const size_t src_bytes = (size_t)(H - 1) * stride + rowb;
                    std::vector<uint8_t *> src((size_t)n);
                    const int fill = (int)(cases % 5); // random, random, all 0, all 255, rows 0 / 255 alternating
                    for (int j = 0; j < n; j++) {
                        src[(size_t)j] = (uint8_t *)malloc(src_bytes);
                        if (!src[(size_t)j]) return 3;
                        for (size_t i = 0; i < src_bytes; i++)
                            src[(size_t)j][i] = fill == 2 ? 0 : fill == 3 ? 255 : fill == 4 ? (uint8_t)(((i / stride + (size_t)j) & 1) ? 255 : 0) : next_byte();
                    }
                    std::vector<Plane> prev, curr;
                    std::vector<uint8_t *> pp, pc;
                    for (int k = 0; k < n - 1; k++) { prev.emplace_back(W, H, ds); curr.emplace_back(W, H, ds); }
                    for (int k = 0; k < n - 1; k++) { pp.push_back(prev[(size_t)k].data()); pc.push_back(curr[(size_t)k].data()); }
                    if (hspre::preprocess_sequence_host(format, flags, src.data(), n, stride, W, H, pp.data(), pc.data(), ds) != 0) return 4;
                    std::vector<uint8_t> p((size_t)W * H);
                    for (int k = 0; k < n - 1; k++) {
                        if (!prev[(size_t)k].guards_intact() || !curr[(size_t)k].guards_intact()) return 5;
                        for (int y = 0; y + 1 < H; y++) // the padding between rows stays untouched
                            for (size_t q = 0; q < pad; q++)
                                if (pp[(size_t)k][(size_t)y * ds + (size_t)W + q] != 0xA5 || pc[(size_t)k][(size_t)y * ds + (size_t)W + q] != 0xA5) return 5;
                        const bool reblur = (flags & 1) && (k > 0 || (flags & 2));
                        for (int y = 0; y < H; y++)
                            for (int x = 0; x < W; x++) p[(size_t)y * W + x] = direct(format, src[(size_t)k], stride, W, H, x, y);
                        for (int y = 0; y < H; y++)
                            for (int x = 0; x < W; x++) {
                                const uint8_t want_prev = reblur ? direct(1, p.data(), (size_t)W, W, H, x, y) : p[(size_t)y * W + x];
                                const uint8_t want_curr = direct(format, src[(size_t)k + 1], stride, W, H, x, y);
                                if (pp[(size_t)k][(size_t)y * ds + x] != want_prev || pc[(size_t)k][(size_t)y * ds + x] != want_curr) {
                                    printf("mismatch: format %d, flags %d, n %d, %d x %d, pair %d at (%d, %d)\n", format, flags, n, W, H, k, x, y);
                                    return 1;
                                }
                            }
                    }
                    for (uint8_t *s : src) free(s);
                    cases++;
                }
    // argument checks of the rule itself
    uint8_t a[3] = {1, 2, 3}, b[3] = {4, 5, 6}, o0[1], o1[1];
    const uint8_t *two[2] = {a, b}, *holed[2] = {a, nullptr};
    uint8_t *op[1] = {o0}, *oc[1] = {o1}, *none[1] = {nullptr};
    if (hspre::preprocess_sequence_host(3, 0, two, 2, 3, 1, 1, op, oc, 1) != 0) return 6;
    if (hspre::preprocess_sequence_host(4, 0, two, 2, 3, 1, 1, op, oc, 1) != 1 || hspre::preprocess_sequence_host(3, 2, two, 2, 3, 1, 1, op, oc, 1) != 1) return 6;
    if (hspre::preprocess_sequence_host(3, 4, two, 2, 3, 1, 1, op, oc, 1) != 1 || hspre::preprocess_sequence_host(3, 0, two, 1, 3, 1, 1, op, oc, 1) != 1) return 6;
    if (hspre::preprocess_sequence_host(3, 0, nullptr, 2, 3, 1, 1, op, oc, 1) != 1 || hspre::preprocess_sequence_host(3, 0, holed, 2, 3, 1, 1, op, oc, 1) != 1) return 6;
    if (hspre::preprocess_sequence_host(3, 0, two, 2, 3, 1, 1, none, oc, 1) != 1 || hspre::preprocess_sequence_host(3, 0, two, 2, 3, 1, 1, op, nullptr, 1) != 1) return 6;
    if (hspre::preprocess_sequence_host(3, 0, two, 2, 2, 1, 1, op, oc, 1) != 2 || hspre::preprocess_sequence_host(1, 0, two, 2, 1, 0, 1, op, oc, 1) != 2) return 6;
    if (hspre::preprocess_sequence_host(1, 0, two, 2, 2, 2, 1, op, oc, 1) != 2) return 6;
    printf("pre sequence ok: %ld cases, strip rows %d\n", cases, S);
    return 0;
}
