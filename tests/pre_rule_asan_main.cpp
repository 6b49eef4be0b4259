// Stand-alone check of csrc/hs_pre_rule.h (built by tests/test_pre_host.py with -fsanitize=address,undefined): the host
// rule over every shape of the test list, with source and destination allocated EXACTLY to size -- a clamp that reads
// or writes one byte outside its frame aborts the program -- and compared with a direct evaluation of the definition.
#include "hs_pre_rule.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint32_t rng_state = 12345u;
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

int main(int argc, char **argv)
{
    const int S = argc > 1 ? atoi(argv[1]) : HSFLOW_PRE_STRIP_ROWS;
    const int widths[] = {1, 2, 3, 4, 5, 7, 255, 256, 257, 260};
    const int heights[] = {1, 2, 3, S - 1, S, S + 1, 2 * S + 1};
    long cases = 0;
    for (int format = 0; format <= 3; format++)
        for (int W : widths)
            for (int H : heights)
                for (int pad = 0; pad <= 5; pad += 5) {
                    if (H < 1) continue;
                    const size_t rowb = (size_t)W * (format >= 2 ? 3 : 1), stride = rowb + (size_t)pad;
                    const size_t src_bytes = (size_t)(H - 1) * stride + rowb, dst_bytes = (size_t)(H - 1) * (W + (size_t)pad) + W;
                    uint8_t *src = (uint8_t *)malloc(src_bytes), *dst = (uint8_t *)malloc(dst_bytes);
                    if (!src || !dst) return 3;
                    const int fill = (int)(cases % 4); // random, random, all 0, all 255
                    for (size_t i = 0; i < src_bytes; i++) src[i] = fill == 2 ? 0 : fill == 3 ? 255 : next_byte();
                    memset(dst, 0xA5, dst_bytes);
                    if (hspre::preprocess_host(format, src, stride, W, H, dst, (size_t)W + (size_t)pad) != 0) return 4;
                    for (int y = 0; y < H; y++)
                        for (int x = 0; x < W; x++)
                            if (dst[(size_t)y * (W + (size_t)pad) + x] != direct(format, src, stride, W, H, x, y)) {
                                printf("mismatch: format %d, %d x %d, pad %d at (%d, %d)\n", format, W, H, pad, x, y);
                                return 1;
                            }
                    for (int y = 0; y + 1 < H; y++) // the padding between rows stays untouched
                        for (int k = 0; k < pad; k++)
                            if (dst[(size_t)y * (W + (size_t)pad) + W + k] != 0xA5) return 5;
                    free(src);
                    free(dst);
                    cases++;
                }
    // argument checks of the rule itself
    uint8_t one[3] = {1, 2, 3}, out[1];
    if (hspre::preprocess_host(4, one, 3, 1, 1, out, 1) != 1 || hspre::preprocess_host(-1, one, 3, 1, 1, out, 1) != 1) return 6;
    if (hspre::preprocess_host(1, nullptr, 1, 1, 1, out, 1) != 1 || hspre::preprocess_host(1, one, 1, 1, 1, nullptr, 1) != 1) return 6;
    if (hspre::preprocess_host(3, one, 2, 1, 1, out, 1) != 2 || hspre::preprocess_host(1, one, 1, 0, 1, out, 1) != 2) return 6;
    printf("pre rule ok: %ld cases, strip rows %d\n", cases, S);
    return 0;
}
