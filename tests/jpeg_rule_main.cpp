// Stand-alone check of csrc/hs_jpeg_rule.h (built by tests/test_jpeg_host.py with -fsanitize=address,undefined): the host
// rule over every residue of the width and of the height modulo 16, with the picture and the file allocated EXACTLY to
// size -- an edge clamp that reads one byte outside the picture, or a byte written at or beyond the capacity, aborts the
// program.  What the bytes must be is the business of the Python tests (the CLI's writer, PIL, the reference's files);
// here: the size is found with capacity 0, the file fits that size exactly, one byte less is refused with the same
// size, and the frame of the file (SOI, the picture's size in SOF0, EOI) is there.
#include "hs_jpeg_rule.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint32_t rng_state = 2463534242u;
static uint32_t next_word()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

int main()
{
    const int qualities[] = {1, 10, 30, 50, 75, 95, 100};
    long cases = 0;
    for (int rw = 0; rw < 16; rw++)
        for (int rh = 0; rh < 16; rh++) {
            const int W = rw + 1 + 16 * (int)(next_word() % 4u), H = rh + 1 + 16 * (int)(next_word() % 3u);
            const int q = qualities[cases % 7], kind = (int)(cases % 4); // noise, constant, two-level, sparse
            const size_t pad = cases % 2 ? 5 : 0, rowb = (size_t)W * 3, stride = rowb + pad, src_bytes = (size_t)(H - 1) * stride + rowb;
            uint8_t *src = (uint8_t *)malloc(src_bytes);
            if (!src) return 3;
            for (size_t i = 0; i < src_bytes; i++) {
                const uint32_t r = next_word();
                src[i] = (uint8_t)(kind == 0 ? r : kind == 1 ? 77 : kind == 2 ? ((r & 1u) ? 255 : 0) : ((r % 29u) ? 0 : 255));
            }
            size_t need = 0, got = 0;
            if (hsjpeg::encode_host(src, stride, W, H, q, nullptr, 0, &need) != 2) return 4; // capacity 0: the size, nothing written
            if (need < (size_t)hsjpeg::kHeaderBytes + 3 || need > hsjpeg::bound(W, H)) { printf("size %zu out of range for %d x %d\n", need, W, H); return 5; }
            uint8_t *file = (uint8_t *)malloc(need), *shorter = (uint8_t *)malloc(need - 1);
            if (!file || !shorter) return 3;
            if (hsjpeg::encode_host(src, stride, W, H, q, file, need, &got) != 0 || got != need) return 6;
            got = 0;
            if (hsjpeg::encode_host(src, stride, W, H, q, shorter, need - 1, &got) != 2 || got != need) return 7;
            if (memcmp(file, shorter, need - 1) != 0) return 8;
            if (file[0] != 0xFF || file[1] != 0xD8 || file[need - 2] != 0xFF || file[need - 1] != 0xD9) return 9;
            // SOF0 lies behind SOI + APP0 (20 bytes) and two DQT (69 each): FF C0, length 17, precision 8, height, width
            const uint8_t *sof = file + 20 + 2 * 69;
            if (sof[0] != 0xFF || sof[1] != 0xC0 || ((sof[5] << 8) | sof[6]) != H || ((sof[7] << 8) | sof[8]) != W) return 10;
            for (size_t i = hsjpeg::kHeaderBytes; i + 2 < need; i++) // every 0xFF of the stream is stuffed
                if (file[i] == 0xFF && file[i + 1] != 0x00) { printf("unstuffed FF at %zu of %zu, %d x %d\n", i, need, W, H); return 11; }
            free(src);
            free(file);
            free(shorter);
            cases++;
        }
    // argument checks of the rule itself
    uint8_t px[3] = {1, 2, 3}, out[4096];
    size_t n = 0;
    if (hsjpeg::encode_host(nullptr, 3, 1, 1, 95, out, sizeof out, &n) != 1 || hsjpeg::encode_host(px, 3, 1, 1, 95, out, sizeof out, nullptr) != 1) return 12;
    if (hsjpeg::encode_host(px, 3, 1, 1, 95, nullptr, 8, &n) != 1) return 12;
    if (hsjpeg::encode_host(px, 3, 1, 1, 0, out, sizeof out, &n) != 1 || hsjpeg::encode_host(px, 3, 1, 1, 101, out, sizeof out, &n) != 1) return 12;
    if (hsjpeg::encode_host(px, 2, 1, 1, 95, out, sizeof out, &n) != 2 || hsjpeg::encode_host(px, 3, 0, 1, 95, out, sizeof out, &n) != 2) return 12;
    if (hsjpeg::encode_host(px, 3, 1, 65536, 95, out, sizeof out, &n) != 2) return 12;
    if (hsjpeg::bound(1, 1) != 3121 || hsjpeg::bound(1920, 1080) != 20367985 || hsjpeg::bound(0, 5) != 0) return 13;
    printf("jpeg rule ok: %ld cases\n", cases);
    return 0;
}
