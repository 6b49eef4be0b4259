// hs_warp_rule.h -- backward warping of a picture by a dense flow field and the residual it leaves, ONE definition for
// the device kernel (hs_kernels_warp.hip.h) and the host twin (hsflow_warp_host), the way hs_color_rule.h serves both
// sides of the colour picture.  The direction is the solver's: It = B - A, so curr(x + u, y + v) ~ prev(x, y) and the
// warped second frame approximates the FIRST.
// All arithmetic is fp32 and every operation is rounded on its own (the library is built with -ffp-contract=off), so host
// and device give the same bytes.  For the pixel (x, y) with flow (a, b), a picture src of C interleaved u8 channels and
// the fraction t of the flow to apply:
//   unknown  iff !hscolor::known(a, b) (NaN, or a magnitude above 1e9): every channel is fill[c]
//   fx       = fl((float)x + fl(a * t)),  fy = fl((float)y + fl(b * t))
//   outside  iff !(fx >= 0 && fx <= W-1 && fy >= 0 && fy <= H-1): CONSTANT -- the pixel is fill; REPLICATE -- fx and fy are
//              clamped to those ranges and sampling goes on
//   x0       = (int)floorf(fx),  x1 = min(x0 + 1, W-1),  ax = fl(fx - (float)x0);  y0, y1, ay alike
//   channel  top = fl(p00 + fl(ax * fl(p10 - p00))), bot alike from row y1; val = fl(top + fl(ay * fl(bot - top)));
//              byte = min((int)fl(val + 0.5f), 255)
// The statistics are exact integers over the INSIDE pixels (known and not outside), all channels: their order of
// accumulation does not matter.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "hs_color_rule.h"

#if defined(__clang__)
#pragma clang fp contract(off) // (what -ffp-contract=off says for the whole library, said again where it matters)
#endif

#if defined(__HIPCC__)
#define HSW_FN __host__ __device__ inline
#else
#define HSW_FN inline
#endif
#if defined(__clang__)
#define HSW_UNROLL _Pragma("unroll")
#else
#define HSW_UNROLL
#endif

namespace hswarp {

constexpr int kBorderConstant = 0, kBorderReplicate = 1; // HSFLOW_WARP_BORDER_*
constexpr int kInside = 0, kOutside = 1, kUnknown = 2;
constexpr float kMaxT = 1e6f; // |t| beyond this is refused: fl(a * t) stays finite for every known a

// Where one pixel samples.  cls: kInside / kOutside / kUnknown; sample: the taps are read (else the pixel is fill).
struct Tap {
    int x0, x1, y0, y1;
    float ax, ay;
    int cls;
    bool sample;
};

HSW_FN Tap locate(float a, float b, int x, int y, float t, int W, int H, int border)
{
    Tap p;
    p.x0 = p.x1 = p.y0 = p.y1 = 0;
    p.ax = p.ay = 0.0f;
    p.cls = kUnknown;
    p.sample = false;
    if (!hscolor::known(a, b)) return p;
    const float da = a * t, db = b * t;
    float fx = (float)x + da, fy = (float)y + db;
    const float xm = (float)(W - 1), ym = (float)(H - 1);
    if (!(fx >= 0.0f && fx <= xm && fy >= 0.0f && fy <= ym)) {
        p.cls = kOutside;
        if (border != kBorderReplicate) return p;
        fx = fx < 0.0f ? 0.0f : fx > xm ? xm : fx;
        fy = fy < 0.0f ? 0.0f : fy > ym ? ym : fy;
    } else {
        p.cls = kInside;
    }
    p.sample = true;
    p.x0 = (int)floorf(fx);
    p.y0 = (int)floorf(fy);
    p.x1 = p.x0 + 1 < W - 1 ? p.x0 + 1 : W - 1;
    p.y1 = p.y0 + 1 < H - 1 ? p.y0 + 1 : H - 1;
    p.ax = fx - (float)p.x0;
    p.ay = fy - (float)p.y0;
    return p;
}

// One channel from its four taps.
HSW_FN uint32_t blend(uint8_t p00, uint8_t p10, uint8_t p01, uint8_t p11, float ax, float ay)
{
    const float a0 = (float)p00, b0 = (float)p01;
    const float dt = (float)p10 - a0, db = (float)p11 - b0;
    const float st = ax * dt, sb = ax * db;
    const float top = a0 + st, bot = b0 + sb;
    const float dv = bot - top;
    const float sv = ay * dv;
    const float val = top + sv;
    const float r = val + 0.5f;
    const int i = (int)r;
    return (uint32_t)(i < 255 ? i : 255);
}

// The C channels of one pixel as c0 | c1 << 8 | c2 << 16.  fill: packed the same way.  rows of src are `stride` bytes apart.
template <int C>
HSW_FN uint32_t pixel(const uint8_t *src, long long stride, const Tap &p, uint32_t fill)
{
    if (!p.sample) return fill;
    const uint8_t *r0 = src + (long long)p.y0 * stride, *r1 = src + (long long)p.y1 * stride;
    uint32_t out = 0u;
    HSW_UNROLL
    for (int c = 0; c < C; c++)
        out |= blend(r0[C * p.x0 + c], r0[C * p.x1 + c], r1[C * p.x0 + c], r1[C * p.x1 + c], p.ax, p.ay) << (8 * c);
    return out;
}

// What one lane, or the host loop, gathers.  32 bits hold a lane's share (hs_kernels_warp.hip.h); the host sums in Sums.
struct Acc {
    uint32_t inside, outside, unknown, sad_warped, sad_plain, max_warped, max_plain;
};

// One pixel's share: warped, plain, ref packed as pixel() packs; ref_valid: there is a reference picture.
template <int C>
HSW_FN void account(Acc &s, int cls, uint32_t warped, uint32_t plain, uint32_t ref, bool ref_valid)
{
    s.inside += cls == kInside;
    s.outside += cls == kOutside;
    s.unknown += cls == kUnknown;
    if (cls != kInside || !ref_valid) return;
    HSW_UNROLL
    for (int c = 0; c < C; c++) {
        const int r = (int)((ref >> (8 * c)) & 255u), w = (int)((warped >> (8 * c)) & 255u), q = (int)((plain >> (8 * c)) & 255u);
        const uint32_t dw = (uint32_t)(w > r ? w - r : r - w), dq = (uint32_t)(q > r ? q - r : r - q);
        s.sad_warped += dw;
        s.sad_plain += dq;
        s.max_warped = dw > s.max_warped ? dw : s.max_warped;
        s.max_plain = dq > s.max_plain ? dq : s.max_plain;
    }
}

template <int C>
HSW_FN uint32_t load_pixel(const uint8_t *p)
{
    uint32_t out = 0u;
    HSW_UNROLL
    for (int c = 0; c < C; c++) out |= (uint32_t)p[c] << (8 * c);
    return out;
}

// The sums of a whole picture (the first 56 bytes of hsflow_warp_stats).
struct Sums {
    uint64_t inside, outside, unknown, sad_warped, sad_plain;
    uint32_t max_warped, max_plain;
};

// A whole picture in host memory.  u, v: rows us / vs BYTES apart.  ref, dst, sums may each be null.  Writes C * W bytes
// of every row of dst and nothing else.
template <int C>
inline void warp_rows(const float *u, size_t us, const float *v, size_t vs, int W, int H, float t, int border, uint32_t fill, const uint8_t *src,
                      size_t ss, const uint8_t *ref, size_t rs, uint8_t *dst, size_t ds, Sums *sums)
{
    Sums total = {0, 0, 0, 0, 0, 0, 0};
    for (int y = 0; y < H; y++) {
        const float *ru = (const float *)((const uint8_t *)u + (size_t)y * us), *rv = (const float *)((const uint8_t *)v + (size_t)y * vs);
        for (int x = 0; x < W; x++) {
            Acc one = {0, 0, 0, 0, 0, 0, 0};
            const Tap p = locate(ru[x], rv[x], x, y, t, W, H, border);
            const uint32_t w = pixel<C>(src, (long long)ss, p, fill);
            if (dst)
                for (int c = 0; c < C; c++) dst[(size_t)y * ds + (size_t)C * x + c] = (uint8_t)(w >> (8 * c));
            if (sums) {
                const uint32_t q = load_pixel<C>(src + (size_t)y * ss + (size_t)C * x);
                const uint32_t r = ref ? load_pixel<C>(ref + (size_t)y * rs + (size_t)C * x) : 0u;
                account<C>(one, p.cls, w, q, r, ref != nullptr);
            }
            total.inside += one.inside; total.outside += one.outside; total.unknown += one.unknown;
            total.sad_warped += one.sad_warped; total.sad_plain += one.sad_plain;
            total.max_warped = one.max_warped > total.max_warped ? one.max_warped : total.max_warped;
            total.max_plain = one.max_plain > total.max_plain ? one.max_plain : total.max_plain;
        }
    }
    if (sums) *sums = total;
}

} // namespace hswarp
