// hs_fb_rule.h -- the forward-backward consistency of two dense flow fields, ONE definition for the device kernel
// (hs_kernels_fb.hip.h) and the host twin (hsflow_fb_host), the way hs_warp_rule.h serves both sides of the warp.
// Forward flow (uf, vf) of a pair (A, B), backward flow (ub, vb) of the pair (B, A), both W x H.  Following the forward
// vector and reading the backward flow there, the two cancel where both are right; where they do not, the pixel is
// occluded or mis-estimated (Sundaram, Brox and Keutzer 2010).
// All arithmetic is fp32 and every operation is rounded on its own (the library is built with -ffp-contract=off), so host
// and device give the same bits.  For the pixel (x, y) with a = uf[y][x], b = vf[y][x]:
//   UNKNOWN (3)  iff !hscolor::known(a, b) (NaN, or a magnitude above 1e9)
//   fx = fl((float)x + a), fy = fl((float)y + b)
//   OUTSIDE (2)  iff !(fx >= 0 && fx <= W-1 && fy >= 0 && fy <= H-1): a target outside the frame has no backward flow
//   x0 = (int)floorf(fx), x1 = min(x0 + 1, W-1), ax = fl(fx - (float)x0); y0, y1, ay alike -- hswarp::locate with t = 1
//   UNKNOWN      iff any of the four taps of (ub, vb) is not known, even where its weight is 0
//   c = bilinear of ub in the warp's order: top = fl(p00 + fl(ax * fl(p10 - p00))), bot alike from row y1,
//       fl(top + fl(ay * fl(bot - top))); d alike from vb
//   ex = fl(a + c), ey = fl(b + d), err2 = fl(fl(ex * ex) + fl(ey * ey))
//   mag2 = fl(fl(fl(a * a) + fl(b * b)) + fl(fl(c * c) + fl(d * d))), bound = fl(fl(alpha * mag2) + beta)
//   CONSISTENT (0) iff err2 <= bound, else INCONSISTENT (1); these two classes are the "evaluated" pixels.
// Known components are at most 1e9, so err2 <= 8e18 and mag2 <= 4e18: nothing overflows, and with alpha <= 1e6 and
// beta <= 1e30 neither does the bound.
// The statistics are exact integers over the pixels: their order of accumulation does not matter.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hs_color_rule.h"
#include "hs_warp_rule.h"

#if defined(__clang__)
#pragma clang fp contract(off) // (what -ffp-contract=off says for the whole library, said again where it matters)
#endif

#if defined(__HIPCC__)
#define HSFB_FN __host__ __device__ inline
#else
#define HSFB_FN inline
#endif

namespace hsfb {

constexpr int kConsistent = 0, kInconsistent = 1, kOutside = 2, kUnknown = 3;
constexpr uint32_t kNanBits = 0x7fc00000u; // err2 of a pixel that was not evaluated: the colour picture calls it unknown
constexpr float kMaxAlpha = 1e6f, kMaxBeta = 1e30f;

// One plane sampled at the taps of p, in the warp's order of operations.
HSFB_FN float bilinear(float p00, float p10, float p01, float p11, float ax, float ay)
{
    const float dt = p10 - p00, db = p11 - p01;
    const float st = ax * dt, sb = ax * db;
    const float top = p00 + st, bot = p01 + sb;
    const float dv = bot - top;
    const float sv = ay * dv;
    return top + sv;
}

// The class of one pixel and, where it was evaluated, its squared error (else 0).
struct Pixel {
    int cls;
    float err2;
};

// ub, vb: the backward planes, rows ubs / vbs BYTES apart.
HSFB_FN Pixel decide(float a, float b, int x, int y, int W, int H, const float *ub, long long ubs, const float *vb, long long vbs, float alpha, float beta)
{
    Pixel r;
    r.cls = kUnknown;
    r.err2 = 0.0f;
    const hswarp::Tap p = hswarp::locate(a, b, x, y, 1.0f, W, H, hswarp::kBorderConstant);
    if (p.cls == hswarp::kUnknown) return r;
    if (p.cls == hswarp::kOutside) {
        r.cls = kOutside;
        return r;
    }
    const float *u0 = (const float *)((const uint8_t *)ub + (long long)p.y0 * ubs), *u1 = (const float *)((const uint8_t *)ub + (long long)p.y1 * ubs);
    const float *v0 = (const float *)((const uint8_t *)vb + (long long)p.y0 * vbs), *v1 = (const float *)((const uint8_t *)vb + (long long)p.y1 * vbs);
    const float c00 = u0[p.x0], c10 = u0[p.x1], c01 = u1[p.x0], c11 = u1[p.x1];
    const float d00 = v0[p.x0], d10 = v0[p.x1], d01 = v1[p.x0], d11 = v1[p.x1];
    if (!(hscolor::known(c00, d00) && hscolor::known(c10, d10) && hscolor::known(c01, d01) && hscolor::known(c11, d11))) return r;
    const float c = bilinear(c00, c10, c01, c11, p.ax, p.ay), d = bilinear(d00, d10, d01, d11, p.ax, p.ay);
    const float ex = a + c, ey = b + d;
    const float exx = ex * ex, eyy = ey * ey;
    const float err2 = exx + eyy;
    const float aa = a * a, bb = b * b, cc = c * c, dd = d * d;
    const float mf = aa + bb, mb = cc + dd;
    const float mag2 = mf + mb;
    const float am = alpha * mag2;
    const float bound = am + beta;
    r.cls = err2 <= bound ? kConsistent : kInconsistent;
    r.err2 = err2;
    return r;
}

// The squared error in 1/256 px^2, saturated at 256 px^2.
HSFB_FN uint32_t quantise(float err2)
{
    const float q = err2 * 256.0f;
    return (uint32_t)(q < 65535.0f ? q : 65535.0f);
}

// The bits of the err2 plane at a pixel.
HSFB_FN uint32_t err2_bits(const Pixel &r) { return r.cls <= kInconsistent ? hscolor::float_bits(r.err2) : kNanBits; }

// What one lane, or the host loop, gathers.  32 bits hold a lane's share (hs_kernels_fb.hip.h); the host sums in Sums.
struct Acc {
    uint32_t cls[4], sum_q, max_bits;
};

HSFB_FN void account(Acc &s, const Pixel &r)
{
    s.cls[0] += r.cls == kConsistent;
    s.cls[1] += r.cls == kInconsistent;
    s.cls[2] += r.cls == kOutside;
    s.cls[3] += r.cls == kUnknown;
    if (r.cls > kInconsistent) return;
    s.sum_q += quantise(r.err2);
    const uint32_t bits = hscolor::float_bits(r.err2); // (never negative, never NaN: the bits order like the value)
    s.max_bits = bits > s.max_bits ? bits : s.max_bits;
}

// The sums of a whole check (the first 44 bytes of hsflow_fb_stats).
struct Sums {
    uint64_t cls[4], sum_q;
    uint32_t max_bits;
};

// A whole check in host memory.  Strides in BYTES.  mask, err2, sums may each be null.  Writes W bytes of every row of
// mask, W floats of every row of err2 and nothing else.
inline void fb_rows(const float *uf, size_t ufs, const float *vf, size_t vfs, const float *ub, size_t ubs, const float *vb, size_t vbs, int W, int H,
                    float alpha, float beta, const uint8_t value[4], uint8_t *mask, size_t ms, float *err2, size_t es, Sums *sums)
{
    Sums total = {{0, 0, 0, 0}, 0, 0};
    for (int y = 0; y < H; y++) {
        const float *ru = (const float *)((const uint8_t *)uf + (size_t)y * ufs), *rv = (const float *)((const uint8_t *)vf + (size_t)y * vfs);
        uint8_t *re = err2 ? (uint8_t *)err2 + (size_t)y * es : nullptr;
        for (int x = 0; x < W; x++) {
            const Pixel r = decide(ru[x], rv[x], x, y, W, H, ub, (long long)ubs, vb, (long long)vbs, alpha, beta);
            if (mask) mask[(size_t)y * ms + (size_t)x] = value[r.cls];
            if (re) {
                const uint32_t bits = err2_bits(r);
                memcpy(re + 4 * (size_t)x, &bits, sizeof bits);
            }
            Acc one = {{0, 0, 0, 0}, 0, 0};
            account(one, r);
            for (int k = 0; k < 4; k++) total.cls[k] += one.cls[k];
            total.sum_q += one.sum_q;
            total.max_bits = one.max_bits > total.max_bits ? one.max_bits : total.max_bits;
        }
    }
    if (sums) *sums = total;
}

} // namespace hsfb
