// hs_gmotion_rule.h -- the single global motion that explains a dense flow field (the camera's motion), fitted by a trimmed
// least squares, ONE definition for the device kernels (hs_kernels_gmotion.hip.h) and the host twin
// (hsflow_gmotion_fit_host), the way hs_warp_rule.h serves both sides of the warp.
//   Model.  Six fp32 parameters p[6]; with X = x - (W-1)/2 and Y = y - (H-1)/2 (exact in fp32: X = (float)(2x-(W-1)) * 0.5f)
//     mu = fl(fl(p0 + fl(p1 * X)) + fl(p2 * Y)),   mv = fl(fl(p3 + fl(p4 * X)) + fl(p5 * Y))
//   TRANSLATION: p1 = p2 = p4 = p5 = 0.  SIMILARITY: p1 = p5, p2 = -p4.  AFFINE: all six free.
//   Classes of a pixel with flow (a, b); the first that applies is final:
//     UNKNOWN (3)    !hscolor::known(a, b), or |a| > kMaxFlow or |b| > kMaxFlow
//     UNTRUSTED (2)  a state plane is given and its byte is 0
//     OUTLIER (1) / INLIER (0)  by r2 = fl(fl(ru * ru) + fl(rv * rv)) <= T with ru = fl(a - mu), rv = fl(b - mv); equality
//                    is an inlier; a NaN r2 (a model that overflows) is an outlier, and a NaN residual is written as kNanBits
//   Fit.  P passes.  Pass 0 takes every pixel that is neither UNKNOWN nor UNTRUSTED and gives M_0; pass j >= 1 takes the
//   INLIERS under M_{j-1} and T_j and gives M_j.  The outputs are classified under M_{P-1} and T_P.
//   Sums.  Exact integers, so the order of accumulation cannot matter and device and host agree bit for bit: the flow is
//   quantised q = (int)rintf(fl(a * 256)) (ties to even), coordinates are the doubled centred integers Xi = 2x - (W-1),
//   Yi = 2y - (H-1), and twelve int64 sums are taken (Sums).  The overflow proof is the static_asserts below.
//   Solve.  From the sums to p[6] in double, + - * / only, in the order written in solve(); every operation is IEEE on both
//   sides (-ffp-contract=off), the parameters are rounded to fp32 at the end.
//   Degenerate sets fall back AFFINE -> SIMILARITY -> TRANSLATION -> zero model (usable()).  The counts are integers; the
//   spreads A = n Sxx - Sx^2, C = n Syy - Sy^2 and the determinant A C - B^2 are doubles of integers -- exact while
//   n * Sxx < 2^53, rounded once per operation beyond -- and are compared RELATIVELY (kRel), so a set on one row, one column
//   or one line is refused at every frame size, and both sides, doing the same IEEE operations, take the same branch.
//   Threshold.  FIXED: T_j = fl(inlier_px * inlier_px) for every j >= 1.  AUTO: T_j comes from an exact 256-bin histogram of
//   r2 under M_{j-1} over all pixels that are neither UNKNOWN nor UNTRUSTED: bin = clamp((bits(r2) >> 21) - kBinBase, 0,
//   255), four bins per octave of r2 and no square root anywhere; T_j = max(min_thr2, fl(scale2 * upper edge of the bin
//   that holds the median)).  AUTO costs one more read of the flow per pass; that is accepted.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "hs_warp_rule.h"

#if defined(__clang__)
#pragma clang fp contract(off) // (what -ffp-contract=off says for the whole library, said again where it matters)
#endif

namespace hsgm {

constexpr int kTranslation = 0, kSimilarity = 1, kAffine = 2, kZero = 3; // HSFLOW_GMOTION_*; kZero: only as "used"
constexpr int kFixed = 0, kAuto = 1;                                      // HSFLOW_GMOTION_THRESHOLD_*
constexpr int kInlier = 0, kOutlier = 1, kUntrusted = 2, kUnknown = 3;
constexpr int kMaxPasses = 8;
constexpr unsigned kFlagFallback = 1u; // the model kind asked for could not be fitted; bits 8 .. 9: the kind that was
constexpr int kUsedShift = 8;
constexpr uint32_t kNanBits = 0x7fc00000u;

constexpr float kMaxFlow = 2048.0f;        // a component beyond this magnitude is UNKNOWN to the fit
constexpr int kQuantShift = 8;             // q = rint(a * 256)
constexpr int kMaxSide = 16384;            // the largest width and height the entry points accept
constexpr long long kMaxPixels = 1LL << 30; // ... and the largest W * H (hsflow_create's own bound on a plane)

// ---- no sum overflows -------------------------------------------------------------------------------------------------------
constexpr long long kMaxQ = (long long)kMaxFlow << kQuantShift; // |q| <= 2^19: |a * 256| <= 2^19 is exact in fp32, rintf keeps it
constexpr long long kMaxXi = kMaxSide - 1;                      // |Xi| <= W - 1, |Yi| <= H - 1
constexpr long long kInt64Max = 0x7fffffffffffffffLL;
static_assert(kMaxQ == 1LL << 19, "the quantised flow has 20 bits and a sign");
static_assert(kMaxPixels <= kInt64Max / (kMaxXi * kMaxXi), "sum of Xi^2, Xi Yi, Yi^2 over every pixel stays inside int64");
static_assert(kMaxPixels <= kInt64Max / (kMaxQ * kMaxXi), "sum of q Xi, q Yi over every pixel stays inside int64");
static_assert(kMaxPixels <= kInt64Max / kMaxQ && kMaxPixels <= kInt64Max / kMaxXi, "the first-order sums stay inside int64");
static_assert(kMaxPixels < (1LL << 32), "a histogram bin is 32 bits");

constexpr int kBinBase = (127 - 32) << 2; // bin 0 ends at r2 = 2^-32, bin 255 begins below 2^32
constexpr int kBins = 256;
constexpr double kRel = 1.0 / 68719476736.0; // 2^-36: rounding stays 2^16 below it, two columns at the far edge 2^8 above

struct Model {
    float p[6];
};

// The twelve sums of a set of pixels.
struct Sums {
    long long n, x, y, xx, xy, yy, u, ux, uy, v, vx, vy;
};

HSW_FN float centred(int i2) { return (float)i2 * 0.5f; } // i2 = 2x - (W-1): below 2^15, so the product is exact

// The model's motion at doubled centred coordinates (Xi, Yi).
HSW_FN void eval(const Model &m, int Xi, int Yi, float *mu, float *mv)
{
    const float X = centred(Xi), Y = centred(Yi);
    const float ax = m.p[1] * X, ay = m.p[2] * Y;
    const float s0 = m.p[0] + ax;
    *mu = s0 + ay;
    const float bx = m.p[4] * X, by = m.p[5] * Y;
    const float s1 = m.p[3] + bx;
    *mv = s1 + by;
}

// UNKNOWN / UNTRUSTED, or -1: the pixel is usable.  trusted: the state byte, 1 where no state plane is given.
HSW_FN int usable_class(float a, float b, unsigned trusted)
{
    if (!hscolor::known(a, b) || fabsf(a) > kMaxFlow || fabsf(b) > kMaxFlow) return kUnknown;
    if (!trusted) return kUntrusted;
    return -1;
}

// The squared residual of a usable pixel and its two components.
HSW_FN float residual2(float a, float b, float mu, float mv, float *ru, float *rv)
{
    *ru = a - mu;
    *rv = b - mv;
    const float uu = *ru * *ru, vv = *rv * *rv;
    return uu + vv;
}

// A residual component as the planes hold it: the quiet NaN kNanBits for an UNKNOWN pixel and for every NaN (whatever sign
// or payload the subtraction gave it), else the value's bits.
HSW_FN uint32_t residual_bits(float r, int cls) { return cls == kUnknown || r != r ? kNanBits : hscolor::float_bits(r); }

HSW_FN int quant(float a)
{
    const float s = a * 256.0f;
    return (int)rintf(s);
}

HSW_FN int bin_of(float r2)
{
    const int k = (int)(hscolor::float_bits(r2) >> 21) - kBinBase;
    return k < 0 ? 0 : k > kBins - 1 ? kBins - 1 : k;
}

HSW_FN float bin_upper(int k) { return hscolor::bits_float((uint32_t)(k + kBinBase + 1) << 21); }

// The threshold of AUTO from the histogram of r2 (hist[kBins], 32-bit counts).
HSW_FN float auto_threshold(const uint32_t *hist, float scale2, float min_thr2)
{
    unsigned long long total = 0;
    for (int k = 0; k < kBins; k++) total += hist[k];
    if (total == 0) return min_thr2;
    const unsigned long long target = (total + 1) / 2;
    unsigned long long cum = 0;
    int k = 0;
    for (; k < kBins - 1; k++) {
        cum += hist[k];
        if (cum >= target) break;
    }
    const float t = scale2 * bin_upper(k);
    return t > min_thr2 ? t : min_thr2;
}

// From the sums to the model.  kind: what was asked for; returns the flags (the kind used, kFlagFallback).
HSW_FN unsigned solve(const Sums &s, int kind, Model *out)
{
    const double n = (double)s.n, Sx = (double)s.x, Sy = (double)s.y, Sxx = (double)s.xx, Sxy = (double)s.xy, Syy = (double)s.yy;
    const double Su = (double)s.u, Sux = (double)s.ux, Suy = (double)s.uy, Sv = (double)s.v, Svx = (double)s.vx, Svy = (double)s.vy;
    const double nxx = n * Sxx, nyy = n * Syy;
    const double A = nxx - Sx * Sx, B = n * Sxy - Sx * Sy, C = nyy - Sy * Sy;
    const double Eu = n * Sux - Sx * Su, Fu = n * Suy - Sy * Su, Ev = n * Svx - Sx * Sv, Fv = n * Svy - Sy * Sv;
    const double AC = A * C, D = AC - B * B;
    const bool spread_x = A > nxx * kRel, spread_y = C > nyy * kRel;
    double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // in quantised flow per doubled coordinate
    int used = kZero;
    if (kind == kAffine && s.n >= 3 && spread_x && spread_y && D > AC * kRel) {
        used = kAffine;
        q[1] = (Eu * C - Fu * B) / D;
        q[2] = (Fu * A - Eu * B) / D;
        q[4] = (Ev * C - Fv * B) / D;
        q[5] = (Fv * A - Ev * B) / D;
        q[0] = (Su - q[1] * Sx - q[2] * Sy) / n;
        q[3] = (Sv - q[4] * Sx - q[5] * Sy) / n;
    } else if (kind >= kSimilarity && s.n >= 2 && (spread_x || spread_y)) {
        used = kSimilarity;
        const double den = A + C;
        const double a = (Eu + Fv) / den, b = (Ev - Fu) / den;
        q[1] = a; q[2] = -b; q[4] = b; q[5] = a;
        q[0] = (Su - a * Sx + b * Sy) / n;
        q[3] = (Sv - b * Sx - a * Sy) / n;
    } else if (s.n >= 1) {
        used = kTranslation;
        q[0] = Su / n;
        q[3] = Sv / n;
    }
    // q / 256 is the flow in pixels; a doubled coordinate is half a pixel, so a slope per pixel is 2 q / 256
    out->p[0] = (float)(q[0] / 256.0); out->p[1] = (float)(q[1] / 128.0); out->p[2] = (float)(q[2] / 128.0);
    out->p[3] = (float)(q[3] / 256.0); out->p[4] = (float)(q[4] / 128.0); out->p[5] = (float)(q[5] / 128.0);
    return (unsigned)used << kUsedShift | (used != kind ? kFlagFallback : 0u);
}

// One pixel's share of the sums.
HSW_FN void add(Sums &s, int Xi, int Yi, int qu, int qv)
{
    const long long X = Xi, Y = Yi, U = qu, V = qv;
    s.n += 1; s.x += X; s.y += Y; s.xx += X * X; s.xy += X * Y; s.yy += Y * Y;
    s.u += U; s.ux += U * X; s.uy += U * Y; s.v += V; s.vx += V * X; s.vy += V * Y;
}

// ---- a whole field in host memory ---------------------------------------------------------------------------------------------

struct Field {
    const float *u, *v;
    size_t fs; // rows of u and v fs BYTES apart
    const uint8_t *state; // or NULL
    size_t ss;
    int W, H;
};

struct Fit {
    int kind, passes, mode;
    float fixed_thr, scale2, min_thr2;
};

struct Result {
    Model m;
    float thr;
    unsigned flags;
    uint64_t cls[4];
};

inline const float *frow(const float *p, size_t stride, int y) { return (const float *)((const uint8_t *)p + (size_t)y * stride); }

// One pass over the field: the sums of the pixels that take part (first: all usable ones; else the inliers under m and
// thr) and, where hist is not NULL, the histogram of r2 under m over the usable ones.
inline void pass_rows(const Field &f, bool first, const Model &m, float thr, Sums *sums, uint32_t *hist)
{
    for (int y = 0; y < f.H; y++) {
        const float *ru = frow(f.u, f.fs, y), *rv = frow(f.v, f.fs, y);
        const int Yi = 2 * y - (f.H - 1);
        for (int x = 0; x < f.W; x++) {
            const float a = ru[x], b = rv[x];
            if (usable_class(a, b, f.state ? f.state[(size_t)y * f.ss + x] : 1u) >= 0) continue;
            const int Xi = 2 * x - (f.W - 1);
            bool in = true;
            if (!first) {
                float mu, mv, du, dv;
                eval(m, Xi, Yi, &mu, &mv);
                const float r2 = residual2(a, b, mu, mv, &du, &dv);
                in = r2 <= thr;
                if (hist) hist[bin_of(r2)]++;
            }
            if (sums && in) add(*sums, Xi, Yi, quant(a), quant(b));
        }
    }
}

// The fit, then the outputs under the final model and threshold: mask (value[class]), the residual planes ru, rv (rows rs
// bytes apart), each may be NULL.  Writes W bytes / W floats of every row and nothing else.
inline void fit_rows(const Field &f, const Fit &fit, const uint8_t value[4], uint8_t *mask, size_t ms, float *resu, float *resv, size_t rs, Result *res)
{
    Model m = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};
    float thr = fit.fixed_thr;
    unsigned flags = 0;
    uint32_t hist[kBins];
    for (int j = 0; j <= fit.passes; j++) {
        if (j > 0 && fit.mode == kAuto) {
            for (int k = 0; k < kBins; k++) hist[k] = 0;
            pass_rows(f, false, m, thr, nullptr, hist);
            thr = auto_threshold(hist, fit.scale2, fit.min_thr2);
        }
        if (j == fit.passes) break;
        Sums s = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        pass_rows(f, j == 0, m, thr, &s, nullptr);
        flags = solve(s, fit.kind, &m);
    }
    uint64_t cls[4] = {0, 0, 0, 0};
    for (int y = 0; y < f.H; y++) {
        const float *ru = frow(f.u, f.fs, y), *rv = frow(f.v, f.fs, y);
        const int Yi = 2 * y - (f.H - 1);
        for (int x = 0; x < f.W; x++) {
            const float a = ru[x], b = rv[x];
            int c = usable_class(a, b, f.state ? f.state[(size_t)y * f.ss + x] : 1u);
            float mu, mv, du, dv;
            eval(m, 2 * x - (f.W - 1), Yi, &mu, &mv);
            const float r2 = residual2(a, b, mu, mv, &du, &dv);
            if (c < 0) c = r2 <= thr ? kInlier : kOutlier;
            cls[c]++;
            if (mask) mask[(size_t)y * ms + x] = value[c];
            if (resu) {
                uint32_t *pu = (uint32_t *)((uint8_t *)resu + (size_t)y * rs) + x, *pv = (uint32_t *)((uint8_t *)resv + (size_t)y * rs) + x;
                *pu = residual_bits(du, c);
                *pv = residual_bits(dv, c);
            }
        }
    }
    if (res) {
        res->m = m;
        res->thr = thr;
        res->flags = flags;
        for (int k = 0; k < 4; k++) res->cls[k] = cls[k];
    }
}

// A picture warped backwards by the model: hswarp's rule with (a, b) = (mu, mv) at every pixel; no flow plane is read.
template <int C>
inline void warp_rows(const Model &m, int W, int H, float t, int border, uint32_t fill, const uint8_t *src, size_t ss, const uint8_t *ref, size_t rs,
                      uint8_t *dst, size_t ds, hswarp::Sums *sums)
{
    hswarp::Sums total = {0, 0, 0, 0, 0, 0, 0};
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            hswarp::Acc one = {0, 0, 0, 0, 0, 0, 0};
            float mu, mv;
            eval(m, 2 * x - (W - 1), 2 * y - (H - 1), &mu, &mv);
            const hswarp::Tap p = hswarp::locate(mu, mv, x, y, t, W, H, border);
            const uint32_t w = hswarp::pixel<C>(src, (long long)ss, p, fill);
            if (dst)
                for (int c = 0; c < C; c++) dst[(size_t)y * ds + (size_t)C * x + c] = (uint8_t)(w >> (8 * c));
            if (sums) {
                const uint32_t q = hswarp::load_pixel<C>(src + (size_t)y * ss + (size_t)C * x);
                const uint32_t r = ref ? hswarp::load_pixel<C>(ref + (size_t)y * rs + (size_t)C * x) : 0u;
                hswarp::account<C>(one, p.cls, w, q, r, ref != nullptr);
            }
            total.inside += one.inside; total.outside += one.outside; total.unknown += one.unknown;
            total.sad_warped += one.sad_warped; total.sad_plain += one.sad_plain;
            total.max_warped = one.max_warped > total.max_warped ? one.max_warped : total.max_warped;
            total.max_plain = one.max_plain > total.max_plain ? one.max_plain : total.max_plain;
        }
    if (sums) *sums = total;
}

// "First m1, then m2" on positions, and the inverse map; in double, rounded to fp32.  A position is centred: X' = X + m(X),
// so the linear part of the map is I + [[p1, p2], [p4, p5]] and its shift (p0, p3).
inline void compose(const Model &m1, const Model &m2, Model *out)
{
    const double a1[4] = {1.0 + (double)m1.p[1], (double)m1.p[2], (double)m1.p[4], 1.0 + (double)m1.p[5]};
    const double a2[4] = {1.0 + (double)m2.p[1], (double)m2.p[2], (double)m2.p[4], 1.0 + (double)m2.p[5]};
    const double t1[2] = {(double)m1.p[0], (double)m1.p[3]}, t2[2] = {(double)m2.p[0], (double)m2.p[3]};
    out->p[0] = (float)(a2[0] * t1[0] + a2[1] * t1[1] + t2[0]);
    out->p[3] = (float)(a2[2] * t1[0] + a2[3] * t1[1] + t2[1]);
    out->p[1] = (float)(a2[0] * a1[0] + a2[1] * a1[2] - 1.0);
    out->p[2] = (float)(a2[0] * a1[1] + a2[1] * a1[3]);
    out->p[4] = (float)(a2[2] * a1[0] + a2[3] * a1[2]);
    out->p[5] = (float)(a2[2] * a1[1] + a2[3] * a1[3] - 1.0);
}

// false: the linear part is singular (or not finite).
inline bool invert(const Model &m, Model *out)
{
    const double a = 1.0 + (double)m.p[1], b = (double)m.p[2], c = (double)m.p[4], d = 1.0 + (double)m.p[5];
    const double det = a * d - b * c;
    if (!(det != 0.0) || !isfinite(det)) return false;
    const double ia = d / det, ib = -b / det, ic = -c / det, id = a / det;
    const double tx = (double)m.p[0], ty = (double)m.p[3];
    out->p[0] = (float)(-(ia * tx + ib * ty));
    out->p[3] = (float)(-(ic * tx + id * ty));
    out->p[1] = (float)(ia - 1.0);
    out->p[2] = (float)ib;
    out->p[4] = (float)ic;
    out->p[5] = (float)(id - 1.0);
    for (int k = 0; k < 6; k++)
        if (!isfinite(out->p[k])) return false;
    return true;
}

} // namespace hsgm
