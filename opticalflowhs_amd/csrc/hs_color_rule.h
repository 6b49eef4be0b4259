// hs_color_rule.h -- the colour picture of a dense flow field, ONE definition for the device kernels
// (hs_kernels_color.hip.h) and the host twin (hsflow_color_flow_host), the way hs_pre_rule.h serves both sides of the
// pre-processing.  The picture is the Middlebury colour wheel (Baker et al., "A Database and Evaluation Methodology for
// Optical Flow", colorcode.cpp / flowIO.h; KITTI's and Sintel's tools and flow_to_image reproduce it): hue is the
// direction, saturation the magnitude, zero flow is white, unknown flow is black.
// All arithmetic is fp32 and every operation is rounded on its own (the library is built with -ffp-contract=off; sqrtf
// and / are the correctly rounded ones on both sides), so host and device give the same bytes.  Three departures from the
// Middlebury program, written down in include/hsflow.h:
//   the RADIUS is normalised, after the square root, not the components before it: with the scale taken from the
//     picture itself rad <= 1 then holds exactly, and the pixel that sets the scale cannot fall into the "> 1" branch;
//   the angle is this header's own atan2 (a six-term odd polynomial on [0, 1] and the usual unfolding), not a library's;
//   inside the scale the saturation 1 - rad (1 - col) is formed as (1 - rad) + rad col: the same quantity, but exact at both
//     ends -- white at rad = 0 and the wheel's own level at rad = 1, where fl(1 - fl(1 - col)) loses a level for every
//     wheel level 1 .. 64 and every even one up to 126 (43 / 255 -> 0.16862744 -> 42).  It never exceeds 1.
// For one pixel with flow (a, b) and scale m:
//   unknown  iff isnan(a) || isnan(b) || |a| > 1e9 || |b| > 1e9: (0, 0, 0), and it does not count for the scale
//   r        = sqrt(fl(fl(a*a) + fl(b*b))),  rad = fl(r / m)
//   theta    = atan2_rule(-b, -a),  fk = fl(fl(fl(fl(theta / pi) + 1) * 0.5) * 54),  k0 = min((int)fk, 54),
//              k1 = k0 == 54 ? 0 : k0 + 1,  f = fl(fk - k0)
//   channel  c0 = fl(wheel[k0] / 255), c1 alike; col = fl(fl(fl(1 - f) * c0) + fl(f * c1));
//              rad <= 1: col = fl(fl(1 - rad) + fl(rad * col)), else col = fl(col * 0.75);  byte = (int)fl(255 * col)
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__clang__)
#pragma clang fp contract(off) // (what -ffp-contract=off says for the whole library, said again where it matters)
#endif

#if defined(__HIPCC__)
#define HSC_FN __host__ __device__ inline
#else
#define HSC_FN inline
#endif

namespace hscolor {

constexpr int kWheel = 55;            // RY 15, YG 6, GC 4, CB 11, BM 13, MR 6
constexpr float kUnknown = 1e9f;      // a component beyond this magnitude is "unknown flow" (flowIO.h: UNKNOWN_FLOW_THRESH)
constexpr float kPi = 3.14159274f;    // fl(pi)
constexpr float kHalfPi = 1.57079637f; // fl(pi / 2)

// Entry k of the wheel as R | G << 8 | B << 16, by Middlebury's integer arithmetic (makecolorwheel).
HSC_FN uint32_t wheel_entry(int k)
{
    if (k < 15) return 255u | (uint32_t)(255 * k / 15) << 8;
    k -= 15;
    if (k < 6) return (uint32_t)(255 - 255 * k / 6) | 255u << 8;
    k -= 6;
    if (k < 4) return 255u << 8 | (uint32_t)(255 * k / 4) << 16;
    k -= 4;
    if (k < 11) return (uint32_t)(255 - 255 * k / 11) << 8 | 255u << 16;
    k -= 11;
    if (k < 13) return (uint32_t)(255 * k / 13) | 255u << 16;
    k -= 13;
    return 255u | (uint32_t)(255 - 255 * k / 6) << 16;
}

HSC_FN uint32_t float_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

HSC_FN float bits_float(uint32_t u)
{
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

HSC_FN bool known(float a, float b) { return !(a != a || b != b || fabsf(a) > kUnknown || fabsf(b) > kUnknown); }

// The raw radius of a known pixel: never negative, never NaN, so its bit pattern orders like the value.
HSC_FN float radius(float a, float b)
{
    const float aa = a * a, bb = b * b;
    const float s = aa + bb;
    return sqrtf(s);
}

// The scale of a picture whose largest raw radius has the bit pattern `bits` (0: no known pixel moves).
HSC_FN float auto_scale(uint32_t bits) { return bits == 0u ? 1.0f : bits_float(bits); }

// atan t on [0, 1] as t * P(t * t): six terms, a least-squares fit at Chebyshev nodes reweighted towards equal ripple,
// rounded to fp32.  max |p - atan t| over 2^22 evenly spaced t and the 4096 floats next to either end: 1.76e-6
// (tests/test_color_host.py holds 4e-6).
HSC_FN float atan_unit(float t)
{
    const float s = t * t;
    float p = -0.011719128116965294f;
    p = p * s; p = p + 0.052647337317466736f;
    p = p * s; p = p + -0.11642647534608841f;
    p = p * s; p = p + 0.19354037940502167f;
    p = p * s; p = p + -0.33262282609939575f;
    p = p * s; p = p + 0.9999772310256958f;
    return t * p;
}

// atan2 with C's conventions for signed zeros: (+0, -0) is pi, (-0, -0) is -pi, (-0, +0) is -0.
HSC_FN float atan2_rule(float y, float x)
{
    const float ay = fabsf(y), ax = fabsf(x);
    const float mn = ay < ax ? ay : ax, mx = ay < ax ? ax : ay;
    const float t = mx == 0.0f ? 0.0f : mn / mx;
    float p = atan_unit(t);
    if (ay > ax) p = kHalfPi - p;
    if (float_bits(x) >> 31) p = kPi - p;
    if (float_bits(y) >> 31) p = -p;
    return p;
}

// Channel c of wheel entry k as the rule uses it: fl(level / 255).  Both sides keep the 165 of them in a table (`levels`
// below: entry k's three at 3 k) instead of dividing six times per pixel; the values are the same.
HSC_FN float wheel_level(int k, int c) { return (float)((wheel_entry(k) >> (8 * c)) & 255u) / 255.0f; }

// One pixel as R | G << 8 | B << 16.  levels: the 165 values of wheel_level.  m: the scale, > 0.
HSC_FN uint32_t pixel(float a, float b, float m, const float *levels)
{
    if (!known(a, b)) return 0u;
    const float rad = radius(a, b) / m;
    const float theta = atan2_rule(-b, -a);
    float fk = theta / kPi;
    fk = fk + 1.0f;
    fk = fk * 0.5f;
    fk = fk * 54.0f;
    int k0 = (int)fk;
    if (k0 > kWheel - 1) k0 = kWheel - 1;
    const int k1 = k0 == kWheel - 1 ? 0 : k0 + 1;
    const float f = fk - (float)k0, g = 1.0f - f;
    uint32_t out = 0u;
    for (int c = 0; c < 3; c++) {
        const float c0 = levels[3 * k0 + c], c1 = levels[3 * k1 + c];
        const float lo = g * c0, hi = f * c1;
        float col = lo + hi;
        if (rad <= 1.0f) { // 1 - rad (1 - col) as (1 - rad) + rad col: exact at rad = 0 and at rad = 1
            const float w = 1.0f - rad, s = rad * col;
            col = w + s;
        } else {
            col = col * 0.75f;
        }
        out |= (uint32_t)(int)(255.0f * col) << (8 * c);
    }
    return out;
}

// A whole picture in host memory.  u, v: rows us / vs BYTES apart.  fixed_m > 0: the scale; otherwise it is taken from the
// picture.  Writes 3 * W bytes of every row and nothing else; returns the scale it used.
inline float color_rows(const float *u, size_t us, const float *v, size_t vs, int W, int H, float fixed_m, uint8_t *rgb, size_t stride)
{
    float levels[3 * kWheel];
    for (int k = 0; k < 3 * kWheel; k++) levels[k] = wheel_level(k / 3, k % 3);
    float m = fixed_m;
    if (!(m > 0.0f)) {
        uint32_t bits = 0u;
        for (int y = 0; y < H; y++) {
            const float *ru = (const float *)((const uint8_t *)u + (size_t)y * us), *rv = (const float *)((const uint8_t *)v + (size_t)y * vs);
            for (int x = 0; x < W; x++)
                if (known(ru[x], rv[x])) {
                    const uint32_t r = float_bits(radius(ru[x], rv[x]));
                    if (r > bits) bits = r;
                }
        }
        m = auto_scale(bits);
    }
    for (int y = 0; y < H; y++) {
        const float *ru = (const float *)((const uint8_t *)u + (size_t)y * us), *rv = (const float *)((const uint8_t *)v + (size_t)y * vs);
        uint8_t *d = rgb + (size_t)y * stride;
        for (int x = 0; x < W; x++) {
            const uint32_t c = pixel(ru[x], rv[x], m, levels);
            d[3 * x] = (uint8_t)c;
            d[3 * x + 1] = (uint8_t)(c >> 8);
            d[3 * x + 2] = (uint8_t)(c >> 16);
        }
    }
    return m;
}

} // namespace hscolor
