// hs_chain_rule.h -- following pixels and points through a sequence of dense flow fields, ONE definition for the device
// kernels (hs_kernels_chain.hip.h) and the host twins (hsflow_chain_flow_host, hsflow_track_points_host), the way
// hs_fb_rule.h serves both sides of the forward-backward check, which is a chain of two.
// Flow planes (u_k, v_k), k = 0 .. n-1, all W x H: plane k is the flow from frame k to frame k + 1.  Optional state planes
// s_k (u8, non-zero = trusted: the default mask of hsflow_fb as it is).  Composition is not the sum of the planes: the
// vector of plane k is read where the pixel HAS ARRIVED in frame k, by bilinear interpolation.
// All arithmetic is fp32 and every operation is rounded on its own (the library is built with -ffp-contract=off), so host
// and device give the same bits.  Four classes: ALIVE 0, LEFT 1, UNTRUSTED 2, UNKNOWN 3.
//   One step, advance(a, b, x, y, plane k) -- (a, b) is what was accumulated so far, (x, y) where it started:
//     p = hswarp::locate(a, b, x, y, 1.0f, W, H, kBorderConstant): fx = fl((float)x + a), fy alike
//     UNKNOWN    iff p.cls is unknown (!hscolor::known(a, b));  LEFT iff p.cls is outside (the position left the frame)
//     UNKNOWN    iff any of the four taps of (u_k, v_k) at p is not known, even where its weight is 0
//     UNTRUSTED  iff there is a state plane k and any of its four taps is zero
//     c = hsfb::bilinear of the u taps, d of the v taps; a' = fl(a + c), b' = fl(b + d)
//     UNKNOWN    iff !known(a', b'), else ALIVE with (a', b')
//   Dense chain, pixel (x, y): the start is (u_0, v_0)[y][x] verbatim (no sampling, no addition: n = 1 is a copy, -0.0
//     included), UNKNOWN if not known, else UNTRUSTED if s_0[y][x] == 0, and the pixel advances through planes 1 .. n-1;
//     or the start is the caller's (U0, V0)[y][x], UNKNOWN if not known, no state is tested at the start, and the pixel
//     advances through all of 0 .. n-1.  The first class other than ALIVE is final and the walk ends there.
//     age = the number of planes of this call the pixel passed (n iff ALIVE; the verbatim start counts as plane 0).
//     The last plane's vector may point outside the frame: only known() is asked of the result.
//   Point (px, py) in frame 0: UNKNOWN if not known, else it advances through ALL n planes with advance(px, py, 0, 0, k), so
//     what accumulates is the position.  Row j of its track is the position after j planes for j <= age, the NaN bits
//     beyond; row 0 is the start as given.
//   Statistics, exact integers that do not depend on the order: the four class counts, the sum of the ages, and the bits of
//     the largest fl(fl(U*U) + fl(V*V)) over ALIVE (for points U = fl(px_n - px_0), V alike).  Known components are at most
//     1e9 (differences 2e9), so nothing overflows.
// Every tap that locate() names lies inside the W x H plane, and a position that is not sampled names tap (0, 0), so the
// gathers can be issued before the class is looked at (the kernels do).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hs_color_rule.h"
#include "hs_fb_rule.h"
#include "hs_warp_rule.h"

#if defined(__clang__)
#pragma clang fp contract(off) // (what -ffp-contract=off says for the whole library, said again where it matters)
#endif

#if defined(__HIPCC__)
#define HSCHAIN_FN __host__ __device__ inline
#else
#define HSCHAIN_FN inline
#endif

namespace hschain {

constexpr int kAlive = 0, kLeft = 1, kUntrusted = 2, kUnknown = 3;
constexpr int kMaxPairs = 32;              // HSFLOW_CHAIN_MAX_PAIRS
constexpr int kMaxPoints = 1 << 24;        // points of one call
constexpr uint32_t kNanBits = 0x7fc00000u; // U, V and track rows of what is not ALIVE: the colour picture calls it unknown

// One plane of the chain: rows of u and v `fs` BYTES apart, of s (or null: no test) `ss` bytes apart.
struct Plane {
    const float *u, *v;
    const uint8_t *s;
    long long fs, ss;
};

// The eight flow taps and the state taps of one position.
struct Taps {
    float c00, c10, c01, c11, d00, d10, d01, d11;
    bool trusted;
};

HSCHAIN_FN Taps gather(const hswarp::Tap &p, const Plane &f)
{
    Taps t;
    const long long o0 = (long long)p.y0 * f.fs, o1 = (long long)p.y1 * f.fs;
    const float *u0 = (const float *)((const uint8_t *)f.u + o0), *u1 = (const float *)((const uint8_t *)f.u + o1);
    const float *v0 = (const float *)((const uint8_t *)f.v + o0), *v1 = (const float *)((const uint8_t *)f.v + o1);
    t.c00 = u0[p.x0]; t.c10 = u0[p.x1]; t.c01 = u1[p.x0]; t.c11 = u1[p.x1];
    t.d00 = v0[p.x0]; t.d10 = v0[p.x1]; t.d01 = v1[p.x0]; t.d11 = v1[p.x1];
    t.trusted = true;
    if (f.s) {
        const uint8_t *s0 = f.s + (long long)p.y0 * f.ss, *s1 = f.s + (long long)p.y1 * f.ss;
        t.trusted = (s0[p.x0] != 0) & (s0[p.x1] != 0) & (s1[p.x0] != 0) & (s1[p.x1] != 0);
    }
    return t;
}

// The class of the step from the position p with the taps t; (a, b) move on where it is ALIVE.
HSCHAIN_FN int settle(float &a, float &b, const hswarp::Tap &p, const Taps &t)
{
    if (p.cls == hswarp::kUnknown) return kUnknown;
    if (p.cls == hswarp::kOutside) return kLeft;
    if (!(hscolor::known(t.c00, t.d00) && hscolor::known(t.c10, t.d10) && hscolor::known(t.c01, t.d01) && hscolor::known(t.c11, t.d11))) return kUnknown;
    if (!t.trusted) return kUntrusted;
    const float c = hsfb::bilinear(t.c00, t.c10, t.c01, t.c11, p.ax, p.ay), d = hsfb::bilinear(t.d00, t.d10, t.d01, t.d11, p.ax, p.ay);
    const float a2 = a + c, b2 = b + d;
    if (!hscolor::known(a2, b2)) return kUnknown;
    a = a2;
    b = b2;
    return kAlive;
}

HSCHAIN_FN int advance(float &a, float &b, int x, int y, int W, int H, const Plane &f)
{
    const hswarp::Tap p = hswarp::locate(a, b, x, y, 1.0f, W, H, hswarp::kBorderConstant);
    return settle(a, b, p, gather(p, f));
}

// The class of a dense start.  s0: the byte of the state plane there (1 where none is tested).
HSCHAIN_FN int start_class(float a, float b, unsigned s0) { return !hscolor::known(a, b) ? kUnknown : s0 == 0u ? kUntrusted : kAlive; }

HSCHAIN_FN uint32_t mag2_bits(float U, float V)
{
    const float uu = U * U, vv = V * V;
    return hscolor::float_bits(uu + vv); // (never negative, never NaN: the bits order like the value)
}

// What one lane, or the host loop, gathers.  32 bits hold a lane's share (hs_kernels_chain.hip.h); the host sums in Sums.
struct Acc {
    uint32_t cls[4], sum_age, max_bits;
};

HSCHAIN_FN void account(Acc &s, int cls, unsigned age, float U, float V)
{
    s.cls[0] += cls == kAlive;
    s.cls[1] += cls == kLeft;
    s.cls[2] += cls == kUntrusted;
    s.cls[3] += cls == kUnknown;
    s.sum_age += age;
    if (cls != kAlive) return;
    const uint32_t bits = mag2_bits(U, V);
    s.max_bits = bits > s.max_bits ? bits : s.max_bits;
}

// The sums of a whole call (the first 44 bytes of hsflow_chain_stats).
struct Sums {
    uint64_t cls[4], sum_age;
    uint32_t max_bits;
};

inline void add(Sums &total, const Acc &one)
{
    for (int k = 0; k < 4; k++) total.cls[k] += one.cls[k];
    total.sum_age += one.sum_age;
    total.max_bits = one.max_bits > total.max_bits ? one.max_bits : total.max_bits;
}

inline void put_bits(void *row, size_t x, uint32_t bits) { memcpy((uint8_t *)row + 4 * x, &bits, sizeof bits); }

// A whole dense chain in host memory.  planes: n of them.  U0, V0: the start planes (both or neither), rows s0s BYTES
// apart.  U, V (rows os bytes apart), status, age, sums may each be null.  Writes W floats of every row of U and V, W bytes
// of every row of status and age and nothing else.
inline void chain_rows(const Plane *planes, int n, int W, int H, const float *U0, const float *V0, size_t s0s, const uint8_t value[4], float *U, float *V,
                       size_t os, uint8_t *status, size_t sts, uint8_t *age, size_t as, Sums *sums)
{
    Sums total = {{0, 0, 0, 0}, 0, 0};
    const bool given = U0 != nullptr;
    for (int y = 0; y < H; y++) {
        const float *ru = (const float *)((const uint8_t *)(given ? U0 : planes[0].u) + (size_t)y * (given ? s0s : (size_t)planes[0].fs));
        const float *rv = (const float *)((const uint8_t *)(given ? V0 : planes[0].v) + (size_t)y * (given ? s0s : (size_t)planes[0].fs));
        const uint8_t *rs = !given && planes[0].s ? planes[0].s + (size_t)y * (size_t)planes[0].ss : nullptr;
        for (int x = 0; x < W; x++) {
            float a = ru[x], b = rv[x];
            int cls = start_class(a, b, rs ? rs[x] : 1u);
            int k = given ? 0 : 1;
            unsigned passed = cls == kAlive ? (unsigned)k : 0u;
            for (; cls == kAlive && k < n; k++) {
                cls = advance(a, b, x, y, W, H, planes[k]);
                passed += cls == kAlive;
            }
            if (U) {
                put_bits((uint8_t *)U + (size_t)y * os, (size_t)x, cls == kAlive ? hscolor::float_bits(a) : kNanBits);
                put_bits((uint8_t *)V + (size_t)y * os, (size_t)x, cls == kAlive ? hscolor::float_bits(b) : kNanBits);
            }
            if (status) status[(size_t)y * sts + (size_t)x] = value[cls];
            if (age) age[(size_t)y * as + (size_t)x] = (uint8_t)passed;
            Acc one = {{0, 0, 0, 0}, 0, 0};
            account(one, cls, passed, a, b);
            add(total, one);
        }
    }
    if (sums) *sums = total;
}

// One point through the n planes.  row(j, bits of x, bits of y) receives the track, j = 0 .. n.  Returns the class; *passed
// the age, (*lx, *ly) the bits of the last position (the NaN bits unless ALIVE), *mag the bits for the statistics.
template <class Row>
HSCHAIN_FN int track_point(const Plane *planes, int n, int W, int H, float px, float py, Row row, unsigned *passed, uint32_t *lx, uint32_t *ly, uint32_t *mag)
{
    float a = px, b = py;
    int cls = start_class(a, b, 1u);
    unsigned k = 0;
    row(0, hscolor::float_bits(px), hscolor::float_bits(py));
    for (int j = 0; j < n; j++) {
        if (cls == kAlive) {
            cls = advance(a, b, 0, 0, W, H, planes[j]);
            k += cls == kAlive;
        }
        row(j + 1, cls == kAlive ? hscolor::float_bits(a) : kNanBits, cls == kAlive ? hscolor::float_bits(b) : kNanBits);
    }
    *passed = k;
    *lx = cls == kAlive ? hscolor::float_bits(a) : kNanBits;
    *ly = cls == kAlive ? hscolor::float_bits(b) : kNanBits;
    const float dx = a - px, dy = b - py;
    *mag = cls == kAlive ? mag2_bits(dx, dy) : 0u;
    return cls;
}

// m points in host memory.  xy: m pairs.  track ((n + 1) rows of m pairs), last (m pairs), status, age (m bytes), sums may
// each be null.
inline void track_rows(const Plane *planes, int n, int W, int H, const float *xy, int m, const uint8_t value[4], float *track, float *last, uint8_t *status,
                       uint8_t *age, Sums *sums)
{
    Sums total = {{0, 0, 0, 0}, 0, 0};
    for (int i = 0; i < m; i++) {
        unsigned passed = 0;
        uint32_t lx = 0, ly = 0, mag = 0;
        const int cls = track_point(
            planes, n, W, H, xy[2 * (size_t)i], xy[2 * (size_t)i + 1],
            [&](int j, uint32_t bx, uint32_t by) {
                if (!track) return;
                put_bits(track, ((size_t)j * (size_t)m + (size_t)i) * 2, bx);
                put_bits(track, ((size_t)j * (size_t)m + (size_t)i) * 2 + 1, by);
            },
            &passed, &lx, &ly, &mag);
        if (last) {
            put_bits(last, 2 * (size_t)i, lx);
            put_bits(last, 2 * (size_t)i + 1, ly);
        }
        if (status) status[i] = value[cls];
        if (age) age[i] = (uint8_t)passed;
        total.cls[cls]++;
        total.sum_age += passed;
        total.max_bits = mag > total.max_bits ? mag : total.max_bits;
    }
    if (sums) *sums = total;
}

} // namespace hschain
