// hs_pyramid_rule.h -- the two rules a coarse-to-fine solve adds to the solver, the warp (hs_warp_rule.h) and the median
// (hs_median_rule.h): `down`, a frame at half the size, and `prolong`, a flow plane at twice the size.  ONE definition for
// the device kernels (hs_kernels_pyramid.hip.h) and the host twins (hsflow_pyramid_down_host, hsflow_pyramid_prolong_host),
// the way hs_warp_rule.h serves both sides of the warp.
//   down     a u8 plane of W x H gives one of ceil(W/2) x ceil(H/2):
//              dst(x, y) = (sum_{i,j=-2..2} k_i k_j src(clamp(2x+i, 0, W-1), clamp(2y+j, 0, H-1)) + 128) >> 8,  k = (1, 4, 6, 4, 1).
//            Exact integers: nothing depends on the order.  The sum of one row's five taps is at most 16 * 255 = 4080 and
//            fits 16 bits; both sides filter separably, rows first.
//   prolong  a coarse plane c of Wc x Hc floats gives a fine one of W x H, Wc = ceil(W/2), Hc = ceil(H/2).  All fp32, every
//            operation rounded on its own (the library is built with -ffp-contract=off):
//              h(x, r)  = c(x>>1, r) for even x;  fl(fl(c(k, r) + c(min(k+1, Wc-1), r)) * 0.5f), k = x>>1, for odd x
//              g(x, y)  = h(x, y>>1) for even y;  fl(fl(h(x, r) + h(x, min(r+1, Hc-1))) * 0.5f), r = y>>1, for odd y
//              dst(x, y) = fl(2 * g(x, y))
//            Even positions copy: they take part in no arithmetic, so a NaN or an Inf beside them stays where it is.
//   total    the flow after a step is fl(u0 + du), fl(v0 + dv): one fp32 addition per component.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off) // (what -ffp-contract=off says for the whole library, said again where it matters)
#endif

#if defined(__HIPCC__)
#define HSP_FN __host__ __device__ inline
#else
#define HSP_FN inline
#endif

namespace hspyr {

constexpr int kMaxLevels = 8; // HSFLOW_PYRAMID_MAX_LEVELS
constexpr int kMaxWarps = 8;  // HSFLOW_PYRAMID_MAX_WARPS

HSP_FN int half_up(int n) { return (n + 1) >> 1; }
HSP_FN int clampi(int i, int hi) { return i < 0 ? 0 : i > hi ? hi : i; }

// ---- down ----------------------------------------------------------------------------------------------------------------

// Five taps along one axis: bytes give a row sum (<= 4080), row sums give the pixel's sum (<= 65280).
HSP_FN int taps5(int a, int b, int c, int d, int e) { return a + 4 * b + 6 * c + 4 * d + e; }
HSP_FN uint8_t down_finish(int sum) { return (uint8_t)((sum + 128) >> 8); }

// The row sum of source row yy (already clamped) around the output column x.
HSP_FN int down_row_sum(const uint8_t *row, int W, int x)
{
    const int m = W - 1, c = 2 * x;
    return taps5(row[clampi(c - 2, m)], row[clampi(c - 1, m)], row[clampi(c, m)], row[clampi(c + 1, m)], row[clampi(c + 2, m)]);
}

HSP_FN uint8_t down_pixel(const uint8_t *src, long long stride, int W, int H, int x, int y)
{
    int s[5];
    for (int j = 0; j < 5; j++) s[j] = down_row_sum(src + (long long)clampi(2 * y + j - 2, H - 1) * stride, W, x);
    return down_finish(taps5(s[0], s[1], s[2], s[3], s[4]));
}

// A whole plane in host memory.  Writes ceil(W/2) bytes of each of the ceil(H/2) rows of dst and nothing else.
inline void down_rows(const uint8_t *src, size_t ss, int W, int H, uint8_t *dst, size_t ds)
{
    const int Wd = half_up(W), Hd = half_up(H);
    for (int y = 0; y < Hd; y++)
        for (int x = 0; x < Wd; x++) dst[(size_t)y * ds + (size_t)x] = down_pixel(src, (long long)ss, W, H, x, y);
}

// ---- prolong -------------------------------------------------------------------------------------------------------------

HSP_FN float mid(float a, float b)
{
    const float s = a + b;
    return s * 0.5f;
}

// One axis: the value at fine position i between the coarse neighbours a = c(i>>1) and b = c(min((i>>1)+1, n-1)).
HSP_FN float along(float a, float b, int i) { return (i & 1) ? mid(a, b) : a; }

// The fine pixel (x, y) from its four coarse neighbours: c00 = c(k, r), c10 = c(k1, r), c01 = c(k, r1), c11 = c(k1, r1)
// with k = x>>1, k1 = min(k+1, Wc-1), r = y>>1, r1 = min(r+1, Hc-1).
HSP_FN float prolong_value(float c00, float c10, float c01, float c11, int x, int y)
{
    const float h0 = along(c00, c10, x);
    if (!(y & 1)) return 2.0f * h0;
    const float h1 = along(c01, c11, x);
    return 2.0f * mid(h0, h1);
}

// c: rows cs BYTES apart.
HSP_FN float prolong_pixel(const float *c, long long cs, int Wc, int Hc, int x, int y)
{
    const int k = x >> 1, k1 = k + 1 < Wc - 1 ? k + 1 : Wc - 1, r = y >> 1, r1 = r + 1 < Hc - 1 ? r + 1 : Hc - 1;
    const float *row0 = (const float *)((const uint8_t *)c + (long long)r * cs), *row1 = (const float *)((const uint8_t *)c + (long long)r1 * cs);
    return prolong_value(row0[k], row0[k1], row1[k], row1[k1], x, y);
}

// A whole plane in host memory: the fine plane is W x H, the coarse one ceil(W/2) x ceil(H/2).  Strides in bytes.
inline void prolong_rows(const float *c, size_t cs, int W, int H, float *dst, size_t ds)
{
    const int Wc = half_up(W), Hc = half_up(H);
    for (int y = 0; y < H; y++) {
        float *row = (float *)((uint8_t *)dst + (size_t)y * ds);
        for (int x = 0; x < W; x++) row[x] = prolong_pixel(c, (long long)cs, Wc, Hc, x, y);
    }
}

// ---- the plan ------------------------------------------------------------------------------------------------------------

// The level sizes of a W x H context.  levels 0: as many as keep min(W_l, H_l) >= min_size, at most kMaxLevels, level 0
// always; else `levels` as given.  Returns the number of levels, or 0 where an explicit level would be coarser than 1 x 1
// (a level of 1 x 1 can be halved no further).
inline int plan(int W, int H, int levels, int min_size, int *widths, int *heights)
{
    int n = 1;
    widths[0] = W; heights[0] = H;
    const int want = levels > 0 ? levels : kMaxLevels;
    while (n < want) {
        const int w = widths[n - 1], h = heights[n - 1];
        const int wn = half_up(w), hn = half_up(h);
        if (levels > 0) {
            if (w == 1 && h == 1) return 0;
        } else if ((wn < hn ? wn : hn) < min_size) break;
        widths[n] = wn; heights[n] = hn;
        n++;
    }
    return n;
}

} // namespace hspyr
