// hs_median_rule.h -- the median filter and the hole filling of a dense flow field, ONE definition for the device kernel
// (hs_kernels_median.hip.h) and the host twin (hsflow_median_host), the way hs_fb_rule.h serves both sides of the check.
// Flow planes u, v (W x H fp32), an optional u8 state plane, radius r in {1, 2} (window 3x3 or 5x5), a mode and
// min_votes in 1 .. (2r+1)^2.  One pass at the pixel p = (x, y), a = u[p], b = v[p]:
//   known(p)  the colour picture's test, hscolor::known(a, b) (no NaN, no magnitude above 1e9)
//   s(p)      0 INVALID if !known(p) or the state byte is 0; 2 FILLED if the byte is 2; 1 KEPT for every other byte and
//             where there is no state plane (so the default mask of hsflow_fb, 255 = consistent, is a state plane)
//   voters    the pixels q of the window around p that lie inside the frame (the window is clipped, not replicated) and
//             have s(q) != 0; p itself votes if it is valid; n = their number
//   median    of a component: over the keys key(f) = bits(f) ^ (bits(f) >> 31 ? 0xffffffff : 0x80000000), an
//             order-preserving map with -0.0 < +0.0, the voter key of rank (n - 1) >> 1 in ascending order (the lower
//             median), mapped back to its bits; u and v on their own
//   FILTER    n >= min_votes: the two medians, s_out = s if s != 0, else 2; otherwise the input bits and s_out = s
//   FILL      s != 0: the input bits and s_out = s; s == 0 and n >= min_votes: the two medians and s_out = 2; otherwise
//             the input bits (NaNs bit for bit) and s_out = 0
// A selection on integers: every correct algorithm gives the same bits.  Voter keys are never 0x00000000 or 0xffffffff
// (the keys of two NaN patterns, and a voter is known), so both are free as sentinels.
// The selection keeps its result at a fixed position, so that nothing is indexed by a run-time rank: the k-th non-voter
// of the window scan (k = 0, 1, ...) is replaced by the low sentinel when k is even and by the high sentinel when k is
// odd.  Of N = (2r+1)^2 slots with m = N - n non-voters, ceil(m / 2) lie below all voters and floor(m / 2) above, so the
// element of rank (N - 1) / 2 of all N is the voter of rank (N - 1) / 2 - ceil(m / 2) = (n - 1) >> 1, for odd and even n
// (tests/test_median_host.py checks the identity and the network on the host).  mid_of<N> finds that element by a fixed
// sequence of min/max exchanges ("forgetful selection"): of any N / 2 + 2 elements neither the smallest nor the largest is
// the middle one of N, so both are dropped and the next element taken in, until three are left.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hs_color_rule.h"

#if defined(__HIPCC__)
#define HSMED_FN __host__ __device__ inline
#else
#define HSMED_FN inline
#endif
#if defined(__clang__)
#define HSMED_UNROLL _Pragma("unroll")
#else
#define HSMED_UNROLL
#endif

namespace hsmed {

constexpr int kFilter = 0, kFill = 1;          // HSFLOW_MEDIAN_FILTER, HSFLOW_MEDIAN_FILL
constexpr int kUnfilled = 0, kKept = 1, kFilledState = 2;
constexpr uint32_t kLow = 0x00000000u, kHigh = 0xffffffffu; // the two sentinels; kLow is also the "no voter here" key
constexpr int kMaxPasses = 64;

HSMED_FN uint32_t key_of(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
HSMED_FN uint32_t bits_of(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }

// The input state of a pixel from its flow and its state byte (255 where there is no plane).
HSMED_FN int state_of(float a, float b, unsigned byte) { return (!hscolor::known(a, b) || byte == 0u) ? kUnfilled : byte == 2u ? kFilledState : kKept; }

HSMED_FN void exchange(uint32_t &lo, uint32_t &hi)
{
    const uint32_t a = lo < hi ? lo : hi, b = lo < hi ? hi : lo;
    lo = a;
    hi = b;
}

// The element of rank (N - 1) / 2 of a[0 .. N), N = 9 or 25.  Every index is a constant once the loops are unrolled.
// (T is uint32_t; a test instantiates the same sequence of exchanges on 64 zero-one inputs at a time.)
template <int N, class T>
HSMED_FN T mid_of(const T (&a)[N])
{
    constexpr int S = N / 2 + 2;
    T w[S];
    HSMED_UNROLL
    for (int i = 0; i < S; i++) w[i] = a[i];
    HSMED_UNROLL
    for (int len = S; len >= 3; len--) {
        // the smallest of w[0 .. len) to w[0], the largest to w[len - 1]
        const int half = len / 2;
        HSMED_UNROLL
        for (int i = 0; i < half; i++) exchange(w[i], w[len - 1 - i]);
        const int low_end = (len & 1) ? half : half - 1; // (an odd length's middle element belongs to both halves)
        HSMED_UNROLL
        for (int i = 1; i <= low_end; i++) exchange(w[0], w[i]);
        HSMED_UNROLL
        for (int i = half; i < len - 1; i++) exchange(w[i], w[len - 1]);
        // both are dropped; the next element takes the smallest one's place, the largest one's goes with the length
        if (len > 3) w[0] = a[S + (S - len)];
    }
    return w[1];
}

// What the window scan gathers: the slots of both components with the non-voters replaced, and the number of voters.
template <int N>
struct Window {
    uint32_t ku[N], kv[N];
    int n;
};

// Slot j of the scan.  ku == kLow says "no voter here" (out of the frame or s == 0); kv is then kLow too.
template <int N>
HSMED_FN void take(Window<N> &w, int j, uint32_t ku, uint32_t kv)
{
    const bool voter = ku != kLow;
    const uint32_t fill = ((j - w.n) & 1) ? kHigh : kLow; // j - n non-voters came before this slot
    w.ku[j] = voter ? ku : fill;
    w.kv[j] = voter ? kv : fill;
    w.n += voter;
}

struct Out {
    uint32_t ubits, vbits;
    int s_out;
};

// The decision at a pixel from its own bits and state, the number of voters and the two medians' keys.
HSMED_FN Out decide(uint32_t abits, uint32_t bbits, int s, int n, uint32_t mu, uint32_t mv, int fill_mode, int min_votes)
{
    Out o;
    const bool take_median = n >= min_votes && (!fill_mode || s == kUnfilled);
    o.ubits = take_median ? bits_of(mu) : abits;
    o.vbits = take_median ? bits_of(mv) : bbits;
    o.s_out = take_median && s == kUnfilled ? kFilledState : s;
    return o;
}

// What one lane, or the host loop, counts.
struct Acc {
    uint32_t kept, filled, unfilled, newly_filled, changed;
};

HSMED_FN void account(Acc &c, const Out &o, uint32_t abits, uint32_t bbits, int s)
{
    c.kept += o.s_out == kKept;
    c.filled += o.s_out == kFilledState;
    c.unfilled += o.s_out == kUnfilled;
    c.newly_filled += s == kUnfilled && o.s_out == kFilledState;
    c.changed += o.ubits != abits || o.vbits != bbits;
}

struct Sums {
    uint64_t kept, filled, unfilled, newly_filled, changed;
};

// One pass over a whole field in host memory.  Strides in BYTES.  state, u_out / v_out (together), state_out and sums may
// each be null.  Writes W floats of every row of u_out and v_out, W bytes of every row of state_out and nothing else.
template <int R>
inline void median_rows_r(const float *u, size_t us, const float *v, size_t vs, const uint8_t *state, size_t ss, int W, int H, int fill_mode, int min_votes,
                          float *u_out, float *v_out, size_t os, uint8_t *state_out, size_t sos, Sums *sums)
{
    constexpr int N = (2 * R + 1) * (2 * R + 1);
    Sums total = {0, 0, 0, 0, 0};
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            Window<N> w;
            w.n = 0;
            int j = 0;
            for (int dy = -R; dy <= R; dy++)
                for (int dx = -R; dx <= R; dx++, j++) {
                    const int qx = x + dx, qy = y + dy;
                    uint32_t ku = kLow, kv = kLow;
                    if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                        const float a = *(const float *)((const uint8_t *)u + (size_t)qy * us + 4 * (size_t)qx);
                        const float b = *(const float *)((const uint8_t *)v + (size_t)qy * vs + 4 * (size_t)qx);
                        if (state_of(a, b, state ? state[(size_t)qy * ss + (size_t)qx] : 255u) != kUnfilled) {
                            ku = key_of(hscolor::float_bits(a));
                            kv = key_of(hscolor::float_bits(b));
                        }
                    }
                    take(w, j, ku, kv);
                }
            uint32_t abits, bbits;
            memcpy(&abits, (const uint8_t *)u + (size_t)y * us + 4 * (size_t)x, 4);
            memcpy(&bbits, (const uint8_t *)v + (size_t)y * vs + 4 * (size_t)x, 4);
            const int s = state_of(hscolor::bits_float(abits), hscolor::bits_float(bbits), state ? state[(size_t)y * ss + (size_t)x] : 255u);
            const Out o = decide(abits, bbits, s, w.n, mid_of(w.ku), mid_of(w.kv), fill_mode, min_votes);
            if (u_out) {
                memcpy((uint8_t *)u_out + (size_t)y * os + 4 * (size_t)x, &o.ubits, 4);
                memcpy((uint8_t *)v_out + (size_t)y * os + 4 * (size_t)x, &o.vbits, 4);
            }
            if (state_out) state_out[(size_t)y * sos + (size_t)x] = (uint8_t)o.s_out;
            Acc one = {0, 0, 0, 0, 0};
            account(one, o, abits, bbits, s);
            total.kept += one.kept; total.filled += one.filled; total.unfilled += one.unfilled;
            total.newly_filled += one.newly_filled; total.changed += one.changed;
        }
    }
    if (sums) *sums = total;
}

inline void median_rows(int radius, const float *u, size_t us, const float *v, size_t vs, const uint8_t *state, size_t ss, int W, int H, int fill_mode,
                        int min_votes, float *u_out, float *v_out, size_t os, uint8_t *state_out, size_t sos, Sums *sums)
{
    if (radius == 1) median_rows_r<1>(u, us, v, vs, state, ss, W, H, fill_mode, min_votes, u_out, v_out, os, state_out, sos, sums);
    else median_rows_r<2>(u, us, v, vs, state, ss, W, H, fill_mode, min_votes, u_out, v_out, os, state_out, sos, sums);
}

} // namespace hsmed
