// hs_interp_rule.h -- the frame at time t between the two frames of a pair (Baker et al., "A Database and Evaluation
// Methodology for Optical Flow", section 3.3.2), ONE definition for the device kernels (hs_kernels_interp.hip.h) and the
// host twin (hsflow_interp_host / hsflow_project_flow_host), the way hs_warp_rule.h serves both sides of the warp.
// All arithmetic is fp32 and every operation is rounded on its own (the library is built with -ffp-contract=off); the
// integer parts are exact, so host and device give the same bits.  The forward flow (u, v) of the pair (A, B) = (prev,
// curr), pictures of C interleaved u8 channels, a time 0 <= t <= 1:
//   P  projection.  The source pixel p = (x, y) with a = u[p], b = v[p]:
//        unknown  iff !hscolor::known(a, b): it contributes nothing
//        cost     hswarp::locate(a, b, x, y, 1, W, H, CONSTANT) not inside: 1023; else the sum over the channels of
//                 |prev_c[p] - hswarp::blend(the four taps of curr)_c| (0 .. 765): the photo-consistency of the vector
//        target   hx = fl(fl((float)x + fl(a * t)) + 0.5f), hy alike; left iff !(hx >= 0 && hx < (float)W && hy >= 0 &&
//                 hy < (float)H), tested on the floats; else q = ((int)floorf(hx), (int)floorf(hy))
//        key      (uint64)cost << 32 | (uint32)(y * W + x); the cell q keeps the MINIMUM key of all that land on it: the
//                 lowest cost wins, at equal cost the lower source index, whatever the order of arrival
//      A cell with a key gets the bits of (u, v) of that key's source and state 1; an empty cell is a hole: +0.0, +0.0,
//      state 0.  holes: the empty cells; collisions: sources landed - cells hit.
//   F  fill.  `passes` passes of hs_median_rule.h in FILL mode over (ut, vt, state); unfilled: the state-0 cells left.
//   B  blend.  The output pixel (x, y) with the filled vector (a, b), wA = fl(1 - t), wB = t:
//        tA = hswarp::locate(a, b, x, y, -t, W, H, REPLICATE), tB = locate(a, b, x, y, wA, W, H, REPLICATE); inA / inB:
//        the class is inside
//        fa       per channel the bilinear value of prev at tA in the warp's order, UNROUNDED: top = fl(p00 + fl(ax *
//                 fl(p10 - p00))), bot alike, fa = fl(top + fl(ay * fl(bot - top))); fb alike from curr at tB
//        nearest  tap of a side: (ax >= 0.5f ? x1 : x0, ay >= 0.5f ? y1 : y0)
//        class    inA && inB: occA iff vis_prev is given and its byte at tA's nearest tap is 0, occB alike with vis_curr at
//                 tB; occA && !occB: PREV_ONLY, occB && !occA: CURR_ONLY, else BLENDED.  Only inA: PREV_ONLY.  Only inB:
//                 CURR_ONLY.  Neither: CLAMPED, the blend of the two clamped samples.
//        byte     BLENDED / CLAMPED: m = fl(fl(wA * fa) + fl(wB * fb)); PREV_ONLY: m = fa; CURR_ONLY: m = fb;
//                 byte = min((int)fl(m + 0.5f), 255)
// t = 0 gives prev and t = 1 gives curr byte for byte where no vis plane is given (ax = ay = 0 on that side, the other
// side's weight is 0 or it is not asked).  The statistics are exact integers: their order of accumulation does not matter.
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
#define HSI_FN __host__ __device__ inline
#else
#define HSI_FN inline
#endif
#if defined(__clang__)
#define HSI_UNROLL _Pragma("unroll")
#else
#define HSI_UNROLL
#endif

namespace hsinterp {

constexpr int kBlended = 0, kPrevOnly = 1, kCurrOnly = 2, kClamped = 3; // HSFLOW_INTERP_*
constexpr int kLanded = 0, kLeft = 1, kUnknown = 2;
constexpr uint32_t kCostOutside = 1023u;
constexpr uint64_t kEmpty = ~(uint64_t)0; // a cell no source has landed on (no key is all-ones: a cost is at most 1023)
constexpr int kBatchMax = 8;              // HSFLOW_INTERP_BATCH_MAX

// ---- P ---------------------------------------------------------------------------------------------------------------------

// What one source pixel does: cls kLanded / kLeft / kUnknown; landed: its cell (qx, qy) and its key.
struct Splat {
    int cls, qx, qy;
    uint64_t key;
};

// Where the source (x, y) is at time t, without its cost (key stays kEmpty).
HSI_FN Splat target(float a, float b, int x, int y, float t, int W, int H)
{
    Splat s;
    s.cls = kUnknown;
    s.qx = s.qy = 0;
    s.key = kEmpty;
    if (!hscolor::known(a, b)) return s;
    const float da = a * t, db = b * t;
    const float tx = (float)x + da, ty = (float)y + db;
    const float hx = tx + 0.5f, hy = ty + 0.5f;
    s.cls = kLeft;
    if (!(hx >= 0.0f && hx < (float)W && hy >= 0.0f && hy < (float)H)) return s;
    // 0 <= hx < fl(W): floorf(hx) is a whole number below W (the float below fl(W) is below W, too); the integers are
    // tested once more all the same -- the key plane is written at this address
    const int qx = (int)floorf(hx), qy = (int)floorf(hy);
    if ((unsigned)qx >= (unsigned)W || (unsigned)qy >= (unsigned)H) return s;
    s.cls = kLanded;
    s.qx = qx;
    s.qy = qy;
    return s;
}

template <int C>
HSI_FN Splat splat(float a, float b, int x, int y, float t, int W, int H, const uint8_t *prev, long long ps, const uint8_t *curr, long long cs)
{
    Splat s = target(a, b, x, y, t, W, H);
    if (s.cls != kLanded) return s;
    uint32_t cost = kCostOutside;
    const hswarp::Tap p = hswarp::locate(a, b, x, y, 1.0f, W, H, hswarp::kBorderConstant);
    if (p.cls == hswarp::kInside) {
        const uint32_t w = hswarp::pixel<C>(curr, cs, p, 0u);
        const uint8_t *own = prev + (long long)y * ps + (long long)C * x;
        cost = 0u;
        HSI_UNROLL
        for (int c = 0; c < C; c++) {
            const int m = (int)((w >> (8 * c)) & 255u), o = (int)own[c];
            cost += (uint32_t)(m > o ? m - o : o - m);
        }
    }
    s.key = ((uint64_t)cost << 32) | (uint32_t)(y * W + x);
    return s;
}

// What one lane of the resolve counts.  At the cell (x, y) the SOURCE (x, y) is classified as well (target()): one pass
// over the plane counts both sides, and collisions = landed - hit = holes - left - unknown.
struct ProjAcc {
    uint32_t holes, left, unknown;
};

// ---- B ---------------------------------------------------------------------------------------------------------------------

// One channel from its four taps, the warp's order of operations without the last rounding to a byte.
HSI_FN float sample(uint8_t p00, uint8_t p10, uint8_t p01, uint8_t p11, float ax, float ay)
{
    const float a0 = (float)p00, b0 = (float)p01;
    const float dt = (float)p10 - a0, db = (float)p11 - b0;
    const float st = ax * dt, sb = ax * db;
    const float top = a0 + st, bot = b0 + sb;
    const float dv = bot - top;
    const float sv = ay * dv;
    return top + sv;
}

HSI_FN bool occluded(const uint8_t *vis, long long stride, const hswarp::Tap &p)
{
    if (!vis) return false;
    const int nx = p.ax >= 0.5f ? p.x1 : p.x0, ny = p.ay >= 0.5f ? p.y1 : p.y0;
    return vis[(long long)ny * stride + nx] == 0u;
}

// The C channels of the output pixel (x, y) as c0 | c1 << 8 | c2 << 16 and its class, from the filled vector (a, b).
template <int C>
HSI_FN uint32_t pixel(float a, float b, int x, int y, float t, int W, int H, const uint8_t *prev, long long ps, const uint8_t *curr, long long cs,
                      const uint8_t *vis_prev, long long vps, const uint8_t *vis_curr, long long vcs, int *cls_out)
{
    const float wA = 1.0f - t, wB = t;
    const hswarp::Tap tA = hswarp::locate(a, b, x, y, -t, W, H, hswarp::kBorderReplicate);
    const hswarp::Tap tB = hswarp::locate(a, b, x, y, wA, W, H, hswarp::kBorderReplicate);
    const bool inA = tA.cls == hswarp::kInside, inB = tB.cls == hswarp::kInside;
    int cls = kClamped;
    if (inA && inB) {
        const bool occA = occluded(vis_prev, vps, tA), occB = occluded(vis_curr, vcs, tB);
        cls = occA && !occB ? kPrevOnly : occB && !occA ? kCurrOnly : kBlended;
    } else if (inA) {
        cls = kPrevOnly;
    } else if (inB) {
        cls = kCurrOnly;
    }
    *cls_out = cls;
    // (a vector that is not known never gets here from P and F; its taps are those of the pixel (0, 0), inside the picture)
    const uint8_t *a0 = prev + (long long)tA.y0 * ps, *a1 = prev + (long long)tA.y1 * ps;
    const uint8_t *b0 = curr + (long long)tB.y0 * cs, *b1 = curr + (long long)tB.y1 * cs;
    uint32_t out = 0u;
    HSI_UNROLL
    for (int c = 0; c < C; c++) {
        const float fa = sample(a0[C * tA.x0 + c], a0[C * tA.x1 + c], a1[C * tA.x0 + c], a1[C * tA.x1 + c], tA.ax, tA.ay);
        const float fb = sample(b0[C * tB.x0 + c], b0[C * tB.x1 + c], b1[C * tB.x0 + c], b1[C * tB.x1 + c], tB.ax, tB.ay);
        const float ma = wA * fa, mb = wB * fb;
        const float mix = ma + mb;
        const float m = cls == kPrevOnly ? fa : cls == kCurrOnly ? fb : mix;
        const float r = m + 0.5f;
        const int i = (int)r;
        out |= (uint32_t)(i < 255 ? i : 255) << (8 * c);
    }
    return out;
}

// What one lane, or the host loop, gathers of B.  32 bits hold a lane's share (hs_kernels_interp.hip.h).
struct Acc {
    uint32_t cls[4], sad, max_diff;
};

// One pixel's share: out, ref packed as pixel() packs; ref_valid: there is a reference picture.
template <int C>
HSI_FN void account(Acc &s, int cls, uint32_t out, uint32_t ref, bool ref_valid)
{
    s.cls[0] += cls == kBlended;
    s.cls[1] += cls == kPrevOnly;
    s.cls[2] += cls == kCurrOnly;
    s.cls[3] += cls == kClamped;
    if (!ref_valid) return;
    HSI_UNROLL
    for (int c = 0; c < C; c++) {
        const int r = (int)((ref >> (8 * c)) & 255u), w = (int)((out >> (8 * c)) & 255u);
        const uint32_t d = (uint32_t)(w > r ? w - r : r - w);
        s.sad += d;
        s.max_diff = d > s.max_diff ? d : s.max_diff;
    }
}

// ---- whole pictures in host memory ------------------------------------------------------------------------------------------

// The record of a whole call (the layout of hsflow_interp_stats).
struct Sums {
    uint64_t blended, prev_only, curr_only, clamped, sad;
    uint32_t holes, unfilled, collisions, left, unknown, max_diff;
};

// P.  u, v: rows us / vs BYTES apart.  keys: W * H words of scratch.  ut, vt, state: packed planes of W * H elements.
// Sets holes, collisions, left, unknown of sums (and unfilled = holes: no pass has run yet).
template <int C>
inline void project_rows(const float *u, size_t us, const float *v, size_t vs, int W, int H, float t, const uint8_t *prev, size_t ps, const uint8_t *curr,
                         size_t cs, uint64_t *keys, float *ut, float *vt, uint8_t *state, Sums *sums)
{
    const size_t px = (size_t)W * H;
    for (size_t k = 0; k < px; k++) keys[k] = kEmpty;
    uint64_t landed = 0, left = 0, unknown = 0, hit = 0;
    for (int y = 0; y < H; y++) {
        const float *ru = (const float *)((const uint8_t *)u + (size_t)y * us), *rv = (const float *)((const uint8_t *)v + (size_t)y * vs);
        for (int x = 0; x < W; x++) {
            const Splat s = splat<C>(ru[x], rv[x], x, y, t, W, H, prev, (long long)ps, curr, (long long)cs);
            landed += s.cls == kLanded;
            left += s.cls == kLeft;
            unknown += s.cls == kUnknown;
            if (s.cls != kLanded) continue;
            uint64_t &cell = keys[(size_t)s.qy * W + s.qx];
            cell = s.key < cell ? s.key : cell;
        }
    }
    for (size_t k = 0; k < px; k++) {
        uint32_t abits = 0u, bbits = 0u;
        const bool have = keys[k] != kEmpty;
        if (have) {
            const uint32_t src = (uint32_t)keys[k];
            const int sy = (int)(src / (uint32_t)W), sx = (int)(src - (uint32_t)sy * (uint32_t)W);
            memcpy(&abits, (const uint8_t *)u + (size_t)sy * us + 4 * (size_t)sx, 4);
            memcpy(&bbits, (const uint8_t *)v + (size_t)sy * vs + 4 * (size_t)sx, 4);
        }
        memcpy(ut + k, &abits, 4);
        memcpy(vt + k, &bbits, 4);
        state[k] = have ? 1u : 0u;
        hit += have;
    }
    sums->holes = sums->unfilled = (uint32_t)(px - hit);
    sums->collisions = (uint32_t)(landed - hit);
    sums->left = (uint32_t)left;
    sums->unknown = (uint32_t)unknown;
}

// B.  ut, vt: packed planes.  vis_prev, vis_curr, ref, dst, cls may each be null.  Writes C * W bytes of every row of dst,
// W bytes of every row of cls and nothing else.  Sets the class counts, sad and max_diff of sums.
template <int C>
inline void blend_rows(const float *ut, const float *vt, int W, int H, float t, const uint8_t *prev, size_t ps, const uint8_t *curr, size_t cs,
                       const uint8_t *vis_prev, size_t vps, const uint8_t *vis_curr, size_t vcs, const uint8_t *ref, size_t rs, uint8_t *dst, size_t ds,
                       uint8_t *cls, size_t cls_s, Sums *sums)
{
    uint64_t count[4] = {0, 0, 0, 0}, sad = 0;
    uint32_t max_diff = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int k = 0;
            const size_t p = (size_t)y * W + x;
            const uint32_t w = pixel<C>(ut[p], vt[p], x, y, t, W, H, prev, (long long)ps, curr, (long long)cs, vis_prev, (long long)vps, vis_curr,
                                        (long long)vcs, &k);
            if (dst)
                for (int c = 0; c < C; c++) dst[(size_t)y * ds + (size_t)C * x + c] = (uint8_t)(w >> (8 * c));
            if (cls) cls[(size_t)y * cls_s + x] = (uint8_t)k;
            Acc one = {{0, 0, 0, 0}, 0, 0};
            account<C>(one, k, w, ref ? hswarp::load_pixel<C>(ref + (size_t)y * rs + (size_t)C * x) : 0u, ref != nullptr);
            for (int j = 0; j < 4; j++) count[j] += one.cls[j];
            sad += one.sad;
            max_diff = one.max_diff > max_diff ? one.max_diff : max_diff;
        }
    sums->blended = count[0]; sums->prev_only = count[1]; sums->curr_only = count[2]; sums->clamped = count[3];
    sums->sad = sad;
    sums->max_diff = max_diff;
}

} // namespace hsinterp
