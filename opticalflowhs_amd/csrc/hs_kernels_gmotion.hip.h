// hs_kernels_gmotion.hip.h -- the global motion of a flow field (hs_gmotion_rule.h) fitted where the flow lies.  Five
// kernels; the field is blockIdx.z, field i reads its own planes from an argument block by value and owns record i of the
// scratch (GmScratch: the twelve sums, the model, the threshold, the flags, the histogram).
// k_gm_accum: grid (ceil(W / 1024), rows, fields), 256 lanes, a lane takes 4 consecutive pixels of a row -- one 16-byte
// load each of u and v where base and stride are multiples of 16 and the group lies inside the row (a context's planes
// always allow it), float by float otherwise -- classifies them and adds the row's share to twelve per-lane sums.  A
// workgroup takes at most kGmRowsPerLane rows (the host picks the grid with stats_rows), so a lane sees at most 32
// pixels: the count and the first-order sums stay in 32 bits (32 * 2^19 = 2^24 for the quantised flow, 32 * 2^14 for a
// coordinate), the second-order sums are 64 bits.  The wavefront reduces by shuffles on 64-bit values, the four wavefronts
// through LDS, and every non-zero sum gets ONE 64-bit atomicAdd per workgroup.  All are integers: the result does not depend
// on the order of execution.  No workgroup waits for another.
// k_gm_hist (AUTO only): the same walk; an LDS histogram of the bins of r2, flushed with one 32-bit atomic per non-empty bin.
// k_gm_solve: one lane per field.  Derives the threshold from the histogram and / or the model from the sums, and zeroes
// what it has read for the next pass, so there is no memset between passes; the last one writes the result record.
// k_gm_apply: the classes under the final model and threshold -- the mask, the residual planes, the class counts (32-bit
// per lane, one 64-bit atomicAdd per class and workgroup into the result record).
// k_gm_warp<C>: hs_kernels_warp.hip.h's kernel with the model's motion in place of the flow planes; no flow plane is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_gmotion_rule.h"

namespace hsk {

constexpr int kGmBatchMax = 32;    // fields per launch (the argument block by value)
constexpr int kGmRowsPerLane = 8;  // rows a workgroup takes at most (stats_rows)
static_assert(kGmRowsPerLane * 4 * hsgm::kMaxQ < (1LL << 31) && kGmRowsPerLane * 4 * hsgm::kMaxXi < (1LL << 31), "a lane's first-order sums fit 32 bits");

// What a field's kernels keep between launches, one per field of a batch.  Sums and histogram are zero between calls.
struct GmScratch {
    long long sums[12];
    float p[6];
    float thr;
    unsigned flags;
    unsigned hist[hsgm::kBins];
};

// The layout of hsflow_gmotion_result (include/hsflow.h) as the kernels write it.
struct GmResultWords {
    float p[6];
    float thr;
    unsigned flags;
    unsigned long long cls[4];
};
static_assert(sizeof(GmResultWords) == 64, "hsflow_gmotion_result is 64 bytes");

// The planes of a batch, handed to the kernels by value.
struct GmPlanes {
    const float *u[kGmBatchMax], *v[kGmBatchMax];
    const uint8_t *s[kGmBatchMax];            // or NULL: every pixel is trusted
    uint8_t *mask[kGmBatchMax];               // or NULL
    float *ru[kGmBatchMax], *rv[kGmBatchMax]; // or NULL (both)
    long long fs, ss, ms, rs;                 // strides in BYTES: flow, state, mask, residual planes
    int W, H;
    unsigned wide_in, wide_state, wide_mask, wide_res; // bit i: field i's planes allow 16-byte (flow, residual) / 4-byte (bytes) moves
    unsigned value;                           // value[class] of the mask, class 0 in the low byte
};
static_assert(sizeof(GmPlanes) + 64 <= 2048, "the argument block stays well inside the 4 KiB of kernel arguments");

constexpr int kGmSolveModel = 1, kGmSolveThreshold = 2, kGmSolveResult = 4; // k_gm_solve's `what`

#if defined(HS_GMOTION_KERNELS) // the kernels themselves: hs_gmotion_kernels.hip alone defines it (they are no templates)

__device__ __forceinline__ long long gm_wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned gm_wave_sum32(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned gm_wave_max32(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Four pixels of row y from column x0: flow and state byte (1 where there is no state plane); columns beyond W: NaN flow.
__device__ __forceinline__ void gm_load(const GmPlanes &pl, unsigned i, int x0, int y, float a[4], float b[4], unsigned tr[4])
{
    const int W = pl.W;
    const bool whole = x0 + 4 <= W;
    const float *ru = (const float *)((const uint8_t *)pl.u[i] + (long long)y * pl.fs) + x0;
    const float *rv = (const float *)((const uint8_t *)pl.v[i] + (long long)y * pl.fs) + x0;
    if (((pl.wide_in >> i) & 1u) && whole) {
        const float4 fa = *(const float4 *)ru, fb = *(const float4 *)rv;
        a[0] = fa.x; a[1] = fa.y; a[2] = fa.z; a[3] = fa.w;
        b[0] = fb.x; b[1] = fb.y; b[2] = fb.z; b[3] = fb.w;
    } else {
        const float nan = hscolor::bits_float(hsgm::kNanBits);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            a[j] = x0 + j < W ? ru[j] : nan;
            b[j] = x0 + j < W ? rv[j] : nan;
        }
    }
    const uint8_t *s = pl.s[i];
    if (!s) {
        tr[0] = tr[1] = tr[2] = tr[3] = 1u;
    } else if (((pl.wide_state >> i) & 1u) && whole) {
        const uint32_t w = *(const uint32_t *)(s + (long long)y * pl.ss + x0);
        tr[0] = w & 255u; tr[1] = (w >> 8) & 255u; tr[2] = (w >> 16) & 255u; tr[3] = w >> 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) tr[j] = x0 + j < W ? s[(long long)y * pl.ss + x0 + j] : 0u;
    }
}

// Grid: (ceil(W / 1024), rows, fields); 256 lanes; every lane stays to the end: the wavefront reduces together.
// first: pass 0, every usable pixel takes part; else the inliers under the scratch's model and threshold.
__global__ __launch_bounds__(256) void k_gm_accum(const GmPlanes pl, GmScratch *__restrict__ scr, int first)
{
    const unsigned i = blockIdx.z;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int W = pl.W, H = pl.H;
    int n = 0, sx = 0, sy = 0, su = 0, sv = 0;
    long long sxx = 0, sxy = 0, syy = 0, sux = 0, suy = 0, svx = 0, svy = 0;
    if (x0 < W) {
        hsgm::Model m;
#pragma unroll
        for (int k = 0; k < 6; k++) m.p[k] = scr[i].p[k];
        const float thr = scr[i].thr;
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            float a[4], b[4];
            unsigned tr[4];
            gm_load(pl, i, x0, y, a, b, tr);
            const int Yi = 2 * y - (H - 1);
            int c = 0, cx = 0, cxx = 0, qu = 0, qv = 0;
            long long qux = 0, qvx = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                bool in = x0 + j < W && hsgm::usable_class(a[j], b[j], tr[j]) < 0;
                const int Xi = 2 * (x0 + j) - (W - 1);
                if (!first) {
                    float mu, mv, du, dv;
                    hsgm::eval(m, Xi, Yi, &mu, &mv);
                    in = in && hsgm::residual2(a[j], b[j], mu, mv, &du, &dv) <= thr;
                }
                if (in) {
                    const int u = hsgm::quant(a[j]), v = hsgm::quant(b[j]);
                    c += 1; cx += Xi; cxx += Xi * Xi; // (4 * 2^28 = 2^30: inside int)
                    qu += u; qv += v;
                    qux += (long long)u * Xi; qvx += (long long)v * Xi;
                }
            }
            n += c; sx += cx; sy += c * Yi; su += qu; sv += qv;
            sxx += cxx; sxy += (long long)cx * Yi; syy += (long long)c * Yi * Yi;
            sux += qux; suy += (long long)qu * Yi; svx += qvx; svy += (long long)qv * Yi;
        }
    }
    const long long part[12] = {gm_wave_sum(n),  gm_wave_sum(sx),  gm_wave_sum(sy),  gm_wave_sum(sxx), gm_wave_sum(sxy), gm_wave_sum(syy),
                                gm_wave_sum(su), gm_wave_sum(sux), gm_wave_sum(suy), gm_wave_sum(sv),  gm_wave_sum(svx), gm_wave_sum(svy)};
    __shared__ long long lds[4][12];
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (int k = 0; k < 12; k++) lds[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x < 12u) {
        const unsigned k = threadIdx.x;
        const long long sum = lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k];
        if (sum) atomicAdd((unsigned long long *)&scr[i].sums[k], (unsigned long long)sum); // (two's complement: the sum of the shares)
    }
}

// Grid as k_gm_accum.  The histogram of r2 under the scratch's model over the usable pixels.
__global__ __launch_bounds__(256) void k_gm_hist(const GmPlanes pl, GmScratch *__restrict__ scr)
{
    __shared__ unsigned bins[hsgm::kBins];
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned i = blockIdx.z;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int W = pl.W, H = pl.H;
    if (x0 < W) {
        hsgm::Model m;
#pragma unroll
        for (int k = 0; k < 6; k++) m.p[k] = scr[i].p[k];
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            float a[4], b[4];
            unsigned tr[4];
            gm_load(pl, i, x0, y, a, b, tr);
            const int Yi = 2 * y - (H - 1);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (x0 + j >= W || hsgm::usable_class(a[j], b[j], tr[j]) >= 0) continue;
                float mu, mv, du, dv;
                hsgm::eval(m, 2 * (x0 + j) - (W - 1), Yi, &mu, &mv);
                atomicAdd(&bins[hsgm::bin_of(hsgm::residual2(a[j], b[j], mu, mv, &du, &dv))], 1u);
            }
        }
    }
    __syncthreads();
    const unsigned cnt = bins[threadIdx.x];
    if (cnt) atomicAdd(&scr[i].hist[threadIdx.x], cnt);
}
static_assert(hsgm::kBins == 256, "k_gm_hist: one lane per bin");

// Grid: ceil(n / 64); 64 lanes, one per field.  what: kGmSolve*.  results: n records, or NULL.
__global__ __launch_bounds__(64) void k_gm_solve(GmScratch *__restrict__ scr, int n, int what, int kind, int mode, float fixed_thr, float scale2,
                                                 float min_thr2, GmResultWords *__restrict__ results)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    GmScratch &s = scr[i];
    if (what & kGmSolveThreshold) {
        if (mode == hsgm::kAuto) {
            s.thr = hsgm::auto_threshold(s.hist, scale2, min_thr2);
            for (int k = 0; k < hsgm::kBins; k++) s.hist[k] = 0u;
        } else {
            s.thr = fixed_thr;
        }
    }
    if (what & kGmSolveModel) {
        const hsgm::Sums sums = {s.sums[0], s.sums[1], s.sums[2], s.sums[3], s.sums[4], s.sums[5], s.sums[6], s.sums[7], s.sums[8], s.sums[9], s.sums[10], s.sums[11]};
        hsgm::Model m;
        s.flags = hsgm::solve(sums, kind, &m);
#pragma unroll
        for (int k = 0; k < 6; k++) s.p[k] = m.p[k];
#pragma unroll
        for (int k = 0; k < 12; k++) s.sums[k] = 0;
    }
    if ((what & kGmSolveResult) && results) {
        GmResultWords &r = results[i];
#pragma unroll
        for (int k = 0; k < 6; k++) r.p[k] = s.p[k];
        r.thr = s.thr;
        r.flags = s.flags;
#pragma unroll
        for (int k = 0; k < 4; k++) r.cls[k] = 0ull;
    }
}

// Grid as k_gm_accum.  results: the batch's records (the class counts are added to them), or NULL.
__global__ __launch_bounds__(256) void k_gm_apply(const GmPlanes pl, const GmScratch *__restrict__ scr, GmResultWords *__restrict__ results)
{
    const unsigned i = blockIdx.z;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int W = pl.W, H = pl.H;
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    if (x0 < W) {
        hsgm::Model m;
#pragma unroll
        for (int k = 0; k < 6; k++) m.p[k] = scr[i].p[k];
        const float thr = scr[i].thr;
        const bool whole = x0 + 4 <= W;
        uint8_t *mask = pl.mask[i];
        float *resu = pl.ru[i], *resv = pl.rv[i];
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            float a[4], b[4];
            unsigned tr[4], ub[4], vb[4], mb[4];
            gm_load(pl, i, x0, y, a, b, tr);
            const int Yi = 2 * y - (H - 1);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int c = hsgm::usable_class(a[j], b[j], tr[j]);
                float mu, mv, du, dv;
                hsgm::eval(m, 2 * (x0 + j) - (W - 1), Yi, &mu, &mv);
                const float r2 = hsgm::residual2(a[j], b[j], mu, mv, &du, &dv);
                if (c < 0) c = r2 <= thr ? hsgm::kInlier : hsgm::kOutlier;
                ub[j] = hsgm::residual_bits(du, c);
                vb[j] = hsgm::residual_bits(dv, c);
                mb[j] = (pl.value >> (8 * c)) & 255u;
                if (x0 + j < W) cnt[c] += 1u;
            }
            if (mask) {
                uint8_t *d = mask + (long long)y * pl.ms + x0;
                if (((pl.wide_mask >> i) & 1u) && whole) {
                    *(uint32_t *)d = mb[0] | (mb[1] << 8) | (mb[2] << 16) | (mb[3] << 24);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (x0 + j < W) d[j] = (uint8_t)mb[j];
                }
            }
            if (resu) {
                uint32_t *du = (uint32_t *)((uint8_t *)resu + (long long)y * pl.rs) + x0, *dv = (uint32_t *)((uint8_t *)resv + (long long)y * pl.rs) + x0;
                if (((pl.wide_res >> i) & 1u) && whole) {
                    *(uint4 *)du = make_uint4(ub[0], ub[1], ub[2], ub[3]);
                    *(uint4 *)dv = make_uint4(vb[0], vb[1], vb[2], vb[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (x0 + j < W) {
                            du[j] = ub[j];
                            dv[j] = vb[j];
                        }
                }
            }
        }
    }
    if (!results) return;
    const unsigned part[4] = {gm_wave_sum32(cnt[0]), gm_wave_sum32(cnt[1]), gm_wave_sum32(cnt[2]), gm_wave_sum32(cnt[3])};
    __shared__ unsigned lds[4][4];
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (int k = 0; k < 4; k++) lds[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x < 4u) {
        const unsigned k = threadIdx.x;
        const unsigned long long sum = (unsigned long long)lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k];
        if (sum) atomicAdd(&results[i].cls[k], sum);
    }
}

// Grid: (ceil(W / 1024), rows); 256 lanes.  k_warp_batch for one picture with the model's motion as the flow.
template <int C, bool STATS>
__global__ __launch_bounds__(256) void k_gm_warp(const hsgm::Model m, const uint8_t *__restrict__ src, const uint8_t *__restrict__ ref, uint8_t *__restrict__ dst,
                                                 int wide_dst, long long src_stride, long long ref_stride, long long dst_stride, int W, int H, float t, int border,
                                                 unsigned fill, unsigned long long *__restrict__ stats /* hsflow_warp_stats: five sums, two 32-bit maxima */)
{
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    hswarp::Acc acc = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (x0 < W) {
        const bool wide = wide_dst && x0 + 4 <= W;
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                w[j] = 0u;
                if (x0 + j < W) {
                    float mu, mv;
                    hsgm::eval(m, 2 * (x0 + j) - (W - 1), 2 * y - (H - 1), &mu, &mv);
                    const hswarp::Tap p = hswarp::locate(mu, mv, x0 + j, y, t, W, H, border);
                    w[j] = hswarp::pixel<C>(src, src_stride, p, fill);
                    if (STATS) {
                        const unsigned q = hswarp::load_pixel<C>(src + (long long)y * src_stride + (long long)C * (x0 + j));
                        const unsigned r = ref ? hswarp::load_pixel<C>(ref + (long long)y * ref_stride + (long long)C * (x0 + j)) : 0u;
                        hswarp::account<C>(acc, p.cls, w[j], q, r, ref != nullptr);
                    }
                }
            }
            if (!dst) continue;
            uint8_t *d = dst + (long long)y * dst_stride + (long long)C * x0;
            if (wide) {
                uint32_t *dw = (uint32_t *)d;
                if (C == 1) {
                    dw[0] = w[0] | (w[1] << 8) | (w[2] << 16) | (w[3] << 24);
                } else {
                    dw[0] = w[0] | (w[1] << 24);
                    dw[1] = (w[1] >> 8) | (w[2] << 16);
                    dw[2] = (w[2] >> 16) | (w[3] << 8);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (x0 + j < W)
#pragma unroll
                        for (int c = 0; c < C; c++) d[C * j + c] = (uint8_t)(w[j] >> (8 * c));
            }
        }
    }
    if (!STATS) return;
    unsigned part[7] = {gm_wave_sum32(acc.inside),    gm_wave_sum32(acc.outside),    gm_wave_sum32(acc.unknown), gm_wave_sum32(acc.sad_warped),
                        gm_wave_sum32(acc.sad_plain), gm_wave_max32(acc.max_warped), gm_wave_max32(acc.max_plain)};
    __shared__ unsigned lds[4][7];
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (int k = 0; k < 7; k++) lds[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x < 7u) {
        const unsigned k = threadIdx.x;
        unsigned long long *sums = stats;
        if (k < 5u) {
            const unsigned long long sum = (unsigned long long)lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k];
            if (sum) atomicAdd(sums + k, sum);
        } else {
            unsigned mx = lds[0][k];
            for (int wv = 1; wv < 4; wv++) mx = lds[wv][k] > mx ? lds[wv][k] : mx;
            unsigned *word = (unsigned *)(sums + 5) + (k - 5u);
            if (mx > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, mx);
        }
    }
}

#endif // HS_GMOTION_KERNELS

// hs_gmotion_kernels.hip: the kernels and their launches.
hipError_t launch_gm_accum(const dim3 &grid, hipStream_t stream, const GmPlanes &pl, GmScratch *scr, int first);
hipError_t launch_gm_hist(const dim3 &grid, hipStream_t stream, const GmPlanes &pl, GmScratch *scr);
hipError_t launch_gm_solve(hipStream_t stream, GmScratch *scr, int n, int what, int kind, int mode, float fixed_thr, float scale2, float min_thr2,
                           GmResultWords *results);
hipError_t launch_gm_apply(const dim3 &grid, hipStream_t stream, const GmPlanes &pl, const GmScratch *scr, GmResultWords *results);
hipError_t launch_gm_warp(const dim3 &grid, hipStream_t stream, int channels, const hsgm::Model &m, const uint8_t *src, const uint8_t *ref, uint8_t *dst,
                          int wide_dst, long long src_stride, long long ref_stride, long long dst_stride, int W, int H, float t, int border, unsigned fill,
                          unsigned long long *stats);

} // namespace hsk
