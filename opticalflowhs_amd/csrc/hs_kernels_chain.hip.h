// hs_kernels_chain.hip.h -- pixels and points followed through up to 32 flow planes (hs_chain_rule.h) in ONE launch: the
// trajectory stays in registers, no intermediate plane goes to memory.  An argument block by value carries, per plane,
// the u, v and state pointers; one stride in bytes serves all flow planes and one all state planes.
// k_chain_dense: grid (ceil(W / 1024), rows), 256 lanes, a lane takes 4 consecutive pixels of a row.  The start is one
// 16-byte load each of u and v where base and stride are multiples of 16 and the group lies inside the row (a context's
// planes always allow it: base at a 256-byte multiple, pitch a multiple of 64 floats), float by float otherwise.  The
// lane then walks its four pixels through the planes TOGETHER: per plane the four positions are located, the 4 x 8 flow
// taps (and 4 x 4 state taps) are gathered from global memory, and only then are the classes looked at -- a pixel that is
// no longer ALIVE gathers at tap (0, 0), which always lies inside the plane (locate() keeps every tap inside W x H).  Four
// independent dependent-gather chains per lane are the latency hiding, beside the occupancy.  A wavefront leaves the
// plane loop when none of its pixels is ALIVE any more (one ballot per plane).  U and V go out as one 16-byte store each
// where base and stride are multiples of 16 and the group lies inside the row, float by float otherwise and for the
// ragged end; status and age as one word each where multiples of 4, else bytes.  Nothing beyond W floats or W bytes of a
// row is written.
// k_chain_points: one lane per point, 256 lanes, grid ceil(m / 256), the same advance(); row j of the track is one
// 8-byte store per lane, consecutive lanes to consecutive addresses (two 4-byte stores where the base is no multiple of 8).
// With statistics (STATS) every lane counts in 32-bit registers.  A dense lane sees at most ceil(H / gridDim.y) <= 258 rows
// (pitch * H <= 2^30, pitch >= 64, gridDim.y = min(ceil(H / per), 65535)) of 4 pixels: a class counter stays below 2^11,
// and sum_age, at most 32 per pixel, below 258 * 4 * 32 < 2^16, its wave sum below 2^22.  A points lane sees one point.
// The four waves add up through LDS in 64 bits; every counter gets one 64-bit atomicAdd per workgroup (none for a zero
// sum), the maximum one 32-bit atomicMax and only where the word is smaller, into the call's hsflow_chain_stats, zero
// before.  All are integers: the result does not depend on the order of execution.  No workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_chain_rule.h"

namespace hsk {

// The planes of a chain, handed to the kernels by value.
struct ChainPlanes {
    const float *u[hschain::kMaxPairs], *v[hschain::kMaxPairs];
    const uint8_t *s[hschain::kMaxPairs]; // or NULL: no test for that plane
};

// Everything else a dense chain is told.
struct ChainDense {
    const float *U0, *V0;   // the start planes, or NULL: plane 0 is the start
    float *U, *V;           // or NULL
    uint8_t *status, *age;  // or NULL
    long long fs, ss, s0s, os, sts, as; // strides in BYTES: flow planes, state planes, start planes, U / V, status, age
    int n, W, H;
    unsigned value;         // value[class] of the status plane, class 0 in the low byte
    unsigned wide;          // kChainWide*
};
constexpr unsigned kChainWideStart = 1u, kChainWideOut = 2u, kChainWideStatus = 4u, kChainWideAge = 8u;

// Everything else a set of points is told.
struct ChainPoints {
    const float *xy;
    float *track, *last;   // or NULL
    uint8_t *status, *age; // or NULL
    long long fs, ss;
    int n, m, W, H;
    unsigned value;
    unsigned wide;         // bit 0: xy, bit 1: track, bit 2: last -- a multiple of 8
};
static_assert(sizeof(ChainPlanes) + sizeof(ChainDense) + 64 <= 2048 && sizeof(ChainPlanes) + sizeof(ChainPoints) + 64 <= 2048,
              "the argument blocks stay well inside the 4 KiB of kernel arguments");

// The layout of hsflow_chain_stats (include/hsflow.h) as the kernels write it.
struct ChainStatsWords {
    unsigned long long cls[4], sum_age;
    unsigned max_mag2_bits;
    unsigned reserved[5];
};
static_assert(sizeof(ChainStatsWords) == 64, "hsflow_chain_stats is 64 bytes");

__device__ __forceinline__ unsigned chain_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned chain_wave_max(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// A workgroup's share into the record: every lane of the four waves comes here.
__device__ __forceinline__ void chain_reduce(const hschain::Acc &acc, ChainStatsWords *stats)
{
    const unsigned long long part[6] = {chain_wave_sum(acc.cls[0]), chain_wave_sum(acc.cls[1]), chain_wave_sum(acc.cls[2]),
                                        chain_wave_sum(acc.cls[3]), chain_wave_sum(acc.sum_age), chain_wave_max(acc.max_bits)};
    __shared__ unsigned long long lds[4][6];
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (int k = 0; k < 6; k++) lds[threadIdx.x >> 6][k] = part[k];
    __syncthreads();
    if (threadIdx.x < 6u) {
        const unsigned k = threadIdx.x;
        unsigned long long *sums = (unsigned long long *)stats; // five sums, then the maximum
        if (k < 5u) {
            const unsigned long long sum = lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k];
            if (sum) atomicAdd(sums + k, sum);
        } else { // (a maximum only ever grows: the atomic is left out where the word already holds as much)
            unsigned m = (unsigned)lds[0][k];
            for (int wv = 1; wv < 4; wv++) m = (unsigned)lds[wv][k] > m ? (unsigned)lds[wv][k] : m;
            unsigned *word = (unsigned *)(sums + 5);
            if (m > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, m);
        }
    }
}

constexpr int kChainAbsent = 4; // a column beyond W: no class, nothing stored, nothing counted

// Grid: (ceil(W / 1024), rows); 256 lanes.  With STATS every lane stays to the end: the wavefront reduces together.
template <bool STATS>
__global__ __launch_bounds__(256) void k_chain_dense(const ChainPlanes pl, const ChainDense d, ChainStatsWords *__restrict__ stats)
{
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int W = d.W, H = d.H, n = d.n;
    hschain::Acc acc = {{0u, 0u, 0u, 0u}, 0u, 0u};
    if (x0 < W) {
        const bool given = d.U0 != nullptr;
        const uint8_t *su = (const uint8_t *)(given ? d.U0 : pl.u[0]), *sv = (const uint8_t *)(given ? d.V0 : pl.v[0]);
        const uint8_t *s0 = given ? nullptr : pl.s[0];
        const long long sstride = given ? d.s0s : d.fs;
        const bool whole = x0 + 4 <= W;
        const int first = given ? 0 : 1;
        const float nan = hscolor::bits_float(hschain::kNanBits);
        for (int y = blockIdx.y; y < H; y += gridDim.y) {
            float a[4], b[4];
            int cls[4];
            unsigned age[4];
            const float *ru = (const float *)(su + (long long)y * sstride) + x0, *rv = (const float *)(sv + (long long)y * sstride) + x0;
            if ((d.wide & kChainWideStart) && whole) {
                const float4 fa = *(const float4 *)ru, fb = *(const float4 *)rv;
                a[0] = fa.x; a[1] = fa.y; a[2] = fa.z; a[3] = fa.w;
                b[0] = fb.x; b[1] = fb.y; b[2] = fb.z; b[3] = fb.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    a[j] = x0 + j < W ? ru[j] : 0.0f;
                    b[j] = x0 + j < W ? rv[j] : 0.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                unsigned tr = 1u;
                if (s0 && x0 + j < W) tr = s0[(long long)y * d.ss + x0 + j];
                cls[j] = x0 + j < W ? hschain::start_class(a[j], b[j], tr) : kChainAbsent;
                age[j] = cls[j] == hschain::kAlive ? (unsigned)first : 0u;
            }
            for (int k = first; k < n; k++) {
                const int alive = (cls[0] == hschain::kAlive) | (cls[1] == hschain::kAlive) | (cls[2] == hschain::kAlive) | (cls[3] == hschain::kAlive);
                if (!__any(alive)) break;
                const hschain::Plane f = {pl.u[k], pl.v[k], pl.s[k], d.fs, d.ss};
                hswarp::Tap p[4];
                hschain::Taps t[4];
#pragma unroll
                for (int j = 0; j < 4; j++) p[j] = hswarp::locate(cls[j] == hschain::kAlive ? a[j] : nan, b[j], x0 + j, y, 1.0f, W, H, hswarp::kBorderConstant);
#pragma unroll
                for (int j = 0; j < 4; j++) t[j] = hschain::gather(p[j], f);
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (cls[j] == hschain::kAlive) {
                        cls[j] = hschain::settle(a[j], b[j], p[j], t[j]);
                        age[j] += cls[j] == hschain::kAlive;
                    }
            }
            unsigned ub[4], vb[4], sb[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool ok = cls[j] == hschain::kAlive;
                ub[j] = ok ? hscolor::float_bits(a[j]) : hschain::kNanBits;
                vb[j] = ok ? hscolor::float_bits(b[j]) : hschain::kNanBits;
                sb[j] = (d.value >> (8 * (cls[j] & 3))) & 255u;
                if (STATS && cls[j] != kChainAbsent) hschain::account(acc, cls[j], age[j], a[j], b[j]);
            }
            if (d.U) {
                uint32_t *du = (uint32_t *)((uint8_t *)d.U + (long long)y * d.os) + x0, *dv = (uint32_t *)((uint8_t *)d.V + (long long)y * d.os) + x0;
                if ((d.wide & kChainWideOut) && whole) {
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
            if (d.status) {
                uint8_t *ds = d.status + (long long)y * d.sts + x0;
                if ((d.wide & kChainWideStatus) && whole) {
                    *(uint32_t *)ds = sb[0] | (sb[1] << 8) | (sb[2] << 16) | (sb[3] << 24);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (x0 + j < W) ds[j] = (uint8_t)sb[j];
                }
            }
            if (d.age) {
                uint8_t *da = d.age + (long long)y * d.as + x0;
                if ((d.wide & kChainWideAge) && whole) {
                    *(uint32_t *)da = age[0] | (age[1] << 8) | (age[2] << 16) | (age[3] << 24);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (x0 + j < W) da[j] = (uint8_t)age[j];
                }
            }
        }
    }
    if (STATS) chain_reduce(acc, stats);
}

// Grid: ceil(m / 256); 256 lanes, one point each.
template <bool STATS>
__global__ __launch_bounds__(256) void k_chain_points(const ChainPlanes pl, const ChainPoints d, ChainStatsWords *__restrict__ stats)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    hschain::Acc acc = {{0u, 0u, 0u, 0u}, 0u, 0u};
    if (i < d.m) {
        const int n = d.n, W = d.W, H = d.H;
        float px, py;
        if (d.wide & 1u) {
            const float2 s = *(const float2 *)(d.xy + 2 * i);
            px = s.x; py = s.y;
        } else {
            px = d.xy[2 * i]; py = d.xy[2 * i + 1];
        }
        float a = px, b = py;
        int cls = hschain::start_class(a, b, 1u);
        unsigned age = 0u;
        uint32_t *row = d.track ? (uint32_t *)d.track + 2 * i : nullptr;
        const bool wide_track = (d.wide & 2u) != 0u;
        unsigned bx = hscolor::float_bits(px), by = hscolor::float_bits(py);
        for (int j = 0; j <= n; j++) {
            if (row) {
                if (wide_track) {
                    *(uint2 *)row = make_uint2(bx, by);
                } else {
                    row[0] = bx; row[1] = by;
                }
                row += 2 * (long long)d.m;
            }
            if (j == n) break;
            if (cls == hschain::kAlive) {
                const hschain::Plane f = {pl.u[j], pl.v[j], pl.s[j], d.fs, d.ss};
                cls = hschain::advance(a, b, 0, 0, W, H, f);
                age += cls == hschain::kAlive;
            }
            bx = cls == hschain::kAlive ? hscolor::float_bits(a) : hschain::kNanBits;
            by = cls == hschain::kAlive ? hscolor::float_bits(b) : hschain::kNanBits;
        }
        const bool ok = cls == hschain::kAlive;
        if (d.last) {
            uint32_t *l = (uint32_t *)d.last + 2 * i;
            const unsigned lx = ok ? hscolor::float_bits(a) : hschain::kNanBits, ly = ok ? hscolor::float_bits(b) : hschain::kNanBits;
            if (d.wide & 4u) {
                *(uint2 *)l = make_uint2(lx, ly);
            } else {
                l[0] = lx; l[1] = ly;
            }
        }
        if (d.status) d.status[i] = (uint8_t)((d.value >> (8 * cls)) & 255u);
        if (d.age) d.age[i] = (uint8_t)age;
        if (STATS) {
            const float dx = a - px, dy = b - py;
            hschain::account(acc, cls, age, dx, dy);
        }
    }
    if (STATS) chain_reduce(acc, stats);
}

// hs_chain_kernels.hip: the instantiations and their launch.
hipError_t launch_chain_dense(const dim3 &grid, hipStream_t stream, const ChainPlanes &pl, const ChainDense &d, ChainStatsWords *stats);
hipError_t launch_chain_points(const dim3 &grid, hipStream_t stream, const ChainPlanes &pl, const ChainPoints &d, ChainStatsWords *stats);

} // namespace hsk
