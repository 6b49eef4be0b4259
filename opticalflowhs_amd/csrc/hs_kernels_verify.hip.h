// hs_kernels_verify.hip.h -- k_plane_compare: two planes in, one hsflow_plane_diff record out (hs_verify_rule.h is the
// rule, shared with the host twin).  What a consumer on the device otherwise does through a download of both planes
// and a loop on the host.
//
// A bandwidth-bound reduction: the plane is cut into chunks of one row x 1024 columns, a grid sized from the CU count
// strides over them, a lane takes four neighbouring pixels -- with one 16-byte load per plane where both base
// pointers and both strides are 16-byte aligned (`vec`), else (and for the columns beyond the last multiple of four)
// with scalar loads.  Six accumulators per lane, reduced across the wavefront with shuffles, across the workgroup
// through LDS, then ONE set of global atomics per workgroup -- and none at all from a workgroup that saw nothing to
// report, which is every workgroup of a passing comparison.  Sums of counts, maxima and one minimum only: the record
// does not depend on the order of execution.
//
// The record in device memory (5 x 64 bit, cleared to zero before the launch; hs_verify.hip.h turns it into the
// hsflow_plane_diff of the header): differing, failing, nonfinite, the COMPLEMENT of the lowest failing raster index
// under atomicMax (so that zero means "none" and one memset clears the lot: the minimum of i is the maximum of ~i),
// then max_abs_diff's bit pattern (non-negative floats order like their bits) and max_ulp as two 32-bit words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_verify_rule.h"

namespace hsk {

constexpr int kCmpThreads = 256;
constexpr int kCmpChunk = kCmpThreads * 4; // columns per chunk
constexpr int kCmpRecWords = 5;            // 64-bit words per record

struct CmpAcc {
    unsigned differing = 0u, failing = 0u, nonfinite = 0u, max_abs = 0u, max_ulp = 0u, first = 0xFFFFFFFFu;
};

// WORDS: the planes hold opaque 32-bit words (packed derivatives): differing and the first differing index only.
template <bool WORDS>
__device__ __forceinline__ void cmp_one(CmpAcc &acc, uint32_t a, uint32_t b, unsigned idx)
{
    if (WORDS) {
        if (a != b) {
            acc.differing++;
            acc.failing++;
            acc.first = min(acc.first, idx);
        }
        return;
    }
    const hsverify::Elem e = hsverify::classify(a, b);
    acc.nonfinite += e.nonfinite ? 1u : 0u;
    if (!e.differing) return;
    acc.differing++;
    if (e.measured) {
        acc.max_abs = max(acc.max_abs, hsverify::as_bits(e.abs_diff));
        acc.max_ulp = max(acc.max_ulp, e.ulp);
    }
    if (e.failing) {
        acc.failing++;
        acc.first = min(acc.first, idx);
    }
}

// a, b: planes of W x H 32-bit elements, rows a_stride / b_stride BYTES apart (multiples of 4).  cbs = chunks per row,
// nchunks = H * cbs.  W * H <= 2^31 - 1 (raster indices are kept in 32 bits until the end).
template <bool WORDS>
__global__ __launch_bounds__(kCmpThreads) void k_plane_compare(const char *__restrict__ a, long long a_stride, const char *__restrict__ b,
                                                               long long b_stride, int W, int H, int cbs, unsigned nchunks, int vec,
                                                               unsigned long long *__restrict__ rec)
{
    CmpAcc acc;
    const int tid = threadIdx.x;
    for (unsigned ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int y = (int)(ch / (unsigned)cbs), x = (int)(ch % (unsigned)cbs) * kCmpChunk + tid * 4;
        if (x >= W) continue;
        const uint32_t *pa = (const uint32_t *)(a + (long long)y * a_stride) + x;
        const uint32_t *pb = (const uint32_t *)(b + (long long)y * b_stride) + x;
        const unsigned idx = (unsigned)y * (unsigned)W + (unsigned)x;
        if (vec && x + 4 <= W) {
            const uint4 va = *(const uint4 *)pa, vb = *(const uint4 *)pb;
            cmp_one<WORDS>(acc, va.x, vb.x, idx);
            cmp_one<WORDS>(acc, va.y, vb.y, idx + 1u);
            cmp_one<WORDS>(acc, va.z, vb.z, idx + 2u);
            cmp_one<WORDS>(acc, va.w, vb.w, idx + 3u);
        } else {
            const int n = min(4, W - x);
            for (int k = 0; k < n; k++) cmp_one<WORDS>(acc, pa[k], pb[k], idx + (unsigned)k);
        }
    }
    // across the wavefront (64 lanes) ...
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        acc.differing += __shfl_xor(acc.differing, m);
        acc.failing += __shfl_xor(acc.failing, m);
        acc.nonfinite += __shfl_xor(acc.nonfinite, m);
        acc.max_abs = max(acc.max_abs, __shfl_xor(acc.max_abs, m));
        acc.max_ulp = max(acc.max_ulp, __shfl_xor(acc.max_ulp, m));
        acc.first = min(acc.first, __shfl_xor(acc.first, m));
    }
    // ... across the workgroup ...
    __shared__ unsigned part[kCmpThreads / 64][6];
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        part[wave][0] = acc.differing; part[wave][1] = acc.failing; part[wave][2] = acc.nonfinite;
        part[wave][3] = acc.max_abs; part[wave][4] = acc.max_ulp; part[wave][5] = acc.first;
    }
    __syncthreads();
    if (tid != 0) return;
    unsigned long long differing = 0ull, failing = 0ull, nonfinite = 0ull;
    unsigned max_abs = 0u, max_ulp = 0u, first = 0xFFFFFFFFu;
    for (int w = 0; w < kCmpThreads / 64; w++) {
        differing += part[w][0]; failing += part[w][1]; nonfinite += part[w][2];
        max_abs = max(max_abs, part[w][3]); max_ulp = max(max_ulp, part[w][4]); first = min(first, part[w][5]);
    }
    // ... and one set of atomics per workgroup, only for what it has to report
    if (differing) atomicAdd(rec + 0, differing);
    if (failing) atomicAdd(rec + 1, failing);
    if (nonfinite) atomicAdd(rec + 2, nonfinite);
    if (first != 0xFFFFFFFFu) atomicMax(rec + 3, ~(unsigned long long)first);
    unsigned *tail = (unsigned *)(rec + 4);
    if (max_abs) atomicMax(tail + 0, max_abs);
    if (max_ulp) atomicMax(tail + 1, max_ulp);
}

} // namespace hsk
