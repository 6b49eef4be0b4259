// hs_pyramid_kernels.hip -- part of libhsflow.so: the kernels of the coarse-to-fine solve (hs_kernels_pyramid.hip.h) and
// their launches, a translation unit of its own so that its device code is a code object of its own.
#include "hs_kernels_pyramid.hip.h"

namespace hsk {

namespace {
dim3 row_grid(int W, long long rows) { return dim3((unsigned)((W + 1023) / 1024), (unsigned)(rows < 65535 ? rows : 65535)); }
} // namespace

hipError_t launch_pyr_down(hipStream_t stream, int pairs, const uint8_t *prev, const uint8_t *curr, long long splane, int Ps, int W, int H, uint8_t *prev_out,
                           uint8_t *curr_out, long long dplane, int Pd)
{
    const int Wd = hspyr::half_up(W), Hd = hspyr::half_up(H);
    const dim3 grid((unsigned)((Wd + kPyrTileX - 1) / kPyrTileX), (unsigned)((Hd + kPyrTileY - 1) / kPyrTileY), (unsigned)(2 * pairs));
    hipLaunchKernelGGL((k_pyr_down<kPyrTileX, kPyrTileY>), grid, dim3(256), 0, stream, prev, curr, splane, Ps, W, H, prev_out, curr_out, dplane, Pd);
    return hipGetLastError();
}

hipError_t launch_pyr_step(hipStream_t stream, int mode, int pairs, const float *bu, const float *bv, const float *iu, const float *iv, long long cplane, int Pc,
                           int Wc, int Hc, float *u0, float *v0, const uint8_t *curr, uint8_t *warped, long long plane, int P, int W, int H)
{
    const long long rows = (long long)pairs * H;
    const dim3 grid = row_grid(W, rows);
    if (mode == kPyrProlong)
        hipLaunchKernelGGL((k_pyr_step<kPyrProlong>), grid, dim3(256), 0, stream, bu, bv, iu, iv, cplane, Pc, Wc, Hc, u0, v0, curr, warped, plane, P, W, H, rows);
    else if (mode == kPyrSame)
        hipLaunchKernelGGL((k_pyr_step<kPyrSame>), grid, dim3(256), 0, stream, bu, bv, iu, iv, cplane, Pc, Wc, Hc, u0, v0, curr, warped, plane, P, W, H, rows);
    else
        hipLaunchKernelGGL((k_pyr_step<kPyrSameAdd>), grid, dim3(256), 0, stream, bu, bv, iu, iv, cplane, Pc, Wc, Hc, u0, v0, curr, warped, plane, P, W, H, rows);
    return hipGetLastError();
}

hipError_t launch_pyr_total(hipStream_t stream, int pairs, const float *u0, const float *v0, float *u, float *v, long long plane, int P, int W, int H)
{
    const long long rows = (long long)pairs * H;
    hipLaunchKernelGGL((k_pyr_total<256>), row_grid(W, rows), dim3(256), 0, stream, u0, v0, u, v, plane, P, W, H, rows);
    return hipGetLastError();
}

} // namespace hsk
