// hs_link_kernels.hip -- part of libhsflow.so: the kernels of hs_kernels_link.hip.h and their launches, a translation unit
// of its own so that its device code is a code object of its own.
#define HS_LINK_KERNELS
#include "hs_kernels_link.hip.h"

namespace hsk {

// The launches of one set of `steps` steps (at most kLnBatchMax), always the same eight in the same order: what they do
// depends on the planes, their grids on the sizes and the arguments alone.
hipError_t launch_link(hipStream_t stream, const LnPlanes &pl, int steps, dim3 vote)
{
    const unsigned n = (unsigned)steps;
    const unsigned cells = pl.cap_a * pl.cap_b, words = cells + 2u * pl.cap_a + 1u;
    const unsigned clear = (words + 255u) / 256u;
    const dim3 blocks((cells + 255u) / 256u, 1u, n);
    hipLaunchKernelGGL(k_ln_clear, dim3(clear < 4096u ? clear : 4096u, 1u, n), dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_ln_vote, vote, dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_ln_count, blocks, dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_ln_scan, dim3(1u, 1u, n), dim3(1024), 0, stream, pl);
    hipLaunchKernelGGL(k_ln_number, blocks, dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_ln_rows, dim3((pl.cap_a + 3u) / 4u, 1u, n), dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_ln_cols, dim3((pl.cap_b + 63u) / 64u, 1u, n), dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_ln_finish, dim3(1u, 1u, n), dim3(1024), 0, stream, pl);
    return hipGetLastError();
}

} // namespace hsk
