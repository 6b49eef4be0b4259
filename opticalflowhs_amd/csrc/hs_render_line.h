// hs_render_line.h -- the line iterator of the flow picture in closed form, shared by the render kernel
// (hs_kernels_render.hip.h) and the host (hsflow_render_line_pixels, which the CPU tests compare with the stepping loop).
//
// The host drawing (csrc/host/pnm.hpp line(), OpenCV 2.1's LineIterator behind cvLine at OpticalFlowOpenCV.cpp:44 and
// HSOpticalFlowOpenCL.cpp:767) starts at the LEFT end point and takes major + 1 steps along the longer axis with the
// error term e = major - 2*minor: while e < 0 the step is diagonal (e += 2*major - 2*minor), else straight
// (e -= 2*minor).  Before the decision of step i the error is
//     e_i = major - 2*minor*(i + 1) + 2*major*d_i,
// d_i = diagonal steps taken so far = ceil((2*minor*i - major) / (2*major)) = floor((2*minor*i + major - 1) / (2*major)),
// and the pixel of step i is (x0 + i, y0 + sy*d_i), or (x0 + d_i, y0 + sy*i) on a steep line.  Both coordinates are
// monotonic in i, so the steps that fall inside the image are ONE interval [lo, hi]: a lane jumps to lo, works out d and e
// there and walks to hi -- the work per line is bounded by the image, not by the line's length.
// 64-bit intermediates: 2*minor*i reaches 2^42 for end points near 2^20.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HS_HD __host__ __device__
#else
#define HS_HD
#endif

namespace hsline {

struct Walk {
    long long count;      // steps inside the image (0: nothing to draw)
    int x, y;             // pixel of the first of them
    int sy, steep;        // direction of y; 1 if y is the major axis
    long long major, minor, err; // err: the error term before the decision of that first step
};

// diagonal steps taken before step i
HS_HD inline long long diag_steps(long long major, long long minor, long long i)
{
    return major > 0 ? (2 * minor * i + major - 1) / (2 * major) : 0;
}

// The in-image part of the line (xa, ya) -> (xb, yb) on a width x height image.
HS_HD inline Walk clip(int xa, int ya, int xb, int yb, int width, int height)
{
    Walk w;
    long long dx = (long long)xb - xa, dy = (long long)yb - ya;
    long long x0 = xa, y0 = ya;
    if (dx < 0) { x0 = xb; y0 = yb; dx = -dx; dy = -dy; }
    w.sy = dy < 0 ? -1 : 1;
    if (dy < 0) dy = -dy;
    w.steep = dy > dx ? 1 : 0;
    w.major = w.steep ? dy : dx;
    w.minor = w.steep ? dx : dy;
    // the major coordinate advances by one per step, the minor one by one per diagonal step
    const long long xmax = (long long)width - 1, ymax = (long long)height - 1;
    long long lo = 0, hi = w.major, dlo, dhi;
    if (!w.steep) {
        if (-x0 > lo) lo = -x0;
        if (xmax - x0 < hi) hi = xmax - x0;
        dlo = w.sy > 0 ? -y0 : y0 - ymax;
        dhi = w.sy > 0 ? ymax - y0 : y0;
    } else {
        const long long ilo = w.sy > 0 ? -y0 : y0 - ymax, ihi = w.sy > 0 ? ymax - y0 : y0;
        if (ilo > lo) lo = ilo;
        if (ihi < hi) hi = ihi;
        dlo = -x0;
        dhi = xmax - x0;
    }
    if (dlo < 0) dlo = 0;
    w.count = 0;
    w.x = w.y = 0;
    w.err = 0;
    if (dhi < dlo) return w; // (d_i >= 0 always)
    if (w.minor == 0) {
        if (dlo > 0) return w; // d_i = 0 for every i
    } else {
        // d_i >= dlo  <=>  2*minor*i + major - 1 >= 2*major*dlo;   d_i <= dhi  <=>  2*minor*i <= 2*major*dhi + major
        if (dlo > 0) {
            const long long need = 2 * w.major * dlo - w.major + 1; // > 0
            const long long i0 = (need + 2 * w.minor - 1) / (2 * w.minor);
            if (i0 > lo) lo = i0;
        }
        const long long i1 = (2 * w.major * dhi + w.major) / (2 * w.minor);
        if (i1 < hi) hi = i1;
    }
    if (lo > hi) return w;
    const long long d = diag_steps(w.major, w.minor, lo);
    w.err = w.major - 2 * w.minor * (lo + 1) + 2 * w.major * d;
    w.x = (int)(w.steep ? x0 + d : x0 + lo);
    w.y = (int)(w.steep ? y0 + w.sy * lo : y0 + w.sy * d);
    w.count = hi - lo + 1;
    return w;
}

// One step of the iterator (after the pixel w.x, w.y has been used).
HS_HD inline void advance(Walk &w)
{
    if (w.err < 0) { w.err += 2 * w.major - 2 * w.minor; w.x++; w.y += w.sy; }
    else {
        w.err -= 2 * w.minor;
        if (w.steep) w.y += w.sy; else w.x++;
    }
}

} // namespace hsline
