// verify_line.hpp -- the line an SDK sample prints after verifyResults() ("Passed!" / "Failed",
// SDKUtil/include/SDKApplication.hpp's contract; the reference's own verifyResults was a stub,
// HSOpticalFlowOpenCL.cpp:894), made from a report of hsflow_verify.  A free function of the report alone, so that it
// can be fed hand-made reports without a device.
#pragma once
#include <cstdio>
#include <string>

#include "../../../include/hsflow.h"

// width: of the frame, to turn first_failing into x and y (<= 0: the raster index only).
inline std::string verify_line(const hsflow_verify_report &r, int width = 0)
{
    char buf[512];
    std::string s = r.ok ? "Passed!" : "Failed";
    snprintf(buf, sizeof(buf),
             " pair %d: u differing %llu failing %llu, v differing %llu failing %llu, derivative words differing %llu, "
             "nonfinite %llu; sweeps %d, reference pass %d",
             (int)r.pair, (unsigned long long)r.u.differing, (unsigned long long)r.u.failing, (unsigned long long)r.v.differing,
             (unsigned long long)r.v.failing, (unsigned long long)r.deriv_differing, (unsigned long long)(r.u.nonfinite + r.v.nonfinite),
             (int)r.iterations_done, (int)r.iterations_ref);
    s += buf;
    if (r.ok) return s;
    const bool in_u = r.u.failing != 0, in_v = !in_u && r.v.failing != 0, in_d = !in_u && !in_v && r.deriv_differing != 0;
    if (!in_u && !in_v && !in_d) return s + "; the two passes stopped on different sweeps";
    const hsflow_plane_diff &d = in_u ? r.u : r.v;
    const long long idx = in_d ? (long long)r.deriv_first : (long long)d.first_failing;
    snprintf(buf, sizeof(buf), "; first in plane %s pair %d", in_u ? "u" : in_v ? "v" : "derivatives", (int)r.pair);
    s += buf;
    if (width > 0) snprintf(buf, sizeof(buf), " x %lld y %lld", idx % width, idx / width);
    else snprintf(buf, sizeof(buf), " index %lld", idx);
    s += buf;
    if (!in_d) {
        snprintf(buf, sizeof(buf), ", max_abs_diff %.9g max_ulp %u", (double)d.max_abs_diff, (unsigned)d.max_ulp);
        s += buf;
    }
    return s;
}
