// hs_verify_rule.h -- the comparison rule of hsflow_verify / hsflow_compare_*, ONE definition for the device kernel
// (hs_kernels_verify.hip.h) and its host twin (hsflow_compare_planes_host), the way hs_render_line.h serves both sides
// of the picture.  Bits in, a handful of per-element figures out; what is done with them (sums, maxima, a minimum) is
// the caller's business and independent of the order of execution.
//
// One pair of fp32 values, `a` (what the context holds) against `b` (the reference side):
//   differing  the 32 bits differ.  +0 and -0 differ; two NaNs with the same bits do not.
//   failing    differing and not exempt.  The one exemption is the project's standing one: the strip
//              kernels carry a scaled state inside a launch, so flow that would be denormal keeps bits that depend on
//              where launch boundaries fall -- results are bit for bit "except where both values lie below 1e-30".  A
//              differing pair is exempt iff both are finite and fabsf(a) < HSFLOW_VERIFY_TINY && fabsf(b) < HSFLOW_VERIFY_TINY.
//   nonfinite  a is NaN or Inf (whether or not it differs).
//   measured   differing and both finite: abs_diff = fabsf(a - b), and ulp = the distance between the two values on the
//              ordered integer line (i = bits; if (i < 0) i = INT32_MIN - i), as unsigned: a flip of the lowest mantissa
//              bit is 1 apart.
// +0 against -0 is the one differing pair that is 0 apart, in ulp and in abs_diff; it is differing, and exempt by the
// rule above, so it is not failing.
#pragma once

#include <stdint.h>
#include <string.h>

#ifndef HSFLOW_VERIFY_TINY
#define HSFLOW_VERIFY_TINY 1e-30f /* include/hsflow.h */
#endif

#if defined(__HIPCC__)
#define HSV_FN __host__ __device__ inline
#else
#define HSV_FN inline
#endif

namespace hsverify {

struct Elem {
    bool differing, failing, nonfinite, measured;
    float abs_diff; // measured only
    uint32_t ulp;   // measured only
};

HSV_FN float as_float(uint32_t bits)
{
    float f;
    memcpy(&f, &bits, sizeof f);
    return f;
}

HSV_FN uint32_t as_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

HSV_FN bool finite_bits(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// position on the ordered integer line, shifted by 2^31 so that it is unsigned: -x < -0 == +0 < +x
HSV_FN uint32_t ordered(uint32_t bits) { return (bits & 0x80000000u) ? 0x80000000u - (bits & 0x7fffffffu) : 0x80000000u + bits; }

HSV_FN Elem classify(uint32_t abits, uint32_t bbits)
{
    Elem e;
    e.nonfinite = !finite_bits(abits);
    e.differing = abits != bbits;
    e.failing = false;
    e.measured = false;
    e.abs_diff = 0.f;
    e.ulp = 0u;
    if (!e.differing) return e;
    const bool both_finite = !e.nonfinite && finite_bits(bbits);
    if (both_finite) {
        const float a = as_float(abits), b = as_float(bbits);
        const float fa = as_float(abits & 0x7fffffffu), fb = as_float(bbits & 0x7fffffffu);
        e.measured = true;
        e.abs_diff = as_float(as_bits(a - b) & 0x7fffffffu); // sign bit off: -0 - +0 is -0, and the maximum is taken on the bits
        const uint32_t oa = ordered(abits), ob = ordered(bbits);
        e.ulp = oa > ob ? oa - ob : ob - oa;
        e.failing = !(fa < HSFLOW_VERIFY_TINY && fb < HSFLOW_VERIFY_TINY);
    } else {
        e.failing = true;
    }
    return e;
}

} // namespace hsverify
