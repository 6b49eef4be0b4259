// hs_stop_rule.h -- the host's half of the ITER|EPS witness: which threshold the witness launches get, and whether a
// launch of T sweeps can use it at all.  Host only, no HIP: compiled into the library (hs_solve.hip.h, multi_gpu.cpp)
// and, alone, into the check of tests/test_stop_rule_host.py, the way hs_verify_rule.h and hs_pre_rule.h are.
//
// The stop rule itself is strict and decided in double: a solve stops after the first sweep k with (double)Eps_k <
// epsilon (first_eps_hit, hs_solve.hip.h).  A witness launch proves the opposite for all its sweeps, "Eps_k >= thr":
//   threshold  the smallest NORMAL float >= epsilon (FLT_MIN for epsilon <= 0, where no sweep can ever stop), so that
//              Eps_k >= thr implies Eps_k >= epsilon also for an epsilon between two floats.
//   scalable   the kernels keep the flow of sweep s of a launch at scale 4^(s+1) and compare it with thr * 4^(s+1), which
//              they form by adding (s + 1) << 24 to the bits of thr (hs_kernels_strip.hip.h: scalar integer work).  That is
//              the product exactly while it is a finite normal float: thr normal and exponent field + 2 T <= 254.  Beyond
//              that the sum first reads +inf and then carries into the sign bit, where every change would pass the test.
//   usable     a witness pass may run: epsilon is no NaN (nothing compares >= NaN, so nothing could be proven) and the
//              threshold is scalable over the longest launch of the pass.  Where it is not, the solve measures every sweep
//              (the exact pass), which needs no threshold.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace hsstop {

inline float witness_threshold(double epsilon)
{
    if (!(epsilon > (double)FLT_MIN)) return FLT_MIN; // zero, negative, NaN, denormal as a float
    if (epsilon > (double)FLT_MAX) return INFINITY;
    float thr = (float)epsilon; // (to nearest: may land below)
    if ((double)thr < epsilon) thr = nextafterf(thr, INFINITY);
    return thr;
}

inline bool witness_scalable(float thr, int T)
{
    uint32_t b;
    memcpy(&b, &thr, sizeof b);
    if (T < 1 || T > 127 || b < 0x00800000u || b >= 0x7f800000u) return false; // (sign bit set: b >= 0x80000000)
    return b + ((uint32_t)T << 24) < 0x7f800000u;
}

inline bool witness_usable(double epsilon, int T) { return epsilon == epsilon && witness_scalable(witness_threshold(epsilon), T); }

} // namespace hsstop
