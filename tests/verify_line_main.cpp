// Hand-made hsflow_verify reports through verify_line (opticalflowhs_amd/csrc/host/verify_line.hpp), for
// tests/test_verify_host.py: no library, no device.  argv[1]: the frame width.
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "../opticalflowhs_amd/csrc/host/verify_line.hpp"

static hsflow_verify_report passing()
{
    hsflow_verify_report r;
    std::memset(&r, 0, sizeof(r));
    r.struct_size = sizeof(r);
    r.ok = 1;
    r.iterations_done = r.iterations_ref = 100;
    r.u.first_failing = r.v.first_failing = r.deriv_first = -1;
    return r;
}

int main(int argc, char **argv)
{
    const int W = argc > 1 ? atoi(argv[1]) : 600;
    hsflow_verify_report r = passing();
    std::cout << verify_line(r, W) << "\n";
    r = passing(); // one element of u, a flip of the lowest bit
    r.ok = 0;
    r.u.differing = r.u.failing = 1;
    r.u.first_failing = 123LL * W + 45;
    r.u.max_abs_diff = 5.9604645e-08f;
    r.u.max_ulp = 1;
    std::cout << verify_line(r, W) << "\n";
    r = passing(); // v only, pair 2
    r.ok = 0;
    r.pair = 2;
    r.v.differing = r.v.failing = 1;
    r.v.first_failing = 7LL * W + 599;
    r.v.max_abs_diff = 0.25f;
    r.v.max_ulp = 4194304;
    std::cout << verify_line(r, W) << "\n";
    r = passing(); // derivative words only
    r.ok = 0;
    r.deriv_differing = 3;
    r.deriv_first = 2LL * W + 1;
    std::cout << verify_line(r, W) << "\n";
    r = passing(); // the stopping sweeps differ
    r.ok = 0;
    r.iterations_done = 37;
    r.iterations_ref = 41;
    std::cout << verify_line(r, W) << "\n";
    return 0;
}
