// The atan polynomial of csrc/hs_color_rule.h against the C library's double atan, compiled with g++ alone
// (tests/test_color_host.py): over N evenly spaced fp32 t in [0, 1] and the K floats nearest 0 and nearest 1 prints
// max |p - atan t|; then theta of atan2_rule against atan2 on the axes and diagonals with every combination of signs.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../opticalflowhs_amd/csrc/hs_color_rule.h"

int main(int argc, char **argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 1l << 22, k = argc > 2 ? atol(argv[2]) : 4096;
    double worst = 0.0;
    auto probe = [&](float t) {
        const double e = fabs((double)hscolor::atan_unit(t) - atan((double)t));
        if (e > worst) worst = e;
    };
    for (long i = 0; i < n; i++) probe((float)((double)i / (double)(n - 1)));
    float lo = 0.0f, hi = 1.0f;
    for (long i = 0; i < k; i++) {
        probe(lo);
        probe(hi);
        lo = nextafterf(lo, 1.0f);
        hi = nextafterf(hi, 0.0f);
    }
    printf("%.9g\n", worst);
    double worst2 = 0.0;
    const float s[5] = {-1.0f, -0.0f, 0.0f, 1.0f, 3.5f};
    for (float y : s)
        for (float x : s) {
            const double e = fabs((double)hscolor::atan2_rule(y, x) - atan2((double)y, (double)x));
            if (e > worst2) worst2 = e;
            if (std::signbit(hscolor::atan2_rule(y, x)) != std::signbit(atan2((double)y, (double)x))) worst2 = 1.0;
        }
    printf("%.9g\n", worst2);
    return 0;
}
