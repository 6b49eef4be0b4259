// The witness rule of csrc/hs_stop_rule.h, alone (tests/test_stop_rule_host.py): reads the bits of one double per line
// (hex) from stdin and prints, per line, the bits of witness_threshold(epsilon) and one digit per launch length T = 1 ..
// argv[1]: 1 where witness_usable(epsilon, T).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hs_stop_rule.h"

int main(int argc, char **argv)
{
    const int tmax = argc > 1 ? atoi(argv[1]) : 0;
    if (tmax < 1 || tmax > 200) return 2;
    uint64_t bits;
    while (scanf("%" SCNx64, &bits) == 1) {
        double eps;
        memcpy(&eps, &bits, sizeof eps);
        const float thr = hsstop::witness_threshold(eps);
        uint32_t tb;
        memcpy(&tb, &thr, sizeof tb);
        printf("%08" PRIx32 " ", tb);
        for (int T = 1; T <= tmax; T++) putchar(hsstop::witness_usable(eps, T) ? '1' : '0');
        putchar('\n');
    }
    return 0;
}
