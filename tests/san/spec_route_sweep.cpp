// Stand-alone driver for spec_route (csrc/spec_route.h) under AddressSanitizer / UBSan (host code only, no HIP, no GPU):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I impdar_amd/csrc tests/san/spec_route_sweep.cpp -o sweep && ./sweep
// The sweep of tests/test_spec_route.py -- every n in 1 ... 2100 and the large lengths, each with the row counts of that test --
// through the probe, checked for what spectrum.hip relies on: the blocks of rows cover every row once and none is empty, the
// LDS fits a compute unit, a thread's bins fit its accumulators, and the buffer sizes hold what the kernels write.  Exit code
// 0 = every call returned and held that; the sanitizers abort on a finding.
#define SPEC_ROUTE_PROBE 1
#include "spec_route.h"
#include <cstdio>
#include <vector>

static int check(int n, long long rows)
{
    int ints[8];
    long long longs[8];
    if (impdar_spec_route_full_probe(n, rows, ints, longs) != 0) {
        fprintf(stderr, "no route for n %d rows %lld\n", n, rows);
        return 1;
    }
    const int kind = ints[0], M = ints[1], bins = ints[3], threads = ints[5];
    const long long wg = longs[0], per = longs[1], lds = longs[2];
    bool ok = wg >= 1 && per >= 1 && (wg - 1) * per < rows && wg * per >= rows && bins == n / 2 + 1 && M == n / 2;
    ok = ok && lds <= SPEC_LDS_MAX && longs[3] == wg * bins && longs[4] == rows * n && longs[6] == rows * bins;
    if (kind == SPEC_ROCFFT) ok = ok && longs[5] == 2 * rows * bins && lds == 0 && wg <= SPEC_POWER_BLOCKS;
    else ok = ok && n % 2 == 0 && (M + threads) / threads <= spec_row_acc(threads) && lds >= (long long)(spec_pad(M) + 1) * 16 + threads * 8 && (1 << ints[2]) >= M;
    if (!ok) fprintf(stderr, "route of n %d rows %lld breaks a rule\n", n, rows);
    return ok ? 0 : 1;
}

int main()
{
    const long long rows[] = {1, 2, 255, 256, 257, 4096, 10000, 16384};
    std::vector<int> lengths;
    for (int n = 1; n <= 2100; ++n) lengths.push_back(n);
    for (int n : {4096, 8192, 10000, 16384, 16386, 20000, 40000}) lengths.push_back(n);
    long calls = 0;
    for (int n : lengths)
        for (long long r : rows) {
            if (check(n, r)) return 1;
            ++calls;
        }
    int ints[8];
    long long longs[8];
    if (impdar_spec_route_full_probe(0, 4, ints, longs) == 0 || impdar_spec_route_full_probe(8, 0, ints, longs) == 0) return 1;      // refused
    printf("%ld routes hold\n", calls);
    return 0;
}
