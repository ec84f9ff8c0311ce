// Stand-alone driver for the cover of kirch_quad_kernel's quad-aligned window (csrc/kirch_route.h: kq_win_first_quad, kq_win_acc,
// kirch_walk_range, kirch_tile_origin / kirch_tile_count through impdar_kirch_quadwin_cover_probe) under AddressSanitizer /
// UBSan (host code only, no HIP, no GPU):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I impdar_amd/csrc tests/san/kirch_quadwin_fuzz.cpp -o fuzz && ./fuzz
// A few thousand random launches -- profile lengths from one trace, output blocks that start and end anywhere, the three tile
// widths with one to three tiles per workgroup, both ring depths, walks in one, two and four pieces, apertures of no pair at
// all (hmax 0) up to wider than the profile, both window kinds -- and for each what tests/test_kirch_quadwin.py asserts on its
// fixed cases: every (output, offset) pair whose input trace lies in the profile taken exactly once, no other pair twice, no
// read off a staged ring group, every component on the slot of its pair, every column written.  Exit code 0 = every call
// returned and held that; the sanitizers abort on a finding.
#define KIRCH_ROUTE_PROBE 1
#include "kirch_route.h"
#include <cstdio>
#include <random>

int main()
{
    std::mt19937 rng(20261020);
    auto pick = [&](std::initializer_list<int> v) { return *(v.begin() + rng() % v.size()); };
    long launches = 0, pairs = 0, refused = 0;
    for (int it = 0; it < 4000; ++it) {
        const int tnum = pick({1, 2, 7, 31, 64, 65, 128, 300, 341, 1000});
        const int xb = pick({24, 32, 40}), nh = pick({1, 1, 2, 3}), lk = (int)(rng() % 2);
        const int pl2 = nh == 1 ? pick({0, 0, 1, 2}) : 0;
        const int hmax = pick({0, 1, 3, 9, 38, 120, 438, 1200});
        const int window = (int)(rng() % 4 != 0);
        const int xlo = (int)(rng() % tnum), xhi = (rng() % 3 == 0) ? tnum : xlo + 1 + (int)(rng() % (tnum - xlo));
        const int nx = xhi - xlo, span = 2 * hmax + 1;
        std::vector<int> count((size_t)nx * span + 1, 0), written((size_t)nx + 1, 0);
        count.back() = written.back() = -7;
        long long stats[8];
        // (an argument the kernel has no instantiation for must be refused, not walked)
        if (it % 211 == 0) {
            if (impdar_kirch_quadwin_cover_probe(tnum, xlo, xhi, 28, nh, lk, hmax, pl2, window, count.data(), written.data(), stats) != -1 ||
                impdar_kirch_quadwin_cover_probe(tnum, xhi, xlo, xb, nh, lk, hmax, pl2, window, count.data(), written.data(), stats) != -1) {
                fprintf(stderr, "launch %d: bad arguments were taken\n", it);
                return 1;
            }
            ++refused;
        }
        if (impdar_kirch_quadwin_cover_probe(tnum, xlo, xhi, xb, nh, lk, hmax, pl2, window, count.data(), written.data(), stats) != 0) {
            fprintf(stderr, "launch %d refused\n", it);
            return 1;
        }
        ++launches;
        bool ok = count.back() == -7 && written.back() == -7 && stats[4] == 0 && stats[5] == 0 && (!window || stats[3] == 0) &&
                  stats[2] * 4 == stats[1] * (window ? xb : xb + 3);
        for (int x = xlo; x < xhi && ok; ++x) {
            ok = written[x - xlo] >= 1 && written[x - xlo] <= (1 << pl2) && (pl2 || written[x - xlo] == 1);
            for (int n = -hmax; n <= hmax && ok; ++n) {
                const int c = count[(size_t)(x - xlo) * span + n + hmax];
                const bool valid = x + n >= 0 && x + n < tnum;
                ok = valid ? c == 1 : c <= 1;
                pairs += valid;
            }
        }
        if (!ok) {
            fprintf(stderr, "launch %d (tnum %d, [%d, %d), xb %d, nh %d, lk %d, hmax %d, pieces %d, window %d): the cover does not hold\n", it, tnum,
                    xlo, xhi, xb, nh, lk, hmax, 1 << pl2, window);
            return 1;
        }
    }
    printf("kirch_quadwin_fuzz ok: %ld launches, %ld pairs, %ld refused\n", launches, pairs, refused);
    return 0;
}
