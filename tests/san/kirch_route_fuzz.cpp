// Stand-alone driver for csrc/kirch_route.h under AddressSanitizer / UBSan (host code only, no HIP, no GPU):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I impdar_amd/csrc tests/san/kirch_route_fuzz.cpp -o fuzz && ./fuzz
// A few thousand random geometries and knob settings through the probe -- the route, the host tables and the tile map of
// each -- with the degenerate ones mixed in: one trace, two samples, equal positions, a first sample at t = 0, a moveout
// no ring can hold, a spacing far below a sample.  Exit code 0 = every call returned; the sanitizers abort on a finding.
#define KIRCH_ROUTE_PROBE 1
#include "kirch_route.h"
#include <cstdio>
#include <random>

int main()
{
    std::mt19937 rng(20251018);
    auto pick = [&](std::initializer_list<double> v) { return *(v.begin() + rng() % v.size()); };
    long routes = 0, tables = 0, maps = 0;
    for (int it = 0; it < 4000; ++it) {
        const int snum = (int)pick({2, 3, 4, 64, 255, 256, 257, 300, 700}), tnum = (int)pick({1, 2, 7, 31, 32, 33, 96, 500, 9000});
        const double dt = pick({1e-8, 1e-9, 4e-8}), vel = pick({1.69e8, 3e8, 1e7});
        const double dx = pick({0.0, 1e-9, 1e-3, 0.5, 1.0, 3.4, 8.0, 17.0, 30.0, 1e6, 1e300});        // equal positions .. a moveout of 1e300 samples
        const double t0 = pick({0.0, 0.0, -3e-8, 5e-8, 1e-3});
        std::vector<double> tt(snum), dist(tnum);
        for (int k = 0; k < snum; ++k) tt[k] = t0 + k * dt;
        for (int j = 0; j < tnum; ++j) dist[j] = j * dx;
        const int shape = rng() % 8;
        if (shape == 1) for (int j = 0; j < tnum; ++j) dist[j] += (j % 3) * 0.2 * dx;            // sorted, not uniform
        if (shape == 2) for (int j = 0; j < tnum; ++j) dist[j] += (j % 2) * 2.5 * dx;            // not sorted
        if (shape == 3) for (int k = 1; k < snum; k += 2) tt[k] += 1e-10 * dt;
        if (shape == 4 && snum > 2) tt[snum / 2] = tt[snum / 2 - 1];                             // not increasing
        if (shape == 5) for (int j = 0; j < tnum; ++j) dist[j] += 4.0e4;                         // far along the line
        int knobs[15];
        for (int i = 0; i < 12; i += 2) {
            knobs[i] = rng() % 3 == 0;
            knobs[i + 1] = knobs[i] ? (int)pick({0, 1, 2, 3, 4, 7, 16, 20, 24, 32, 40, -1}) : 0;
        }
        knobs[12] = rng() % 4 == 0 ? rng() % 3 : 0;
        knobs[13] = rng() % 4 == 0 ? rng() % 3 : 0;
        knobs[14] = rng() % 8 == 0;
        const int dtype = rng() % 2, mode = rng() % 3, near = rng() % 4 == 0, nranks = (int)pick({1, 1, 2, 4, 8});
        const double tlim = tt[snum - 1] * 0.999;
        const bool given = rng() % 8 == 0;
        const long long ties = (long long)pick({-1, 0, 5, 1 << 20, (1 << 20) + 1});
        int ints[32];
        double dbls[16];
        impdar_kirch_route_probe(dtype, snum, tnum, dist.data(), tt.data(), vel, near, mode, nranks, given ? &tlim : nullptr, given && rng() % 2,
                                 knobs, ties, 1 << 20, ints, dbls);
        ++routes;
        if (ints[0] != 0 || !ints[18] || !(ints[19] && ints[21])) continue;        // refused, not increasing, not uniform
        // the tables of plans whose pick table stays small (hglob <= tnum + 128 bounds every array)
        const int nch = (snum + 255) / 256;
        const size_t big = (size_t)nch * (tnum + 256) * 2 + 4096;
        int sizes[8] = {0};
        std::vector<int> h_half(snum), hmax(nch), klo(big), khi(big), win(big);
        std::vector<float> c32(3 * (size_t)snum), gen2(2 * (size_t)snum);
        std::vector<double> c64(3 * (size_t)snum), genc(2 * (size_t)nch);
        if (impdar_kirch_tables_probe(dtype, snum, tnum, dist.data(), tt.data(), vel, near, mode, nranks, knobs, sizes, h_half.data(), c32.data(),
                                      c64.data(), gen2.data(), genc.data(), hmax.data(), klo.data(), khi.data(), win.data()) != 0)
            continue;
        ++tables;
        if ((size_t)sizes[0] * sizes[1] > big || (size_t)sizes[6] > big) {
            fprintf(stderr, "table sizes %d x %d / %d beyond the bound %zu\n", sizes[0], sizes[1], sizes[6], big);
            return 1;
        }
        if (!sizes[0] || !(ints[6] || ints[7])) continue;
        // the tile map of one launch over a random output block, as launch_ring would ask for it
        const int S = ints[7] ? 4 : 8, tile_w = ints[8] * ints[9], mask = S - 1;
        const int xlo = (int)(rng() % tnum), xhi = xlo + 1 + (int)(rng() % (tnum - xlo));
        const int nxt = (xhi - (xlo & ~mask) + tile_w - 1) / tile_w, G = nxt >= 256 ? 4 : 1;
        const int tpx = ((nxt + 8 * G - 1) / (8 * G)) * G;
        std::vector<short> map((size_t)nch * tpx * 8);
        impdar_kirch_tilemap_probe(hmax.data(), nch, tnum, xlo, xhi, tile_w, mask, (ints[8] + 15 + 7) / 8, S, G, tpx, map.data());
        ++maps;
    }
    // the tie grouping, empty and full of duplicates
    {
        std::vector<int> ties, g_ti(64), g_off(65), g_n(64);
        impdar_kirch_ties_probe(ties.data(), 0, g_ti.data(), g_off.data(), g_n.data());
        for (int i = 0; i < 63; ++i) {
            ties.push_back((int)(rng() % 5));
            ties.push_back((int)(rng() % 9));
        }
        impdar_kirch_ties_probe(ties.data(), 63, g_ti.data(), g_off.data(), g_n.data());
    }
    printf("kirch_route_fuzz ok: %ld routes, %ld table sets, %ld tile maps\n", routes, tables, maps);
    return 0;
}
