// Stand-alone driver for kirch_gangmap (csrc/kirch_route.h) under AddressSanitizer / UBSan (host code only, no HIP, no GPU):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I impdar_amd/csrc tests/san/kirch_gangmap_fuzz.cpp -o fuzz && ./fuzz
// A few thousand random launches through the probe -- profile lengths, output blocks that start and end anywhere, tile widths
// and alignments of both ring kernels, gang sizes (the rule's own, the knob's three, and some no knob can give) in both
// orders -- with the degenerate ones mixed in: a block of one trace, apertures of no pair at all (hmax 0) and wider than the
// profile, one chunk, more tiles than an item encodes.  Every list is checked for what the kernel relies on: each
// (chunk, tile) of the launch exactly once, nothing else.  Exit code 0 = every call returned and held that; the sanitizers
// abort on a finding.
#define KIRCH_ROUTE_PROBE 1
#include "kirch_route.h"
#include <cstdio>
#include <random>

int main()
{
    std::mt19937 rng(20261019);
    auto pick = [&](std::initializer_list<int> v) { return *(v.begin() + rng() % v.size()); };
    long maps = 0, refused = 0, items_total = 0;
    for (int it = 0; it < 6000; ++it) {
        const int tnum = pick({1, 2, 7, 31, 64, 65, 300, 341, 5000, 10000, 40000, 1000000});
        const int nch = pick({1, 1, 2, 3, 5, 16, 40});
        const int step = pick({4, 8}), mask = step - 1;
        const int tile_w = it % 97 == 0 ? 16 : pick({16, 20, 24, 32, 40, 64, 80, 120});
        const int ring_blocks = pick({5, 6, 7, 8, 9});
        const int G = pick({0, 1, 2, 4, 4, 3, 8}), order = (int)(rng() % 3) - 1;        // -1: by the launch
        const int xlo = (int)(rng() % tnum), xhi = (rng() % 4 == 0) ? tnum : xlo + 1 + (int)(rng() % (tnum - xlo));
        std::vector<int> hmax(nch);
        for (int &h : hmax) h = pick({0, 1, 9, 120, 438, 3461, 70000});
        const int nxt = (xhi - (xlo & ~mask) + tile_w - 1) / tile_w;
        std::vector<int> items((size_t)nch * nxt > 4000000 ? 1 : (size_t)nch * nxt + 1, -7);
        if (items.size() == 1 && nxt <= 32767) continue;           // (a launch this fuzz does not hold; the lists would be that long)
        int lens[8];
        const int n = impdar_kirch_gangmap_probe(hmax.data(), nch, tnum, xlo, xhi, tile_w, mask, ring_blocks, step, G, order, lens, items.data());
        if (n == 0) {
            if (nxt <= 32767) {
                fprintf(stderr, "no lists for %d chunks x %d tiles\n", nch, nxt);
                return 1;
            }
            ++refused;
            continue;
        }
        ++maps;
        items_total += n;
        std::vector<char> seen((size_t)nch * nxt, 0);
        bool ok = n == nch * nxt && items[(size_t)n] == -7 && lens[0] + lens[1] + lens[2] + lens[3] + lens[4] + lens[5] + lens[6] + lens[7] == n;
        for (int i = 0; i < n && ok; ++i) {
            const int c = items[i] >> 16, t = items[i] & 0xffff;
            ok = items[i] >= 0 && c < nch && t < nxt && !seen[(size_t)c * nxt + t];
            if (ok) seen[(size_t)c * nxt + t] = 1;
        }
        if (!ok) {
            fprintf(stderr, "lists of launch %d (tnum %d, [%d, %d), tile %d, G %d, order %d) are no permutation of its %d x %d items\n", it, tnum, xlo,
                    xhi, tile_w, G, order, nch, nxt);
            return 1;
        }
    }
    printf("kirch_gangmap_fuzz ok: %ld launches, %ld items, %ld beyond an item's range\n", maps, items_total, refused);
    return 0;
}
