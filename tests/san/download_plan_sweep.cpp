// Stand-alone driver for download_plan / DlRing (csrc/download_plan.h) under AddressSanitizer / UBSan (host code only, no HIP, no GPU):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I impdar_amd/csrc tests/san/download_plan_sweep.cpp -o sweep && ./sweep
// The sweep of tests/test_download_plan.py -- ring capacities of 256 ... 8192 bytes, element sizes 1, 4 and 8, granules of
// 1 ... 70 elements, 1 ... 4 blocks of 0 ... 40 granules, the named edge cases -- through the probe, checked for what
// download.hip relies on: the pieces of a block are in order, start on a granule and cover the block once; no piece is
// larger than the ring; the replay "place, else retire the oldest and try again" ends, and in it no two live pieces
// overlap and none reaches past the ring; a granule above the ring, and nothing else, is refused.  Exit code 0 = every
// plan held that; the sanitizers abort on a finding.
#define DOWNLOAD_PLAN_PROBE 1
#include "download_plan.h"
#include <cstdio>
#include <vector>

struct Blk {
    size_t count, gran;
};

static std::vector<long long> g_out(6 * 8192);

// 0: the plan holds (or is refused as it must be); 1: a rule breaks
static int check(size_t cap, size_t elem, const std::vector<Blk> &blocks, long long *npieces = nullptr)
{
    std::vector<size_t> count, gran;
    bool too_wide = false;
    for (const Blk &b : blocks) {
        count.push_back(b.count);
        gran.push_back(b.gran);
        if (b.count > 0 && (b.count < b.gran ? b.count : b.gran) * elem > cap) too_wide = true;
    }
    const long long rc = impdar_download_plan_probe(cap, elem, (int)blocks.size(), count.data(), gran.data(), g_out.data(), 8192);
    if (npieces) *npieces = rc;
    if (too_wide || rc < 0) return (too_wide && rc == -1) ? 0 : 1;
    bool ok = true;
    long long k = 0, last = 0;
    for (size_t i = 0; i < blocks.size(); ++i) {
        size_t at = 0;
        for (; k < rc && g_out[6 * k] == (long long)i; ++k) {
            const size_t first = (size_t)g_out[6 * k + 1], cnt = (size_t)g_out[6 * k + 2], bytes = (size_t)g_out[6 * k + 3];
            ok = ok && blocks[i].count > 0 && first == at && first % blocks[i].gran == 0 && cnt > 0 && bytes == cnt * elem && bytes <= cap;
            at += cnt;
        }
        ok = ok && at == blocks[i].count;
    }
    ok = ok && k == rc;
    for (k = 0; k < rc && ok; ++k) {
        const long long bytes = g_out[6 * k + 3], off = g_out[6 * k + 4], retired = g_out[6 * k + 5];
        ok = ok && last <= retired && retired <= k && off >= 0 && off % (long long)elem == 0 && off + bytes <= (long long)cap;
        last = retired;
        for (long long j = retired; j < k; ++j) {
            const long long oj = g_out[6 * j + 4], bj = g_out[6 * j + 3];
            ok = ok && (off + bytes <= oj || oj + bj <= off);
        }
    }
    if (!ok) fprintf(stderr, "the plan of cap %zu elem %zu, %zu blocks (first: %zu of %zu) breaks a rule\n", cap, elem, blocks.size(),
                     blocks[0].count, blocks[0].gran);
    return ok ? 0 : 1;
}

int main()
{
    const size_t caps[] = {256, 260, 1000, 1024, 4099, 8192}, elems[] = {1, 4, 8};
    long calls = 0;
    for (size_t ci = 0; ci < 6; ++ci)
        for (size_t elem : elems)
            for (size_t gran = 1; gran <= 70; ++gran)
                for (size_t nblk = 1; nblk <= 4; ++nblk)
                    for (size_t v = 0; v < 3; ++v) {
                        std::vector<Blk> blocks;
                        for (size_t b = 0; b < nblk; ++b) {
                            const size_t g = (7 * gran + 13 * b + 11 * v + 5 * nblk + 3 * ci + elem) % 41;
                            const size_t cut = v == 2 && g > 0 ? (3 * v + b + 1) % gran : 0;
                            blocks.push_back(Blk{g * gran - cut, gran});
                        }
                        if (check(caps[ci], elem, blocks)) return 1;
                        ++calls;
                    }
    // the named cases of the test: a total below the ring, a piece of exactly the ring, a granule between a quarter of the
    // ring and the ring, a zero-width block between two others, a ragged flat block, a flat block shorter than a granule,
    // many rings long
    long long n = 0;
    if (check(4096, 4, {{100, 16}}, &n) || n != 1) return 1;
    if (check(1024, 4, {{64, 16}, {256, 256}, {64, 16}}, &n) || n != 3) return 1;
    if (check(1024, 4, {{700, 100}}, &n) || n != 7) return 1;
    if (check(1024, 8, {{30 * 7, 7}, {0, 0}, {30 * 9, 9}}, &n) || n <= 0) return 1;
    if (check(8192, 4, {{1003, 16}}, &n) || n != 2) return 1;
    if (check(20, 4, {{5, 16}}, &n) || n != 1) return 1;
    if (check(256, 1, {{5000, 16}, {3000, 1}}, &n) || n <= 0) return 1;
    calls += 7;
    // a granule above the ring is refused; one of exactly the ring, and one that holds nothing, are not
    if (check(1024, 8, {{129 * 3, 129}}, &n) || n != -1) return 1;
    if (check(1024, 8, {{64, 16}, {129, 129}}, &n) || n != -1) return 1;
    if (check(1024, 8, {{128 * 3, 128}}, &n) || n != 3) return 1;
    if (check(1024, 8, {{0, 129}}, &n) || n != 0) return 1;
    calls += 4;
    printf("%ld plans hold\n", calls);
    return 0;
}
