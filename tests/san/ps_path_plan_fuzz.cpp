// Stand-alone driver for csrc/ps_path_plan.h under AddressSanitizer / UBSan (host code only, no HIP, no GPU):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I impdar_amd/csrc tests/san/ps_path_plan_fuzz.cpp -o fuzz && ./fuzz
// A few thousand random velocity profiles through the probe -- the three plans of each, the arrays sized exactly as the probe
// documents them -- with the degenerate ones mixed in: one step, every step a run of its own, NaN / inf / zero at a random
// step, zero everywhere, 97 and more runs, frequency counts that are no multiple of 32, a constant velocity.  Exit code 0 =
// every call returned and every taken plan fits its arrays; the sanitizers abort on a finding.
#define PS_PATH_PLAN_PROBE 1
#include "ps_path_plan.h"
#include <cstdio>
#include <limits>
#include <random>

int main()
{
    std::mt19937 rng(20251019);
    auto pick = [&](std::initializer_list<int> v) { return *(v.begin() + rng() % v.size()); };
    long calls = 0, taken[3] = {0, 0, 0};
    for (int it = 0; it < 6000; ++it) {
        // a profile as runs of constant velocity: how many, how long
        const int shape = rng() % 10;
        std::vector<double> v;
        if (shape == 0) {
            v.assign(1, 1.7e8);                                                  // one step
        } else if (shape == 1) {
            const int n = pick({2, 63, 64, 300, 1000});
            for (int i = 0; i < n; ++i) v.push_back(1.6e8 + 1e5 * i);           // all single steps
        } else {
            const int nruns = shape == 2 ? pick({97, 98, 130, 300}) : pick({1, 2, 3, 4, 5, 8, 16, 17, 40, 96});
            for (int r = 0; r < nruns; ++r) {
                const int len = pick({1, 1, 2, 3, 8, 9, 16, 63, 64, 65, 200, 511, 512, 513, 1024, 1025, 2049, 4097});
                v.insert(v.end(), (size_t)len, 1.6e8 + 1e6 * (r % 37));
                if (v.size() > 20000) break;
            }
        }
        const int snum = (int)v.size();
        if (shape == 3) v[rng() % snum] = std::numeric_limits<double>::quiet_NaN();
        if (shape == 4) v[rng() % snum] = std::numeric_limits<double>::infinity();
        if (shape == 5) v[rng() % snum] = 0.0;
        if (shape == 6) std::fill(v.begin(), v.end(), 0.0);                      // zero velocities
        if (shape == 7) for (double &x : v) x *= 1.0 + 4e-13 * ((int)(rng() % 1024) - 512) / 512.0;     // the noise of a table
        const bool constant = shape == 8;                                        // one constant instead of the profile
        const double *vmig = constant ? nullptr : v.data();
        const int dbl = rng() % 2, pairs = rng() % 2, vz = constant ? 0 : 1, herm = rng() % 8 != 0;
        const int nf = pick({1, 31, 32, 63, 64, 100, 224, 255, 256, 1000, 1024, 2080, 4096, 4100, 4128, 6144, 6176, 16384});
        const int cap = snum + 16;
        int ints[8];
        {
            std::vector<int> pi(4 * (size_t)cap);
            std::vector<double> pv(cap), pvs(PN_SHORT * (size_t)cap), e1(snum);
            if (impdar_pn_plan_probe(dbl, snum, nf, pairs, vz, herm, 1.69e8, vmig, cap, ints, pi.data(), pv.data(), pvs.data(), e1.data()) != 0) {
                fprintf(stderr, "pn: %d pieces beyond %d\n", ints[1], cap);
                return 1;
            }
            taken[0] += ints[0];
        }
        {
            std::vector<int> ri(4 * (size_t)cap), si(24 * (size_t)cap);
            std::vector<double> rv(cap);
            if (impdar_pr_plan_probe(dbl, snum, nf, 1.69e8, vmig, cap, ints, ri.data(), rv.data(), si.data()) != 0) {
                fprintf(stderr, "pr: %d runs beyond %d\n", ints[1], cap);
                return 1;
            }
            taken[1] += ints[0];
        }
        {
            std::vector<int> tab(2 * (size_t)cap);
            int long_of[PM_MAX_RUNS];
            if (impdar_pm_plan_probe(dbl, snum, nf, vz, 1.69e8, vmig, cap, ints, tab.data(), long_of) != 0) {
                fprintf(stderr, "pm: row blocks beyond %d\n", cap);
                return 1;
            }
            taken[2] += ints[0];
        }
        calls += 3;
    }
    for (int W : {8, 14})
        for (int l = 4; l <= 12; ++l) {
            std::vector<double> out((size_t)(1 << l) / 2 + 1);
            if (impdar_pn_corr_probe(W, l, out.data()) != (int)out.size()) return 1;
        }
    double dw;
    const double w1[2] = {-2.0, 1.0}, w2[3] = {3.0, 1.0, 2.0};
    if (ps_axis_uniform(w1, 2, 1e-9, &dw) != true || ps_axis_uniform(w2, 3, 2e-15, &dw) != true || ps_thr_off_band(w1, 0) != true) return 1;
    printf("%ld planner calls: %ld / %ld / %ld plans taken (transform, many-runs, matrix-core)\n", calls, taken[0], taken[1], taken[2]);
    return taken[0] && taken[1] && taken[2] ? 0 : 1;
}
