// The host-side route of the attenuation window search (attsearch.hip): the argument check of impdar_att_search /
// impdar_att_search_plan, the launch and the device bytes of a call -- plain C++, no HIP include, compiled by itself in
// tests/test_att_route.py.  attsearch.hip decides nothing that this header does not.
//
// One workgroup of ATT_THREADS threads per centre (a trace of method 3, a depth of method 6b).  A window is staged through
// LDS in tiles of ATT_TILE (z - mean z, pc - mean pc) pairs; a thread owns one rate and one of `parts` interleaved parts
// of the window, `chunk` rates are in hand at a time (parts x chunk <= ATT_THREADS).  The device holds z, pc, the rates,
// the centres of the depth form, per centre one row of C (the window in hand), the rate index, the width and the outcome
// code, plus the probe table.
#pragma once
#include <cstddef>

enum { ATT_THREADS = 256, ATT_WAVES = ATT_THREADS / 64, ATT_TILE = 1024 };
enum { ATT_INDEX = 0, ATT_DEPTH = 1 };                                    // method 3, method 6b
enum { ATT_VALUE = 0, ATT_NOT_ENTERED = 1, ATT_TIE = 2, ATT_NONFINITE = 3 };   // what a centre ended as
constexpr long long ATT_MAX_GRID = 0x7fffffffLL;          // workgroups of one launch
constexpr double ATT_MAX_WIDTH = 4611686018427387904.0;   // 2^62: an index width is an exact integer below it
constexpr double ATT_MAX_WINDOWS = 1048576.0;             // 2^20 steps across the depth range, at most (an index walk has no more than n / 2 windows)

struct AttRoute {
    int flavour = 0;
    long long n = 0, nn = 0, ncent = 0, probe_cap = 0;
    int threads = 0;
    long long workgroups = 0;
    int parts = 0;                   // interleaved parts of a window, each summed by one thread per rate
    int chunk = 0;                   // rates in hand at a time
    long long in_doubles = 0;        // z[n], pc[n], ns[nn], centres[ncent] (depth form)
    long long out_doubles = 0;       // C rows [ncent][nn], idx[ncent] (64-bit integers), win[ncent], probe [probe_cap][nn], rows
    long long out_ints = 0;          // code[ncent]
    long long scratch_bytes = 0;     // all of them, each block rounded up to 16 bytes
    bool ok = false;
    const char *why = "";
};

static inline bool att_mul(long long a, long long b, long long *r) { return !__builtin_mul_overflow(a, b, r); }
static inline bool att_add(long long a, long long b, long long *r) { return !__builtin_add_overflow(a, b, r); }

// probe < 0: none (probe_cap is not looked at); else a centre, and at least one row for its table
static inline bool att_probe_ok(long long probe, long long ncent, long long probe_cap)
{
    return probe < 0 || (probe < ncent && probe_cap >= 1);
}

// n pairs (z, pc), nn rates, ncent centres; win_init / win_step as the call has them (integers of the index form as doubles)
static inline AttRoute att_route(int flavour, long long n, long long nn, long long ncent, double win_init, double win_step,
                                 long long probe, long long probe_cap)
{
    AttRoute R;
    R.flavour = flavour;
    R.n = n;
    R.nn = nn;
    R.ncent = ncent;
    if (flavour != ATT_INDEX && flavour != ATT_DEPTH) { R.why = "flavour must be 0 (index windows) or 1 (depth windows)"; return R; }
    if (n < 1) { R.why = "no (z, pc) pairs"; return R; }
    if (nn < 1) { R.why = "no rates"; return R; }
    if (ncent < 1) { R.why = "no centres"; return R; }
    if (ncent > ATT_MAX_GRID) { R.why = "more centres than one launch has workgroups"; return R; }
    if (flavour == ATT_INDEX) {
        // (a NaN fails every comparison below)
        if (!(win_init >= 2.0 && win_init < ATT_MAX_WIDTH) || win_init != (double)(long long)win_init) { R.why = "win_init must be an integer >= 2"; return R; }
        if (!(win_step >= 1.0 && win_step < ATT_MAX_WIDTH) || win_step != (double)(long long)win_step) { R.why = "win_step must be an integer >= 1"; return R; }
    } else {
        if (!(win_init > 0.0 && win_init <= 1.7e308)) { R.why = "win_init must be positive and finite"; return R; }
        if (!(win_step > 0.0 && win_step <= 1.7e308)) { R.why = "win_step must be positive and finite"; return R; }
    }
    if (!att_probe_ok(probe, ncent, probe_cap)) { R.why = "probe is no centre, or its table has no row"; return R; }
    R.probe_cap = probe < 0 ? 0 : probe_cap;
    long long n2, in, crow, prow, out, ints, bytes;
    if (!att_mul(n, 2, &n2) || !att_add(n2, nn, &in) || !att_add(in, flavour == ATT_DEPTH ? ncent : 0, &in) ||
        !att_mul(ncent, nn, &crow) || !att_mul(R.probe_cap, nn, &prow) || !att_add(crow, prow, &out) ||
        !att_add(out, 2 * ncent + 1, &out) || !att_add(in, out, &bytes) || !att_add(bytes, 2 * 10, &bytes) ||
        !att_mul(bytes, 8, &bytes) || !att_mul(ncent, 4, &ints) || !att_add(bytes, ints, &bytes)) {
        R.why = "the sizes overflow";
        return R;
    }
    R.threads = ATT_THREADS;
    R.workgroups = ncent;
    R.parts = nn >= ATT_THREADS ? 1 : (int)(ATT_THREADS / nn);
    R.chunk = nn >= ATT_THREADS ? ATT_THREADS : (int)nn;
    R.in_doubles = in;
    R.out_doubles = out;
    R.out_ints = ncent;
    R.scratch_bytes = bytes;         // 10 blocks, each at most 16 bytes of padding
    R.ok = true;
    return R;
}

// the rest of the argument check: the index of the rate 0, the first trace of the index form
static inline bool att_call_ok(const AttRoute &R, long long j0, long long first)
{
    long long last;
    return R.ok && j0 >= 0 && j0 < R.nn && (R.flavour == ATT_DEPTH || (first >= 0 && att_add(first, R.ncent, &last)));
}

// z of the depth form is non-decreasing and holds no NaN: 0, else 1 + the index of the first element that breaks it
static inline long long att_depths_bad(const double *z, long long n)
{
    for (long long k = 0; k < n; ++k) {
        if (z[k] != z[k]) return k + 1;
        if (k > 0 && z[k] < z[k - 1]) return k + 1;
    }
    return 0;
}

// The depth walk ends: a window is visited only while d - win/2 >= z[0] and d + win/2 <= z[n-1], so no visited width
// exceeds span = z[n-1] - z[0] but by a rounding.  The walk is finite when the ends are finite and the repeated float64 sum
// win += win_step keeps moving: half the step must still change a width of 2 span, i.e. win_step is at least one unit in
// the last place of any width the walk can reach (a step that the width absorbs would leave win where it is for ever; one
// of half a unit moves some widths and not others).  Every addition then advances win by at least win_step / 2, so a walk
// has at most 2 span / win_step windows, and that quotient is capped: span / win_step <= ATT_MAX_WINDOWS.  The reference
// spins on the host for the input refused here; a kernel must not.
// Null when the walk is bounded, else why not.  z0 = z[0], zn = z[n-1] of the sorted depths.
static inline const char *att_depth_walk_bad(double z0, double zn, double win_step)
{
    if (!(z0 >= -1.7e308 && z0 <= 1.7e308 && zn >= -1.7e308 && zn <= 1.7e308)) return "the depths are not finite";
    const double span = zn - z0, widest = 2.0 * span;
    if (!(widest <= 1.7e308)) return "the depth range is not finite";
    volatile double moved = widest + win_step / 2.0;      // (rounded to float64 before it is compared)
    if (moved == widest) return "win_step does not advance a window as wide as the depth range";
    if (!(span / win_step <= ATT_MAX_WINDOWS)) return "more than 2^20 steps between the shallowest and the deepest pick";
    return nullptr;
}

#ifdef ATT_ROUTE_PROBE
// what tests/test_att_route.py calls.  longs[8]: threads, workgroups, parts, chunk, in_doubles, out_doubles, out_ints,
// scratch_bytes.  z may be null (sizes alone).  Returns 0 when the call would be accepted.
extern "C" int impdar_att_route_full_probe(int flavour, long long n, long long nn, long long ncent, double win_init, double win_step,
                                           long long probe, long long probe_cap, long long j0, long long first, const double *z,
                                           long long *longs)
{
    const AttRoute R = att_route(flavour, n, nn, ncent, win_init, win_step, probe, probe_cap);
    if (R.ok && (!att_call_ok(R, j0, first) ||
                 (z && flavour == ATT_DEPTH && (att_depths_bad(z, n) || att_depth_walk_bad(z[0], z[n - 1], win_step))))) {
        for (int k = 0; k < 8; ++k) longs[k] = 0;
        return 1;
    }
    const long long l[8] = {R.threads, R.workgroups, R.parts, R.chunk, R.in_doubles, R.out_doubles, R.out_ints, R.scratch_bytes};
    for (int k = 0; k < 8; ++k) longs[k] = l[k];
    return R.ok ? 0 : 1;
}
#endif
