// The host-side route of the GPS time-offset search (gpstrack.hip): the argument check of impdar_gps_cc /
// impdar_gps_cc_plan, the launch and the device bytes of a call -- plain C++, no HIP include, compiled by itself in
// tests/test_gps_route.py.  gpstrack.hip decides nothing that this header does not.
//
// One workgroup of GPS_THREADS threads per candidate offset; trace j of a candidate goes to thread j % GPS_THREADS.  The
// device holds the three GPS arrays, the three trace arrays, the candidates, and per candidate one correlation and one
// count, plus the two probe rows.
#pragma once
#include <cstddef>

enum { GPS_THREADS = 256, GPS_WAVES = GPS_THREADS / 64 };
constexpr long long GPS_MAX_GRID = 0x7fffffffLL;          // workgroups of one launch

struct GpsRoute {
    long long ngps = 0, tnum = 0, ncand = 0;
    int extrapolate = 0;
    int threads = 0;
    long long workgroups = 0;
    long long in_doubles = 0;        // gps_t, gps_lat, gps_lon, t, lat, lon, search
    long long out_doubles = 0;       // cc[ncand], nout[ncand] (as 64-bit integers), probe_lat[tnum], probe_lon[tnum]
    long long scratch_bytes = 0;     // both, each block rounded up to 16 bytes
    bool ok = false;
    const char *why = "";
};

static inline bool gps_mul(long long a, long long b, long long *r) { return !__builtin_mul_overflow(a, b, r); }
static inline bool gps_add(long long a, long long b, long long *r) { return !__builtin_add_overflow(a, b, r); }

// the sizes alone: what impdar_gps_cc_plan answers
static inline GpsRoute gps_route(long long ngps, long long tnum, long long ncand, int extrapolate)
{
    GpsRoute R;
    R.ngps = ngps;
    R.tnum = tnum;
    R.ncand = ncand;
    R.extrapolate = extrapolate;
    if (ngps < 2) { R.why = "fewer than 2 GPS fixes"; return R; }
    if (tnum < 1) { R.why = "no traces"; return R; }
    if (ncand < 1) { R.why = "no candidate offsets"; return R; }
    if (extrapolate != 0 && extrapolate != 1) { R.why = "extrapolate must be 0 or 1"; return R; }
    if (ncand > GPS_MAX_GRID) { R.why = "more candidates than one launch has workgroups"; return R; }
    long long g3, t3, t2, c2, work, in, out, bytes;
    // the bracket-and-multiply steps of a call, and every byte count, stay inside 64 bits
    if (!gps_mul(ncand, tnum, &work) || !gps_mul(work, 2, &work)) { R.why = "ncand x tnum overflows"; return R; }
    if (!gps_mul(ngps, 3, &g3) || !gps_mul(tnum, 3, &t3) || !gps_mul(tnum, 2, &t2) || !gps_mul(ncand, 2, &c2) ||
        !gps_add(g3, t3, &in) || !gps_add(in, ncand, &in) || !gps_add(c2, t2, &out) || !gps_add(in, out, &bytes) ||
        !gps_add(bytes, 2 * 11, &bytes) || !gps_mul(bytes, 8, &bytes)) {
        R.why = "the sizes overflow";
        return R;
    }
    R.threads = GPS_THREADS;
    R.workgroups = ncand;
    R.in_doubles = in;
    R.out_doubles = out;
    R.scratch_bytes = bytes;         // 11 blocks, each at most 8 bytes of padding
    R.ok = true;
    return R;
}

// gps_t is non-decreasing and holds no NaN: 0, else 1 + the index of the first fix that breaks it
static inline long long gps_times_bad(const double *gps_t, long long ngps)
{
    for (long long k = 0; k < ngps; ++k) {
        if (gps_t[k] != gps_t[k]) return k + 1;
        if (k > 0 && gps_t[k] < gps_t[k - 1]) return k + 1;
    }
    return 0;
}

// probe < 0: none; else a candidate
static inline bool gps_probe_ok(long long probe, long long ncand) { return probe < ncand; }

#ifdef GPS_ROUTE_PROBE
// what tests/test_gps_route.py calls.  gps_t may be null (sizes alone).  longs[6]: threads, workgroups, in_doubles,
// out_doubles, scratch_bytes, first bad fix (1-based, 0: none).  Returns 0 when the call would be accepted.
extern "C" int impdar_gps_route_full_probe(long long ngps, long long tnum, long long ncand, int extrapolate, long long probe,
                                           const double *gps_t, long long *longs)
{
    const GpsRoute R = gps_route(ngps, tnum, ncand, extrapolate);
    const long long bad = R.ok && gps_t ? gps_times_bad(gps_t, ngps) : 0;
    const long long l[6] = {R.threads, R.workgroups, R.in_doubles, R.out_doubles, R.scratch_bytes, bad};
    for (int k = 0; k < 6; ++k) longs[k] = l[k];
    return R.ok && !bad && gps_probe_ok(probe, ncand) ? 0 : 1;
}
#endif
