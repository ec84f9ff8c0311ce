// What an f-k call (fk.hip: fan filter, f-k spectrum) decides on the host before its first HIP call: whether its arguments are a
// fan at all, which transforms it runs on (Stolt's, always: the plan is shared), how many rows come back and whether the inverse
// needs a plan beside Stolt's, and the kernel string of the metrics line.  Plain C++, no device code -- compiled into the
// library by fk.hip and, by itself with g++, into the CPU suite's checker (tests/test_fk_route.py).
#pragma once
#include "fk_weight.h"
#include "stolt_route.h"

// Null for a fan the entries take, else what is wrong with it (the text of the argument error).
static inline const char *fk_fan_refusal(int snum, int tnum, double va_lo, double va_hi, double taper, int mode, int dip)
{
    const bool has_lo = !(va_lo != va_lo), has_hi = !(va_hi != va_hi);
    const double big = 1.7976931348623157e308;
    if (snum < 2 || tnum < 2) return "need snum >= 2 and tnum >= 2";
    if (!has_lo && !has_hi) return "need va_lo or va_hi (both are NaN)";
    if (has_lo && !(va_lo > 0 && va_lo <= big)) return "va_lo must be finite and positive";
    if (has_hi && !(va_hi > 0 && va_hi <= big)) return "va_hi must be finite and positive";
    if (!(taper >= 0 && taper < 1)) return "taper must lie in [0, 1)";
    if (has_lo && has_hi && (1.0 / va_hi) * (1.0 + taper) > (1.0 / va_lo) * (1.0 - taper)) return "the tapers of va_lo and va_hi overlap";
    if (mode != FK_PASS && mode != FK_REJECT) return "mode must be 0 (pass) or 1 (reject)";
    if (dip != FK_DIP_BOTH && dip != FK_DIP_DOWN_RIGHT && dip != FK_DIP_DOWN_LEFT) return "dip must be 0 (both), 1 (down_right) or 2 (down_left)";
    return nullptr;
}

// The transforms are those of a Stolt call at the size (stolt_route), the forward half bit for bit.  The filtered radargram has
// snum rows; Stolt's inverse has 2 (snum / 2), one fewer at odd snum (rocFFT only): there the inverse is a 2-D real plan of
// snum rows kept beside Stolt's, under either form of the rocFFT knob.
struct FkRoute {
    StoltRoute route;
    int out_rows;
    bool own_inverse_plan;
};
static inline FkRoute fk_route(int snum, int tnum, const double *kx, const StoltKnobs &K)
{
    FkRoute r;
    r.route = stolt_route(snum, tnum, kx, K);
    r.out_rows = snum;
    r.own_inverse_plan = snum % 2 != 0;
    return r;
}

// The kernel string of the metrics line, of the filter or of the spectrum.
static inline const char *fk_kernel_label(const StoltShape &s, bool power)
{
    if (s.route == STOLT_OWN_ROWS) {
        if (power) return s.mixed ? "fk_power_t (+ the library's own row transforms, traces first, mixed radix)" : "fk_power_t (+ the library's own row transforms, traces first)";
        return s.mixed ? "fk_fan_rows (+ the library's own row transforms, traces first, mixed radix)" : "fk_fan_rows (+ the library's own row transforms, traces first)";
    }
    if (s.use_own) {
        if (power) return s.mixed ? "fk_power_wkx (+ the library's own row transforms, mixed radix)" : "fk_power_wkx (+ the library's own row transforms)";
        return s.mixed ? "fk_fan_wkx (+ the library's own row transforms, mixed radix)" : "fk_fan_wkx (+ the library's own row transforms)";
    }
    return power ? "fk_power_t (+ rocFFT 2-D real transforms)" : "fk_fan_kxw (+ rocFFT 2-D real transforms)";
}
