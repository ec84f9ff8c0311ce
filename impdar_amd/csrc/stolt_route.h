// What a Stolt call (stolt.hip) decides on the host before its first HIP call: the IMPDAR_STOLT_FFT knob, which transforms the
// call runs on, the sizes that follow from (snum, tnum) and the route, the key of the cached plan, the batches of a velocity
// scan, and the kernel string of the metrics line.  Plain C++, no device code -- compiled into the library by stolt.hip and,
// by itself with g++, into the CPU suite's checker (tests/test_stolt_route.py).
#pragma once
#include "own_fft_len.h"
#include "own_fft_mixed_plan.h"
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

// IMPDAR_STOLT_FFT, read once per call (nothing is kept across calls: the plan's key holds what its plans were made under):
// "1d" = four 1-D rocFFT passes; "rocfft" = rocFFT's 2-D real plans also where the own transforms apply; "own" = the default,
// spelled out (tests that pin one implementation); "mixed" = the own mixed-radix transforms at every size they take, not only
// where rocFFT has kernels to compile
struct StoltKnobs {
    bool use2d = true, no_own = false, want_mixed = false;
    static StoltKnobs from_env()
    {
        StoltKnobs K;
        const char *e = getenv("IMPDAR_STOLT_FFT");
        K.use2d = !(e && !strcmp(e, "1d"));
        K.no_own = e && !strcmp(e, "rocfft");
        K.want_mixed = e && !strcmp(e, "mixed");
        return K;
    }
    bool operator==(const StoltKnobs &o) const { return use2d == o.use2d && no_own == o.no_own && want_mixed == o.want_mixed; }
};

// Which transforms a call runs on.  Both forms of the own transforms need snum even.
//   rows ("traces first", seven passes): R2C / C2R over the traces (complex length tnum / 2) and C2C of snum over time, on the
//     wavenumbers k = 0 .. tnum / 2 alone, which holds the other half through kx[k] == -kx[tnum - k]; tnum >= 64
//   [w][kx] (ten passes): R2C / C2R over time (complex length snum / 2), C2C of tnum over the traces; tnum may be odd
// Power-of-two sizes keep the gate they had (the [w][kx] lengths decide, the rows form where snum fits too).  Any other size
// takes the own transforms where the mixed-radix kernel has the lengths of a form (own_fft_mixed_plan.h), the rows form first --
// by default only where rocFFT would compile kernels at run time (a length above 1024); IMPDAR_STOLT_FFT=mixed: wherever
// the lengths allow.  "1d" and "rocfft" keep every size on rocFFT.
// (power-of-two sizes run on the library's own row transforms (own_fft.h), every call: 0.35 ms at 4096^2 against 0.37 on
// rocFFT's 2-D plans (round 5: the stretch on the frequency-major spectrum, two transposes fewer), nothing compiled at
// run time, no plan to make (rocFFT: 0.3-3 s per process for lengths above 1024))
enum StoltRoute { STOLT_ROCFFT = 0, STOLT_OWN_WKX = 1, STOLT_OWN_ROWS = 2 };
static inline bool stolt_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
static inline StoltRoute stolt_route(int snum, int tnum, const double *kx, const StoltKnobs &K)
{
    if (!K.use2d || K.no_own) return STOLT_ROCFFT;
    if (snum % 2) return STOLT_ROCFFT;
    if (stolt_pow2(snum) && stolt_pow2(tnum)) {
        if (!(own_fft_len_ok(snum / 2) && own_fft_len_ok(tnum))) return STOLT_ROCFFT;
        return own_fft_len_ok(snum) && tnum >= 64 ? STOLT_OWN_ROWS : STOLT_OWN_WKX;
    }
    if (!(K.want_mixed || snum > 1024 || tnum > 1024)) return STOLT_ROCFFT;
    auto len_ok = [](int M) { return own_fft_len_ok(M) || own_fft_mixed_len_ok(M); };
    if (tnum % 2 == 0 && tnum >= 64 && len_ok(tnum / 2) && len_ok(snum)) {
        bool antisym = true;
        for (int k = 1; k < tnum / 2 && antisym; ++k) antisym = kx[k] == -kx[tnum - k];
        if (antisym) return STOLT_OWN_ROWS;
    }
    return len_ok(snum / 2) && len_ok(tnum) ? STOLT_OWN_WKX : STOLT_ROCFFT;
}

// What the stages of one call share: the sizes, the route and what follows from it.
struct StoltShape {
    int dtype, snum, tnum;
    int m, nz, nout;        // frequencies snum / 2 + 1, stretched rows snum / 2, output rows 2 (snum / 2)
    int hs;                 // wavenumbers k = 0 .. tnum / 2 of the rows form
    StoltRoute route;
    bool use_own, mixed;    // mixed: a transform of the call runs on the mixed-radix kernel (the metrics line says so)
    // elements of the plan's buffers: X [tnum][snum] real; F and K complex, the larger of [tnum][m] and the rows form's
    // [snum][hs] / [hs][snum]; Y [tnum][nout] real
    size_t x_elems, spec_elems, y_elems;
};
static inline StoltShape stolt_shape(int dtype, int snum, int tnum, StoltRoute route)
{
    StoltShape s;
    s.dtype = dtype;
    s.snum = snum;
    s.tnum = tnum;
    s.m = snum / 2 + 1;
    s.nz = snum / 2;
    s.nout = 2 * (snum / 2);
    s.hs = tnum / 2 + 1;
    s.route = route;
    s.use_own = route != STOLT_ROCFFT;
    s.mixed = s.use_own && !(stolt_pow2(snum) && stolt_pow2(tnum));
    s.x_elems = (size_t)tnum * snum;
    s.spec_elems = std::max((size_t)tnum * s.m, (size_t)snum * s.hs);
    s.y_elems = (size_t)tnum * s.nout;
    return s;
}

// What the cached plan (its rocFFT plans and buffers) was made for; `owner`: the context whose device and stream they live on.
struct StoltPlanKey {
    const void *owner = nullptr;
    int dtype = -1, snum = 0, tnum = 0;
    bool use2d = true, no_own = false;
    int route = -1;
    bool operator==(const StoltPlanKey &o) const
    {
        return owner == o.owner && dtype == o.dtype && snum == o.snum && tnum == o.tnum && use2d == o.use2d && no_own == o.no_own &&
               route == o.route;
    }
};

// What one velocity of a scan batch may hold on the device, spectra and image together: the batch is as large as fits.
constexpr size_t STOLT_SCAN_BUDGET_BYTES = (size_t)2 << 30;
constexpr int STOLT_SCAN_MAX_BATCH = 1024;

// The batches of a velocity scan of nv velocities on elements of esz bytes; max_batch > 0 caps them.
struct StoltScanPlan {
    size_t plane;           // one spectrum of the batch, in complex numbers: [hs][snum] on the rows route, [m][tnum] (then [tnum][m]) on the other; rocFFT: 0
    size_t iplane;          // one image, in reals
    size_t per;             // bytes per velocity: the spectrum twice (a transpose is out of place) and the image
    int B, batches;
};
static inline StoltScanPlan stolt_scan_plan(const StoltShape &s, size_t esz, int nv, int max_batch)
{
    StoltScanPlan p;
    p.plane = !s.use_own ? 0 : (s.route == STOLT_OWN_ROWS ? (size_t)s.hs * s.snum : (size_t)s.m * s.tnum);
    p.iplane = (size_t)s.nout * s.tnum;
    p.per = 2 * p.plane * 2 * esz + std::max(p.iplane, (size_t)1) * esz;
    p.B = (int)std::min<size_t>(std::max<size_t>(STOLT_SCAN_BUDGET_BYTES / p.per, 1), (size_t)std::min(nv, STOLT_SCAN_MAX_BATCH));
    if (max_batch > 0) p.B = std::min(p.B, max_batch);
    p.batches = (nv + p.B - 1) / p.B;
    return p;
}

// The kernel string of the metrics line, of a single call or of a scan.
static inline const char *stolt_kernel_label(const StoltShape &s, bool scan)
{
    if (s.route == STOLT_OWN_ROWS) {
        if (scan)
            return s.mixed ? "stolt_stretch_scan_rows (+ the library's own row transforms, traces first, mixed radix)"
                           : "stolt_stretch_scan_rows (+ the library's own row transforms, traces first)";
        return s.mixed ? "stolt_stretch_rows (+ the library's own row transforms, traces first, mixed radix)"
                       : "stolt_stretch_rows (+ the library's own row transforms, traces first)";
    }
    if (s.use_own) {
        if (scan)
            return s.mixed ? "stolt_stretch_scan_t (+ the library's own row transforms, mixed radix)"
                           : "stolt_stretch_scan_t (+ the library's own row transforms)";
        return s.mixed ? "stolt_stretch (+ the library's own row transforms, mixed radix)" : "stolt_stretch (+ the library's own row transforms)";
    }
    return scan ? "stolt_stretch (+ rocFFT 2-D real transforms, one velocity at a time)" : "stolt_stretch (+ rocFFT 2-D real transforms)";
}
