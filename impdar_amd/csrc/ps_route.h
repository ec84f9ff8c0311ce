// What the phase shift (ps_run, phaseshift.hip) decides on the host before and between its launches: the walk over the
// frequencies, the runs of constant velocity, the layout of the spectrum and the ORDER in which the frequency-sum kernels
// are tried.  Plain C++, no device code -- compiled into the library by phaseshift.hip and, by itself with g++, into the
// CPU suite's checker (tests/test_ps_route.py).  A path runner may still decline for reasons of its own (a non-uniform
// frequency axis, lists that overflow, no memory) and hand the call to the next attempt of the list.
#pragma once
#include "own_fft_len.h"
#include "ps_path_plan.h"      // PsMfmaRun, PM_SHORT, PN_SHORT, PN_NFMAX; the planners of the paths under the attempts
#include "ps_series_plan.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

// The knobs of a call.  Read per call, not cached: the tests flip them inside one process.
struct PsKnobs {
    // IMPDAR_PS_FFT=strided: the transforms over the traces / wavenumbers as rocFFT's strided plans on the arrays as they lie
    // (rounds 1-3a); default: transpose, contiguous plan, transpose (see ps_transpose_c).  rocfft: rocFFT's plans also where the
    // library's own row transforms apply; own: that default spelled out (tests that pin one)
    bool rows_form = true, no_own = false;
    bool hermitian = true;  // IMPDAR_PS_HERMITIAN=0: the reference's walk over all nt frequencies
    // IMPDAR_PS_MFMA: 0 the vector kernels only; 2 / 3 only ps_mfma_kernel / only ps_runs_kernel of the matrix-core paths (A/B
    // runs, tests); 6 only the transform path (ps_nufft.h) ahead of them, at any number of layers; 7 only the series path (ps_series.h)
    int mfma = 1;
    bool edge_overflow = false;     // IMPDAR_PS_TEST_EDGE_OVERFLOW (test hook): the matrix-core paths behave as if their boundary lists overflowed
};

static inline PsKnobs ps_knobs_read()
{
    const char *fe = getenv("IMPDAR_PS_FFT"), *he = getenv("IMPDAR_PS_HERMITIAN"), *me = getenv("IMPDAR_PS_MFMA");
    return PsKnobs{!(fe && strcmp(fe, "strided") == 0), fe && strcmp(fe, "rocfft") == 0, !(he && atoi(he) == 0), me ? atoi(me) : 1,
                   getenv("IMPDAR_PS_TEST_EDGE_OVERFLOW") != nullptr};
}

enum PsAttemptKind { PS_SERIES = 0, PS_NUFFT = 1, PS_RUNS = 2, PS_MFMA = 3, PS_SMOOTH = 4, PS_VECTOR = 5 };
struct PsAttempt {
    int kind;
    double alt;             // PS_SERIES: what would run otherwise, in ms (<= 0: see ps_series_run)
};

struct PsRoute {
    bool herm = false;                      // Hermitian walk (see ps_load_slot, ps_common.h): nf frequency slots per wavenumber, rows of fstride
    int nf = 0, fstride = 0;
    std::vector<int> k_zero;                // ... the wavenumbers with kx = 0 (the zero-frequency row propagates there)
    double w0 = 0.0;                        // what stands for the zero frequency (:400-402)
    std::vector<double> w, thr;             // the frequencies in slot order; (tau / tau_max)^2 per step (v(z))
    bool use_own = false;                   // the transforms run on the library's own row kernels (own_fft.h)
    std::vector<int> sched;                 // v(z): sched[i] = 1 where a run of constant velocity starts, then a bit per 16-step tile that holds a start
    std::vector<double> epsum;              // ... the float64 kernel's velocity noise per tile
    bool use_sched = false;                 // ... and whether the runs kernels of the vector path go by it
    std::vector<PsMfmaRun> runs;            // the runs (one for a constant velocity); cut short at a velocity that is not finite
    bool vfinite = true;                    // every velocity of a profile finite and non-zero
    int long_runs = 0;                      // runs longer than a smeared layer boundary (PM_SHORT)
    int long_runs_metric = 0;               // ... as the metrics line reports them
    bool nufft_first = false;               // the transform path's estimate beats the runs kernels' (read where use_sched holds)
    double nufft_ms = 0.0, runs_ms = 0.0;   // ... the two estimates (float32)
    bool kx_antisym = false;                // kx[k] == -kx[tnum - k] for 2k < tnum
    bool half_front = false;                // the transform over the traces first, k >= 0 with all frequencies (but for its device buffer)
    std::vector<PsAttempt> attempts;
};

// Hermitian walk: the radargram is real, so frequencies 1..nt/2-1 also stand for their mirror images.  Taken only when the
// axes are exactly antisymmetric and the replaced zero frequency is evanescent wherever kx != 0 (it always is for a physical
// geometry: |v kx / 2| >= v pi / (tnum dx) against 1e-10/dt); anything else -- and IMPDAR_PS_HERMITIAN=0 -- keeps the
// reference's walk over all nt frequencies.
static inline void ps_route_walk(PsRoute &R, int snum, int tnum, int nt, const double *kx, const double *ws, double vconst,
                                 const double *vmig, int vlen, const PsKnobs &K)
{
    bool herm = nt >= 4 && (nt & (nt - 1)) == 0 && ws[0] == 0.0 && K.hermitian;
    if (herm) {
        for (int i = 1; i < nt / 2 && herm; ++i) herm = std::isfinite(ws[i]) && ws[i] != 0.0 && ws[nt - i] == -ws[i];
        herm = herm && std::isfinite(ws[nt / 2]) && ws[nt / 2] != 0.0;
        double vmin = std::fabs(vconst);
        if (vlen) {
            vmin = std::fabs(vmig[0]);
            for (int i = 0; i < snum; ++i) {
                herm = herm && std::isfinite(vmig[i]);
                vmin = std::min(vmin, std::fabs(vmig[i]));
            }
        }
        herm = herm && std::isfinite(vmin) && std::isfinite(R.w0);
        for (int k = 0; k < tnum && herm; ++k) {
            // (the wavenumber Nyquist row of an even trace count is its own mirror image: only kx^2 enters)
            const int km = (tnum - k) % tnum;
            herm = std::isfinite(kx[k]) && (km == k || kx[km] == -kx[k]);
            if (kx[k] == 0.0) R.k_zero.push_back(k);
            else herm = herm && std::fabs(0.5 * vmin * kx[k]) > 2.0 * R.w0;     // w0 evanescent with a wide margin
        }
        herm = herm && R.k_zero.size() <= 4;
    }
    R.herm = herm;
    R.nf = herm ? nt / 2 : nt;
    R.fstride = herm ? nt / 2 + 1 : nt;
    if (herm) R.w[0] = ws[nt / 2];          // slot order: Nyquist first, then rows 1..nt/2-1 (already in place)
}

// Runs of constant velocity (ps_vz32_kernel): a step starts a new run when its velocity differs from the run's first by
// more than vtol (relative) -- 2*gradient(z(t)) of a layered table is constant inside a layer up to ~4e-13 of rounding
// noise, and a 1e-10 velocity error moves the phase by < 3e-6 rad over 8192 steps (float32: ignored; float64: vtol 1e-11
// and the deviation is carried along as a phase, ps_vz64_kernel).  Profiles that change at (nearly) every step keep the
// per-step kernels.
static inline void ps_route_runs(PsRoute &R, bool dbl, int snum, double vconst, const double *vmig, int vlen)
{
    if (!vlen) {
        R.runs.push_back(PsMfmaRun{vconst, 0, snum});
    } else {
        const double vtol = dbl ? 1e-11 : 1e-10;
        const int ntile = (snum + 15) / 16;
        R.sched.assign((size_t)snum + (ntile + 31) / 32, 0);
        R.epsum.assign(ntile, 0.0);
        double vrun = -1.0;
        int ndirty = 0;
        for (int i = 0; i < snum; ++i) {
            if (i == 0 || std::fabs(vmig[i] - vrun) > vtol * std::fabs(vmig[i])) {     // a run always starts at step 0
                const int tile = i / 16;
                const unsigned bit = 1u << (tile & 31);
                unsigned word;
                memcpy(&word, &R.sched[snum + tile / 32], sizeof word);
                R.sched[i] = 1;
                ndirty += (word & bit) ? 0 : 1;
                word |= bit;
                memcpy(&R.sched[snum + tile / 32], &word, sizeof word);
                vrun = vmig[i];
            }
            R.epsum[i / 16] += vmig[i] / vrun - 1.0;      // float64 kernel: the run's velocity noise, tile by tile
            R.vfinite = R.vfinite && std::isfinite(vmig[i]) && vmig[i] != 0.0;     // (NaN / inf entries: the per-step kernel)
        }
        bool ok = true;
        for (int i = 0; i < snum && ok; ++i) {          // (ends with the first velocity that is not finite)
            ok = std::isfinite(vmig[i]) && vmig[i] != 0.0;
            if (R.sched[i]) R.runs.push_back(PsMfmaRun{vmig[i], i, 0});
            R.runs.back().len += 1;
        }
        // the per-step tiles of the runs kernels cost several quiet tiles each: beyond a share of such tiles the
        // per-step kernel is faster for float32 (2048^2, 40 / 80 / 160 layers: 4.6 / 7.5 / 12.2 ms against
        // 5.5 / 6.8 / 9.5 ms); the float64 runs kernel stays ahead until every tile holds a change (10.1 / 16.6 /
        // 27.5 ms against 26.4 ms throughout: its per-step tiles pay the square root and sincos at the changes
        // only).  profiles/tools/ps_dirty.py.
        const double dirty_max = dbl ? 0.9 : 0.5;
        R.use_sched = R.vfinite && ((double)ndirty <= dirty_max * ntile || snum <= 64);
    }
    for (const PsMfmaRun &r : R.runs) R.long_runs += r.len > PM_SHORT;
}

// Will the transform path (ps_nufft_kernel) take a v(z) table?  Its cost is per PIECE (a run of constant velocity, cut at
// 4096 / 2048 steps) and per directly summed step of the short runs between them, and hardly depends on the record's length; the
// runs kernels' is per (frequency, step) plus a term per run.  Device ms per 8192 wavenumbers, pairs of wavenumbers per transform
// (profiles/r06_transforms.txt section 4: tables of 4 ... 41 rows at 8192^2, 4096^2, 2048^2):
//   float32  ps_nufft_kernel (0.135 + 0.06 nf/4096) (pieces + short steps / 3)     ps_runs_kernel 1.2 + 8.5 (nf/4096)(snum/8192) + 0.05 runs nf/4096
//   float64  up to 24 thick layers from 2048 frequencies on (33.6 against ps_vz64_kernel's 57.2 ms at 41 rows / 21 layers, 8192^2; level at
//            4096^2), 16 below
static inline void ps_route_estimate(PsRoute &R, bool dbl, int snum)
{
    int pieces = 0, nshort = 0;
    const int lmax = dbl ? 2048 : 4096;
    for (const PsMfmaRun &r : R.runs) {
        if (r.len > PN_SHORT) pieces += (r.len + lmax - 1) / lmax;
        else nshort += r.len;
    }
    const double fq = (double)R.nf / 4096.0;
    R.nufft_ms = (0.135 + 0.06 * fq) * ((double)pieces + (double)nshort / 3.0);
    R.runs_ms = 1.2 + 8.5 * fq * ((double)snum / 8192.0) + 0.05 * (double)R.runs.size() * fq;
    R.nufft_first = dbl ? R.long_runs <= (R.nf >= 2048 ? 24 : 16) : nshort <= 128 && R.nufft_ms <= R.runs_ms;
}

// The order of attempts.  (8192^2 device ms behind it --
//  ps_mfma_kernel against ps_runs_kernel, equal layers, profiles/r05_ps_runs.txt: ps_mfma_kernel 12.9 / 15.7 / 16.0 / 19.7 / 26.8 at
//  3 / 4 / 5 / 7 / 11 long runs -- and 10.8 on the config-5 table; ps_runs_kernel, two wavenumbers per workgroup, 11.8 / 11.9 / 12.4 /
//  12.8 / 13.8 at 3 / 4 / 5 / 7 / 11 long runs, 15.3 at 21, 21.3 at 42, 12.0 on the config-5 table;
//  the transform path, profiles/r05_ps_nufft.txt, at 3 / 5 / 7 / 11 / 16 / 21 long runs: 5.1 / 6.1 / 7.2 / 9.5 / 13.0 / 16.8 against
//  ps_runs_kernel's 11.8 / 12.4 / 12.8 / 13.7 / 14.4 / 15.3; config 5: 4.5 against ps_mfma_kernel's 10.6, constant velocity 3.0 against 6.8;
//  what the series path replaces, profiles/r06_series.txt -- float32: ps_smooth32_kernel 5.3e-6 ms per alive pair; ps_runs_kernel 8 ms +
//  0.036 per run, long or single step -- 41 / 81 / 161 table rows = 160 / 320 / 640 runs: 13.8 / 19.8 / 30.5 ms; a firn column's 1470: 70;
//  float64: ps_smooth_kernel 10.8e-6 ms per alive pair; ps_vz64_kernel 43 ms for the record + 0.09 per step that starts a run (4-row
//  table 43, 41 rows 56, a firn column's 1960 changing steps 226; 4096^2: 14 / 121 per 8192 wavenumbers).)
//   NUFFT   a constant velocity, or a table the estimate above gives it (6: any table with a schedule).  float64 tables: with the
//           runs' velocity noise as its first-order term (ps_nufft.h)
//   SERIES  any other v(z) profile -- a velocity that changes at every step, more than 64 runs (float32: ahead of NUFFT, the two
//           exclude each other; float64: after it) -- against `alt`
//   MFMA / RUNS (float32): up to 3 long runs ps_mfma_kernel first (64-step tiles, phases from a table), more ps_runs_kernel (8-step
//           tiles, phases generated in the kernel); whichever declines hands over to the other
//   SMOOTH  no runs of constant velocity to live on (the velocity changes in most 16-step tiles): ps_smooth_kernel
//   VECTOR  ps_dispatch (ps_direct.h): the runs kernels of the vector path with a schedule, else the per-step kernel.  Always last, never declines.
static inline void ps_route_attempts(PsRoute &R, bool dbl, int snum, double vconst, int vlen, const PsKnobs &K)
{
    const int pref = K.mfma;
    const bool vz = vlen != 0, sched = R.use_sched;
    const double fq = (double)R.nf / 4096.0, sq = (double)snum / 8192.0, nruns = (double)R.runs.size();
    // float32: every velocity of a profile finite and non-zero, and no test hook; float64 tests neither here (its conditions imply the first)
    const bool ok = dbl || !vz || R.vfinite, hook = !dbl && K.edge_overflow;
    const bool nufft = dbl ? (vz ? sched && (pref == 6 || (pref == 1 && R.nufft_first)) : pref != 0 && std::isfinite(vconst) && vconst != 0.0)
                           : ok && !hook && (pref == 6 || (pref == 1 && (!vz || (sched && R.nufft_first))));
    const bool series = vz && ok && !hook &&
                        (pref == 7 || (pref == 1 && (dbl || (!(sched && R.nufft_first) && (!sched || R.runs.size() > 64)))));
    const double alt = pref == 7 ? 0.0
                       : !sched  ? (dbl ? -SR_MS_PER_PAIR_F64 : -SR_MS_PER_PAIR_F32)
                       : dbl     ? 43.0 * fq * sq + 0.09 * nruns * fq
                                 : 8.0 * fq * sq + 0.036 * nruns * fq;
    if (series && !dbl) R.attempts.push_back(PsAttempt{PS_SERIES, alt});
    if (nufft) R.attempts.push_back(PsAttempt{PS_NUFFT, 0.0});
    if (series && dbl) R.attempts.push_back(PsAttempt{PS_SERIES, alt});
    if (!dbl && ok && pref != 0 && pref != 7) {
        const bool runs_first = vz && R.long_runs > 3;
        for (int turn = 0; turn < 2; ++turn) {
            if ((turn == 0) == runs_first) {
                if (pref != 2 && vz && !hook) R.attempts.push_back(PsAttempt{PS_RUNS, 0.0});
            } else if (pref != 3) {
                R.attempts.push_back(PsAttempt{PS_MFMA, 0.0});      // (declines through its own use of the hook)
            }
        }
    }
    if (vz && !sched) R.attempts.push_back(PsAttempt{PS_SMOOTH, 0.0});
    R.attempts.push_back(PsAttempt{PS_VECTOR, 0.0});
    R.long_runs_metric = !dbl || (vz && sched && (pref == 1 || pref == 6)) ? R.long_runs : 0;
}

// tk_out: a rank of a kx-sharded run (wavenumbers [k0, k0 + nk), the sums go to the caller, no inverse transform)
static inline PsRoute ps_route(bool dbl, int snum, int tnum, int nt, const double *kx, const double *ws, double dt, const double *tt_us,
                               double vconst, const double *vmig, int vlen, int k0, int nk, bool tk_out, const PsKnobs &K)
{
    PsRoute R;
    R.w0 = 1e-10 / dt;
    R.w.assign(ws, ws + nt);
    R.thr.assign(snum, 0.0);
    for (int i = 0; i < nt; ++i)
        if (R.w[i] == 0.0) R.w[i] = R.w0;                               // :400-402
    ps_route_walk(R, snum, tnum, nt, kx, ws, vconst, vmig, vlen, K);
    // Power-of-two sizes run their transforms on the library's own row kernels (own_fft.h), every call: nothing to compile,
    // no plan to make (rocFFT: 0.25-3 s per process, its kernels for lengths above 1024 are compiled at run time), and within
    // 0.1 ms of rocFFT's plans at 8192^2 since the long rows run 1024 threads (round 5; until then the first call of a size
    // only).  (Plans made on a thread during a first call: a process that exits while rocFFT is still compiling on
    // another thread crashes in its teardown -- rc -11 / -6 in 2 of 2 such exits, profiles/r05_first_call.txt.)
    R.use_own = R.herm && K.rows_form && !K.no_own && own_fft_len_ok(nt / 2) && own_fft_len_ok(tnum);
    if (vlen)
        for (int i = 0; i < snum; ++i) {
            const double tau = tt_us[i] / 1.0e6;                         // :441
            const double r = tau / tt_us[snum - 1] / 1e6;                // :484
            R.thr[i] = r * r;
        }
    ps_route_runs(R, dbl, snum, vconst, vmig, vlen);
    if (vlen) ps_route_estimate(R, dbl, snum);
    R.kx_antisym = true;
    for (int k = 1; 2 * k < tnum && R.kx_antisym; ++k) R.kx_antisym = kx[k] == -kx[tnum - k];
    // Which layout of the spectrum (P.fhalf).  When ps_nufft_kernel will take the call with a pair of wavenumbers per workgroup
    // (the whole axis, antisymmetric kx; a constant velocity or a table the estimate gives it -- the conditions of the attempts
    // that can be told before the transforms), the transform over the TRACES goes first, on the radargram's own rows with the
    // taper applied on their way in, and only the wavenumbers k = 0 .. tnum/2 are kept, with all frequencies:
    //   R2C over x [snum][tnum] -> [snum][tnum/2 + 1];  transpose (zero rows up to nt) -> [tnum/2 + 1][nt];  C2C over t in place
    // instead of taper + transpose, R2C over t, transpose, C2C over x, transpose: two passes over the array less.  The pair
    // (k, tnum - k) reads both of its rows out of row k (FK[tnum - k][w] = conj FK[k][-w]).  Should the kernel hand the call on
    // after all (boundary frequencies beyond its lists), the transforms are repeated in the other layout.
    R.half_front = R.herm && R.use_own && K.rows_form && !tk_out && k0 == 0 && nk == tnum && tnum % 2 == 0 && tnum >= 64 && own_fft_len_ok(nt) &&
                   R.nf >= 64 && R.nf <= PN_NFMAX && snum >= 64 && (K.mfma == 1 || K.mfma == 6) &&
                   !(R.k_zero.size() > 1 || (R.k_zero.size() == 1 && R.k_zero[0] != 0)) && R.kx_antisym &&
                   (vlen ? R.use_sched && (K.mfma == 6 || R.nufft_first) : std::isfinite(vconst) && vconst != 0.0);
    ps_route_attempts(R, dbl, snum, vconst, vlen, K);
    return R;
}

// Launch order of the runs kernels of the vector path.  A wavenumber that holds a frequency on the evanescent boundary of a
// run walks it in fp64 in every tile of that run (~2x the tile time); spread over the launch, the last such rows finish
// alone after everything else (2 ms at config 5).  They go first, longest first.  The test here only orders the launch --
// generous tolerance, the kernel decides for itself: |0.5 v kx| within 1e-7 of some |w|.  Empty: the natural order.
// (~2 ms of host time at config 5 with the GPU idle: made when those kernels are about to be launched, and kept by the caller.)
static inline std::vector<int> ps_row_order(const double *kx, int tnum, const double *ws, int nt, const std::vector<PsMfmaRun> &runs,
                                            double dt, bool dbl)
{
    std::vector<int> rowmap;
    if (runs.size() > 64 || tnum < 512) return rowmap;
    std::vector<double> aw(nt);
    for (int j = 0; j < nt; ++j) aw[j] = std::fabs(ws[j] == 0.0 ? 1e-10 / dt : ws[j]);
    std::sort(aw.begin(), aw.end());
    std::vector<std::pair<int, int>> score(tnum);      // (-steps spent walking, row)
    int flagged = 0;
    for (int k = 0; k < tnum; ++k) {
        int steps = 0;
        for (const PsMfmaRun &r : runs) {
            const double target = 0.5 * r.v * std::fabs(kx[k]);
            const auto it = std::lower_bound(aw.begin(), aw.end(), target);
            const double hi = it != aw.end() ? *it : aw.back(), lo = it != aw.begin() ? *(it - 1) : aw.front();
            const double band = dbl ? 2e-6 : 1e-7;
            if (std::fabs(hi - target) <= band * target || std::fabs(lo - target) <= band * target) steps += r.len;
        }
        score[k] = std::make_pair(-steps, k);
        flagged += steps > 0;
    }
    if (flagged > 0 && flagged < tnum) {
        std::stable_sort(score.begin(), score.end());
        rowmap.resize(tnum);
        for (int b = 0; b < tnum; ++b) rowmap[b] = score[b].second;
    }
    return rowmap;
}

#ifdef PS_ROUTE_PROBE
// the route as flat arrays (tests/test_ps_route.py compiles this header by itself).  fft: 0 default, 1 strided, 2 rocfft.
// ints[16]: herm, nf, fstride, zero wavenumbers, use_own, use_sched, runs, long_runs, long_runs_metric, nufft_first, kx_antisym,
// half_front, attempts, length of the row order (made when with_rows), vfinite; dbls[2]: the two estimates of nufft_first.
extern "C" int impdar_ps_route_probe(int dbl, int snum, int tnum, int nt, const double *kx, const double *ws, double dt, const double *tt_us,
                                     double vconst, const double *vmig, int vlen, int k0, int nk, int tk_out, int fft, int hermitian,
                                     int mfma, int edge_overflow, int with_rows, int *ints, double *dbls, int *k_zero /* [4] */,
                                     double *w /* [nt] */, int *attempt_kinds /* [8] */, double *attempt_alts /* [8] */, int *rowmap /* [tnum] */)
{
    const PsKnobs K{fft != 1, fft == 2, hermitian != 0, mfma, edge_overflow != 0};
    const PsRoute R = ps_route(dbl != 0, snum, tnum, nt, kx, ws, dt, tt_us, vconst, vmig, vlen, k0, nk, tk_out != 0, K);
    const std::vector<int> rows = with_rows ? ps_row_order(kx, tnum, ws, nt, R.runs, dt, dbl != 0) : std::vector<int>();
    const int I[15] = {R.herm, R.nf, R.fstride, (int)R.k_zero.size(), R.use_own, R.use_sched, (int)R.runs.size(), R.long_runs, R.long_runs_metric,
                       R.nufft_first, R.kx_antisym, R.half_front, (int)R.attempts.size(), (int)rows.size(), R.vfinite};
    if (R.attempts.size() > 8) return -1;
    std::copy(I, I + 15, ints);
    dbls[0] = R.nufft_ms;
    dbls[1] = R.runs_ms;
    std::copy(R.k_zero.begin(), R.k_zero.begin() + std::min<size_t>(R.k_zero.size(), 4), k_zero);
    std::copy(R.w.begin(), R.w.begin() + R.nf, w);
    std::copy(rows.begin(), rows.end(), rowmap);
    for (size_t i = 0; i < R.attempts.size(); ++i) {
        attempt_kinds[i] = R.attempts[i].kind;
        attempt_alts[i] = R.attempts[i].alt;
    }
    return 0;
}
#endif
