// The host-side route of the spectra (spectrum.hip): for `rows` real sequences of length n, which transform runs them and
// with what launch -- plain C++, no HIP include, compiled by itself in tests/test_spec_route.py.  spectrum.hip decides
// nothing that this header does not.
//
// A row of n reals is M = n / 2 complex numbers for the library's own transforms (own_fft.h): a power-of-two M takes the
// radix-4 passes, any other 2 3 5 7-smooth M the mixed-radix passes, both for 16 <= M <= 8192.  Every other length -- odd n,
// M < 16, M > 8192, a prime factor above 7 -- goes through a rocFFT plan into a [rows][n / 2 + 1] spectrum; n = 1 is its
// own transform and needs no plan.
//
// The rows are cut into contiguous blocks in row order, one per workgroup: block w holds rows [w rows_per_wg,
// min(rows, (w + 1) rows_per_wg)), and no block is empty.
#pragma once
#include <cstddef>
#include "own_fft_len.h"
#include "own_fft_mixed_plan.h"

enum { SPEC_OWN_POW2 = 0, SPEC_OWN_MIXED = 1, SPEC_ROCFFT = 2 };
enum {
    SPEC_CUS = 256,                 // compute units of an MI355X
    SPEC_LDS_MAX = 160 * 1024,      // LDS of one
    SPEC_CU_THREADS = 2048,
    SPEC_MAX_ACC = 16,              // bins a thread of spec_rows_kernel accumulates at most: ceil((M + 1) / threads), spec_row_acc
    SPEC_POWER_THREADS = 256,       // spec_power_kernel: one thread per bin
    SPEC_POWER_BLOCKS = 1024,       // ... and at most so many blocks of rows
    SPEC_TILE = 32                  // the transposes' tile (pitch SPEC_TILE + 1)
};

// own_fft.h's own_pad: where complex number i of a row sits in LDS
constexpr int spec_pad(int i) { return i + (i >> 5); }

struct SpecRoute {
    int kind = SPEC_ROCFFT;
    int n = 0, M = 0, logm = 0, bins = 0;
    int identity = 0;               // n == 1: the spectrum is the sample
    int threads = 0;
    long long rows = 0, workgroups = 0, rows_per_wg = 0;
    size_t lds = 0;                 // dynamic LDS of spec_rows_kernel (0 on the rocFFT route)
    size_t partial_doubles = 0;     // [workgroups][bins], the mean spectra's partial sums
    size_t rowbuf_doubles = 0;      // [rows][n] float64: the transposed / widened / windowed rows, where the route needs them
    size_t spectrum_doubles = 0;    // [rows][bins] complex, the rocFFT route's spectrum
    size_t image_doubles = 0;       // [rows][bins], the periodogram before its transpose
    bool ok = false;
};

// threads of a row of M complex doubles: own_fft_launch's
static inline int spec_row_threads(int M) { return M >= 4096 ? 1024 : (M >= 2048 ? 512 : (M >= 1024 ? 256 : 64)); }

// ... and the bins one of them accumulates at most: M <= 1023 on 64 threads, M + 1 <= 8 threads + 1 on the larger workgroups
constexpr int spec_row_acc(int threads) { return threads == 64 ? SPEC_MAX_ACC : 9; }

static inline SpecRoute spec_route(int n, long long rows)
{
    SpecRoute R;
    if (n < 1 || rows < 1) return R;
    R.n = n;
    R.rows = rows;
    R.bins = n / 2 + 1;
    R.M = n / 2;
    const bool even = n % 2 == 0;
    if (even && own_fft_len_ok(R.M)) R.kind = SPEC_OWN_POW2;
    else if (even && own_fft_mixed_len_ok(R.M)) R.kind = SPEC_OWN_MIXED;
    else R.kind = SPEC_ROCFFT;
    long long most;
    if (R.kind == SPEC_ROCFFT) {
        R.identity = n == 1;
        R.threads = SPEC_POWER_THREADS;
        R.lds = 0;
        most = SPEC_POWER_BLOCKS;
        R.spectrum_doubles = 2 * (size_t)rows * (size_t)R.bins;
    } else {
        while ((1 << R.logm) < R.M) ++R.logm;
        R.threads = spec_row_threads(R.M);
        // the row, one spare slot, and the tree of the mean
        R.lds = (size_t)(spec_pad(R.M) + 1) * 2 * sizeof(double) + (size_t)R.threads * sizeof(double);
        long long per_cu = (long long)(SPEC_LDS_MAX / R.lds);
        if (per_cu > SPEC_CU_THREADS / R.threads) per_cu = SPEC_CU_THREADS / R.threads;
        if (per_cu > 8) per_cu = 8;
        if (per_cu < 1) per_cu = 1;
        most = SPEC_CUS * per_cu;
        if ((R.M + 1 + R.threads - 1) / R.threads > spec_row_acc(R.threads) || R.lds > (size_t)SPEC_LDS_MAX) return R;
    }
    const long long wg = rows < most ? rows : most;
    R.rows_per_wg = (rows + wg - 1) / wg;
    R.workgroups = (rows + R.rows_per_wg - 1) / R.rows_per_wg;
    R.partial_doubles = (size_t)R.workgroups * (size_t)R.bins;
    R.rowbuf_doubles = (size_t)rows * (size_t)n;
    R.image_doubles = (size_t)rows * (size_t)R.bins;
    R.ok = true;
    return R;
}

#ifdef SPEC_ROUTE_PROBE
// what tests/test_spec_route.py calls.  ints[8]: kind, M, logm, bins, identity, threads, ok, (spare); longs[8]: workgroups,
// rows_per_wg, lds, partial, rowbuf, spectrum, image, (spare)
extern "C" int impdar_spec_route_full_probe(int n, long long rows, int *ints, long long *longs)
{
    const SpecRoute R = spec_route(n, rows);
    const int i[8] = {R.kind, R.M, R.logm, R.bins, R.identity, R.threads, R.ok ? 1 : 0, 0};
    const long long l[8] = {R.workgroups, R.rows_per_wg, (long long)R.lds, (long long)R.partial_doubles, (long long)R.rowbuf_doubles,
                            (long long)R.spectrum_doubles, (long long)R.image_doubles, 0};
    for (int k = 0; k < 8; ++k) {
        ints[k] = i[k];
        longs[k] = l[k];
    }
    return R.ok ? 0 : 1;
}
#endif
