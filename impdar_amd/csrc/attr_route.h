// Complex-trace attributes of a (snum, tnum) radargram (attr.hip; an extension: the reference has no Hilbert transform): the
// contract, every refusal with its reason, and the route -- which transform runs the traces, with what launch and how much
// scratch.  Plain C++, no HIP include: compiled into the library by attr.hip and, by itself with g++, into the CPU suite's
// checker (tests/test_attr_route.py).  attr.hip decides nothing that this header does not.
//
// THE CONTRACT.  For every trace x (a column; n = snum samples), float64 arithmetic for both dtypes:
//   1. quadrature  X = rfft(x);  Y[k] = -i X[k] for 0 < k < n / 2, Y[0] = 0, Y[n / 2] = 0 when n is even (for odd n the index
//      (n - 1) / 2 takes the -i factor);  q = irfft(Y, n) -- imag(scipy.signal.hilbert(x)).  x itself is never transformed
//      back: the real part of the analytic signal z = x + i q is the data bit for bit.  n = 1 and n = 2 give q = 0.
//   2. kind 0 quadrature  q[k]
//      kind 1 envelope    e[k] = hypot(x[k], q[k])
//      kind 2 phase       atan2(q[k], x[k])  (radians)
//      kind 3 frequency   f[k] = arg(z[k + 1] conj z[k]) / (2 pi dt) = atan2(q[k+1] x[k] - x[k+1] q[k], x[k+1] x[k] + q[k+1] q[k])
//                         / (2 pi dt) for k < n - 1 (Hz), f[n - 1] = f[n - 2], f = 0 for n = 1.  smooth = 1: f as it is.
//                         smooth = W > 1 (odd, <= 255): f_W[k] = (sum_j w[j] f[j]) / (sum_j w[j]), w[j] = x[j]^2 + q[j]^2, both sums
//                         over |j - k| <= (W - 1) / 2 clipped to the trace with j rising; 0 where the denominator is 0.
//   3. the result is rounded once to the radargram's dtype.
//   4. a trace holding any sample that is not finite is NaN in every output sample of every kind -- decided by a reduction
//      over the trace before its transform, not by what a transform makes of an Inf.
//   5. a trace that is all zero gives zeros (decided by the same reduction).
//   6. refused before any device work (IMPDAR_ERR_ARG, the reason below): an unknown kind; smooth even or outside 1 .. 255;
//      smooth > 1 with a kind other than frequency; dt not finite or not positive (frequency only); an empty radargram;
//      another dtype.
// Every output sample is one chain of operations in an order fixed by n, kind and W alone -- no floating-point atomics -- so
// two calls give the same bits, and on the own-transform routes a trace gives the bits it gives alone.
//
// THE ROUTE is spec_route.h's for tnum rows of length n: own transforms in LDS (n even, n / 2 a power of two or 2 3 5 7-smooth
// in 16 .. 8192) -- one kernel per call, the spectrum and q never leave LDS -- or rocFFT (every other length): a real-forward
// plan, the multiply, a real-inverse plan, the attribute kernel.  n <= 2 needs no transform at all (q = 0).  Either way the
// columns are transposed into [tnum][n] float64 rows first and the attribute rows are transposed back with the rounding.
#pragma once
#include "spec_route.h"

enum { ATTR_QUADRATURE = 0, ATTR_ENVELOPE = 1, ATTR_PHASE = 2, ATTR_FREQUENCY = 3 };
enum {
    ATTR_MAX_SMOOTH = 255,
    ATTR_GLOBAL_THREADS = 256       // the rocFFT route's kernels: one workgroup of so many threads per trace
};

// samples pairs (x[2 m], x[2 m + 1]) a thread of the own-transform kernel holds at most: ceil(M / threads) -- M <= 1023 on 64
// threads, M <= 8 threads on the larger workgroups (spec_row_threads)
constexpr int attr_row_acc(int threads) { return threads == 64 ? 16 : 8; }

static inline bool attr_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

// Null for a call the entries take, else what is wrong with it.
static inline const char *attr_refusal(int snum, int tnum, int kind, int smooth, double dt)
{
    if (kind < ATTR_QUADRATURE || kind > ATTR_FREQUENCY) return "kind must be 0 (quadrature), 1 (envelope), 2 (phase) or 3 (frequency)";
    if (smooth < 1 || smooth > ATTR_MAX_SMOOTH || smooth % 2 == 0) return "smooth must be odd and lie in 1 .. 255";
    if (smooth > 1 && kind != ATTR_FREQUENCY) return "smooth above 1 goes with kind 3 (frequency) alone";
    if (kind == ATTR_FREQUENCY && !(attr_finite(dt) && dt > 0.0)) return "dt must be finite and positive";
    if (snum < 1 || tnum < 1) return "empty radargram";
    return nullptr;
}

struct AttrRoute {
    SpecRoute spec;                 // the transform, threads, workgroups, rows per workgroup and LDS of the row kernel
    int trivial = 0;                // n <= 2: q = 0, no transform
    long long tiles_x = 0, tiles_y = 0;     // the transposes' SPEC_TILE x SPEC_TILE tiles over (snum, tnum)
    size_t out_pitch = 0;           // doubles between the attribute rows the transpose back reads
    // scratch, in doubles: the [tnum][n] rows (x on the way in; on the own routes the attribute on the way out), and on the
    // rocFFT route the [tnum][n / 2 + 1] complex spectrum (afterwards the attribute rows, pitch 2 (n / 2 + 1)) and the
    // [tnum][n] quadrature; one int per trace for the reduction of rule 4 and 5
    size_t rowbuf_doubles = 0, spectrum_doubles = 0, quad_doubles = 0, flag_ints = 0;
    const char *label = "";
    bool ok = false;
};

// smooth > 1 on the rocFFT route writes its result over the x rows (the spectrum rows hold w f, the quadrature rows w)
static inline AttrRoute attr_route(int snum, int tnum, int kind, int smooth)
{
    AttrRoute A;
    A.spec = spec_route(snum, tnum);
    if (!A.spec.ok) return A;
    const SpecRoute &R = A.spec;
    A.trivial = snum <= 2;
    A.tiles_x = ((long long)tnum + SPEC_TILE - 1) / SPEC_TILE;
    A.tiles_y = ((long long)snum + SPEC_TILE - 1) / SPEC_TILE;
    if (A.tiles_x * A.tiles_y >= (1LL << 31)) return A;
    A.rowbuf_doubles = R.rowbuf_doubles;
    if (R.kind == SPEC_ROCFFT) {
        A.spectrum_doubles = R.spectrum_doubles;
        A.quad_doubles = R.rowbuf_doubles;
        A.flag_ints = (size_t)tnum;
        A.out_pitch = kind == ATTR_FREQUENCY && smooth > 1 ? (size_t)snum : 2 * (size_t)R.bins;
        A.label = A.trivial ? "attr_global_kernel" : "rocFFT forward + attr_multiply_kernel + rocFFT inverse + attr_global_kernel";
    } else {
        A.out_pitch = (size_t)snum;
        A.label = R.kind == SPEC_OWN_MIXED ? "attr_rows_kernel (mixed radix)" : "attr_rows_kernel (radix 4)";
    }
    A.ok = true;
    return A;
}

#ifdef ATTR_ROUTE_PROBE
// what tests/test_attr_route.py calls.  ints[8]: kind of route, M, threads, trivial, ok, pairs a thread holds, (spare);
// longs[10]: workgroups, rows_per_wg, lds, rowbuf, spectrum, quad, flags, out_pitch, tiles_x, tiles_y
extern "C" const char *attr_probe_refusal(int snum, int tnum, int kind, int smooth, double dt) { return attr_refusal(snum, tnum, kind, smooth, dt); }
extern "C" const char *attr_probe_route(int snum, int tnum, int kind, int smooth, int *ints, long long *longs)
{
    const AttrRoute A = attr_route(snum, tnum, kind, smooth);
    const SpecRoute &R = A.spec;
    const int i[8] = {R.kind, R.M, R.threads, A.trivial, A.ok ? 1 : 0, R.kind == SPEC_ROCFFT ? 0 : attr_row_acc(R.threads), 0, 0};
    const long long l[10] = {R.workgroups, R.rows_per_wg, (long long)R.lds, (long long)A.rowbuf_doubles, (long long)A.spectrum_doubles,
                             (long long)A.quad_doubles, (long long)A.flag_ints, (long long)A.out_pitch, A.tiles_x, A.tiles_y};
    for (int k = 0; k < 8; ++k) ints[k] = i[k];
    for (int k = 0; k < 10; ++k) longs[k] = l[k];
    return A.label;
}
#endif
