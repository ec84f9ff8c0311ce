// Predictive (gapped, Wiener-Levinson) deconvolution and trace autocorrelation of a (snum, tnum) radargram -- an extension: the
// reference has neither.  The contract, stated once; decon.hip, decon_kernels.h, decon_route.h, decon.py and the tests cite it.
// Plain C++ that g++ compiles by itself; the same functions are the device's (DECON_HD).
//
// One trace x[k], k = 0 .. snum - 1, is one column.  Design window [s0, s1), operator length n = oplen in 1 .. 256, prediction
// distance g = gap >= 1 (1: spiking deconvolution), prewhitening eps = prewhiten / 100 >= 0.  Everything is float64 for both
// data dtypes; every product-and-add below is one fma.
//
//   1. r[l] = sum_{k = s0}^{s1 - 1 - l} x[k] x[k + l] for the lags of the system, {0 .. n - 1} U {g .. g + n - 1} (DeconLags:
//      none between the two sets when g > n).  Order: the window is cut into blocks of DECON_C samples from s0; within a block
//      the terms are added in rising k to a sum that starts at +0; the block sums are added in rising order to a total that
//      starts at +0.  A term whose k + l >= s1 enters as x[k] * (+0).  The order is a function of (s0, s1) alone.
//   2. c[0] = r[0] (1 + eps), c[l] = r[l]; solve sum_i c[|m - i|] a[i] = r[g + m], m = 0 .. n - 1, by Levinson recursion
//      (decon_levinson_host below is the recursion; the device runs the same phases with DECON_G lanes per trace):
//        p = [1], v = c[0], a[0] = r[g] / v;  for m = 1 .. n - 1:
//          d = sum_{i < m} p[i] c[m - i],  e = sum_{i < m} a[i] c[m - i]          (decon_dot: DECON_G strided chains and a tree)
//          k = -d / v,  v' = fma(k, d, v),  p'[i] = fma(k, p[m - i], p[i]) for i = 0 .. m (p[m] = 0)
//          mu = (r[g + m] - e) / v',  a[i] = fma(mu, p'[m - i], a[i]) for i = 0 .. m (a[m] = 0)
//   3. y[k] = x[k] - S[k], S[k] = sum_{i = 0}^{n - 1} a[i] x[k - g - i] over the whole trace, the terms added in rising i to a sum
//      that starts at +0; samples before the trace's start are +0.
//   4. y is rounded to the data's dtype.
//
// Dead traces.  If r[0] is not finite or not > 0, or an error power v' of the recursion is not finite or not > 0, the trace is
// dead: it passes with its values and the positions of its NaNs unchanged and its operator is all zeros.  With eps = 0 and a
// degenerate trace (a constant, a pure exponential) v' is a difference of equal numbers and the second rule sits on rounding:
// such a trace may be dead on one evaluation and alive on another.  The tests decide the rule only on exactly dead traces --
// all zero, or a NaN or Inf inside the window.  Non-finite samples outside the window spread through step 3 as the
// convolution spreads them (0 * NaN = NaN included).
//
// design 'each' (0): every trace solves its own system.  design 'mean' (1): one operator from R[l] = sum_j r_j[l] over the
// traces whose r_j[0] is finite and > 0, added as sums over blocks of DECON_MEAN_BLOCK traces (a fixed tree, decon_kernels.h)
// which are then added in rising order; the solution does not depend on the scale of R, so nothing is divided.  A trace that
// is dead by the r[0] rule passes unchanged and reports a zero operator; if the mean system is dead, every trace does.
//
// Autocorrelogram: A[l][j] = r_j[l], l = 0 .. maxlag (the same sums as step 1 over the same blocks), (maxlag + 1, tnum)
// float64; normalised, it is divided by r_j[0], and a column whose r_j[0] is not finite or not > 0 is all NaN.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DECON_HD __host__ __device__ __forceinline__
#else
#define DECON_HD static inline
#endif

constexpr int DECON_MAX_OPLEN = 256;
constexpr int DECON_C = 64;            // samples per block, of the sums of step 1 and of the tiles of both sliding kernels
constexpr int DECON_G = 16;            // lanes per trace of the recursion: coefficient i belongs to lane i % DECON_G
constexpr int DECON_MEAN_BLOCK = 256;  // traces per block of the design 'mean' sum
enum { DECON_EACH = 0, DECON_MEAN = 1 };

// The lag table of a call has one row per lag: rows 0 .. n0 - 1 are the lags 0 .. n0 - 1, rows n0 .. n0 + n1 - 1 the lags
// b1 .. b1 + n1 - 1.  Deconvolution: n0 = n, b1 = max(g, n), n1 = min(g, n) -- no lag twice, none of the gap's when g > n.
// The autocorrelogram: n0 = maxlag + 1, n1 = 0.
struct DeconLags {
    int n0, n1, b1;
};
DECON_HD DeconLags decon_lags(int n, int g)
{
    DeconLags L;
    L.n0 = n;
    L.b1 = g > n ? g : n;
    L.n1 = g < n ? g : n;
    return L;
}
DECON_HD int decon_lag_count(const DeconLags &L) { return L.n0 + L.n1; }
// the row of lag l (l in one of the two runs)
DECON_HD int decon_lag_row(const DeconLags &L, int l) { return l < L.n0 ? l : L.n0 + (l - L.b1); }
// the lag of row j
DECON_HD int decon_row_lag(const DeconLags &L, int j) { return j < L.n0 ? j : L.b1 + (j - L.n0); }

// The rows are taken in chunks of at most DECON_C consecutive lags that do not straddle the two runs: chunk q of
// decon_chunk_count covers `count` rows from `row0`, whose lags start at `lag0`.  The taps of step 3 are cut the same way
// (one run of n).
struct DeconChunk {
    int row0, lag0, count;
};
DECON_HD int decon_chunk_count(const DeconLags &L) { return (L.n0 + DECON_C - 1) / DECON_C + (L.n1 + DECON_C - 1) / DECON_C; }
DECON_HD DeconChunk decon_chunk(const DeconLags &L, int q)
{
    const int q0 = (L.n0 + DECON_C - 1) / DECON_C;
    DeconChunk c;
    if (q < q0) {
        c.row0 = q * DECON_C;
        c.lag0 = c.row0;
        c.count = L.n0 - c.row0 < DECON_C ? L.n0 - c.row0 : DECON_C;
    } else {
        const int o = (q - q0) * DECON_C;
        c.row0 = L.n0 + o;
        c.lag0 = L.b1 + o;
        c.count = L.n1 - o < DECON_C ? L.n1 - o : DECON_C;
    }
    return c;
}

DECON_HD bool decon_power_ok(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

// Lane q's chain of the two sums of a step: the terms i = q, q + DECON_G, ... < m in rising i, each sum from +0.  Element i of
// a vector is at [i * st].
DECON_HD void decon_dot_lane(const double *p, const double *a, const double *c, int st, int m, int q, double &d, double &e)
{
    d = 0.0;
    e = 0.0;
    for (int i = q; i < m; i += DECON_G) {
        const double ci = c[(m - i) * st];
        d = fma(p[i * st], ci, d);
        e = fma(a[i * st], ci, e);
    }
}
// The tree over the DECON_G chains: s[q] += s[q ^ 8], then ^ 4, ^ 2, ^ 1 -- every lane ends with the same bits (the device
// does it with lane exchanges, decon_kernels.h).
DECON_HD double decon_tree_host(double *s)
{
    for (int o = DECON_G / 2; o > 0; o >>= 1) {
        double t[DECON_G];
        for (int q = 0; q < DECON_G; ++q) t[q] = s[q] + s[q ^ o];
        for (int q = 0; q < DECON_G; ++q) s[q] = t[q];
    }
    return s[0];
}
// the scalars of a step; false: the error power left (0, inf)
DECON_HD bool decon_step(double d, double e, double rhs, double &v, double &k, double &mu)
{
    k = -d / v;
    v = fma(k, d, v);
    mu = (rhs - e) / v;
    return decon_power_ok(v);
}
DECON_HD double decon_p_next(const double *p, int st, int m, int i, double k) { return fma(k, p[(m - i) * st], p[i * st]); }
DECON_HD double decon_a_next(const double *a, const double *pn, int st, int m, int i, double mu) { return fma(mu, pn[(m - i) * st], a[i * st]); }

// The recursion on the host: c[0 .. n - 1] with the prewhitening in c[0], rhs[m] = r[g + m]; a[0 .. n - 1] out; work: 2 n
// doubles.  False (and a all zeros): a dead trace.
static inline bool decon_levinson_host(const double *c, const double *rhs, int n, double *a, double *work)
{
    double *p = work, *pn = work + n;
    for (int i = 0; i < n; ++i) a[i] = p[i] = pn[i] = 0.0;
    bool ok = decon_power_ok(c[0]);
    double v = c[0];
    p[0] = 1.0;
    a[0] = rhs[0] / v;
    for (int m = 1; m < n && ok; ++m) {
        double sd[DECON_G], se[DECON_G];
        for (int q = 0; q < DECON_G; ++q) decon_dot_lane(p, a, c, 1, m, q, sd[q], se[q]);
        const double d = decon_tree_host(sd), e = decon_tree_host(se);
        double k, mu;
        ok = decon_step(d, e, rhs[m], v, k, mu);
        for (int i = 0; i <= m; ++i) pn[i] = decon_p_next(p, 1, m, i, k);
        for (int i = 0; i <= m; ++i) a[i] = decon_a_next(a, pn, 1, m, i, mu);
        double *t = p;
        p = pn;
        pn = t;
    }
    if (!ok)
        for (int i = 0; i < n; ++i) a[i] = 0.0;
    return ok;
}
