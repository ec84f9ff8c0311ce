// The kernels of the layer-slope steps (slope.hip): the row pass (products and their Gaussian along the traces), the column
// pass (the Gaussian along the samples and the 2 x 2 eigen-analysis) and the gather of the dip-steered mean.  The contract and
// every size are slope_route.h's.  Every index into the radargram, the planes and the slope field is clamped or guarded.
#pragma once
#include "common.h"
#include "slope_route.h"

__device__ __forceinline__ double slope_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// rule 1: a sample that is not finite is read as NaN
template <typename T> __device__ __forceinline__ double slope_load(const T *x, size_t at)
{
    const double v = (double)x[at];
    return fabs(v) <= 1.7976931348623157e308 ? v : slope_nan();
}

// rule 2 along one axis: `at` the sample's offset, `i` its index on the axis, `len` the axis' length, `step` between neighbours
template <typename T> __device__ __forceinline__ double slope_grad(const T *x, size_t at, int i, int len, size_t step)
{
    if (len == 1) return 0.0;
    if (i == 0) return slope_load(x, at + step) - slope_load(x, at);
    if (i == len - 1) return slope_load(x, at) - slope_load(x, at - step);
    return (slope_load(x, at + step) - slope_load(x, at - step)) / 2.0;
}

// Rule 4's accumulation: (hi, lo) <- (hi, lo) + w v with the product taken exactly (its rounding error from one fused
// multiply-add) and the sum's rounding error kept (Knuth's two-sum); the pass returns hi + lo, rounded once.
__device__ __forceinline__ void slope_acc(double &hi, double &lo, double w, double v)
{
    const double p = w * v, pe = fma(w, v, -p);
    const double s = hi + p, t = s - hi, se = (hi - (s - t)) + (p - t);
    hi = s;
    lo = lo + (se + pe);
}

// Row pass.  Workgroup b: row k = b / bx, traces j0 = (b % bx) SLOPE_ROW_TX onwards.  LDS: three rows of W = SLOPE_ROW_TX + 2 rx
// products, the one at position p that of the clamped trace index j0 - rx + p.
template <typename T>
__global__ __launch_bounds__(SLOPE_ROW_TX) void slope_row_kernel(const T *__restrict__ x, int n, int m, int rx, const double *__restrict__ wx,
                                                                 long long bx, double *__restrict__ pa, double *__restrict__ pb,
                                                                 double *__restrict__ pc)
{
    extern __shared__ double slope_lds[];
    const int W = SLOPE_ROW_TX + 2 * rx;
    double *A = slope_lds, *B = slope_lds + W, *Cx = slope_lds + 2 * W;
    const long long b = blockIdx.x;
    const int k = (int)(b / bx), j0 = (int)(b % bx) * SLOPE_ROW_TX;
    if (k >= n) return;
    for (int p = threadIdx.x; p < W; p += SLOPE_ROW_TX) {
        int j = j0 - rx + p;
        j = j < 0 ? 0 : (j > m - 1 ? m - 1 : j);
        const size_t at = (size_t)k * (size_t)m + (size_t)j;
        const double gz = slope_grad(x, at, k, n, (size_t)m), gx = slope_grad(x, at, j, m, (size_t)1);
        A[p] = gz * gz;
        B[p] = gz * gx;
        Cx[p] = gx * gx;
    }
    __syncthreads();
    const int j = j0 + (int)threadIdx.x;
    if (j >= m) return;
    double a = 0.0, bb = 0.0, c = 0.0, al = 0.0, bl = 0.0, cl = 0.0;
    for (int i = 0; i <= 2 * rx; ++i) {
        const double w = wx[i];
        slope_acc(a, al, w, A[threadIdx.x + i]);
        slope_acc(bb, bl, w, B[threadIdx.x + i]);
        slope_acc(c, cl, w, Cx[threadIdx.x + i]);
    }
    const size_t at = (size_t)k * (size_t)m + (size_t)j;
    pa[at] = a + al;
    pb[at] = bb + bl;
    pc[at] = c + cl;
}

// rule 5
__device__ __forceinline__ double slope_field(int kind, double a, double b, double c, double max_slope)
{
    if (kind == SLOPE_KIND_JZZ) return a;
    if (kind == SLOPE_KIND_JZX) return b;
    if (kind == SLOPE_KIND_JXX) return c;
    const double d = a - c, D = sqrt(d * d + 4.0 * b * b);
    if (kind == SLOPE_KIND_DIP) return 0.5 * atan2(-2.0 * b, d);
    if (kind == SLOPE_KIND_COHERENCE) {
        const double s = a + c;
        if (s > 0.0) return D / s;
        return (s != s || D != D) ? slope_nan() : 0.0;         // (s > 0 is false for a NaN: say it)
    }
    double p;
    if (D == 0.0) p = 0.0;
    else if (d >= 0.0) p = -2.0 * b / (d + D);
    else p = -(D - d) / (2.0 * b);                              // (a NaN d or D comes here and stays NaN)
    return p > max_slope ? max_slope : (p < -max_slope ? -max_slope : p);       // (the comparisons keep a NaN)
}

// Column pass.  Workgroup b: tile row b / bx, tile column b % bx.  Thread (tx, ty) = (t % SLOPE_COL_TX, t / SLOPE_COL_TX) owns
// the samples k0 + q SLOPE_COL_GROUPS + ty, q = 0 .. SLOPE_COL_PER_THREAD - 1, of trace j0 + tx.  LDS: (SLOPE_COL_SEG + 2 rz) rows
// of SLOPE_COL_TX doubles, row `row` that of the clamped sample index k0 - rz + row; one plane at a time.
__global__ __launch_bounds__(SLOPE_COL_THREADS) void slope_col_kernel(const double *__restrict__ pa, const double *__restrict__ pb,
                                                                      const double *__restrict__ pc, int n, int m, int rz,
                                                                      const double *__restrict__ wz, long long bx, int kind, double max_slope,
                                                                      double *__restrict__ out)
{
    extern __shared__ double slope_lds[];
    const long long b = blockIdx.x;
    const int k0 = (int)(b / bx) * SLOPE_COL_SEG, j0 = (int)(b % bx) * SLOPE_COL_TX;
    const int tx = (int)threadIdx.x % SLOPE_COL_TX, ty = (int)threadIdx.x / SLOPE_COL_TX;
    const int j = j0 + tx, H = SLOPE_COL_SEG + 2 * rz;
    double acc[3][SLOPE_COL_PER_THREAD];
    const double *planes[3] = {pa, pb, pc};
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        __syncthreads();
        for (int row = ty; row < H; row += SLOPE_COL_GROUPS) {
            int kk = k0 - rz + row;
            kk = kk < 0 ? 0 : (kk > n - 1 ? n - 1 : kk);
            slope_lds[row * SLOPE_COL_TX + tx] = j < m ? planes[pl][(size_t)kk * (size_t)m + (size_t)j] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SLOPE_COL_PER_THREAD; ++q) {
            const int kl = q * SLOPE_COL_GROUPS + ty;
            double s = 0.0, sl = 0.0;
            for (int i = 0; i <= 2 * rz; ++i) slope_acc(s, sl, wz[i], slope_lds[(kl + i) * SLOPE_COL_TX + tx]);
            acc[pl][q] = s + sl;
        }
    }
    if (j >= m) return;
#pragma unroll
    for (int q = 0; q < SLOPE_COL_PER_THREAD; ++q) {
        const int k = k0 + q * SLOPE_COL_GROUPS + ty;
        if (k < n) out[(size_t)k * (size_t)m + (size_t)j] = slope_field(kind, acc[0][q], acc[1][q], acc[2][q], max_slope);
    }
}

// Rule 6: one output sample per thread; y must not be x (slope.hip gathers an in-place call into scratch).
template <typename T>
__global__ __launch_bounds__(SLOPE_GATHER_THREADS) void slope_gather_kernel(const T *__restrict__ x, const double *__restrict__ slope, int n, int m,
                                                                            int half, T *__restrict__ y)
{
    const size_t at = (size_t)blockIdx.x * SLOPE_GATHER_THREADS + threadIdx.x, count = (size_t)n * (size_t)m;
    if (at >= count) return;
    const int k = (int)(at / (size_t)m), j = (int)(at % (size_t)m);
    const double p = slope[at];
    if (p != p) {               // (fmin / fmax below would drop it)
        y[at] = (T)slope_nan();
        return;
    }
    const int lo = j - half < 0 ? -j : -half, hi = j + half > m - 1 ? m - 1 - j : half;
    const double top = (double)(n - 1);
    double sum = 0.0;
    for (int i = lo; i <= hi; ++i) {
        double s = (double)k + p * (double)i;
        if (s != s) s = slope_nan();                            // (an infinite p at i = 0)
        else s = s < 0.0 ? 0.0 : (s > top ? top : s);
        double v;
        if (s != s) {
            v = s;
        } else {
            const int ka = (int)floor(s), kb = ka + 1 > n - 1 ? n - 1 : ka + 1;
            const double f = s - (double)ka;
            const double xa = slope_load(x, (size_t)ka * (size_t)m + (size_t)(j + i)), xb = slope_load(x, (size_t)kb * (size_t)m + (size_t)(j + i));
            v = xa + f * (xb - xa);
        }
        sum = sum + v;
    }
    y[at] = (T)(sum / (double)(hi - lo + 1));
}
