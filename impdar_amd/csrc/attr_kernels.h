// The kernels of the complex-trace attributes (attr.hip); the contract and every launch argument are attr_route.h's.
//
//   attr_transpose_kernel  (snum, tnum) of the dtype -> [tnum][snum] float64 rows, and the attribute rows back with the rounding
//   attr_rows_kernel       the own-transform routes: a trace sits in LDS as n / 2 complex doubles through the forward passes,
//                          the real transform's split, the -i factor with its two zeros, the merge, the inverse passes and the
//                          attribute -- neither the spectrum nor q goes to memory
//   attr_flag_kernel, attr_multiply_kernel, attr_global_kernel
//                          the rocFFT route: the reduction of rules 4 and 5, Y = -i X between the two plans, and the same
//                          attribute arithmetic (attr_point, attr_freq, attr_window_sum) on x and q in memory
#pragma once
#include "common.h"
#include "own_fft.h"
#include "attr_route.h"

static_assert(spec_pad(31) == own_pad(31) && spec_pad(4097) == own_pad(4097) && spec_pad(8192) == own_pad(8192), "spec_route.h restates own_pad");

enum { ATTR_MODE_POINT = 0, ATTR_MODE_FREQ = 1, ATTR_MODE_SMOOTH = 2 };     // what a sample needs: itself, its successor, a window

// in: (rows, cols) of TI, rows in_pitch apart -> out: (cols, rows) of TO, rows out_pitch apart, through an LDS tile of odd
// pitch; the tiles at the ragged edges are range-checked.  One block per tile, tiles numbered row-major in blockIdx.x.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void attr_transpose_kernel(const TI *__restrict__ in, size_t in_pitch, TO *__restrict__ out, size_t out_pitch, int rows,
                                                             int cols, int tiles_x)
{
    __shared__ TO tile[SPEC_TILE][SPEC_TILE + 1];
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const int c0 = bx * SPEC_TILE, r0 = by * SPEC_TILE;
    const int tx = threadIdx.x % SPEC_TILE, ty = threadIdx.x / SPEC_TILE;
    for (int r = ty; r < SPEC_TILE; r += 256 / SPEC_TILE)
        if (r0 + r < rows && c0 + tx < cols) tile[r][tx] = (TO)in[(size_t)(r0 + r) * in_pitch + c0 + tx];
    __syncthreads();
    for (int c = ty; c < SPEC_TILE; c += 256 / SPEC_TILE)
        if (c0 + c < cols && r0 + tx < rows) out[(size_t)(c0 + c) * out_pitch + r0 + tx] = tile[tx][c];
}

// ---- the attribute arithmetic both routes share ---------------------------------------------------------------------------

__device__ __forceinline__ bool attr_dev_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// (attr_point and attr_freq stay out of line: inlined into the row kernel's unrolled epilogue, up to 32 copies of atan2 / hypot
// cost the 1024-thread kernels 190-360 bytes of scratch per lane and the others 30-60 registers)
__device__ __attribute__((noinline)) double attr_point(int kind, double x, double q)
{
    return kind == ATTR_ENVELOPE ? hypot(x, q) : (kind == ATTR_PHASE ? atan2(q, x) : q);
}
// arg(z1 conj z0) / tpd, tpd = 2 pi dt
__device__ __attribute__((noinline)) double attr_freq(double x0, double q0, double x1, double q1, double tpd)
{
    return atan2(q1 * x0 - x1 * q0, x1 * x0 + q1 * q0) / tpd;
}
__device__ __forceinline__ double attr_weight(double x, double q) { return x * x + q * q; }
// d[lo] + ... + d[hi], j rising, for the window of sample i clipped to [0, n)
__device__ __forceinline__ double attr_window_sum(const double *d, int i, int half, int n)
{
    const int lo = i - half < 0 ? 0 : i - half, hi = i + half > n - 1 ? n - 1 : i + half;
    double sum = 0.0;
    for (int j = lo; j <= hi; ++j) sum += d[j];
    return sum;
}
__device__ __forceinline__ double attr_weighted(double num, double den) { return den == 0.0 ? 0.0 : num / den; }

// ---- the own-transform routes ---------------------------------------------------------------------------------------------

template <bool MIXED, bool INV>
__device__ __forceinline__ void attr_passes(OCp<double> *s, int M, int logm, const OwnMixedPlan &pl, int tid, int nth, const OCp<double> *__restrict__ tw)
{
    if (MIXED) {
        for (int p = 0; p < pl.np; ++p) {
            switch (pl.radix[p]) {
            case 4: own_mixed_pass<double, 4, INV>(s, pl, p, tid, nth, tw, 2); break;
            case 2: own_mixed_pass<double, 2, INV>(s, pl, p, tid, nth, tw, 2); break;
            case 3: own_mixed_pass<double, 3, INV>(s, pl, p, tid, nth, tw, 2); break;
            case 5: own_mixed_pass<double, 5, INV>(s, pl, p, tid, nth, tw, 2); break;
            default: own_mixed_pass<double, 7, INV>(s, pl, p, tid, nth, tw, 2); break;
            }
        }
    } else {
        own_fft_passes<double, INV>(s, M, logm, tid, nth, tw, 2);
    }
}

// Workgroup w takes rows [w rows_per_wg, min(nrows, (w + 1) rows_per_wg)) of `rows` ([nrows][n = 2 M] float64) and replaces
// each by its attribute.  Thread t holds the pairs m = t + j NT, j < attr_row_acc(NT): samples 2 m and 2 m + 1.
//   Z = FFT_M(x[2m] + i x[2m+1]) is left at its digit-reversed positions.  With E = Z[k] + conj Z[M-k], D = Z[k] - conj Z[M-k]
//   and w = e^{-2 pi i k / n} the real transform is X[k] = (E - i w D) / 2 and conj X[M-k] = (E + i w D) / 2; Y = -i X on
//   0 < k < M with Y[0] = Y[M] = 0 merges (own_fft_rows' C2R load) to  Z'[k] = conj(w) E - w D,  Z'[0] = 0  -- through registers,
//   because Z'[k] belongs at position k and Z[k] sat elsewhere.  The inverse passes leave n (q[2m] + i q[2m+1]) at the
//   reversed position of m.
// MODE (ATTR_MODE_*); kind: ATTR_* for MODE 0; half = (W - 1) / 2; tpd = 2 pi dt; tw: e^{-2 pi i k / n}, k < n.
// LDS: own_pad(M) + 1 complex doubles (spec_route.h's lds); the window sums read it as n plain doubles.
template <bool MIXED, int MODE, int NT>
__global__ __launch_bounds__(NT) void attr_rows_kernel(double *rows, int M, int logm, const OwnMixedPlan pl, long long nrows, long long rows_per_wg,
                                                        const OCp<double> *__restrict__ tw, int kind, int half, double tpd)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char attr_lds[];
    OCp<double> *s = reinterpret_cast<OCp<double> *>(attr_lds);
    double *d = reinterpret_cast<double *>(attr_lds);
    constexpr int ACC = attr_row_acc(NT);
    const int tid = threadIdx.x, n = 2 * M;
    const double inv_n = 1.0 / (double)n;
    const long long r0 = (long long)blockIdx.x * rows_per_wg, r1 = r0 + rows_per_wg < nrows ? r0 + rows_per_wg : nrows;
    for (long long r = r0; r < r1; ++r) {
        OCp<double> *X = reinterpret_cast<OCp<double> *>(rows + (size_t)r * n);
        int bad = 0, live = 0;
#pragma unroll
        for (int j = 0; j < ACC; ++j) {
            const int m = tid + j * NT;
            if (m < M) {
                const OCp<double> v = X[m];
                bad |= !attr_dev_finite(v.x) || !attr_dev_finite(v.y);
                live |= v.x != 0.0 || v.y != 0.0;
                s[own_pad(m)] = v;
            }
        }
        bad = __syncthreads_or(bad);
        live = __syncthreads_or(live);
        if (bad || !live) {             // (the same for the whole workgroup)
            const double v = bad ? __longlong_as_double(0x7ff8000000000000LL) : 0.0;
#pragma unroll
            for (int j = 0; j < ACC; ++j) {
                const int m = tid + j * NT;
                if (m < M) X[m] = OCp<double>{v, v};
            }
            __syncthreads();            // (the next row overwrites the LDS)
            continue;
        }
        attr_passes<MIXED, false>(s, M, logm, pl, tid, NT, tw);
        {
            OCp<double> zp[ACC];
#pragma unroll
            for (int j = 0; j < ACC; ++j) {
                const int k = tid + j * NT;
                zp[j] = OCp<double>{0.0, 0.0};
                if (k > 0 && k < M) {
                    const int pz = MIXED ? own_mixed_pos(pl, k) : own_rev(k, M, logm), pm = MIXED ? own_mixed_pos(pl, M - k) : own_rev(M - k, M, logm);
                    const OCp<double> a = s[own_pad(pz)], b = own_conj(s[own_pad(pm)]), w = tw[k];
                    zp[j] = own_sub(own_mul(own_conj(w), own_add(a, b)), own_mul(w, own_sub(a, b)));
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < ACC; ++j) {
                const int k = tid + j * NT;
                if (k < M) s[own_pad(k)] = zp[j];
            }
            __syncthreads();
        }
        attr_passes<MIXED, true>(s, M, logm, pl, tid, NT, tw);
        double o[ACC][2], wt[MODE == ATTR_MODE_SMOOTH ? ACC : 1][2];
#pragma unroll
        for (int j = 0; j < ACC; ++j) {
            const int m = tid + j * NT;
            if (m < M) {
                const OCp<double> v = s[own_pad(MIXED ? own_mixed_pos(pl, m) : own_rev(m, M, logm))], x = X[m];
                const double q0 = v.x * inv_n, q1 = v.y * inv_n;
                if constexpr (MODE == ATTR_MODE_POINT) {
                    o[j][0] = attr_point(kind, x.x, q0);
                    o[j][1] = attr_point(kind, x.y, q1);
                } else {
                    const double f0 = attr_freq(x.x, q0, x.y, q1, tpd);
                    double f1 = f0;         // (sample n - 1 repeats f[n - 2])
                    if (m + 1 < M) {
                        const double q2 = s[own_pad(MIXED ? own_mixed_pos(pl, m + 1) : own_rev(m + 1, M, logm))].x * inv_n;
                        f1 = attr_freq(x.y, q1, rows[(size_t)r * n + 2 * m + 2], q2, tpd);
                    }
                    if constexpr (MODE == ATTR_MODE_SMOOTH) {
                        wt[j][0] = attr_weight(x.x, q0);
                        wt[j][1] = attr_weight(x.y, q1);
                        o[j][0] = wt[j][0] * f0;
                        o[j][1] = wt[j][1] * f1;
                    } else {
                        o[j][0] = f0;
                        o[j][1] = f1;
                    }
                }
            }
        }
        __syncthreads();                // every read of q and of a neighbour's x is done: the LDS and the row may be overwritten
        if constexpr (MODE == ATTR_MODE_SMOOTH) {
            double den[ACC][2];
#pragma unroll
            for (int j = 0; j < ACC; ++j) {
                const int m = tid + j * NT;
                if (m < M) {
                    d[2 * m] = wt[j][0];
                    d[2 * m + 1] = wt[j][1];
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < ACC; ++j) {
                const int m = tid + j * NT;
                if (m < M) {
                    den[j][0] = attr_window_sum(d, 2 * m, half, n);
                    den[j][1] = attr_window_sum(d, 2 * m + 1, half, n);
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < ACC; ++j) {
                const int m = tid + j * NT;
                if (m < M) {
                    d[2 * m] = o[j][0];
                    d[2 * m + 1] = o[j][1];
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < ACC; ++j) {
                const int m = tid + j * NT;
                if (m < M) {
                    o[j][0] = attr_weighted(attr_window_sum(d, 2 * m, half, n), den[j][0]);
                    o[j][1] = attr_weighted(attr_window_sum(d, 2 * m + 1, half, n), den[j][1]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < ACC; ++j) {
            const int m = tid + j * NT;
            if (m < M) X[m] = OCp<double>{o[j][0], o[j][1]};
        }
        __syncthreads();                // (the next row overwrites the LDS the window sums read)
    }
}

// ---- the rocFFT route -----------------------------------------------------------------------------------------------------

// flags[r] = 1 for a row of x holding a sample that is not finite, else 2 for a row with a sample that is not zero, else 0
__global__ __launch_bounds__(ATTR_GLOBAL_THREADS) void attr_flag_kernel(const double *__restrict__ x, int n, int *__restrict__ flags)
{
    const double *row = x + (size_t)blockIdx.x * n;
    int bad = 0, live = 0;
    for (int i = threadIdx.x; i < n; i += ATTR_GLOBAL_THREADS) {
        const double v = row[i];
        bad |= !attr_dev_finite(v);
        live |= v != 0.0;
    }
    bad = __syncthreads_or(bad);
    live = __syncthreads_or(live);
    if (threadIdx.x == 0) flags[blockIdx.x] = bad ? 1 : (live ? 2 : 0);
}

// spec: [rows][bins] complex, in place: Y[k] = -i X[k], Y[0] = 0 and, for even n, Y[n / 2] = 0
__global__ __launch_bounds__(256) void attr_multiply_kernel(OCp<double> *__restrict__ spec, int n, int bins, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % (size_t)bins);
        const OCp<double> v = spec[i];
        spec[i] = (k == 0 || (n % 2 == 0 && k == n / 2)) ? OCp<double>{0.0, 0.0} : OCp<double>{v.y, -v.x};
    }
}

// One workgroup per row r: x is [rows][n], q [rows][n] the unnormalised inverse transform (n times the quadrature: the plan
// carries no scale); the attribute goes to out + r out_pitch.  MODE 2 keeps w f in a + r a_pitch,
// then w over q's row, and `out` may be x itself (nothing reads x by then); for MODE 0 and 1 `out` is neither x nor q.
template <int MODE>
__global__ __launch_bounds__(ATTR_GLOBAL_THREADS) void attr_global_kernel(double *xr, double *qr, double *a_, size_t a_pitch, double *out, size_t out_pitch,
                                                                         int n, const int *__restrict__ flags, int kind, int half, double tpd)
{
    const size_t r = blockIdx.x;
    const double inv_n = 1.0 / (double)n;
    double *x = xr + r * n, *q = qr + r * n, *a = a_ + r * a_pitch, *o = out + r * out_pitch;
    const int tid = threadIdx.x, flag = flags[r];
    if (flag != 2) {
        const double v = flag == 1 ? __longlong_as_double(0x7ff8000000000000LL) : 0.0;
        for (int i = tid; i < n; i += ATTR_GLOBAL_THREADS) o[i] = v;
        return;
    }
    if (MODE == ATTR_MODE_POINT) {
        for (int i = tid; i < n; i += ATTR_GLOBAL_THREADS) o[i] = attr_point(kind, x[i], q[i] * inv_n);
        return;
    }
    for (int i = tid; i < n; i += ATTR_GLOBAL_THREADS) {
        const int k = i < n - 1 ? i : n - 2;          // (sample n - 1 repeats f[n - 2])
        const double f = n == 1 ? 0.0 : attr_freq(x[k], q[k] * inv_n, x[k + 1], q[k + 1] * inv_n, tpd);
        if (MODE == ATTR_MODE_SMOOTH) a[i] = attr_weight(x[i], q[i] * inv_n) * f;
        else o[i] = f;
    }
    if (MODE != ATTR_MODE_SMOOTH) return;
    __syncthreads();
    for (int i = tid; i < n; i += ATTR_GLOBAL_THREADS) q[i] = attr_weight(x[i], q[i] * inv_n);
    __syncthreads();
    for (int i = tid; i < n; i += ATTR_GLOBAL_THREADS) o[i] = attr_weighted(attr_window_sum(a, i, half, n), attr_window_sum(q, i, half, n));
}
