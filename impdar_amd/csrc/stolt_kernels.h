// The kernels of the Stolt path (stolt.hip launches them): taper / transposes of the real arrays, the stretch in its three
// layouts for one velocity and for a batch of them, the scan's focus sums.
#pragma once
#include "fft.h"            // impdar_taper_w

template <typename T> struct Cx { T x, y; };

// (snum,tnum) row-major -> tapered, transposed X[tnum][snum]
template <typename T>
__global__ __launch_bounds__(256) void stolt_taper_transpose(const T *__restrict__ in, T *__restrict__ X, int snum,
                                                             int tnum, double htaper, double vtaper, int do_taper)
{
    __shared__ T tile[64][65];
    const int k0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    // the trace weight is the thread's own for all of its rows; the 64 sample weights of the tile are computed once
    // (two float64 divisions per element were most of this kernel's time)
    __shared__ double wrow[64];
    if (threadIdx.x < 64) wrow[threadIdx.x] = impdar_taper_w(min(k0 + (int)threadIdx.x, snum - 1), snum, vtaper);
    const double h = impdar_taper_w(min(j0 + tx, tnum - 1), tnum, htaper);
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, j = j0 + tx;
        T v = 0;
        if (k < snum && j < tnum) {
            v = in[(size_t)k * tnum + j];
            if (do_taper) v = (T)(((double)v * h) * wrow[r]);      // (data*H)*V then astype(dtype), :157
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, k = k0 + tx;
        if (j < tnum && k < snum) X[(size_t)j * snum + k] = tile[tx][r];
    }
}

// Y[tnum][nout] -> out (nout,tnum) row-major
template <typename T>
__global__ __launch_bounds__(256) void stolt_transpose_back(const T *__restrict__ Y, T *__restrict__ out, int nout,
                                                            int tnum)
{
    __shared__ T tile[64][65];
    const int k0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, k = k0 + tx;
        tile[r][tx] = (j < tnum && k < nout) ? Y[(size_t)j * nout + k] : (T)0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, j = j0 + tx;
        if (k < nout && j < tnum) out[(size_t)k * tnum + j] = tile[tx][r];
    }
}

// The Stolt stretch of one output point (zj, |kx|): between which knots of the frequency axis it interpolates, with which
// weight, and its obliquity factor.  The one statement of this arithmetic: every stretch kernel below calls it.
struct StoltKnot {
    int i0;
    double w, sc;
};
__device__ __forceinline__ StoltKnot stolt_knot(const double *__restrict__ ws, double kxi, int zj, int m, double vel)
{
    const double kz = ws[zj] * 2.0 / vel;                       // :180
    const double kk = sqrt(kz * kz + kxi * kxi);                // :188 and :196 (kx^2 + kz^2: the same sum)
    double wq = vel / 2.0 * kk;
    const double wlast = ws[m - 1];
    if (wq > wlast) wq = wlast;                                 // FITPACK clamps to the last knot
    const double dw = ws[1] - ws[0];
    int i0 = (int)floor(wq / dw);
    i0 = min(max(i0, 0), m - 2);
    while (i0 > 0 && ws[i0] > wq) --i0;
    while (i0 < m - 2 && ws[i0 + 1] <= wq) ++i0;
    StoltKnot k;
    k.i0 = i0;
    k.w = (wq - ws[i0]) / (ws[i0 + 1] - ws[i0]);
    k.sc = kz / kk;                                             // :196
    return k;
}
// the interpolated value is stored into the (complex64/128) array, then scaled in place in double and rounded again (:190, :198)
template <typename T> __device__ __forceinline__ Cx<T> stolt_mix(const Cx<T> a, const Cx<T> b, const StoltKnot k)
{
    const T re = (T)((1.0 - k.w) * (double)a.x + k.w * (double)b.x);
    const T im = (T)((1.0 - k.w) * (double)a.y + k.w * (double)b.y);
    Cx<T> o;
    o.x = (T)((double)re * k.sc);
    o.y = (T)((double)im * k.sc);
    return o;
}

// Stolt stretch + obliquity.  One thread per (xi, zj); zj is the fast index so
// loads of F[xi][i0], F[xi][i0+1] walk monotonically along a contiguous row.
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch(const Cx<T> *__restrict__ F, Cx<T> *__restrict__ K,
                                                     const double *__restrict__ kx, const double *__restrict__ ws,
                                                     int m, int nz, int tnum, double vel)
{
    const int zj = blockIdx.x * 256 + threadIdx.x;
    const int xi = blockIdx.y;
    if (zj >= m) return;
    Cx<T> o;
    o.x = 0;
    o.y = 0;
    if (zj < nz) {
        const StoltKnot k = stolt_knot(ws, kx[xi], zj, m, vel);
        o = stolt_mix<T>(F[(size_t)xi * m + k.i0], F[(size_t)xi * m + k.i0 + 1], k);
        if (zj == 0 && xi == 0) {                                   // :200
            o.x = 0;
            o.y = 0;
        }
    }
    K[(size_t)xi * m + zj] = o;
}

// The same on the spectrum as the own transforms leave it after the pass over the traces: frequency-major, F[w][kx].  One
// thread per (zj, xi) with xi the fast index: the two rows a wavenumber interpolates between move slowly with xi (kk grows
// with |kx|), so neighbouring lanes read neighbouring words of the same or the next row -- no transposes around the stretch.
template <typename T>
__device__ __forceinline__ void stolt_point_t(const Cx<T> *__restrict__ F, Cx<T> *__restrict__ K, const double *__restrict__ kx,
                                              const double *__restrict__ ws, int m, int nz, int tnum, double vel, int xi, int zj)
{
    Cx<T> o;
    o.x = 0;
    o.y = 0;
    if (zj < nz) {
        const StoltKnot k = stolt_knot(ws, kx[xi], zj, m, vel);
        o = stolt_mix<T>(F[(size_t)k.i0 * tnum + xi], F[(size_t)(k.i0 + 1) * tnum + xi], k);
        if (zj == 0 && xi == 0) {                                   // :200
            o.x = 0;
            o.y = 0;
        }
    }
    K[(size_t)zj * tnum + xi] = o;
}
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch_t(const Cx<T> *__restrict__ F, Cx<T> *__restrict__ K,
                                                       const double *__restrict__ kx, const double *__restrict__ ws,
                                                       int m, int nz, int tnum, double vel)
{
    const int xi = blockIdx.x * 256 + threadIdx.x;
    if (xi >= tnum) return;
    stolt_point_t<T>(F, K, kx, ws, m, nz, tnum, vel, xi, blockIdx.y);
}

// The same on the spectrum as [kx >= 0][all frequencies] (round 6: the transform over the traces taken first, on the radargram's own
// rows; rows k = 0 .. tnum/2 of snum complex numbers in FFT order).  irfft2 (:202) extends KK Hermitian-wise, KK[-w][kx] =
// conj KK[w][-kx], and conj FK[i][-kx] = FK[-i][kx] for a real radargram: the negative-frequency half of row kx is the same
// interpolation, with the same weights (they depend on |kx| only), between the mirrored knots of the SAME row.  One thread per
// (kx, zj), zj the fast index; the zero-frequency and Nyquist rows of KK are zero (kz = 0 scales the first to zero, :196; KK[:nz]
// alone is filled, :190), so numpy's dropping of their imaginary parts has nothing to drop.
template <typename T>
__device__ __forceinline__ void stolt_point_rows(const Cx<T> *__restrict__ B, Cx<T> *__restrict__ K, const double *__restrict__ kx,
                                                 const double *__restrict__ ws, int m, int nz, int snum, double vel, int xi, int zj)
{
    const Cx<T> *row = B + (size_t)xi * snum;
    Cx<T> *orow = K + (size_t)xi * snum;
    Cx<T> o, om;
    o.x = o.y = om.x = om.y = 0;
    if (zj < nz) {
        const StoltKnot k = stolt_knot(ws, kx[xi], zj, m, vel);
        o = stolt_mix<T>(row[k.i0], row[k.i0 + 1], k);
        if (zj > 0) om = stolt_mix<T>(row[k.i0 == 0 ? 0 : snum - k.i0], row[snum - k.i0 - 1], k);
        if (zj == 0 && xi == 0) {                                   // :200
            o.x = 0;
            o.y = 0;
        }
    }
    orow[zj] = o;                                                   // (zj = nz: the Nyquist row, zero)
    if (zj > 0 && zj < nz) orow[snum - zj] = om;
}
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch_rows(const Cx<T> *__restrict__ B, Cx<T> *__restrict__ K,
                                                          const double *__restrict__ kx, const double *__restrict__ ws,
                                                          int m, int nz, int snum, double vel)
{
    const int zj = blockIdx.x * 256 + threadIdx.x;
    if (zj > nz) return;
    stolt_point_rows<T>(B, K, kx, ws, m, nz, snum, vel, blockIdx.y, zj);
}

// The velocity scan's stretch (impdar_stolt_scan): ONE spectrum, as the forward half of a call leaves it, stretched at nb velocities
// into nb spectra [nb][plane].  Grid z is the velocity and the slowest index of the dispatch: a plane's blocks walk the shared
// spectrum front to back like a single call's, and the next plane re-reads it one plane of output later (the
// reuse distance is spectrum + one plane, inside the 256 MiB Infinity Cache up to 4096 x 4096 float32; small sizes stay in L2).
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch_scan_rows(const Cx<T> *__restrict__ B, Cx<T> *__restrict__ K,
                                                               const double *__restrict__ kx, const double *__restrict__ ws,
                                                               const double *__restrict__ vels, int m, int nz, int snum, size_t plane)
{
    const int zj = blockIdx.x * 256 + threadIdx.x;
    if (zj > nz) return;
    stolt_point_rows<T>(B, K + (size_t)blockIdx.z * plane, kx, ws, m, nz, snum, vels[blockIdx.z], blockIdx.y, zj);
}
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch_scan_t(const Cx<T> *__restrict__ F, Cx<T> *__restrict__ K,
                                                            const double *__restrict__ kx, const double *__restrict__ ws,
                                                            const double *__restrict__ vels, int m, int nz, int tnum, size_t plane)
{
    const int xi = blockIdx.x * 256 + threadIdx.x;
    if (xi >= tnum) return;
    stolt_point_t<T>(F, K + (size_t)blockIdx.z * plane, kx, ws, m, nz, tnum, vels[blockIdx.z], xi, blockIdx.y);
}

// Focus measures of the scan's images Y[nb][nout][tnum]: sum |x|, sum x^2, sum x^4 (x^4 = (x^2)^2) over the traces t0 <= j < t1
// of every row, in float64 -> sums[b][k][3].  One workgroup per (row, velocity).  The order of the additions is a function of the
// trace index alone -- the V = 16 / sizeof(T) traces of group g = j / V go to thread g % 256 in rising order, then a butterfly
// over the wave, then the four waves' partials in wave order -- so a row's sums do not depend on where its image lies in the
// batch, and two calls give the same bits.  A whole group inside the window is one 16-byte load where the row is 16-byte
// aligned; heads, tails and unaligned rows load the same traces one by one.  NaN and Inf propagate as in NumPy.
template <typename T>
__global__ __launch_bounds__(256) void stolt_focus_rows(const T *__restrict__ Y, double *__restrict__ sums, int nout, int tnum,
                                                        int t0, int t1)
{
    constexpr int V = 16 / sizeof(T);
    struct alignas(16) Vec { T v[V]; };
    const T *row = Y + ((size_t)blockIdx.y * nout + blockIdx.x) * tnum;
    const bool aligned = (reinterpret_cast<size_t>(row) & 15) == 0;
    double s1 = 0.0, s2 = 0.0, s4 = 0.0;
    for (int g = t0 / V + (int)threadIdx.x; g * V < t1; g += 256) {
        const int j = g * V;
        const bool whole = j >= t0 && j + V <= t1;
        Vec q;
        if (whole && aligned) {
            q = *reinterpret_cast<const Vec *>(row + j);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) q.v[e] = (j + e >= t0 && j + e < t1) ? row[j + e] : (T)0;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (whole || (j + e >= t0 && j + e < t1)) {
                const double x = (double)q.v[e];
                const double x2 = x * x;
                s1 += fabs(x);
                s2 += x2;
                s4 += x2 * x2;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
        s4 += __shfl_xor(s4, off);
    }
    __shared__ double part[4][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = s1;
        part[wave][1] = s2;
        part[wave][2] = s4;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = part[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) s += part[w][threadIdx.x];
        sums[((size_t)blockIdx.y * nout + blockIdx.x) * 3 + threadIdx.x] = s;
    }
}

// C2R ignores the imaginary part of the DC and Nyquist bins (numpy irfft):
// clear them so any Hermitian-assuming backend agrees.
template <typename T>
__global__ void stolt_fix_hermitian(Cx<T> *K, int m, int tnum)
{
    const int xi = blockIdx.x * 256 + threadIdx.x;
    if (xi >= tnum) return;
    K[(size_t)xi * m].y = 0;
    K[(size_t)xi * m + m - 1].y = 0;
}
