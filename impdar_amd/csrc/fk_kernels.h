// The kernels of the f-k path (fk.hip launches them): the fan weight on the spectrum in each of the three layouts Stolt's forward
// half leaves it in, and |spectrum|^2 out of each of them as [w >= 0][kx] float64 with the columns in fftshift order.
#pragma once
#include "fk_weight.h"
#include "stolt_kernels.h"      // Cx

// weight times element, the product rounded to the data's type
template <typename T> __device__ __forceinline__ Cx<T> fk_scale(const Cx<T> v, double W)
{
    Cx<T> o;
    o.x = (T)((double)v.x * W);
    o.y = (T)((double)v.y * W);
    return o;
}

// The fan kernels take the place of the Stolt stretch: one read and one write of the spectrum, the contiguous axis of the layout
// across the lanes, 16 bytes per lane where the rows are 16-byte aligned (an even row length in float32; element by element
// elsewhere), a few thousand workgroups that stride over the rows (fk.hip: fk_fan_grid), what belongs to a column -- its
// frequency or wavenumber, whether it is a Nyquist one -- held in registers across them.
struct FkAxis {
    double v;       // the frequency or the wavenumber of a row or a column of the layout
    bool nyq;       // ... and whether it is the Nyquist one
};
constexpr int FK_FAN_THREADS = 256;
template <typename T> constexpr int fk_fan_vec() { return 16 / (int)sizeof(Cx<T>); }

// A [nrows][ncols] -> B; COL_IS_W: the columns are frequencies and the rows wavenumbers, else the other way round
template <typename T, bool COL_IS_W, class Col, class Row>
__device__ __forceinline__ void fk_fan_sweep(const Cx<T> *__restrict__ A, Cx<T> *__restrict__ B, int nrows, int ncols, const FkFan fan,
                                             const Col col, const Row row)
{
    constexpr int V = fk_fan_vec<T>();
    struct alignas(16) Vec { Cx<T> v[V]; };
    const int c0 = (blockIdx.x * FK_FAN_THREADS + threadIdx.x) * V;
    if (c0 >= ncols) return;
    const bool whole = ncols % V == 0;          // then every row starts 16-byte aligned and c0 + V <= ncols
    FkAxis cv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) cv[e] = col(min(c0 + e, ncols - 1));
    for (int r = blockIdx.y; r < nrows; r += gridDim.y) {
        const FkAxis rv = row(r);
        const size_t at = (size_t)r * ncols + c0;
        double W[V];
#pragma unroll
        for (int e = 0; e < V; ++e)
            W[e] = COL_IS_W ? fk_weight(fan, cv[e].v, rv.v, cv[e].nyq || rv.nyq) : fk_weight(fan, rv.v, cv[e].v, cv[e].nyq || rv.nyq);
        if (whole) {
            Vec q = *reinterpret_cast<const Vec *>(A + at);
#pragma unroll
            for (int e = 0; e < V; ++e) q.v[e] = fk_scale<T>(q.v[e], W[e]);
            *reinterpret_cast<Vec *>(B + at) = q;
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (c0 + e < ncols) B[at + e] = fk_scale<T>(A[at + e], W[e]);
        }
    }
}

//   [kx >= 0][all w] (rows route; snum and tnum even): row k = 0 .. tnum / 2 holds the snum frequencies in FFT order, w[s] =
//   ws[s] for s <= snum / 2, -ws[snum - s] above; the wavenumbers -k are the Hermitian mirror and never stored
template <typename T>
__global__ __launch_bounds__(FK_FAN_THREADS) void fk_fan_rows(const Cx<T> *__restrict__ A, Cx<T> *__restrict__ B, const double *__restrict__ kx,
                                                              const double *__restrict__ ws, int hs, int snum, int tnum, const FkFan fan)
{
    const int half = snum / 2;
    fk_fan_sweep<T, true>(A, B, hs, snum, fan,
                          [=](int s) { return FkAxis{s <= half ? ws[s] : -ws[snum - s], s == half}; },
                          [=](int k) { return FkAxis{kx[k], 2 * k == tnum}; });
}
//   [w >= 0][kx] (the other own route; snum even, tnum even or odd)
template <typename T>
__global__ __launch_bounds__(FK_FAN_THREADS) void fk_fan_wkx(const Cx<T> *__restrict__ A, Cx<T> *__restrict__ B, const double *__restrict__ kx,
                                                             const double *__restrict__ ws, int m, int snum, int tnum, const FkFan fan)
{
    fk_fan_sweep<T, false>(A, B, m, tnum, fan,
                           [=](int i) { return FkAxis{kx[i], 2 * i == tnum}; },
                           [=](int j) { return FkAxis{ws[j], 2 * j == snum}; });
}
//   [kx][w >= 0] (rocFFT; any snum and tnum)
template <typename T>
__global__ __launch_bounds__(FK_FAN_THREADS) void fk_fan_kxw(const Cx<T> *__restrict__ A, Cx<T> *__restrict__ B, const double *__restrict__ kx,
                                                             const double *__restrict__ ws, int m, int snum, int tnum, const FkFan fan)
{
    fk_fan_sweep<T, true>(A, B, tnum, m, fan,
                          [=](int j) { return FkAxis{ws[j], 2 * j == snum}; },
                          [=](int i) { return FkAxis{kx[i], 2 * i == tnum}; });
}

// wavenumber index i -> its column in fftshift order
__device__ __forceinline__ int fk_shift_col(int i, int tnum) { return (i + tnum / 2) % tnum; }

template <typename T> __device__ __forceinline__ double fk_abs2(const Cx<T> v)
{
    const double re = (double)v.x, im = (double)v.y;
    return re * re + im * im;
}

// P[j][shift(i)] = |K[j][i]|^2 from the [w >= 0][kx] layout: rows to rows
template <typename T>
__global__ __launch_bounds__(256) void fk_power_wkx(const Cx<T> *__restrict__ K, double *__restrict__ P, int m, int tnum)
{
    const int c = blockIdx.x * 256 + threadIdx.x;       // the output column: coalesced stores, loads in two runs
    if (c >= tnum) return;
    const int i = (c + (tnum + 1) / 2) % tnum;
    for (int j = blockIdx.y; j < m; j += gridDim.y) P[(size_t)j * tnum + c] = fk_abs2<T>(K[(size_t)j * tnum + i]);
}

// ... from a layout with the wavenumber as the row: S [nk][ns], through a 64 x 64 LDS tile of odd pitch (loads along the
// frequencies, stores along the wavenumbers; the ragged tiles are range-checked).
//   MIRROR = false (rocFFT, S [tnum][m]): row k is wavenumber index k, column s frequency s: P[s][shift(k)]
//   MIRROR = true (rows route, S [tnum / 2 + 1][snum]): column s is frequency s for s <= snum / 2 and -(snum - s) above;
//     P[s][shift(k)] for s < m, and the wavenumbers the layout leaves out from the Hermitian mirror:
//     P[(snum - s) % snum][shift(tnum - k)] = |S[k][s]|^2 for 0 < k < tnum / 2
template <typename T, bool MIRROR>
__global__ __launch_bounds__(256) void fk_power_t(const Cx<T> *__restrict__ S, double *__restrict__ P, int nk, int ns, int m, int snum,
                                                  int tnum)
{
    __shared__ double tile[64][65];
    const int k0 = blockIdx.y * 64, s0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, s = s0 + tx;
        tile[r][tx] = (k < nk && s < ns) ? fk_abs2<T>(S[(size_t)k * ns + s]) : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int s = s0 + r, k = k0 + tx;
        if (s >= ns || k >= nk) continue;
        const double v = tile[tx][r];
        if (s < m) P[(size_t)s * tnum + fk_shift_col(k, tnum)] = v;
        if (MIRROR) {
            const int jm = s == 0 ? 0 : snum - s;
            if (jm < m && k > 0 && 2 * k < tnum) P[(size_t)jm * tnum + fk_shift_col(tnum - k, tnum)] = v;
        }
    }
}
