// Layout kernels of the phase shift: Cp<T>, taper + zero-pad + transpose on the way in, the transposes between the
// row transforms, the real part on the way out (phaseshift.hip; ffd.hip takes Cp<double>).
#pragma once
#include "fft.h"        // impdar_taper_w

template <typename T> struct Cp { T x, y; };


// (snum,tnum) real -> tapered, zero-padded, transposed complex X[tnum][nt]
template <typename T>
__global__ __launch_bounds__(256) void ps_taper_pad_transpose(const T *__restrict__ in, Cp<T> *__restrict__ X, int snum,
                                                              int tnum, int nt, double htaper, double vtaper)
{
    __shared__ T tile[64][65];
    const int k0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, j = j0 + tx;
        T v = 0;
        if (k < snum && j < tnum) {
            const double hv = impdar_taper_w(j, tnum, htaper) * impdar_taper_w(k, snum, vtaper);
            v = (T)((double)in[(size_t)k * tnum + j] * hv);        // data *= H*V, :258
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, k = k0 + tx;
        if (j < tnum && k < nt) {
            Cp<T> c;
            c.x = tile[tx][r];
            c.y = 0;
            X[(size_t)j * nt + k] = c;
        }
    }
}

// the same, real: X[tnum][nt] for the real-to-complex transform along time of the Hermitian walk
template <typename T>
__global__ __launch_bounds__(256) void ps_taper_pad_transpose_real(const T *__restrict__ in, T *__restrict__ X, int snum, int tnum,
                                                                   int nt, double htaper, double vtaper)
{
    __shared__ T tile[64][65];
    __shared__ double vw[64];
    const int k0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    // (the weights are float64 divisions: the column's once per thread, the tile's 64 rows' once per tile -- two per element
    // until round 6, 141 us at 8192^2 for a pass that moves 0.54 GB)
    const double hw = j0 + tx < tnum ? impdar_taper_w(j0 + tx, tnum, htaper) : 0.0;
    if (threadIdx.x < 64) vw[threadIdx.x] = k0 + (int)threadIdx.x < snum ? impdar_taper_w(k0 + (int)threadIdx.x, snum, vtaper) : 0.0;
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, j = j0 + tx;
        T v = 0;
        if (k < snum && j < tnum) {
            const double hv = hw * vw[r];
            v = (T)((double)in[(size_t)k * tnum + j] * hv);        // data *= H*V, :258
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, k = k0 + tx;
        if (j < tnum && k < nt) X[(size_t)j * nt + k] = tile[tx][r];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ps_taper_inplace(T *__restrict__ d, int snum, int tnum, double htaper,
                                                        double vtaper)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)snum * tnum) return;
    const int k = (int)(i / tnum), j = (int)(i % tnum);
    const double hv = impdar_taper_w(j, tnum, htaper) * impdar_taper_w(k, snum, vtaper);
    d[i] = (T)((double)d[i] * hv);
}

// Z[tnum][snum] complex -> out (snum,tnum) real part
// out[c][r] = in[r][c] for a (rows x cols) complex array: the transforms over the traces / wavenumbers run on
// contiguous rows of the transposed array.  rocFFT's own strided plans for the same transform (stride = row length,
// distance 1) take 1.77 ms at 8192 x 8192 complex64 where this transpose + a contiguous plan take 0.25 + 0.23 ms
// (profiles/r03_fft_strided_probe.txt).
template <typename T, int TS>
__global__ __launch_bounds__(256) void ps_transpose_c(const Cp<T> *__restrict__ in, Cp<T> *__restrict__ out, int rows, int cols)
{
    __shared__ Cp<T> tile[TS][TS + 1];
    const int c0 = blockIdx.x * TS, r0 = blockIdx.y * TS;
    const int tx = threadIdx.x % TS, ty = threadIdx.x / TS;
    for (int r = ty; r < TS; r += 256 / TS)
        if (r0 + r < rows && c0 + tx < cols) tile[r][tx] = in[(size_t)(r0 + r) * cols + c0 + tx];
    __syncthreads();
    for (int c = ty; c < TS; c += 256 / TS)
        if (c0 + c < cols && r0 + tx < rows) out[(size_t)(c0 + c) * rows + r0 + tx] = tile[tx][c];
}

template <typename T> static void ps_launch_transpose(const void *in, void *out, int rows, int cols, hipStream_t st)
{
    constexpr int TS = sizeof(T) == 4 ? 64 : 32;
    hipLaunchKernelGGL((ps_transpose_c<T, TS>), dim3((cols + TS - 1) / TS, (rows + TS - 1) / TS), dim3(256), 0, st,
                       reinterpret_cast<const Cp<T> *>(in), reinterpret_cast<Cp<T> *>(out), rows, cols);
}

// Only the REAL part of the inverse transform over the wavenumbers is kept (mig_python.py:282), and Re sum_k TK[k] e^{+i k x} =
// sum_k G[k] e^{+i k x} with G[k] = (TK[k] + conj TK[-k]) / 2 Hermitian: the transpose forms G for k = 0 .. tnum / 2 on its way
// ([k][tau] -> [tau][k], rows hs apart), and a real inverse transform of HALF the complex length does the rest (round 6: the
// transposed array written is half as large, the transform's row in LDS too).
template <typename T, int TS>
__global__ __launch_bounds__(256) void ps_transpose_herm(const Cp<T> *__restrict__ in, Cp<T> *__restrict__ out, int tnum, int snum, int hs)
{
    __shared__ Cp<T> tile[TS][TS + 1];
    const int c0 = blockIdx.x * TS, r0 = blockIdx.y * TS;          // c: tau, r: k
    const int tx = threadIdx.x % TS, ty = threadIdx.x / TS, nh = tnum / 2;
    for (int r = ty; r < TS; r += 256 / TS) {
        const int k = r0 + r;
        if (k <= nh && c0 + tx < snum) {
            const Cp<T> a = in[(size_t)k * snum + c0 + tx], b = in[(size_t)(k ? tnum - k : 0) * snum + c0 + tx];
            tile[r][tx] = Cp<T>{(T)0.5 * (a.x + b.x), (T)0.5 * (a.y - b.y)};
        }
    }
    __syncthreads();
    for (int c = ty; c < TS; c += 256 / TS)
        if (c0 + c < snum && r0 + tx <= nh) out[(size_t)(c0 + c) * hs + r0 + tx] = tile[tx][c];
}

template <typename T> static void ps_launch_transpose_herm(const void *in, void *out, int tnum, int snum, int hs, hipStream_t st)
{
    constexpr int TS = sizeof(T) == 4 ? 64 : 32;
    hipLaunchKernelGGL((ps_transpose_herm<T, TS>), dim3((snum + TS - 1) / TS, (tnum / 2 + TS) / TS), dim3(256), 0, st,
                       reinterpret_cast<const Cp<T> *>(in), reinterpret_cast<Cp<T> *>(out), tnum, snum, hs);
}

// out[c][r] = in[r][c] for r < rows, 0 for rows <= r < rows_out: [snum][tnum/2 + 1] -> [tnum/2 + 1][nt], the time axis zero-padded
// (the spectrum over the traces on its way to the transform over time, P.fhalf)
template <typename T, int TS>
__global__ __launch_bounds__(256) void ps_transpose_pad(const Cp<T> *__restrict__ in, Cp<T> *__restrict__ out, int rows, int cols, int rows_out)
{
    __shared__ Cp<T> tile[TS][TS + 1];
    const int c0 = blockIdx.x * TS, r0 = blockIdx.y * TS;
    const int tx = threadIdx.x % TS, ty = threadIdx.x / TS;
    for (int r = ty; r < TS; r += 256 / TS)
        tile[r][tx] = (r0 + r < rows && c0 + tx < cols) ? in[(size_t)(r0 + r) * cols + c0 + tx] : Cp<T>{(T)0, (T)0};
    __syncthreads();
    for (int c = ty; c < TS; c += 256 / TS)
        if (c0 + c < cols && r0 + tx < rows_out) out[(size_t)(c0 + c) * rows_out + r0 + tx] = tile[tx][c];
}

// out[i] = Re Z[i] (mig_python.py:282 keeps the real part of the inverse transform)
template <typename T>
__global__ __launch_bounds__(256) void ps_real_part(const Cp<T> *__restrict__ Z, T *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = Z[i].x;
}

template <typename T>
__global__ __launch_bounds__(256) void ps_real_transpose(const Cp<T> *__restrict__ Z, T *__restrict__ out, int snum,
                                                         int tnum)
{
    __shared__ T tile[64][65];
    const int k0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, k = k0 + tx;
        tile[r][tx] = (j < tnum && k < snum) ? Z[(size_t)j * snum + k].x : (T)0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, j = j0 + tx;
        if (k < snum && j < tnum) out[(size_t)k * tnum + j] = tile[tx][r];
    }
}
