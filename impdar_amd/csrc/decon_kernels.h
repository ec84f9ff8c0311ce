// The kernels of decon.hip: the contract is decon_core.h, every launch argument is decon_route.h's.
//
//   decon_acorr_kernel   r[l] of DECON_TG traces for one chunk of <= DECON_C lags.  Lane % 32 is the trace, lane / 32 one of 8
//                        runs of 8 consecutive lags.  Per block of DECON_C samples the workgroup stages the samples x[k] and the
//                        2 DECON_C - 1 shifted ones x[k + lag0 ...] in LDS as float64; a thread then slides down the block
//                        with the 8 shifted values of its lags in registers: two LDS reads for 8 fmas per sample.
//   decon_solve_kernel   the recursion, DECON_G lanes per trace, four traces per single-wave workgroup, the vectors in LDS
//                        interleaved by trace (element i of trace t at [4 i + t]: the 64 lanes read 64 consecutive doubles).
//   decon_apply_kernel   y of DECON_TG traces.  Lane / 32 is one of 8 runs of 8 consecutive output samples; per block of
//                        DECON_C outputs and chunk of <= DECON_C taps the workgroup stages the 2 DECON_C - 1 samples the chunk
//                        reaches and the taps of its traces; a thread walks the taps with the 8 samples of its outputs in
//                        registers.  The blocks are walked from the trace's end to its start and a block is written only
//                        after every chunk of it has been staged: y[k] needs x at k and before, so with y == x nothing that
//                        is still to be read has been written.
//   decon_mean_*         R[l] of design 'mean': a fixed tree over blocks of DECON_MEAN_BLOCK traces, then the blocks in order.
//   decon_norm_kernel    the autocorrelogram's division by r[0].
#pragma once
#include "decon_route.h"
#include "vecwidth.h"

// tile[r][c] = x[row0 + r][col0 + c] as float64 where lo <= row0 + r < hi and col0 + c < tnum, else +0; V traces per access
template <typename T, int V>
__device__ __forceinline__ void decon_stage(const T *x, int tnum, int col0, int row0, int rows, int lo, int hi, double *tile)
{
    constexpr int PER = DECON_TG / V;
    for (int idx = threadIdx.x; idx < rows * PER; idx += DECON_THREADS) {
        const int r = idx / PER, cv = (idx - r * PER) * V;
        const int row = row0 + r, col = col0 + cv;
        RwVec<T, V> v;
#pragma unroll
        for (int c = 0; c < V; ++c) v.v[c] = (T)0;
        if (row >= lo && row < hi && col < tnum) v = rw_load<T, V>(x + (size_t)row * tnum + col);
#pragma unroll
        for (int c = 0; c < V; ++c) tile[r * DECON_TG + cv + c] = (double)v.v[c];
    }
}

template <typename T, int V>
__global__ __launch_bounds__(DECON_THREADS) void decon_acorr_kernel(const T *__restrict__ x, int tnum, int s0, int s1, DeconLags L,
                                                                    double *__restrict__ lag)
{
    extern __shared__ __align__(16) double decon_lds[];
    double *base = decon_lds;                          // [DECON_C][DECON_TG]
    double *band = decon_lds + DECON_C * DECON_TG;     // [2 DECON_C - 1][DECON_TG]
    const int tx = threadIdx.x % DECON_TG, ty = threadIdx.x / DECON_TG;
    const int col0 = blockIdx.x * DECON_TG;
    const DeconChunk ch = decon_chunk(L, blockIdx.y);
    const bool active = ty * DECON_LPT < ch.count;
    double tot[DECON_LPT];
#pragma unroll
    for (int u = 0; u < DECON_LPT; ++u) tot[u] = 0.0;
    for (int k0 = s0; k0 < s1; k0 += DECON_C) {
        __syncthreads();        // (the tiles of the block before have been read)
        decon_stage<T, V>(x, tnum, col0, k0, DECON_C, s0, s1, base);
        decon_stage<T, V>(x, tnum, col0, k0 + ch.lag0, 2 * DECON_C - 1, s0, s1, band);
        __syncthreads();
        if (!active) continue;
        const double *bp = band + ty * DECON_LPT * DECON_TG + tx, *xp = base + tx;
        double acc[DECON_LPT], w[DECON_LPT];
#pragma unroll
        for (int u = 0; u < DECON_LPT; ++u) acc[u] = 0.0;
#pragma unroll
        for (int u = 0; u < DECON_LPT - 1; ++u) w[u] = bp[u * DECON_TG];
        // at sample kk the shifted value of lag u is w[(u + kk) % 8]; the one that enters is row kk + 7
        for (int kb = 0; kb < DECON_C; kb += DECON_LPT) {
#pragma unroll
            for (int s = 0; s < DECON_LPT; ++s) {
                const int kk = kb + s;
                w[(DECON_LPT - 1 + s) % DECON_LPT] = bp[(kk + DECON_LPT - 1) * DECON_TG];
                const double xk = xp[kk * DECON_TG];
#pragma unroll
                for (int u = 0; u < DECON_LPT; ++u) acc[u] = fma(xk, w[(u + s) % DECON_LPT], acc[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < DECON_LPT; ++u) tot[u] += acc[u];
    }
    const int col = col0 + tx;
    if (col < tnum) {
#pragma unroll
        for (int u = 0; u < DECON_LPT; ++u)
            if (ty * DECON_LPT + u < ch.count) lag[(size_t)(ch.row0 + ty * DECON_LPT + u) * tnum + col] = tot[u];
    }
}

// the tree of decon_core.h over the DECON_G lanes of a trace
__device__ __forceinline__ double decon_tree(double s)
{
#pragma unroll
    for (int o = DECON_G / 2; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
    return s;
}

// `nsys` systems whose lag table is lag[row][ld]; operators to op[i][op_ld], one flag per system to dead
__global__ __launch_bounds__(64) void decon_solve_kernel(const double *__restrict__ lag, int ld, int nsys, DeconLags L, int n, int g, double eps,
                                                         double *__restrict__ op, int op_ld, int *__restrict__ dead)
{
    extern __shared__ __align__(16) double decon_lds[];
    constexpr int ST = DECON_SOLVE_TRACES;
    const int t = threadIdx.x / DECON_G, q = threadIdx.x % DECON_G;
    const int sys = blockIdx.x * ST + t;
    const bool live = sys < nsys;
    double *c = decon_lds + t, *rhs = c + n * ST, *a = rhs + n * ST, *p = a + n * ST, *pn = p + n * ST;
    for (int i = q; i < n; i += DECON_G) {
        c[i * ST] = live ? lag[(size_t)decon_lag_row(L, i) * ld + sys] : 0.0;
        rhs[i * ST] = live ? lag[(size_t)decon_lag_row(L, g + i) * ld + sys] : 0.0;
        a[i * ST] = p[i * ST] = pn[i * ST] = 0.0;
    }
    __syncthreads();
    const double r0 = c[0];
    double v = r0 * (1.0 + eps);
    bool ok = decon_power_ok(r0) && decon_power_ok(v);
    __syncthreads();
    if (q == 0) {
        c[0] = v;
        p[0] = 1.0;
        a[0] = rhs[0] / v;
    }
    __syncthreads();
    for (int m = 1; m < n; ++m) {
        double d, e, k, mu;
        decon_dot_lane(p, a, c, ST, m, q, d, e);
        d = decon_tree(d);
        e = decon_tree(e);
        ok = decon_step(d, e, rhs[m * ST], v, k, mu) && ok;
        for (int i = q; i <= m; i += DECON_G) pn[i * ST] = decon_p_next(p, ST, m, i, k);
        __syncthreads();
        for (int i = q; i <= m; i += DECON_G) a[i * ST] = decon_a_next(a, pn, ST, m, i, mu);
        __syncthreads();
        double *sw = p;
        p = pn;
        pn = sw;
    }
    if (live) {
        for (int i = q; i < n; i += DECON_G) op[(size_t)i * op_ld + sys] = ok ? a[i * ST] : 0.0;
        if (q == 0) dead[sys] = ok ? 0 : 1;
    }
}

// y may be x.  op[i][op_ld] with the trace as column, or one operator for all (op_ld == 0); dead_all: the flag of that one
template <typename T, int V>
__global__ __launch_bounds__(DECON_THREADS) void decon_apply_kernel(const T *x, T *y, int snum, int tnum, int n, int g,
                                                                    const double *__restrict__ op, int op_ld, const int *__restrict__ dead,
                                                                    const int *__restrict__ dead_all)
{
    extern __shared__ __align__(16) double decon_lds[];
    double *band = decon_lds;                                   // [2 DECON_C - 1][DECON_TG]
    double *taps = decon_lds + (2 * DECON_C - 1) * DECON_TG;    // [DECON_C][DECON_TG]
    const int tx = threadIdx.x % DECON_TG, ty = threadIdx.x / DECON_TG;
    const int col0 = blockIdx.x * DECON_TG, col = col0 + tx;
    const bool pass = col >= tnum || dead[col] != 0 || (dead_all && *dead_all != 0);
    for (int k0 = (snum - 1) / DECON_C * DECON_C; k0 >= 0; k0 -= DECON_C) {
        double acc[DECON_LPT], w[DECON_LPT];
#pragma unroll
        for (int u = 0; u < DECON_LPT; ++u) acc[u] = 0.0;
        for (int c0 = 0; c0 < n; c0 += DECON_C) {
            const int cn = n - c0 < DECON_C ? n - c0 : DECON_C;
            __syncthreads();    // (the tiles of the chunk before have been read)
            // tile row j is the sample k0 - g - c0 - (DECON_C - 1) + j: output o of the block and tap ii of the chunk meet at j = o - ii + DECON_C - 1
            decon_stage<T, V>(x, tnum, col0, k0 - g - c0 - (DECON_C - 1), 2 * DECON_C - 1, 0, snum, band);
            for (int idx = threadIdx.x; idx < DECON_C * DECON_TG; idx += DECON_THREADS) {
                const int ii = idx / DECON_TG, cc = col0 + idx % DECON_TG;
                taps[idx] = ii < cn && cc < tnum ? op[op_ld ? (size_t)(c0 + ii) * op_ld + cc : (size_t)(c0 + ii)] : 0.0;
            }
            __syncthreads();
            const double *bp = band + (ty * DECON_LPT + DECON_C - 1) * DECON_TG + tx, *ap = taps + tx;
#pragma unroll
            for (int u = 1; u < DECON_LPT; ++u) w[u] = bp[u * DECON_TG];
            // at tap ii the sample of output u is w[(u - ii) % 8]; the one that enters is row -ii of bp
            for (int ib = 0; ib < cn; ib += DECON_LPT) {
#pragma unroll
                for (int s = 0; s < DECON_LPT; ++s) {
                    const int ii = ib + s;
                    if (ii < cn) {          // no tap beyond the operator: 0 * NaN would be NaN
                        w[(DECON_LPT - s) % DECON_LPT] = bp[-ii * DECON_TG];
                        const double ai = ap[ii * DECON_TG];
#pragma unroll
                        for (int u = 0; u < DECON_LPT; ++u) acc[u] = fma(ai, w[(u + DECON_LPT - s) % DECON_LPT], acc[u]);
                    }
                }
            }
        }
        __syncthreads();        // every sample this block needs has been read by every thread: now it may be written
        if (col < tnum) {
#pragma unroll
            for (int u = 0; u < DECON_LPT; ++u) {
                const int k = k0 + ty * DECON_LPT + u;
                if (k < snum) {
                    const T xv = x[(size_t)k * tnum + col];
                    y[(size_t)k * tnum + col] = pass ? xv : (T)((double)xv - acc[u]);
                }
            }
        }
    }
}

// a fixed-order sum over the DECON_MEAN_BLOCK threads: a butterfly over each wave, then the four waves as (0 + 1) + (2 + 3)
__device__ __forceinline__ double decon_block_sum(double v, double *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// part[b][l] = the sum of r_j[l] over the live traces j of block b; dead[j] by the r[0] rule
__global__ __launch_bounds__(DECON_MEAN_BLOCK) void decon_mean_block_kernel(const double *__restrict__ lag, int tnum, int nlags,
                                                                           double *__restrict__ part, int *__restrict__ dead)
{
    __shared__ double red[DECON_MEAN_BLOCK / 64];
    const int j = blockIdx.x * DECON_MEAN_BLOCK + threadIdx.x;
    const bool live = j < tnum && decon_power_ok(lag[j]);
    if (j < tnum) dead[j] = live ? 0 : 1;
    for (int l = 0; l < nlags; ++l) {
        const double s = decon_block_sum(live ? lag[(size_t)l * tnum + j] : 0.0, red);
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * nlags + l] = s;
    }
}

__global__ __launch_bounds__(256) void decon_mean_sum_kernel(const double *__restrict__ part, int blocks, int nlags, double *__restrict__ R)
{
    for (int l = threadIdx.x; l < nlags; l += 256) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += part[(size_t)b * nlags + l];
        R[l] = s;
    }
}

// out[i][j] = the operator applied to trace j: the mean one, or zeros for a trace that passes
__global__ __launch_bounds__(256) void decon_mean_spread_kernel(const double *__restrict__ mop, const int *__restrict__ dead, int n, int tnum,
                                                                double *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= tnum) return;
    const bool pass = dead[j] != 0 || dead[tnum] != 0;
    for (int i = 0; i < n; ++i) out[(size_t)i * tnum + j] = pass ? 0.0 : mop[i];
}

__global__ __launch_bounds__(256) void decon_norm_kernel(double *__restrict__ A, int nl, int tnum)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= tnum) return;
    const double r0 = A[j];
    const bool ok = decon_power_ok(r0);
    for (int l = 0; l < nl; ++l) A[(size_t)l * tnum + j] = ok ? A[(size_t)l * tnum + j] / r0 : __builtin_nan("");
}
