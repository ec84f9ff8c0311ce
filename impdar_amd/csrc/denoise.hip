// The denoise step an impproc/impdar chain runs between the horizontal filters and the re-spacing
// (reference src/impdar/lib/RadarData/_RadarDataFiltering.py:552-587), kept on the device:
//
//   * Wiener (scipy.signal.wiener, mysize = (m, n), N = m * n): lMean = box sum of x / N, lVar = box sum of x**2 / N
//     - lMean**2, both with zero padding and the full N at the edges; noise = mean(lVar) unless given;
//     out = lVar < noise ? lMean : (x - lMean) * (1 - noise / lVar) + lMean, float64.  Output i along an axis of
//     window m covers inputs i - m/2 .. i + (m-1)/2.  float32 squares are rounded to float32 (the reference squares
//     in the data's dtype); everything else is fp64.
//   * median (scipy.ndimage.median_filter, size = (m, n), mode 'reflect'): the element of 0-based rank N/2 of every
//     window, in the data's own dtype.
//
// Data is (snum, tnum) row-major: a row holds one sample of every trace.
//
// Wiener is three kernels whose cost does not depend on the window:
//   wn_vsum_kernel   a thread per column walks a strip of WN_RS rows with running sums over the m rows of each
//                    window (the row that leaves is read again, from cache): V1 = sum (x - p), V2 = sum (x - p)**2
//                    (float32: sum fl32(x*x)), Vc = number of non-finite values.  p is a pivot, one value of the
//                    data per strip of rows, so that a strong flat band (the direct wave) does not eat the digits of
//                    E[x**2] - E[x]**2.  Zero-padded rows enter as x = 0.  Non-finite values enter only Vc: a NaN is
//                    never carried past its window.
//   wn_hsum_kernel   a workgroup per row (persistent over rows) slides the horizontal window along V in tiles of
//                    WN_TILE: S(c) = T + Qex(c) - Pex(c), where T is the window sum at the tile's first column and
//                    Pex / Qex are block scans of the columns that leave / enter; T moves to the next tile by the two
//                    scans' totals.  Padded columns are added analytically.  MODE 0 sums lVar over the row (fixed
//                    order) for the noise estimate; MODE 1 writes the output.
//   wn_noise_kernel  one workgroup sums the row sums in a fixed order: the noise, and so the output, is bitwise
//                    repeatable (no float atomics).
// The statistics (V1, V2, Vc: 20 B per element) are kept between the two passes instead of recomputed.
//
// The median has two kernels:
//   med_small_kernel<T, NB>  N <= NB (16, 32 or 64): a (MD_TR x MD_TW) output tile with its reflected halo in LDS;
//                            each output gathers its window into NB registers (padded with +inf), sorts them with an
//                            unrolled bitonic network and takes rank N/2.
//   med_radix_kernel<T>      any N: an exact radix select on order-preserving integer keys, 4 bits per pass with a
//                            per-thread 16-bin histogram in LDS (8 passes for float32, 16 for float64): O(N) per
//                            output for every window size.
// The file is compiled with -ffp-contract=off, like the rest of the library.
#include "common.h"
#include <cmath>

#define WN_BLOCK 256
#define WN_RS 64                          // output rows per strip of wn_vsum_kernel (one pivot per strip)
#define WN_PER 4                          // consecutive columns per thread in one tile of wn_hsum_kernel
#define WN_TILE (WN_BLOCK * WN_PER)
#define WN_MAX_ROW_BLOCKS 2048            // resident workgroups of wn_hsum_kernel

#define MD_TR 16                          // median tile: output rows
#define MD_TW 64                          // median tile: output columns
#define MD_SMALL 64                       // largest N of the register path
#define MD_LDS ((MD_TR + MD_SMALL - 1) * MD_TW)   // the largest halo tile over m * n <= 64 (m = 64, n = 1)

template <typename T> __device__ __forceinline__ bool wn_finite(T v) { return isfinite(v); }

// the pivot of the strip that holds row t: a finite value of the strip's middle row (0 when it is not finite)
template <typename T>
__device__ __forceinline__ double wn_pivot(const T *__restrict__ x, int t, int snum, int tnum)
{
    int r = (t / WN_RS) * WN_RS + WN_RS / 2;
    if (r >= snum) r = snum - 1;
    const T v = x[(size_t)r * tnum + tnum / 2];
    return wn_finite(v) ? (double)v : 0.0;
}

// the contribution of one (zero-padded) element to the three sums
template <typename T>
__device__ __forceinline__ void wn_term(T v, double p, double &a1, double &a2, int &c)
{
    if (wn_finite(v)) {
        const double y = (double)v - p;
        a1 = y;
        if (sizeof(T) == 4) {
            const float f = (float)v;
            a2 = (double)(float)(f * f);            // the reference squares float32 data in float32
        } else {
            a2 = y * y;
        }
        c = 0;
    } else {
        a1 = 0.0;
        a2 = 0.0;
        c = 1;
    }
}

template <typename T>
__global__ __launch_bounds__(WN_BLOCK) void wn_vsum_kernel(const T *__restrict__ x, double *__restrict__ V1,
                                                           double *__restrict__ V2, int *__restrict__ Vc, int snum,
                                                           int tnum, int lo_v, int hi_v)
{
    const int col = blockIdx.x * WN_BLOCK + threadIdx.x;
    if (col >= tnum) return;
    const int s0 = blockIdx.y * WN_RS;
    const int s1 = s0 + WN_RS < snum ? s0 + WN_RS : snum;
    const double p = wn_pivot(x, s0, snum, tnum);
    auto at = [&](int r) -> T { return r >= 0 && r < snum ? x[(size_t)r * tnum + col] : (T)0; };
    double s1sum = 0.0, s2sum = 0.0;
    int cnt = 0;
    for (int r = s0 - lo_v; r <= s0 + hi_v; ++r) {
        double a1, a2;
        int c;
        wn_term(at(r), p, a1, a2, c);
        s1sum += a1;
        s2sum += a2;
        cnt += c;
    }
    for (int t = s0; t < s1; ++t) {
        const size_t o = (size_t)t * tnum + col;
        V1[o] = s1sum;
        V2[o] = s2sum;
        Vc[o] = cnt;
        if (t + 1 < s1) {
            double a1, a2, b1, b2;
            int c, d;
            wn_term(at(t - lo_v), p, a1, a2, c);
            wn_term(at(t + hi_v + 1), p, b1, b2, d);
            s1sum = (s1sum - a1) + b1;
            s2sum = (s2sum - a2) + b2;
            cnt += d - c;
        }
    }
}

// exclusive block scan of K values per thread (fixed order); tot[k] is the workgroup's total of value k
template <int K>
__device__ __forceinline__ void wn_block_scan(double (&v)[K], double (*wsum)[WN_BLOCK / 64], double (&tot)[K])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double inc = v[k];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        double ex = __shfl_up(inc, 1, 64);
        if (lane == 0) ex = 0.0;
        if (lane == 63) wsum[k][w] = inc;
        v[k] = ex;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double before = 0.0, t = 0.0;
#pragma unroll
        for (int q = 0; q < WN_BLOCK / 64; ++q) {
            const double s = wsum[k][q];
            if (q < w) before += s;
            t += s;
        }
        v[k] += before;
        tot[k] = t;
    }
    __syncthreads();   // wsum is rewritten by the next scan
}

// fixed-order sum over the workgroup (the result is valid in every thread)
__device__ __forceinline__ double wn_block_sum(double v, double *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

// counts ride through the fp64 scans: they are small integers, exact in a double
template <typename T, int MODE>
__global__ __launch_bounds__(WN_BLOCK) void wn_hsum_kernel(const T *__restrict__ x, const double *__restrict__ V1,
                                                           const double *__restrict__ V2, const int *__restrict__ Vc,
                                                           double *__restrict__ rowsum, double *__restrict__ out,
                                                           int snum, int tnum, int m, int n, double noise)
{
    __shared__ double wsum[6][WN_BLOCK / 64];
    __shared__ double red[WN_BLOCK / 64];
    const int lo_h = n / 2, hi_h = (n - 1) / 2;
    const double N = (double)m * (double)n;
    for (int t = blockIdx.x; t < snum; t += gridDim.x) {
        const size_t ro = (size_t)t * tnum;
        const double p = wn_pivot(x, t, snum, tnum);
        // T: the window sum at column 0 (columns 0 .. min(hi_h, tnum - 1); the padded ones are added below)
        const int e0 = hi_h < tnum - 1 ? hi_h : tnum - 1;
        double t1 = 0.0, t2 = 0.0, tc = 0.0;
        for (int j = threadIdx.x; j <= e0; j += WN_BLOCK) {
            t1 += V1[ro + j];
            t2 += V2[ro + j];
            tc += (double)Vc[ro + j];
        }
        t1 = wn_block_sum(t1, red);
        t2 = wn_block_sum(t2, red);
        tc = wn_block_sum(tc, red);
        double acc = 0.0;   // MODE 0: this thread's share of the row's sum of lVar, in column order
        for (int c0 = 0; c0 < tnum; c0 += WN_TILE) {
            const int j0 = c0 + threadIdx.x * WN_PER;
            double P[WN_PER][3], Q[WN_PER][3];
#pragma unroll
            for (int u = 0; u < WN_PER; ++u) {
                const int a = j0 + u - lo_h, b = j0 + u + hi_h + 1;
                const bool ina = j0 + u < tnum && a >= 0 && a < tnum, inb = j0 + u < tnum && b < tnum;
                P[u][0] = ina ? V1[ro + a] : 0.0;
                P[u][1] = ina ? V2[ro + a] : 0.0;
                P[u][2] = ina ? (double)Vc[ro + a] : 0.0;
                Q[u][0] = inb ? V1[ro + b] : 0.0;
                Q[u][1] = inb ? V2[ro + b] : 0.0;
                Q[u][2] = inb ? (double)Vc[ro + b] : 0.0;
            }
            // thread-local inclusive prefixes, then one block scan of the six thread totals
#pragma unroll
            for (int u = 1; u < WN_PER; ++u)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    P[u][k] += P[u - 1][k];
                    Q[u][k] += Q[u - 1][k];
                }
            double v[6], tot[6];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[k] = P[WN_PER - 1][k];
                v[3 + k] = Q[WN_PER - 1][k];
            }
            wn_block_scan<6>(v, wsum, tot);
#pragma unroll
            for (int u = 0; u < WN_PER; ++u) {
                const int j = j0 + u;
                if (j >= tnum) break;
                // exclusive prefixes at column j: the thread's offset plus its own elements before u
                const double pe1 = v[0] + (u ? P[u - 1][0] : 0.0), pe2 = v[1] + (u ? P[u - 1][1] : 0.0),
                             pec = v[2] + (u ? P[u - 1][2] : 0.0);
                const double qe1 = v[3] + (u ? Q[u - 1][0] : 0.0), qe2 = v[4] + (u ? Q[u - 1][1] : 0.0),
                             qec = v[5] + (u ? Q[u - 1][2] : 0.0);
                double s1 = (t1 + qe1) - pe1, s2 = (t2 + qe2) - pe2, sc = (tc + qec) - pec;
                if (n == 1) {   // no horizontal sum: exact, so that a (1, 1) window has lVar == 0 exactly
                    s1 = V1[ro + j];
                    s2 = V2[ro + j];
                    sc = (double)Vc[ro + j];
                }
                // padded columns: z = m zeros each.  They move the mean by -z p / N.  The fp64 variance is taken about
                // the mean of the pivots, p over the N - z in-array elements and 0 over the z padded ones: that adds
                // z (N - z) p**2 / N**2 + 2 z p s1 / N**2 to the variance about p of the in-array part.  Entering the
                // zeros as z (0 - p) and z p**2 like any other element is the same number, but cancels to nothing once
                // the window is much larger than the image (float32: fl32(0 * 0) = 0 adds nothing to s2).
                const int npc = (lo_h - j > 0 ? lo_h - j : 0) + (j + hi_h - (tnum - 1) > 0 ? j + hi_h - (tnum - 1) : 0);
                const double z = (double)npc * (double)m;
                double mean, var;
                if (sc > 0.0) {
                    mean = __builtin_nan("");
                    var = __builtin_nan("");
                } else {
                    const double eu = s1 / N;
                    mean = p + (npc ? (s1 - z * p) / N : eu);
                    if (sizeof(T) == 8) {
                        var = s2 / N - eu * eu;
                        if (npc) var += z * (p * (2.0 * s1 + p * (N - z))) / (N * N);
                    } else {
                        var = s2 / N - mean * mean;
                    }
                }
                if (MODE == 0) {
                    acc += var;
                } else {
                    const double xv = (double)x[ro + j];
                    out[ro + j] = var < noise ? mean : (xv - mean) * (1.0 - noise / var) + mean;
                }
            }
            t1 += tot[3] - tot[0];
            t2 += tot[4] - tot[1];
            tc += tot[5] - tot[2];
        }
        if (MODE == 0) {
            const double s = wn_block_sum(acc, red);
            if (threadIdx.x == 0) rowsum[t] = s;
        }
    }
}

// noise = sum(rowsum) / (snum * tnum), summed in a fixed order by one workgroup
__global__ __launch_bounds__(WN_BLOCK) void wn_noise_kernel(const double *__restrict__ rowsum, int snum, double count,
                                                            double *__restrict__ noise)
{
    __shared__ double red[WN_BLOCK / 64];
    double s = 0.0;
    for (int t = threadIdx.x; t < snum; t += WN_BLOCK) s += rowsum[t];
    s = wn_block_sum(s, red);
    if (threadIdx.x == 0) *noise = s / count;
}

// ------------------------------------------------------------------------------------------------ median

// scipy.ndimage 'reflect' (d c b a | a b c d | d c b a), any distance from the array
__device__ __forceinline__ int md_reflect(int j, int L)
{
    const int per = 2 * L;
    j %= per;
    if (j < 0) j += per;
    return j < L ? j : per - 1 - j;
}

template <typename T> __device__ __forceinline__ T md_inf();
template <> __device__ __forceinline__ float md_inf<float>() { return __builtin_huge_valf(); }
template <> __device__ __forceinline__ double md_inf<double>() { return __builtin_huge_val(); }

template <typename T, int NB>
__global__ __launch_bounds__(256) void med_small_kernel(const T *__restrict__ x, T *__restrict__ out, int snum,
                                                        int tnum, int m, int n)
{
    __shared__ T tile[MD_LDS];
    __shared__ int offs[MD_SMALL];
    const int lo_v = m / 2, lo_h = n / 2;
    const int LW = MD_TW + n - 1, LH = MD_TR + m - 1;
    const int r0 = blockIdx.y * MD_TR, c0 = blockIdx.x * MD_TW;
    for (int k = threadIdx.x; k < LH * LW; k += 256) {
        const int a = k / LW, b = k - a * LW;
        const int r = md_reflect(r0 - lo_v + a, snum), c = md_reflect(c0 - lo_h + b, tnum);
        tile[k] = x[(size_t)r * tnum + c];
    }
    const int N = m * n;
    if (threadIdx.x < N) {
        const int a = threadIdx.x / n;
        offs[threadIdx.x] = a * LW + (threadIdx.x - a * n);
    }
    __syncthreads();
    const int kth = N / 2;
    for (int q = threadIdx.x; q < MD_TR * MD_TW; q += 256) {
        const int a = q / MD_TW, b = q - a * MD_TW;
        const int t = r0 + a, c = c0 + b;
        if (t >= snum || c >= tnum) continue;
        const int base = a * LW + b;
        T v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = k < N ? tile[base + offs[k]] : md_inf<T>();
        // bitonic sort, ascending
#pragma unroll
        for (int size = 2; size <= NB; size <<= 1)
#pragma unroll
            for (int stride = size >> 1; stride > 0; stride >>= 1)
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    const int l = i ^ stride;
                    if (l > i) {
                        const T lo = v[i] < v[l] ? v[i] : v[l];
                        const T hi = v[i] < v[l] ? v[l] : v[i];
                        if ((i & size) == 0) {
                            v[i] = lo;
                            v[l] = hi;
                        } else {
                            v[i] = hi;
                            v[l] = lo;
                        }
                    }
                }
        T r = v[0];
#pragma unroll
        for (int k = 1; k < NB; ++k)
            if (k == kth) r = v[k];
        out[(size_t)t * tnum + c] = r;
    }
}

// order-preserving unsigned keys
template <typename T> struct MdKey;
template <> struct MdKey<float> {
    typedef unsigned int U;
    static constexpr int BITS = 32;
    __device__ static U key(float v)
    {
        const U u = __float_as_uint(v);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    __device__ static float val(U k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
};
template <> struct MdKey<double> {
    typedef unsigned long long U;
    static constexpr int BITS = 64;
    __device__ static U key(double v)
    {
        const U u = (U)__double_as_longlong(v);
        return (u >> 63) ? ~u : (u | (1ull << 63));
    }
    __device__ static double val(U k)
    {
        return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
    }
};

template <typename T>
__global__ __launch_bounds__(256) void med_radix_kernel(const T *__restrict__ x, T *__restrict__ out, int snum,
                                                        int tnum, int m, int n)
{
    typedef typename MdKey<T>::U U;
    __shared__ int hist[16][256];
    const int c = blockIdx.x * 256 + threadIdx.x;
    const bool live = c < tnum;
    const int lo_v = m / 2, lo_h = n / 2;
    for (int t = blockIdx.y; t < snum; t += gridDim.y) {
        int kth = (m * n) / 2;        // rank still to find among the candidates that share `prefix`
        U prefix = 0;
        for (int shift = MdKey<T>::BITS - 4; shift >= 0; shift -= 4) {
#pragma unroll
            for (int b = 0; b < 16; ++b) hist[b][threadIdx.x] = 0;
            if (live) {
                const int hs = shift + 4;
                for (int a = 0; a < m; ++a) {
                    const T *xr = x + (size_t)md_reflect(t - lo_v + a, snum) * tnum;
                    for (int b = 0; b < n; ++b) {
                        const U k = MdKey<T>::key(xr[md_reflect(c - lo_h + b, tnum)]);
                        const bool match = hs >= MdKey<T>::BITS || (k >> hs) == (prefix >> hs);
                        if (match) ++hist[(k >> shift) & 15][threadIdx.x];
                    }
                }
                int b = 0;
                for (; b < 15; ++b) {
                    const int h = hist[b][threadIdx.x];
                    if (kth < h) break;
                    kth -= h;
                }
                prefix |= (U)b << shift;
            }
        }
        if (live) out[(size_t)t * tnum + c] = MdKey<T>::val(prefix);
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct DenoiseBufs {
    DevBuf in, out, v1, v2, vc, rowsum, noise;
    void release()
    {
        in.release();
        out.release();
        v1.release();
        v2.release();
        vc.release();
        rowsum.release();
        noise.release();
    }
};
static StepScratch<DenoiseBufs> g_dn;

void impdar_denoise_forget(impdar_ctx *ctx) { g_dn.forget(ctx); }

// `name` is the entry point's, as the messages have always carried it
static int dn_check(const char *name, impdar_ctx *ctx, const void *data, const void *out, int dtype, int snum, int tnum,
                    int vert_win, int hor_win)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "%s: null argument", name);
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "%s: dtype must be float32 or float64", name);
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "%s: empty radargram", name);
    IMPDAR_ARG_CHECK(vert_win >= 1 && hor_win >= 1, "%s: window sizes must be at least 1, got (%d, %d)", name, vert_win, hor_win);
    IMPDAR_ARG_CHECK(vert_win < (1 << 30) && hor_win < (1 << 30) && (long long)vert_win * hor_win <= 0x7fffffffLL,
                     "%s: window of %d x %d elements is too large", name, vert_win, hor_win);
    return IMPDAR_OK;
}

template <typename T>
static int wn_run(impdar_ctx *ctx, const T *d_x, int snum, int tnum, int m, int n, double noise, int noise_given,
                  double *d_out, double *noise_used)
{
    const size_t ne = (size_t)snum * tnum;
    IMPDAR_HIP_CHECK(g_dn.v1.ensure(ne * sizeof(double)));
    IMPDAR_HIP_CHECK(g_dn.v2.ensure(ne * sizeof(double)));
    IMPDAR_HIP_CHECK(g_dn.vc.ensure(ne * sizeof(int)));
    double *V1 = g_dn.v1.as<double>(), *V2 = g_dn.v2.as<double>();
    int *Vc = g_dn.vc.as<int>();
    const dim3 gv((tnum + WN_BLOCK - 1) / WN_BLOCK, (snum + WN_RS - 1) / WN_RS);
    hipLaunchKernelGGL(wn_vsum_kernel<T>, gv, dim3(WN_BLOCK), 0, ctx->stream, d_x, V1, V2, Vc, snum, tnum, m / 2,
                       (m - 1) / 2);
    const int nblk = snum < WN_MAX_ROW_BLOCKS ? snum : WN_MAX_ROW_BLOCKS;
    if (!noise_given) {
        IMPDAR_HIP_CHECK(g_dn.rowsum.ensure((size_t)snum * sizeof(double)));
        IMPDAR_HIP_CHECK(g_dn.noise.ensure(sizeof(double)));
        hipLaunchKernelGGL((wn_hsum_kernel<T, 0>), dim3(nblk), dim3(WN_BLOCK), 0, ctx->stream, d_x, V1, V2, Vc,
                           g_dn.rowsum.as<double>(), (double *)nullptr, snum, tnum, m, n, 0.0);
        hipLaunchKernelGGL(wn_noise_kernel, dim3(1), dim3(WN_BLOCK), 0, ctx->stream, g_dn.rowsum.as<double>(), snum,
                           (double)ne, g_dn.noise.as<double>());
        IMPDAR_HIP_CHECK(hipGetLastError());
        IMPDAR_HIP_CHECK(hipMemcpyAsync(&noise, g_dn.noise.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        // the reference raises when a window has no variance; here only when none has
        IMPDAR_ARG_CHECK(noise != 0.0, "Could not compute variance, specify noise for denoise");
    }
    hipLaunchKernelGGL((wn_hsum_kernel<T, 1>), dim3(nblk), dim3(WN_BLOCK), 0, ctx->stream, d_x, V1, V2, Vc,
                       (double *)nullptr, d_out, snum, tnum, m, n, noise);
    IMPDAR_HIP_CHECK(hipGetLastError());
    if (noise_used) *noise_used = noise;
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_wiener_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int vert_win,
                                 int hor_win, double noise, int noise_given, double *d_out, double *noise_used)
{
    const auto lock = g_dn.lock();
    const int rc = dn_check("impdar_wiener", ctx, d_data, d_out, dtype, snum, tnum, vert_win, hor_win);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_dn.bind(ctx);
    if (dtype == IMPDAR_F32)
        return wn_run(ctx, (const float *)d_data, snum, tnum, vert_win, hor_win, noise, noise_given, d_out, noise_used);
    return wn_run(ctx, (const double *)d_data, snum, tnum, vert_win, hor_win, noise, noise_given, d_out, noise_used);
}

template <typename T>
static void md_launch(impdar_ctx *ctx, const T *d_x, T *d_out, int snum, int tnum, int m, int n)
{
    const int N = m * n;
    const dim3 gs((tnum + MD_TW - 1) / MD_TW, (snum + MD_TR - 1) / MD_TR);
    if (N <= 16)
        hipLaunchKernelGGL((med_small_kernel<T, 16>), gs, dim3(256), 0, ctx->stream, d_x, d_out, snum, tnum, m, n);
    else if (N <= 32)
        hipLaunchKernelGGL((med_small_kernel<T, 32>), gs, dim3(256), 0, ctx->stream, d_x, d_out, snum, tnum, m, n);
    else if (N <= MD_SMALL)
        hipLaunchKernelGGL((med_small_kernel<T, 64>), gs, dim3(256), 0, ctx->stream, d_x, d_out, snum, tnum, m, n);
    else
        hipLaunchKernelGGL(med_radix_kernel<T>, dim3((tnum + 255) / 256, snum < 65535 ? snum : 65535), dim3(256), 0,
                           ctx->stream, d_x, d_out, snum, tnum, m, n);
}

extern "C" int impdar_median_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int vert_win,
                                 int hor_win, void *d_out)
{
    const auto lock = g_dn.lock();
    const int rc = dn_check("impdar_median", ctx, d_data, d_out, dtype, snum, tnum, vert_win, hor_win);
    if (rc) return rc;
    IMPDAR_ARG_CHECK(d_out != d_data, "impdar_median: the output must be a separate buffer");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    if (dtype == IMPDAR_F32)
        md_launch(ctx, (const float *)d_data, (float *)d_out, snum, tnum, vert_win, hor_win);
    else
        md_launch(ctx, (const double *)d_data, (double *)d_out, snum, tnum, vert_win, hor_win);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer forms: the argument check, then StepScratch::host_form ----------------------------------

extern "C" int impdar_wiener(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int vert_win,
                             int hor_win, double noise, int noise_given, double *out, double *noise_used)
{
    const int rc = dn_check("impdar_wiener", ctx, data, out, dtype, snum, tnum, vert_win, hor_win);
    if (rc) return rc;
    const size_t ne = (size_t)snum * tnum;
    return g_dn.host_form(ctx, g_dn.in, data, ne * impdar_dtype_size(dtype), &g_dn.out, out, ne * sizeof(double),
                          [&](void *d_in, void *d_out) {
                              return impdar_wiener_dev(ctx, d_in, dtype, snum, tnum, vert_win, hor_win, noise, noise_given,
                                                       (double *)d_out, noise_used);
                          });
}

extern "C" int impdar_median(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int vert_win,
                             int hor_win, void *out)
{
    const int rc = dn_check("impdar_median", ctx, data, out, dtype, snum, tnum, vert_win, hor_win);
    if (rc) return rc;
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    return g_dn.host_form(ctx, g_dn.in, data, bytes, &g_dn.out, out, bytes, [&](void *d_in, void *d_out) {
        return impdar_median_dev(ctx, d_in, dtype, snum, tnum, vert_win, hor_win, d_out);
    });
}
