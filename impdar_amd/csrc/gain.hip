// The two gains of a processing chain, kept on the device so that a radargram stays resident across them
// (reference src/impdar/lib/RadarData/_RadarDataProcessing.py:456-496):
//
//   * rangegain(slope): sample i of trace j is multiplied by travel_time[i] * slope from the sample after the
//       trace's trigger on.  NumPy's in-place float32 *= float64 is an fp64 product rounded once:
//         x[i, j] = (T)((double)x[i, j] * g[i])  for i >= start[j]                          (rowwise_kernel)
//   * agc(window, scaling_factor): every sample row is scaled by scaling_factor over the largest |x| of the
//       window // 2 rows above it and the window // 2 - 1 rows below it (half-open, as the reference's slice):
//         agc_rowmax_kernel  one workgroup per row (persistent over rows): max |x| of the row, a NaN in the row
//                            making it NaN as np.max does;
//         agc_scale_kernel   one thread per row: the maximum over the window of that snum-long vector, zeros
//                            replaced by 1e-6, s[i] = (T)(scaling_factor / m) formed in fp64;
//         rowwise_kernel     x[i, j] *= s[i] in the data's own arithmetic.
//
// Every operation is a maximum or one rounding, so both steps equal NumPy bit for bit.  Data is (snum, tnum)
// row-major.  The file is compiled with -ffp-contract=off, like the rest of the library.
#include "rowwise.h"

#define AG_BLOCK 256
#define AG_MAX_ROW_BLOCKS 2048   // resident workgroups of agc_rowmax_kernel

template <typename T> struct RangeGain {
    const double *g;     // snum: travel_time * slope
    const int *start;    // tnum: first row of the trace that is multiplied
    template <int V> __device__ __forceinline__ void operator()(int i, int j, T (&v)[V]) const
    {
        const double gi = g[i];
#pragma unroll
        for (int c = 0; c < V; ++c)
            if (i >= start[j + c]) v[c] = (T)((double)v[c] * gi);
    }
};

template <typename T> struct RowScale {
    const T *s;          // snum
    template <int V> __device__ __forceinline__ void operator()(int i, int, T (&v)[V]) const
    {
        const T si = s[i];
#pragma unroll
        for (int c = 0; c < V; ++c) v[c] = v[c] * si;
    }
};

// the larger of two values that are not NaN, or NaN if either is (fmax would drop the NaN)
__device__ __forceinline__ double ag_nanmax(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
}

// |x| is exact in fp64 for both dtypes, so one reduction serves them
template <typename T, int V>
__global__ __launch_bounds__(AG_BLOCK) void agc_rowmax_kernel(const T *__restrict__ x, double *__restrict__ rowmax,
                                                              int snum, int tnum)
{
    typedef RwVec<T, V> Vec;
    __shared__ double red[AG_BLOCK / 64];
    const int nvec = tnum / V;   // tnum % V == 0
    for (int i = blockIdx.x; i < snum; i += gridDim.x) {
        const T *xr = x + (size_t)i * tnum;
        double m = 0.0;
#pragma unroll 4
        for (int k = threadIdx.x; k < nvec; k += AG_BLOCK) {
            const Vec y = rw_load<T, V>(xr + (size_t)k * V);
#pragma unroll
            for (int c = 0; c < V; ++c) m = ag_nanmax(m, fabs((double)y.v[c]));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = ag_nanmax(m, __shfl_xor(m, o, 64));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) rowmax[i] = ag_nanmax(ag_nanmax(red[0], red[1]), ag_nanmax(red[2], red[3]));
        __syncthreads();   // red is rewritten for the next row
    }
}

template <typename T>
__global__ __launch_bounds__(AG_BLOCK) void agc_scale_kernel(const double *__restrict__ rowmax, T *__restrict__ scale,
                                                             int snum, int half, double scaling)
{
    const int i = blockIdx.x * AG_BLOCK + threadIdx.x;
    if (i >= snum) return;
    const int a = i - half > 0 ? i - half : 0;
    const int b = (long long)i + half < snum ? i + half : snum;
    double m = rowmax[a];   // a < b: half >= 1
    for (int k = a + 1; k < b; ++k) m = ag_nanmax(m, rowmax[k]);
    if (m == 0.0) m = 1.0e-6;
    scale[i] = (T)(scaling / m);
}

// ------------------------------------------------------------------------------------------------ host side

struct GainBufs {
    DevBuf data, tab, rowmax, scale;   // staging of the host-buffer forms, the host tables, the two agc vectors
    void release()
    {
        data.release();
        tab.release();
        rowmax.release();
        scale.release();
    }
};
static StepScratch<GainBufs> g_gn;

void impdar_gain_forget(impdar_ctx *ctx) { g_gn.forget(ctx); }

static int rangegain_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *gain, const int *start)
{
    IMPDAR_ARG_CHECK(ctx && data && gain && start, "impdar_rangegain: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_rangegain: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_rangegain: empty radargram");
    return IMPDAR_OK;
}

extern "C" int impdar_rangegain_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, const double *gain,
                                    const int *start)
{
    const auto lock = g_gn.lock();
    int rc = rangegain_check(ctx, d_data, dtype, snum, tnum, gain, start);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_gn.bind(ctx);
    const void *d_tab[2];
    rc = impdar_upload_tables(ctx, g_gn.tab, {{gain, (size_t)snum * sizeof(double)}, {start, (size_t)tnum * sizeof(int)}}, d_tab);
    if (rc) return rc;
    rowwise_launch(ctx, d_data, dtype, snum, tnum, [&](auto t) {
        return RangeGain<typename decltype(t)::type>{(const double *)d_tab[0], (const int *)d_tab[1]};
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// max |x| of every row of a resident array into g_gn.rowmax
static int gn_rowmax(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum)
{
    IMPDAR_HIP_CHECK(g_gn.rowmax.ensure((size_t)snum * sizeof(double)));
    const int nblk = snum < AG_MAX_ROW_BLOCKS ? snum : AG_MAX_ROW_BLOCKS;
    rw_dispatch(dtype, {d_data}, tnum, [&](auto t, auto v) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL((agc_rowmax_kernel<T, decltype(v)::value>), dim3(nblk), dim3(AG_BLOCK), 0, ctx->stream,
                           (const T *)d_data, g_gn.rowmax.as<double>(), snum, tnum);
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

static int agc_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int half)
{
    IMPDAR_ARG_CHECK(ctx && data, "impdar_agc: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_agc: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_agc: empty radargram");
    IMPDAR_ARG_CHECK(half >= 1, "impdar_agc: window // 2 = %d leaves no sample to take the maximum of", half);
    return IMPDAR_OK;
}

extern "C" int impdar_agc_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, int half, double scaling)
{
    const auto lock = g_gn.lock();
    int rc = agc_check(ctx, d_data, dtype, snum, tnum, half);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_gn.bind(ctx);
    rc = gn_rowmax(ctx, d_data, dtype, snum, tnum);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(g_gn.scale.ensure((size_t)snum * impdar_dtype_size(dtype)));
    const dim3 grid((snum + AG_BLOCK - 1) / AG_BLOCK);
    rw_typed(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(agc_scale_kernel<T>, grid, dim3(AG_BLOCK), 0, ctx->stream, g_gn.rowmax.as<double>(),
                           g_gn.scale.as<T>(), snum, half, scaling);
    });
    rowwise_launch(ctx, d_data, dtype, snum, tnum,
                   [&](auto t) { return RowScale<typename decltype(t)::type>{g_gn.scale.as<typename decltype(t)::type>()}; });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer forms: the argument check, then StepScratch::host_form ----------------------------------

extern "C" int impdar_rangegain(impdar_ctx *ctx, void *data, int dtype, int snum, int tnum, const double *gain,
                                const int *start)
{
    const int rc = rangegain_check(ctx, data, dtype, snum, tnum, gain, start);
    if (rc) return rc;
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    return g_gn.host_form(ctx, g_gn.data, data, bytes, nullptr, data, bytes,
                          [&](void *d, void *) { return impdar_rangegain_dev(ctx, d, dtype, snum, tnum, gain, start); });
}

extern "C" int impdar_agc(impdar_ctx *ctx, void *data, int dtype, int snum, int tnum, int half, double scaling)
{
    const int rc = agc_check(ctx, data, dtype, snum, tnum, half);
    if (rc) return rc;
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    return g_gn.host_form(ctx, g_gn.data, data, bytes, nullptr, data, bytes,
                          [&](void *d, void *) { return impdar_agc_dev(ctx, d, dtype, snum, tnum, half, scaling); });
}

extern "C" int impdar_row_absmax(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, double *rowmax)
{
    IMPDAR_ARG_CHECK(ctx && data && rowmax, "impdar_row_absmax: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_row_absmax: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_row_absmax: empty radargram");
    return g_gn.host_form(ctx, g_gn.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype), &g_gn.rowmax, rowmax,
                          (size_t)snum * sizeof(double), [&](void *d, void *) { return gn_rowmax(ctx, d, dtype, snum, tnum); });
}
