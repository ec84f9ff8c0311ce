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

static bool gn_float(int dtype) { return dtype == IMPDAR_F32 || dtype == IMPDAR_F64; }

extern "C" int impdar_rangegain_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, const double *gain,
                                    const int *start)
{
    const auto lock = g_gn.lock();
    IMPDAR_ARG_CHECK(ctx && d_data && gain && start, "impdar_rangegain: null argument");
    IMPDAR_ARG_CHECK(gn_float(dtype), "impdar_rangegain: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_rangegain: empty radargram");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_gn.bind(ctx);
    // the tables are small: one packed synchronous copy keeps the caller's host arrays free to go away (the stream
    // is drained first because the previous launch may still read the table buffer)
    const size_t db = (size_t)snum * sizeof(double), ib = (size_t)tnum * sizeof(int);
    std::vector<char> pack(db + ib);
    memcpy(pack.data(), gain, db);
    memcpy(pack.data() + db, start, ib);
    IMPDAR_HIP_CHECK(g_gn.tab.ensure(pack.size()));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    IMPDAR_HIP_CHECK(hipMemcpy(g_gn.tab.p, pack.data(), pack.size(), hipMemcpyHostToDevice));
    const double *d_gain = g_gn.tab.as<double>();
    const int *d_start = (const int *)(g_gn.tab.as<char>() + db);
    if (dtype == IMPDAR_F32) rowwise_launch(ctx, (float *)d_data, snum, tnum, RangeGain<float>{d_gain, d_start});
    else rowwise_launch(ctx, (double *)d_data, snum, tnum, RangeGain<double>{d_gain, d_start});
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

template <typename T, int V> static void agc_rowmax_launch(impdar_ctx *ctx, const void *d_data, double *d_rowmax, int snum, int tnum)
{
    const int nblk = snum < AG_MAX_ROW_BLOCKS ? snum : AG_MAX_ROW_BLOCKS;
    hipLaunchKernelGGL((agc_rowmax_kernel<T, V>), dim3(nblk), dim3(AG_BLOCK), 0, ctx->stream, (const T *)d_data, d_rowmax,
                       snum, tnum);
}

// max |x| of every row of a resident array into g_gn.rowmax
static int gn_rowmax(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum)
{
    IMPDAR_HIP_CHECK(g_gn.rowmax.ensure((size_t)snum * sizeof(double)));
    double *d_rowmax = g_gn.rowmax.as<double>();
    const bool wide = rw_aligned16(d_data);
    if (dtype == IMPDAR_F32) {
        if (wide && tnum % 4 == 0) agc_rowmax_launch<float, 4>(ctx, d_data, d_rowmax, snum, tnum);
        else if (wide && tnum % 2 == 0) agc_rowmax_launch<float, 2>(ctx, d_data, d_rowmax, snum, tnum);
        else agc_rowmax_launch<float, 1>(ctx, d_data, d_rowmax, snum, tnum);
    } else {
        if (wide && tnum % 2 == 0) agc_rowmax_launch<double, 2>(ctx, d_data, d_rowmax, snum, tnum);
        else agc_rowmax_launch<double, 1>(ctx, d_data, d_rowmax, snum, tnum);
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

extern "C" int impdar_agc_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, int half, double scaling)
{
    const auto lock = g_gn.lock();
    IMPDAR_ARG_CHECK(ctx && d_data, "impdar_agc: null argument");
    IMPDAR_ARG_CHECK(gn_float(dtype), "impdar_agc: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_agc: empty radargram");
    IMPDAR_ARG_CHECK(half >= 1, "impdar_agc: window // 2 = %d leaves no sample to take the maximum of", half);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_gn.bind(ctx);
    const int rc = gn_rowmax(ctx, d_data, dtype, snum, tnum);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(g_gn.scale.ensure((size_t)snum * impdar_dtype_size(dtype)));
    const dim3 grid((snum + AG_BLOCK - 1) / AG_BLOCK);
    if (dtype == IMPDAR_F32) {
        hipLaunchKernelGGL(agc_scale_kernel<float>, grid, dim3(AG_BLOCK), 0, ctx->stream, g_gn.rowmax.as<double>(),
                           g_gn.scale.as<float>(), snum, half, scaling);
        rowwise_launch(ctx, (float *)d_data, snum, tnum, RowScale<float>{g_gn.scale.as<float>()});
    } else {
        hipLaunchKernelGGL(agc_scale_kernel<double>, grid, dim3(AG_BLOCK), 0, ctx->stream, g_gn.rowmax.as<double>(),
                           g_gn.scale.as<double>(), snum, half, scaling);
        rowwise_launch(ctx, (double *)d_data, snum, tnum, RowScale<double>{g_gn.scale.as<double>()});
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer forms: upload, run, download ------------------------------------------------------------

extern "C" int impdar_rangegain(impdar_ctx *ctx, void *data, int dtype, int snum, int tnum, const double *gain,
                                const int *start)
{
    const auto lock = g_gn.lock();
    IMPDAR_ARG_CHECK(ctx && data && gain && start, "impdar_rangegain: null argument");
    IMPDAR_ARG_CHECK(gn_float(dtype), "impdar_rangegain: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_rangegain: empty radargram");
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    int rc = g_gn.stage_in(ctx, g_gn.data, data, bytes);
    if (rc) return rc;
    rc = impdar_rangegain_dev(ctx, g_gn.data.p, dtype, snum, tnum, gain, start);
    if (rc) return rc;
    return impdar_download(ctx, data, g_gn.data.p, bytes, ctx->stream);
}

extern "C" int impdar_agc(impdar_ctx *ctx, void *data, int dtype, int snum, int tnum, int half, double scaling)
{
    const auto lock = g_gn.lock();
    IMPDAR_ARG_CHECK(ctx && data, "impdar_agc: null argument");
    IMPDAR_ARG_CHECK(gn_float(dtype), "impdar_agc: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_agc: empty radargram");
    IMPDAR_ARG_CHECK(half >= 1, "impdar_agc: window // 2 = %d leaves no sample to take the maximum of", half);
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    int rc = g_gn.stage_in(ctx, g_gn.data, data, bytes);
    if (rc) return rc;
    rc = impdar_agc_dev(ctx, g_gn.data.p, dtype, snum, tnum, half, scaling);
    if (rc) return rc;
    return impdar_download(ctx, data, g_gn.data.p, bytes, ctx->stream);
}

extern "C" int impdar_row_absmax(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, double *rowmax)
{
    const auto lock = g_gn.lock();
    IMPDAR_ARG_CHECK(ctx && data && rowmax, "impdar_row_absmax: null argument");
    IMPDAR_ARG_CHECK(gn_float(dtype), "impdar_row_absmax: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_row_absmax: empty radargram");
    int rc = g_gn.stage_in(ctx, g_gn.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype));
    if (rc) return rc;
    rc = gn_rowmax(ctx, g_gn.data.p, dtype, snum, tnum);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipMemcpyAsync(rowmax, g_gn.rowmax.p, (size_t)snum * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return IMPDAR_OK;
}
