// The two horizontal filters an impproc/impdar chain runs between the band pass and the migration, kept on the
// device so that a radargram stays resident from the first filter to the migrated image:
//
//   * horizontalfilt(ntr1, ntr2)  (reference src/impdar/lib/RadarData/_RadarDataFiltering.py:93-135):
//       every sample row loses mean(row[lo:hi]) * scale[t], the mean and the tapered mean each cast to the data's
//       dtype first (float32 data: float32 mean, float32 subtraction);
//   * adaptivehfilt(window_size)  (:19-90): trace i loses scale[t] * filtfilt([.25]*4, 1, mean(data[:, lo_i:hi_i], -1)).
//       For that 4-tap box filtfilt is exactly the 7-tap stencil [1,2,3,4,3,2,1]/16 on the odd extension of the
//       mean trace (M[-k] = 2 M[0] - M[k], M[snum-1+k] = 2 M[snum-1] - M[snum-1-k], k = 1..3): the 12-sample pad
//       absorbs the steady-state initial conditions before they reach a kept sample.
//
// Data is (snum, tnum) row-major: a row holds one sample of every trace and is contiguous.  adaptivehfilt is two
// passes whose cost does not depend on the window:
//   ahfilt_rowmean_kernel  one workgroup per row (persistent over rows): an fp64 prefix sum of x - x[t, 0] along the
//                          row (chunks of 1024 with a carry, so any tnum), then M[t, i] = x[t, 0] + (P[hi_i] -
//                          P[lo_i]) / (hi_i - lo_i) for the host's window table, NaN for an empty window, stored in
//                          the data's dtype (the reference's mean of float32 data is float32).  The pivot keeps the
//                          difference of two long prefix sums from losing the digits of a row that holds a strong
//                          flat band -- the very thing the filter is for.
//   ahfilt_apply_kernel    one thread per trace walks a strip of rows with M[t-3..t+3] in registers, applies the
//                          stencil and the taper and subtracts in fp64, storing in the data's dtype.
//   * winavg_hfilt(avg_win)  (:353-440): trace i loses scale[t] * mean(data[:, lo_i:hi_i], -1), the mean in the
//       data's dtype, with no vertical smoothing: ahfilt_rowmean_kernel with another window table, then
//       x[t, i] = (T)((double)x[t, i] - (double)M[t, i] * scale[t]) through the in-place frame of rowwise.h.
// The file is compiled with -ffp-contract=off, like the rest of the library.
#include "rowwise.h"

#define HF_BLOCK 256
#define HF_PER 4                          // consecutive elements per thread in one scan chunk
#define HF_CHUNK (HF_BLOCK * HF_PER)
#define HF_ROWS 64                        // rows per thread in ahfilt_apply_kernel
#define HF_MAX_ROW_BLOCKS 2048            // resident workgroups of ahfilt_rowmean_kernel (each owns a prefix-sum row)

// exclusive prefix of one value per thread across the workgroup (fixed order: the host and resident forms agree
// bit for bit); `total` is the workgroup's sum
__device__ __forceinline__ double hf_block_scan(double v, double *wsum, double &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    double ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0.0;
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    double before = 0.0, tot = 0.0;
#pragma unroll
    for (int k = 0; k < HF_BLOCK / 64; ++k) {
        const double s = wsum[k];
        if (k < w) before += s;
        tot += s;
    }
    __syncthreads();   // wsum is rewritten by the next chunk
    total = tot;
    return before + ex;
}

template <typename T>
__global__ __launch_bounds__(HF_BLOCK) void ahfilt_rowmean_kernel(const T *__restrict__ x, T *__restrict__ M,
                                                                  double *__restrict__ Pbuf, const int *__restrict__ lo,
                                                                  const int *__restrict__ hi, int snum, int tnum)
{
    __shared__ double wsum[HF_BLOCK / 64];
    double *P = Pbuf + (size_t)blockIdx.x * (tnum + 1);   // this workgroup's prefix-sum row, P[k] = sum(x[:k] - x[0])
    for (int t = blockIdx.x; t < snum; t += gridDim.x) {
        const T *xr = x + (size_t)t * tnum;
        const double x0 = (double)xr[0];
        double carry = 0.0;
        if (threadIdx.x == 0) P[0] = 0.0;
        for (int c0 = 0; c0 < tnum; c0 += HF_CHUNK) {
            const int j = c0 + threadIdx.x * HF_PER;
            double s[HF_PER];
#pragma unroll
            for (int u = 0; u < HF_PER; ++u) s[u] = j + u < tnum ? (double)xr[j + u] - x0 : 0.0;
#pragma unroll
            for (int u = 1; u < HF_PER; ++u) s[u] += s[u - 1];
            double total;
            const double ex = carry + hf_block_scan(s[HF_PER - 1], wsum, total);
#pragma unroll
            for (int u = 0; u < HF_PER; ++u)
                if (j + u < tnum) P[j + u + 1] = ex + s[u];
            carry += total;
        }
        __syncthreads();   // the whole prefix row is written and visible to the workgroup
        T *Mr = M + (size_t)t * tnum;
#pragma unroll 4
        for (int i = threadIdx.x; i < tnum; i += HF_BLOCK) {
            const int a = lo[i], b = hi[i];
            const double m = b > a ? x0 + (P[b] - P[a]) / (double)(b - a) : __builtin_nan("");
            Mr[i] = (T)m;
        }
        __syncthreads();   // P is rewritten for the next row
    }
}

// row r of the odd extension of the mean traces, in the data's own arithmetic (scipy's odd_ext on a float32 mean
// is a float32 expression), widened; r in [-3, snum + 2] and snum > 12
template <typename T>
__device__ __forceinline__ double hf_mext(const T *__restrict__ M, int r, int i, int snum, int tnum)
{
    if (r < 0) return (double)(T)((T)2 * M[i] - M[(size_t)(-r) * tnum + i]);
    if (r >= snum) {
        const int e = snum - 1;
        return (double)(T)((T)2 * M[(size_t)e * tnum + i] - M[(size_t)(2 * e - r) * tnum + i]);
    }
    return (double)M[(size_t)r * tnum + i];
}

template <typename T>
__global__ __launch_bounds__(256) void ahfilt_apply_kernel(T *__restrict__ x, const T *__restrict__ M,
                                                           const double *__restrict__ scale, int snum, int tnum)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tnum) return;
    const int t0 = blockIdx.y * HF_ROWS;
    const int t1 = t0 + HF_ROWS < snum ? t0 + HF_ROWS : snum;
    double w[7];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = hf_mext(M, t0 - 3 + k, i, snum, tnum);
    for (int t = t0; t < t1; ++t) {
        w[6] = hf_mext(M, t + 3, i, snum, tnum);
        const double s = (w[0] + 2.0 * w[1] + 3.0 * w[2] + 4.0 * w[3] + 3.0 * w[4] + 2.0 * w[5] + w[6]) * 0.0625;
        T *p = x + (size_t)t * tnum + i;
        *p = (T)((double)*p - s * scale[t]);
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = w[k + 1];
    }
}

// the apply pass of winavg_hfilt: the tapered mean trace leaves its trace, in fp64, stored in the data's dtype
template <typename T> struct WinavgApply {
    const T *M;             // (snum, tnum) moving means, as aligned as the data
    const double *scale;    // snum
    int tnum;
    template <int V> __device__ __forceinline__ void operator()(int t, int i, T (&v)[V]) const
    {
        const RwVec<T, V> m = *reinterpret_cast<const RwVec<T, V> *>(M + (size_t)t * tnum + i);
        const double st = scale[t];
#pragma unroll
        for (int c = 0; c < V; ++c) v[c] = (T)((double)v[c] - (double)m.v[c] * st);
    }
};

// one workgroup per row: fp64 sum over [lo, hi), the mean and the tapered mean each cast to T, then the row loses it
// in T's arithmetic (reference: data - (mean(data[:, lo:hi], -1) * scale).astype(data.dtype)[:, None])
template <typename T>
__global__ __launch_bounds__(HF_BLOCK) void hfilt_mean_kernel(T *__restrict__ x, int tnum, int lo, int hi,
                                                              const double *__restrict__ scale)
{
    __shared__ double red[HF_BLOCK / 64];
    const int t = blockIdx.x;
    T *xr = x + (size_t)t * tnum;
    double s = 0.0;
#pragma unroll 4
    for (int j = lo + threadIdx.x; j < hi; j += HF_BLOCK) s += (double)xr[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const double sum = (red[0] + red[1]) + (red[2] + red[3]);
    const T m = (T)(sum / (double)(hi - lo));
    const T a = (T)((double)m * scale[t]);
#pragma unroll 8
    for (int j = threadIdx.x; j < tnum; j += HF_BLOCK) xr[j] = xr[j] - a;
}

// ------------------------------------------------------------------------------------------------ host side

struct HfiltBufs {
    DevBuf data, M, P, tab;
    // pinned staging of the small host tables: copied on the stream without draining it; the next call waits only for
    // the previous table copy before it reuses the buffer
    void *host = nullptr;
    size_t host_bytes = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    void release()
    {
        data.release();
        M.release();
        P.release();
        tab.release();
        if (pending && ev) (void)hipEventSynchronize(ev);
        if (host) (void)hipHostFree(host);
        if (ev) (void)hipEventDestroy(ev);
        host = nullptr;
        host_bytes = 0;
        ev = nullptr;
        pending = false;
    }
};
static StepScratch<HfiltBufs> g_hf;

void impdar_hfilt_forget(impdar_ctx *ctx) { g_hf.forget(ctx); }

// the tables of `blk` into the device table buffer at 16-byte-rounded offsets, enqueued on the compute stream; their
// device addresses into `dev`
template <int N> static int hf_upload_tables(impdar_ctx *ctx, const TableBlock (&blk)[N], const void *(&dev)[N])
{
    size_t total = 0;
    for (int k = 0; k < N; ++k) total += impdar_round16(blk[k].bytes);
    if (g_hf.pending) IMPDAR_HIP_CHECK(hipEventSynchronize(g_hf.ev));
    g_hf.pending = false;
    if (!g_hf.ev) IMPDAR_HIP_CHECK(hipEventCreateWithFlags(&g_hf.ev, hipEventDisableTiming));
    if (g_hf.host_bytes < total) {
        if (g_hf.host) IMPDAR_HIP_CHECK(hipHostFree(g_hf.host));
        g_hf.host = nullptr;
        g_hf.host_bytes = 0;
        IMPDAR_HIP_CHECK(hipHostMalloc(&g_hf.host, total, hipHostMallocDefault));
        g_hf.host_bytes = total;
    }
    IMPDAR_HIP_CHECK(g_hf.tab.ensure(total));
    size_t off = 0;
    for (int k = 0; k < N; ++k) {
        memcpy((char *)g_hf.host + off, blk[k].src, blk[k].bytes);
        dev[k] = g_hf.tab.as<char>() + off;
        off += impdar_round16(blk[k].bytes);
    }
    IMPDAR_HIP_CHECK(hipMemcpyAsync(g_hf.tab.p, g_hf.host, total, hipMemcpyHostToDevice, ctx->stream));
    IMPDAR_HIP_CHECK(hipEventRecord(g_hf.ev, ctx->stream));
    g_hf.pending = true;
    return IMPDAR_OK;
}

// the moving means of ahfilt and winavg: the scratch arrays, the three tables, the row-mean launch
template <class Apply>
static int hf_windowed(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, const int *lo, const int *hi,
                       const double *scale, const Apply &apply)
{
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_hf.bind(ctx);
    const int nblk = snum < HF_MAX_ROW_BLOCKS ? snum : HF_MAX_ROW_BLOCKS;
    IMPDAR_HIP_CHECK(g_hf.M.ensure((size_t)snum * tnum * impdar_dtype_size(dtype)));
    IMPDAR_HIP_CHECK(g_hf.P.ensure((size_t)nblk * (tnum + 1) * sizeof(double)));
    const size_t ib = (size_t)tnum * sizeof(int);
    const void *d_tab[3];
    const int rc = hf_upload_tables(ctx, {{scale, (size_t)snum * sizeof(double)}, {lo, ib}, {hi, ib}}, d_tab);
    if (rc) return rc;
    rw_typed(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(ahfilt_rowmean_kernel<T>, dim3(nblk), dim3(HF_BLOCK), 0, ctx->stream, (const T *)d_data,
                           g_hf.M.as<T>(), g_hf.P.as<double>(), (const int *)d_tab[1], (const int *)d_tab[2], snum, tnum);
    });
    apply((const double *)d_tab[0]);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

static int hfilt_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int lo, int hi, const double *scale)
{
    IMPDAR_ARG_CHECK(ctx && data && scale, "impdar_hfilt: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_hfilt: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_hfilt: empty radargram");
    IMPDAR_ARG_CHECK(lo >= 0 && lo < hi && hi <= tnum, "impdar_hfilt: trace range [%d, %d) not inside [0, %d)", lo, hi, tnum);
    return IMPDAR_OK;
}

extern "C" int impdar_hfilt_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, int lo, int hi,
                                const double *scale)
{
    const auto lock = g_hf.lock();
    int rc = hfilt_check(ctx, d_data, dtype, snum, tnum, lo, hi, scale);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_hf.bind(ctx);
    const void *d_tab[1];
    rc = hf_upload_tables(ctx, {{scale, (size_t)snum * sizeof(double)}}, d_tab);
    if (rc) return rc;
    rw_typed(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(hfilt_mean_kernel<T>, dim3(snum), dim3(HF_BLOCK), 0, ctx->stream, (T *)d_data, tnum, lo, hi,
                           (const double *)d_tab[0]);
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

static int ahfilt_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *lo, const int *hi,
                        const double *scale)
{
    IMPDAR_ARG_CHECK(ctx && data && lo && hi && scale, "impdar_ahfilt: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_ahfilt: dtype must be float32 or float64");
    // scipy.signal.filtfilt's own guard and message (padlen = 3 * 4 taps)
    IMPDAR_ARG_CHECK(snum > 12, "The length of the input vector x must be greater than padlen, which is %d.", 12);
    IMPDAR_ARG_CHECK(tnum >= 1, "impdar_ahfilt: empty radargram");
    for (int i = 0; i < tnum; ++i)
        IMPDAR_ARG_CHECK(lo[i] >= 0 && lo[i] <= hi[i] && hi[i] <= tnum,
                         "impdar_ahfilt: window [%d, %d) of trace %d not inside [0, %d]", lo[i], hi[i], i, tnum);
    return IMPDAR_OK;
}

extern "C" int impdar_ahfilt_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, const int *lo,
                                 const int *hi, const double *scale)
{
    const auto lock = g_hf.lock();
    const int rc = ahfilt_check(ctx, d_data, dtype, snum, tnum, lo, hi, scale);
    if (rc) return rc;
    const dim3 grid2((tnum + 255) / 256, (snum + HF_ROWS - 1) / HF_ROWS);
    return hf_windowed(ctx, d_data, dtype, snum, tnum, lo, hi, scale, [&](const double *d_scale) {
        rw_typed(dtype, [&](auto t) {
            typedef typename decltype(t)::type T;
            hipLaunchKernelGGL(ahfilt_apply_kernel<T>, grid2, dim3(256), 0, ctx->stream, (T *)d_data, (const T *)g_hf.M.as<T>(),
                               d_scale, snum, tnum);
        });
    });
}

static int winavg_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *lo, const int *hi,
                        const double *scale)
{
    IMPDAR_ARG_CHECK(ctx && data && lo && hi && scale, "impdar_winavg: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_winavg: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_winavg: empty radargram");
    for (int i = 0; i < tnum; ++i)
        IMPDAR_ARG_CHECK(lo[i] >= 0 && lo[i] <= hi[i] && hi[i] <= tnum,
                         "impdar_winavg: window [%d, %d) of trace %d not inside [0, %d]", lo[i], hi[i], i, tnum);
    return IMPDAR_OK;
}

extern "C" int impdar_winavg_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, const int *lo,
                                 const int *hi, const double *scale)
{
    const auto lock = g_hf.lock();
    const int rc = winavg_check(ctx, d_data, dtype, snum, tnum, lo, hi, scale);
    if (rc) return rc;
    return hf_windowed(ctx, d_data, dtype, snum, tnum, lo, hi, scale, [&](const double *d_scale) {
        rowwise_launch(ctx, d_data, dtype, snum, tnum, [&](auto t) {
            typedef typename decltype(t)::type T;
            return WinavgApply<T>{g_hf.M.as<T>(), d_scale, tnum};
        });
    });
}

// ---- host-buffer forms: the argument check, then StepScratch::host_form ----------------------------------

extern "C" int impdar_hfilt(impdar_ctx *ctx, void *data, int dtype, int snum, int tnum, int lo, int hi,
                            const double *scale)
{
    const int rc = hfilt_check(ctx, data, dtype, snum, tnum, lo, hi, scale);
    if (rc) return rc;
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    return g_hf.host_form(ctx, g_hf.data, data, bytes, nullptr, data, bytes,
                          [&](void *d, void *) { return impdar_hfilt_dev(ctx, d, dtype, snum, tnum, lo, hi, scale); });
}

extern "C" int impdar_ahfilt(impdar_ctx *ctx, void *data, int dtype, int snum, int tnum, const int *lo, const int *hi,
                             const double *scale)
{
    const int rc = ahfilt_check(ctx, data, dtype, snum, tnum, lo, hi, scale);
    if (rc) return rc;
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    return g_hf.host_form(ctx, g_hf.data, data, bytes, nullptr, data, bytes,
                          [&](void *d, void *) { return impdar_ahfilt_dev(ctx, d, dtype, snum, tnum, lo, hi, scale); });
}

extern "C" int impdar_winavg(impdar_ctx *ctx, void *data, int dtype, int snum, int tnum, const int *lo, const int *hi,
                             const double *scale)
{
    const int rc = winavg_check(ctx, data, dtype, snum, tnum, lo, hi, scale);
    if (rc) return rc;
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    return g_hf.host_form(ctx, g_hf.data, data, bytes, nullptr, data, bytes,
                          [&](void *d, void *) { return impdar_winavg_dev(ctx, d, dtype, snum, tnum, lo, hi, scale); });
}
