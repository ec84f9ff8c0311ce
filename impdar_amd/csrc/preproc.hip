// The two processing steps that sit in front of a migration in an impproc/impdar chain, kept on the device
// so that a radargram stays resident from the first filter to the migrated image:
//
//   * vertical_band_pass  (reference src/impdar/lib/RadarData/_RadarDataFiltering.py:469-549):
//       IIR designs -> scipy.signal.filtfilt(b, a, data, axis=0): odd extension by 3*ntaps samples, steady-state
//       initial conditions, forward pass, backward pass, cast back to the data's dtype;
//       FIR design  -> lfilter(taps, 1, data) shifted up by `order` rows, the last `order` rows untouched.
//   * constant_space      (reference src/impdar/lib/RadarData/_RadarDataProcessing.py:499-583):
//       linear interpolation of every sample row onto equally spaced distances (scipy interp1d, slope form).
//
// All three are HBM-streaming kernels; the arithmetic is fp64 in SciPy's operation order whatever the data
// type (the file is compiled with -ffp-contract=off).  The IIR recurrence (filtfilt_core.h, shared with the
// horizontal frequency filters) is a serial chain along time: a wavefront runs 16 traces, four lanes each (rows
// of the (snum, tnum) array are contiguous across traces, so every access is a coalesced row segment), with the
// loads of the next 32 samples in flight while 32 are filtered.
#include "filtfilt_core.h"

#define FF_MAX_COEF 33

// The recurrence of one trace is spread over the four lanes of a quad (FiltLane<4, K> of filtfilt_core.h, K =
// ceil((NC-1)/4)).  fp64 issues at half rate and a trace-per-lane mapping leaves 85 % of the SIMDs idle at 10000
// traces (157 wavefronts for 1024 SIMDs), so the ~4(NC-1) fp64 operations of a step are the whole cost: split four
// ways they take a third of the issue slots per wavefront on four times as many SIMDs.

#define FF_TRACES 16   // traces per 64-lane wavefront
#define FF_CH 32       // samples per chunk (64 needs more than 256 VGPRs for the 21- and 33-coefficient kernels)
#define FF_PK (FF_CH / 4)

// Memory side.  625 wavefronts with a 64-byte row segment each cannot keep HBM busy unless many rows are in
// flight per wavefront (16 rows in flight = 640 KB on the whole chip = 0.6 TB/s at ~1 us latency), so input
// and output are quad-packed: the four lanes of a quad hold four consecutive samples of their trace (lane q of
// register k holds sample 4k+q of the chunk), one load / store instruction moves four rows, and a 32-sample
// chunk is 8 instructions.  A step takes its sample from lane u&3 of register u>>2 with a quad-broadcast DPP
// move, and lane u&3 keeps the step's output.
//
// With plain loads hipcc waits for the prefetched chunk before the first step of the current one (it treats
// loads and stores pending on vmcnt as completing out of order and drains), which exposes the memory latency
// of every chunk.  The prefetch of the next chunk is therefore issued from inline asm, invisible to that
// bookkeeping, and retired by one explicit s_waitcnt vmcnt(0) at the END of the chunk, tied to the loaded
// registers.  Nothing is assumed about the relative completion order of loads and stores: the outputs of a
// chunk stay in registers and are stored at the top of the next chunk, in front of the next prefetch, so that
// by the time of the wait everything outstanding was issued a whole chunk (~2.5 us) earlier.
// The kernels must stay within the 256 architectural VGPRs: beyond that the compiler parks live values in
// AccVGPRs, and a copy of a register whose asm load has not landed yet copies garbage.
__device__ __forceinline__ void ff_load_async(float &dst, const float *p)
{
    asm volatile("global_load_dword %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void ff_load_async(double &dst, const double *p)
{
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
#define FF_TIE8(r) "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7])
template <typename T> __device__ __forceinline__ void ff_wait_chunk(T (&r)[FF_PK])
{
    static_assert(FF_PK == 8, "operand list above");
    asm volatile("s_waitcnt vmcnt(0)" : FF_TIE8(r) : : "memory");
}

// FF_CH steps on the packed samples in `cur`; the packed outputs go to `held` (converted to TO)
template <typename TI, typename TO, int K>
__device__ __forceinline__ void ff_chunk_steps(FiltLane<4, K> &f, const TI (&cur)[FF_PK], TO (&held)[FF_PK], int q)
{
#pragma unroll
    for (int k = 0; k < FF_PK; ++k) {
        const double y0 = f.step((double)quad_pick<0>(cur[k]));
        const double y1 = f.step((double)quad_pick<1>(cur[k]));
        const double y2 = f.step((double)quad_pick<2>(cur[k]));
        const double y3 = f.step((double)quad_pick<3>(cur[k]));
        const double lo = (q & 1) ? y1 : y0, hi = (q & 1) ? y3 : y2;
        held[k] = (TO)((q & 2) ? hi : lo);
    }
}

// forward pass over the extended trace; Y is (snum + 2*edge, tnum) fp64
template <typename T, int NC>
__global__ __launch_bounds__(64) void ff_forward_kernel(const T *__restrict__ x, double *__restrict__ Y, int snum,
                                                        int tnum, int edge, int nc, FiltCoefs<FF_MAX_COEF> c)
{
    constexpr int K = (NC - 1 + 3) / 4;
    const int j = blockIdx.x * FF_TRACES + (threadIdx.x >> 2), q = threadIdx.x & 3;
    if (j >= tnum) return;   // whole quads leave together
    const int L = snum + 2 * edge;
    const T *xj = x + j;   // the trace: one sample per row of the data
    FiltLane<4, K> f;
    f.init(c, q, nc, (double)filt_odd_ext(xj, 0, snum, edge, (size_t)tnum));
    T cur[FF_PK], nxt[FF_PK];
    double held[FF_PK];
    int held_i = -1;   // first sample of the chunk whose outputs are still in registers (uniform)
#pragma unroll
    for (int k = 0; k < FF_PK; ++k) cur[k] = filt_odd_ext(xj, 4 * k + q, snum, edge, (size_t)tnum);
    for (int i = 0; i < L; i += FF_CH) {
        if (held_i >= 0) {
#pragma unroll
            for (int k = 0; k < FF_PK; ++k) {
                const int r = held_i + 4 * k + q;
                if (r < L) Y[(size_t)r * tnum + j] = held[k];
            }
        }
        const int r0 = i + FF_CH;                                      // first sample of the next chunk
        const bool inside = r0 >= edge && r0 + FF_CH <= edge + snum;   // uniform: plain rows of the data
        if (inside) {
            const T *row = x + (size_t)(r0 - edge + q) * tnum + j;
#pragma unroll
            for (int k = 0; k < FF_PK; ++k) ff_load_async(nxt[k], row + (size_t)(4 * k) * tnum);
        } else if (r0 < L) {
#pragma unroll
            for (int k = 0; k < FF_PK; ++k) nxt[k] = filt_odd_ext(xj, r0 + 4 * k + q, snum, edge, (size_t)tnum);
        }
        ff_chunk_steps(f, cur, held, q);   // samples past L-1 are filtered too; their outputs are never stored
        held_i = i;
        if (inside) ff_wait_chunk(nxt);
#pragma unroll
        for (int k = 0; k < FF_PK; ++k) cur[k] = nxt[k];
    }
#pragma unroll
    for (int k = 0; k < FF_PK; ++k) {
        const int r = held_i + 4 * k + q;
        if (r < L) Y[(size_t)r * tnum + j] = held[k];
    }
}

// backward pass: filters Y from its last row to its first and writes rows [edge, edge+snum) back into the
// data array in its own dtype (the rows in front of `edge` are never needed)
template <typename T, int NC>
__global__ __launch_bounds__(64) void ff_backward_kernel(const double *__restrict__ Y, T *__restrict__ out, int snum,
                                                         int tnum, int edge, int nc, FiltCoefs<FF_MAX_COEF> c)
{
    constexpr int K = (NC - 1 + 3) / 4;
    const int j = blockIdx.x * FF_TRACES + (threadIdx.x >> 2), q = threadIdx.x & 3;
    if (j >= tnum) return;
    const int L = snum + 2 * edge;
    FiltLane<4, K> f;
    f.init(c, q, nc, Y[(size_t)(L - 1) * tnum + j]);
    double cur[FF_PK], nxt[FF_PK];
    T held[FF_PK];
    int held_p = -1;   // position (in the extended trace) of the first sample of the chunk held in registers
#pragma unroll
    for (int k = 0; k < FF_PK; ++k) {
        const int r = L - 1 - (4 * k + q);
        cur[k] = Y[(size_t)(r > 0 ? r : 0) * tnum + j];
    }
    for (int p = L - 1; p >= edge; p -= FF_CH) {   // p: position of the chunk's first sample
        if (held_p >= 0) {
#pragma unroll
            for (int k = 0; k < FF_PK; ++k) {
                const int r = held_p - (4 * k + q) - edge;
                if (r >= 0 && r < snum) out[(size_t)r * tnum + j] = held[k];
            }
        }
        const bool inside = p - 2 * FF_CH + 1 >= 0;   // uniform: the next chunk's rows all exist
        if (inside) {
            const double *row = Y + (size_t)(p - FF_CH - q) * tnum + j;
#pragma unroll
            for (int k = 0; k < FF_PK; ++k) ff_load_async(nxt[k], row - (size_t)(4 * k) * tnum);
        } else {
#pragma unroll
            for (int k = 0; k < FF_PK; ++k) {
                const int r = p - FF_CH - (4 * k + q);
                nxt[k] = Y[(size_t)(r > 0 ? r : 0) * tnum + j];
            }
        }
        ff_chunk_steps(f, cur, held, q);
        held_p = p;
        if (inside) ff_wait_chunk(nxt);
#pragma unroll
        for (int k = 0; k < FF_PK; ++k) cur[k] = nxt[k];
    }
#pragma unroll
    for (int k = 0; k < FF_PK; ++k) {
        const int r = held_p - (4 * k + q) - edge;
        if (r >= 0 && r < snum) out[(size_t)r * tnum + j] = held[k];
    }
}

#define FIR_ROWS 8   // consecutive output rows per thread

struct FirTaps {
    double t[256 + 2 * FIR_ROWS];   // taps[i] at t[FIR_ROWS + i], zeros on both sides
};

// out[k, j] = sum_i taps[i] * x[k + order - i, j] for k < snum - order (lfilter delayed by `order` rows and
// shifted back, _RadarDataFiltering.py:536-540); `out` is a separate array.  A thread owns FIR_ROWS
// consecutive rows of one trace and walks the order + FIR_ROWS input rows they touch once: one coalesced row
// load and one scalar load of FIR_ROWS consecutive taps per input row, FIR_ROWS fp64 FMAs.
template <typename T>
__global__ __launch_bounds__(256) void fir_shift_kernel(const T *__restrict__ x, T *__restrict__ out, int snum, int tnum,
                                                        int ntaps, FirTaps taps)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int k0 = blockIdx.y * FIR_ROWS;
    const int order = ntaps - 1, nout = snum - order;
    if (j >= tnum) return;
    double acc[FIR_ROWS];
#pragma unroll
    for (int u = 0; u < FIR_ROWS; ++u) acc[u] = 0.0;
    // input row k0 + s contributes to output row k0 + u through tap i = u + order - s
#pragma unroll 4
    for (int s = 0; s < order + FIR_ROWS; ++s) {
        const int r = k0 + s;
        const double xv = r < snum ? (double)x[(size_t)r * tnum + j] : 0.0;
        const double *tp = &taps.t[FIR_ROWS + order - s];
#pragma unroll
        for (int u = 0; u < FIR_ROWS; ++u) acc[u] = __builtin_fma(tp[u], xv, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < FIR_ROWS; ++u)
        if (k0 + u < nout) out[(size_t)(k0 + u) * tnum + j] = (T)acc[u];
}

// out[k, m] = (y_hi - y_lo) / den[m] * t[m] + y_lo   (scipy interp1d._call_linear: the difference is taken in
// the data's own arithmetic, everything after it in fp64)
#define LERP_ROWS 8   // sample rows per thread: the four table entries of a column are loaded once for all of them

template <typename T>
__global__ __launch_bounds__(256) void trace_lerp_kernel(const T *__restrict__ x, double *__restrict__ out, int snum,
                                                         int tnum, int n_new, const int *__restrict__ lo,
                                                         const int *__restrict__ hi, const double *__restrict__ den,
                                                         const double *__restrict__ t)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n_new) return;
    const int k0 = blockIdx.y * LERP_ROWS;
    const int jl = lo[m], jh = hi[m];
    const double dm = den[m], tm = t[m];
    T ylo[LERP_ROWS], yhi[LERP_ROWS];
#pragma unroll
    for (int u = 0; u < LERP_ROWS; ++u) {
        const int k = k0 + u < snum ? k0 + u : snum - 1;
        ylo[u] = x[(size_t)k * tnum + jl];
        yhi[u] = x[(size_t)k * tnum + jh];
    }
#pragma unroll
    for (int u = 0; u < LERP_ROWS; ++u) {
        if (k0 + u < snum) {
            const double slope = (double)(T)(yhi[u] - ylo[u]) / dm;
            out[(size_t)(k0 + u) * n_new + m] = slope * tm + (double)ylo[u];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct PreprocBufs {
    DevBuf y, data, aux, idx;   // the fp64 forward pass, staging of the host-buffer forms, FIR / lerp output, lerp tables
    void release()
    {
        y.release();
        data.release();
        aux.release();
        idx.release();
    }
};
static StepScratch<PreprocBufs> g_scr;

void impdar_preproc_forget(impdar_ctx *ctx) { g_scr.forget(ctx); }

template <typename T, int NC>
static int filtfilt_launch(impdar_ctx *ctx, T *d, double *Y, int snum, int tnum, int edge, int nc, const FiltCoefs<FF_MAX_COEF> &c)
{
    const int nb = (tnum + FF_TRACES - 1) / FF_TRACES;
    hipLaunchKernelGGL((ff_forward_kernel<T, NC>), dim3(nb), dim3(64), 0, ctx->stream, d, Y, snum, tnum, edge, nc, c);
    hipLaunchKernelGGL((ff_backward_kernel<T, NC>), dim3(nb), dim3(64), 0, ctx->stream, Y, d, snum, tnum, edge, nc, c);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

template <typename T>
static int filtfilt_dispatch(impdar_ctx *ctx, T *d, double *Y, int snum, int tnum, int edge, int ncoef, const FiltCoefs<FF_MAX_COEF> &c)
{
    if (ncoef <= 5) return filtfilt_launch<T, 5>(ctx, d, Y, snum, tnum, edge, ncoef, c);
    if (ncoef <= 11) return filtfilt_launch<T, 11>(ctx, d, Y, snum, tnum, edge, ncoef, c);
    if (ncoef <= 21) return filtfilt_launch<T, 21>(ctx, d, Y, snum, tnum, edge, ncoef, c);
    // the last branch is FiltLane<4, 8>: more delays per lane than 8 have not been held to the 256-VGPR rule
    static_assert(FF_MAX_COEF - 1 <= 4 * 8, "at most 8 delays per lane at 4 lanes per trace");
    return filtfilt_launch<T, FF_MAX_COEF>(ctx, d, Y, snum, tnum, edge, ncoef, c);
}

static int filtfilt_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *b, const double *a,
                          int ncoef, const double *zi)
{
    IMPDAR_ARG_CHECK(ctx && data && b && a && zi, "impdar_filtfilt: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_filtfilt: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(ncoef >= 2 && ncoef <= FF_MAX_COEF, "impdar_filtfilt: %d filter coefficients (2..%d supported)", ncoef,
                     FF_MAX_COEF);
    IMPDAR_ARG_CHECK(a[0] != 0.0, "impdar_filtfilt: a[0] is zero");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_filtfilt: empty radargram");
    // scipy.signal.filtfilt's own guard and message
    IMPDAR_ARG_CHECK(snum > 3 * ncoef, "The length of the input vector x must be greater than padlen, which is %d.", 3 * ncoef);
    return IMPDAR_OK;
}

extern "C" int impdar_filtfilt_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, const double *b,
                                   const double *a, int ncoef, const double *zi)
{
    const auto lock = g_scr.lock();
    const int bad = filtfilt_check(ctx, d_data, dtype, snum, tnum, b, a, ncoef, zi);
    if (bad) return bad;
    const int edge = 3 * ncoef;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    const FiltCoefs<FF_MAX_COEF> c = filt_coefs<FF_MAX_COEF>(b, a, zi, ncoef);
    g_scr.bind(ctx);
    IMPDAR_HIP_CHECK(g_scr.y.ensure((size_t)(snum + 2 * edge) * tnum * sizeof(double)));
    const int rc = dtype == IMPDAR_F32
                       ? filtfilt_dispatch<float>(ctx, (float *)d_data, g_scr.y.as<double>(), snum, tnum, edge, ncoef, c)
                       : filtfilt_dispatch<double>(ctx, (double *)d_data, g_scr.y.as<double>(), snum, tnum, edge, ncoef, c);
    return rc ? rc : impdar_ctx_mark_produced(ctx);
}

static int fir_shift_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *taps, int ntaps)
{
    IMPDAR_ARG_CHECK(ctx && data && taps, "impdar_fir_shift: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_fir_shift: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(ntaps >= 1 && ntaps <= 256, "impdar_fir_shift: %d taps (1..256 supported)", ntaps);
    IMPDAR_ARG_CHECK(tnum >= 1 && snum >= 1, "impdar_fir_shift: empty radargram");
    return IMPDAR_OK;
}

extern "C" int impdar_fir_shift_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, const double *taps,
                                    int ntaps)
{
    const auto lock = g_scr.lock();
    const int rc = fir_shift_check(ctx, d_data, dtype, snum, tnum, taps, ntaps);
    if (rc) return rc;
    const int order = ntaps - 1;
    if (snum <= order) return IMPDAR_OK;   // data[:-order] is empty: nothing is assigned
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    FirTaps t;
    memset(&t, 0, sizeof(t));
    for (int i = 0; i < ntaps; ++i) t.t[FIR_ROWS + i] = taps[i];
    const size_t es = impdar_dtype_size(dtype), n = (size_t)(snum - order) * tnum;
    g_scr.bind(ctx);
    IMPDAR_HIP_CHECK(g_scr.aux.ensure(n * es));
    const dim3 grid((tnum + 255) / 256, (snum - order + FIR_ROWS - 1) / FIR_ROWS);
    if (dtype == IMPDAR_F32)
        hipLaunchKernelGGL(fir_shift_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float *)d_data,
                           g_scr.aux.as<float>(), snum, tnum, ntaps, t);
    else
        hipLaunchKernelGGL(fir_shift_kernel<double>, grid, dim3(256), 0, ctx->stream, (const double *)d_data,
                           g_scr.aux.as<double>(), snum, tnum, ntaps, t);
    IMPDAR_HIP_CHECK(hipGetLastError());
    IMPDAR_HIP_CHECK(hipMemcpyAsync(d_data, g_scr.aux.p, n * es, hipMemcpyDeviceToDevice, ctx->stream));
    return impdar_ctx_mark_produced(ctx);
}

static int trace_lerp_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *lo, const int *hi,
                            const double *den, const double *t, int n_new, const double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && lo && hi && den && t && out, "impdar_trace_lerp: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_trace_lerp: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 2 && n_new >= 0, "impdar_trace_lerp: bad shape %d x %d -> %d", snum, tnum, n_new);
    for (int m = 0; m < n_new; ++m)
        IMPDAR_ARG_CHECK(lo[m] >= 0 && lo[m] < tnum && hi[m] >= 0 && hi[m] < tnum, "impdar_trace_lerp: column index out of range at %d",
                         m);
    return IMPDAR_OK;
}

extern "C" int impdar_trace_lerp_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const int *lo,
                                     const int *hi, const double *den, const double *t, int n_new, double *d_out)
{
    const auto lock = g_scr.lock();
    int rc = trace_lerp_check(ctx, d_data, dtype, snum, tnum, lo, hi, den, t, n_new, d_out);
    if (rc) return rc;
    if (n_new == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_scr.bind(ctx);
    const size_t ib = (size_t)n_new * sizeof(int), db = (size_t)n_new * sizeof(double);
    const void *d_tab[4];
    rc = impdar_upload_tables(ctx, g_scr.idx, {{den, db}, {t, db}, {lo, ib}, {hi, ib}}, d_tab);
    if (rc) return rc;
    const double *d_den = (const double *)d_tab[0], *d_t = (const double *)d_tab[1];
    const int *d_lo = (const int *)d_tab[2], *d_hi = (const int *)d_tab[3];
    const dim3 grid((n_new + 255) / 256, (snum + LERP_ROWS - 1) / LERP_ROWS);
    if (dtype == IMPDAR_F32)
        hipLaunchKernelGGL(trace_lerp_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float *)d_data, d_out, snum,
                           tnum, n_new, d_lo, d_hi, d_den, d_t);
    else
        hipLaunchKernelGGL(trace_lerp_kernel<double>, grid, dim3(256), 0, ctx->stream, (const double *)d_data, d_out, snum,
                           tnum, n_new, d_lo, d_hi, d_den, d_t);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// element-wise float32 <-> float64 conversion of a resident array (what NumPy's astype does on the host)
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void cast_kernel(const TI *__restrict__ in, TO *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (TO)in[i];
}

extern "C" int impdar_cast_dev(impdar_ctx *ctx, const void *d_src, int src_dtype, void *d_dst, int dst_dtype, size_t n)
{
    IMPDAR_ARG_CHECK(ctx && d_src && d_dst, "impdar_cast_dev: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(src_dtype) && impdar_dtype_ok(dst_dtype),
                     "impdar_cast_dev: dtypes must be float32 or float64");
    if (n == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    if (src_dtype == dst_dtype) {
        IMPDAR_HIP_CHECK(hipMemcpyAsync(d_dst, d_src, n * impdar_dtype_size(src_dtype), hipMemcpyDeviceToDevice, ctx->stream));
        return impdar_ctx_mark_produced(ctx);
    }
    const unsigned nb = (unsigned)((n + 255) / 256);
    if (src_dtype == IMPDAR_F64)
        hipLaunchKernelGGL((cast_kernel<double, float>), dim3(nb), dim3(256), 0, ctx->stream, (const double *)d_src, (float *)d_dst, n);
    else
        hipLaunchKernelGGL((cast_kernel<float, double>), dim3(nb), dim3(256), 0, ctx->stream, (const float *)d_src, (double *)d_dst, n);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer forms: the argument check, then StepScratch::host_form ----------------------------------

extern "C" int impdar_filtfilt(impdar_ctx *ctx, void *data, int dtype, int snum, int tnum, const double *b,
                               const double *a, int ncoef, const double *zi)
{
    const int rc = filtfilt_check(ctx, data, dtype, snum, tnum, b, a, ncoef, zi);
    if (rc) return rc;
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    return g_scr.host_form(ctx, g_scr.data, data, bytes, nullptr, data, bytes,
                           [&](void *d, void *) { return impdar_filtfilt_dev(ctx, d, dtype, snum, tnum, b, a, ncoef, zi); });
}

extern "C" int impdar_fir_shift(impdar_ctx *ctx, void *data, int dtype, int snum, int tnum, const double *taps, int ntaps)
{
    const int rc = fir_shift_check(ctx, data, dtype, snum, tnum, taps, ntaps);
    if (rc) return rc;
    if (snum <= ntaps - 1) return IMPDAR_OK;   // as the resident form: nothing is assigned
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    return g_scr.host_form(ctx, g_scr.data, data, bytes, nullptr, data, bytes,
                           [&](void *d, void *) { return impdar_fir_shift_dev(ctx, d, dtype, snum, tnum, taps, ntaps); });
}

extern "C" int impdar_trace_lerp(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *lo,
                                 const int *hi, const double *den, const double *t, int n_new, double *out)
{
    const int rc = trace_lerp_check(ctx, data, dtype, snum, tnum, lo, hi, den, t, n_new, out);
    if (rc) return rc;
    if (n_new == 0) return IMPDAR_OK;
    return g_scr.host_form(ctx, g_scr.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype), &g_scr.aux, out,
                           (size_t)snum * n_new * sizeof(double), [&](void *d_in, void *d_out) {
                               return impdar_trace_lerp_dev(ctx, d_in, dtype, snum, tnum, lo, hi, den, t, n_new, (double *)d_out);
                           });
}
