// Spectra of a (snum, tnum) radargram where it lies: the mean power spectrum along either axis (the reference's plot_ft and
// plot_hft, src/impdar/lib/plot.py:310-312, 346-355) and the periodogram of every trace (plot_spectrogram, :654-674, through
// scipy.signal.periodogram: detrend 'constant', a window, a one-sided spectrum with every bin but the first -- and, for an even
// length, the last -- doubled).
//
// Arithmetic: float32 and float64 data alike are widened to float64 on load; transforms, powers and sums run in float64 and the
// results are float64 -- "the reference on the data widened to float64" (DESIGN.md 4.13).
//
// A row is one contiguous real sequence of length n.  The rows of the horizontal spectrum are the radargram's own; the columns
// (vertical spectrum, periodogram) are transposed into a [tnum][snum] float64 buffer first.  spec_route.h picks, per (n, rows):
//   own transforms (spec_rows_kernel): a workgroup loops over its block of rows; a row sits in LDS as n / 2 complex doubles, runs
//     own_fft.h's passes, and the even / odd split of a real transform yields |X_k|^2 for k <= n / 2 straight from LDS -- summed
//     in registers over the workgroup's rows (mean spectra: one partial row per workgroup, added up in workgroup order by
//     spec_reduce_kernel) or scaled and stored (periodogram).  No spectrum ever goes to memory.
//   rocFFT (every other length): a batched real-forward plan into [rows][n / 2 + 1], then spec_power_kernel with the same
//     epilogue; detrend and window are a pre-pass on the float64 rows.
// No floating-point atomics anywhere: two calls on the same data give the same bits.
#include "common.h"
#include "fft.h"
#include "own_fft.h"
#include "spec_route.h"

static_assert(spec_pad(31) == own_pad(31) && spec_pad(4097) == own_pad(4097) && spec_pad(8192) == own_pad(8192), "spec_route.h restates own_pad");

enum { SPEC_MEAN = 0, SPEC_PGRAM = 1 };

// in: (rows, cols) of TI, row-major -> out: (cols, rows) of TO, through an LDS tile of odd pitch; the tiles at the ragged edges
// are range-checked.  One block per tile, tiles numbered row-major in blockIdx.x.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void spec_transpose_kernel(const TI *__restrict__ in, TO *__restrict__ out, int rows, int cols, int tiles_x)
{
    __shared__ TO tile[SPEC_TILE][SPEC_TILE + 1];
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const int c0 = bx * SPEC_TILE, r0 = by * SPEC_TILE;
    const int tx = threadIdx.x % SPEC_TILE, ty = threadIdx.x / SPEC_TILE;
    for (int r = ty; r < SPEC_TILE; r += 256 / SPEC_TILE)
        if (r0 + r < rows && c0 + tx < cols) tile[r][tx] = (TO)in[(size_t)(r0 + r) * cols + c0 + tx];
    __syncthreads();
    for (int c = ty; c < SPEC_TILE; c += 256 / SPEC_TILE)
        if (c0 + c < cols && r0 + tx < rows) out[(size_t)(c0 + c) * rows + r0 + tx] = tile[tx][c];
}

template <typename TI, typename TO> static int spec_transpose(const void *in, void *out, int rows, int cols, hipStream_t st)
{
    const long long tx = (cols + SPEC_TILE - 1) / SPEC_TILE, ty = (rows + SPEC_TILE - 1) / SPEC_TILE;
    IMPDAR_ARG_CHECK(tx * ty < (1LL << 31), "spectrum: %d x %d is beyond the transpose's grid", rows, cols);
    hipLaunchKernelGGL((spec_transpose_kernel<TI, TO>), dim3((unsigned)(tx * ty)), dim3(256), 0, st, (const TI *)in, (TO *)out, rows, cols, (int)tx);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

// |X_k|^2 of the real transform of the 2 M reals whose length-M complex transform Z sits in LDS, index k at s[own_pad(pos(k))]:
// X[k] = (Z[k] + conj Z[M-k]) / 2 - i w_k (Z[k] - conj Z[M-k]) / 2, k = 0 .. M (Z[M] = Z[0], w_M = -1) -- the OWN_R2C store of
// own_fft_rows, squared instead of stored
__device__ __forceinline__ double spec_split_power(OCp<double> zk, OCp<double> zmk, OCp<double> w, bool last)
{
    const OCp<double> zm = own_conj(zmk);
    const OCp<double> e = own_add(zk, zm), d = own_sub(zk, zm);
    const OCp<double> o = own_mul(w, d);
    const double sg = last ? -1.0 : 1.0;
    const double re = 0.5 * (e.x + sg * o.y), im = 0.5 * (e.y - sg * o.x);
    return re * re + im * im;
}

// Workgroup w takes rows [w rows_per_wg, min(rows, (w + 1) rows_per_wg)) of `in` (row r at in + r in_dist, n = 2 M reals of TI).
// PGRAM: the row's mean (a fixed tree in float64) is subtracted and sample j multiplied by window[j] (null: by nothing) before
// the transform, and out[r][k] = P_k scale (k = 0 or M) or 2 P_k scale.  Else: out[w][k] = the sum of P_k over the workgroup's
// rows, in row order.  k <= M; tw: e^{-2 pi i k / n}, k < n.  LDS: own_pad(M) + 1 complex doubles and blockDim.x doubles.
// NT: blockDim.x (spec_route.h's spec_row_threads), which bounds the bins a thread accumulates.
template <typename TI, bool MIXED, bool PGRAM, int NT>
__global__ __launch_bounds__(NT) void spec_rows_kernel(const TI *__restrict__ in, size_t in_dist, int M, int logm, const OwnMixedPlan pl,
                                                        long long rows, long long rows_per_wg, const OCp<double> *__restrict__ tw,
                                                        const double *__restrict__ window, double scale, double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char spec_lds[];
    OCp<double> *s = reinterpret_cast<OCp<double> *>(spec_lds);
    double *red = reinterpret_cast<double *>(s + own_pad(M) + 1);
    constexpr int ACC = spec_row_acc(NT);
    const int tid = threadIdx.x, nth = NT, n = 2 * M, bins = M + 1;
    const long long r0 = (long long)blockIdx.x * rows_per_wg, r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
    double acc[ACC];
#pragma unroll
    for (int j = 0; j < ACC; ++j) acc[j] = 0.0;
    for (long long r = r0; r < r1; ++r) {
        const TI *x = in + (size_t)r * in_dist;
        double mean = 0.0;
        if (PGRAM) {
            double part = 0.0;
            for (int i = tid; i < n; i += nth) part += (double)x[i];
            red[tid] = part;
            __syncthreads();
            for (int st = nth >> 1; st > 0; st >>= 1) {
                if (tid < st) red[tid] += red[tid + st];
                __syncthreads();
            }
            mean = red[0] / (double)n;
            __syncthreads();            // (red is written again for the next row)
        }
        for (int i = tid; i < M; i += nth) {
            double a = (double)x[2 * i], b = (double)x[2 * i + 1];
            if (PGRAM) {
                a -= mean;
                b -= mean;
                if (window) {
                    a *= window[2 * i];
                    b *= window[2 * i + 1];
                }
            }
            s[own_pad(i)] = OCp<double>{a, b};
        }
        __syncthreads();
        if (MIXED) {
            for (int p = 0; p < pl.np; ++p) {
                switch (pl.radix[p]) {
                case 4: own_mixed_pass<double, 4, false>(s, pl, p, tid, nth, tw, 2); break;
                case 2: own_mixed_pass<double, 2, false>(s, pl, p, tid, nth, tw, 2); break;
                case 3: own_mixed_pass<double, 3, false>(s, pl, p, tid, nth, tw, 2); break;
                case 5: own_mixed_pass<double, 5, false>(s, pl, p, tid, nth, tw, 2); break;
                default: own_mixed_pass<double, 7, false>(s, pl, p, tid, nth, tw, 2); break;
                }
            }
        } else {
            own_fft_passes<double, false>(s, M, logm, tid, nth, tw, 2);
        }
#pragma unroll
        for (int j = 0; j < ACC; ++j) {
            const int k = tid + j * nth;
            if (k <= M) {
                const int kz = k == M ? 0 : k, km = k == 0 ? 0 : M - k;
                const int pz = MIXED ? own_mixed_pos(pl, kz) : own_rev(kz, M, logm), pm = MIXED ? own_mixed_pos(pl, km) : own_rev(km, M, logm);
                const double P = spec_split_power(s[own_pad(pz)], s[own_pad(pm)], tw[kz], k == M);
                if (PGRAM) out[(size_t)r * bins + k] = (k == 0 || k == M) ? P * scale : 2.0 * (P * scale);
                else acc[j] += P;
            }
        }
        __syncthreads();                // (the next row overwrites the LDS these reads came from)
    }
    if (!PGRAM) {
#pragma unroll
        for (int j = 0; j < ACC; ++j) {
            const int k = tid + j * nth;
            if (k <= M) out[(size_t)blockIdx.x * bins + k] = acc[j];
        }
    }
}

// out[k] = (sum over the workgroups, in their order, of partial[w][k]) / rows for k < bins = n / 2 + 1, and out[n - k] = out[k]:
// the spectrum of real data in full fftfreq order
__global__ __launch_bounds__(256) void spec_reduce_kernel(const double *__restrict__ partial, long long workgroups, int bins, int n, double rows,
                                                         double *__restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= bins) return;
    double sum = 0.0;
    for (long long w = 0; w < workgroups; ++w) sum += partial[(size_t)w * bins + k];
    const double v = sum / rows;
    out[k] = v;
    if (k > 0) out[n - k] = v;
}

// ---- the rocFFT route: float64 rows, a pre-pass, the plan, the powers from the spectrum ----------------------------------

template <typename TI> __global__ __launch_bounds__(256) void spec_widen_kernel(const TI *__restrict__ in, double *__restrict__ out, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) out[i] = (double)in[i];
}

// one block per row of n doubles, in place: x[j] = (x[j] - mean) window[j] (null: no window), the mean by the same fixed tree
__global__ __launch_bounds__(256) void spec_prep_kernel(double *__restrict__ rowbuf, int n, const double *__restrict__ window)
{
    __shared__ double red[256];
    double *x = rowbuf + (size_t)blockIdx.x * n;
    const int tid = threadIdx.x;
    double part = 0.0;
    for (int i = tid; i < n; i += 256) part += x[i];
    red[tid] = part;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    const double mean = red[0] / (double)n;
    for (int i = tid; i < n; i += 256) x[i] = window ? (x[i] - mean) * window[i] : x[i] - mean;
}

// n == 1: the transform of a sample is the sample
__global__ __launch_bounds__(256) void spec_identity_kernel(const double *__restrict__ rowbuf, OCp<double> *__restrict__ spec, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) spec[i] = OCp<double>{rowbuf[i], 0.0};
}

// spec: [rows][bins] complex.  Block (x, w) takes bins [256 x, 256 x + 256) of rows [w rows_per_wg, ...): spec_rows_kernel's
// epilogue, reading the spectrum instead of LDS.
template <bool PGRAM>
__global__ __launch_bounds__(256) void spec_power_kernel(const OCp<double> *__restrict__ spec, int n, int bins, long long rows, long long rows_per_wg,
                                                        double scale, double *__restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= bins) return;
    const long long r0 = (long long)blockIdx.y * rows_per_wg, r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
    const bool single = k == 0 || (n % 2 == 0 && k == n / 2);
    double acc = 0.0;
    for (long long r = r0; r < r1; ++r) {
        const OCp<double> z = spec[(size_t)r * bins + k];
        const double P = z.x * z.x + z.y * z.y;
        if (PGRAM) out[(size_t)r * bins + k] = single ? P * scale : 2.0 * (P * scale);
        else acc += P;
    }
    if (!PGRAM) out[(size_t)blockIdx.y * bins + k] = acc;
}

// ------------------------------------------------------------------------------------------------ host side

struct SpecBufs {
    DevBuf data, rows, spec, partial, image, win, full, out;   // staging, float64 rows, rocFFT spectrum, partial sums, [tnum][bins], window, results
    OwnTwiddles tw;
    FftPlan plan;
    int plan_n = 0;
    long long plan_rows = 0;
    void release()
    {
        for (DevBuf *b : {&data, &rows, &spec, &partial, &image, &win, &full, &out, &tw.buf}) b->release();
        tw.nt = 0;
        plan.release();
        plan_n = 0;
        plan_rows = 0;
    }
};
static StepScratch<SpecBufs> g_sp;

void impdar_spectrum_forget(impdar_ctx *ctx) { g_sp.forget(ctx); }

template <typename TI>
static int spec_launch_rows(impdar_ctx *ctx, const SpecRoute &R, int mode, const void *in, const double *d_win, double scale, double *out)
{
    int rc = g_sp.tw.ensure<double>(R.n, ctx->stream);
    if (rc) return rc;
    OwnMixedPlan pl;
    if (R.kind == SPEC_OWN_MIXED) IMPDAR_ARG_CHECK(own_mixed_plan_make(R.M, pl), "spectrum: no mixed-radix plan for %d", R.M);
    const OCp<double> *t = g_sp.tw.buf.as<OCp<double>>();
#define SPEC_LAUNCH_NT(MIXED, PGRAM, NT)                                                                                          \
    do {                                                                                                                          \
        auto k = spec_rows_kernel<TI, MIXED, PGRAM, NT>;                                                                          \
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.lds));           \
        hipLaunchKernelGGL(k, dim3((unsigned)R.workgroups), dim3(R.threads), R.lds, ctx->stream, (const TI *)in, (size_t)R.n, R.M, R.logm, pl, \
                           R.rows, R.rows_per_wg, t, d_win, scale, out);                                                          \
    } while (0)
#define SPEC_LAUNCH(MIXED, PGRAM)                                                                                                 \
    do {                                                                                                                          \
        if (R.threads == 1024) SPEC_LAUNCH_NT(MIXED, PGRAM, 1024);                                                                \
        else if (R.threads == 512) SPEC_LAUNCH_NT(MIXED, PGRAM, 512);                                                             \
        else if (R.threads == 256) SPEC_LAUNCH_NT(MIXED, PGRAM, 256);                                                             \
        else SPEC_LAUNCH_NT(MIXED, PGRAM, 64);                                                                                    \
    } while (0)
    IMPDAR_ARG_CHECK(R.threads == 1024 || R.threads == 512 || R.threads == 256 || R.threads == 64, "spectrum: %d threads", R.threads);
    if (R.kind == SPEC_OWN_MIXED) {
        if (mode == SPEC_PGRAM) SPEC_LAUNCH(true, true);
        else SPEC_LAUNCH(true, false);
    } else {
        if (mode == SPEC_PGRAM) SPEC_LAUNCH(false, true);
        else SPEC_LAUNCH(false, false);
    }
#undef SPEC_LAUNCH
#undef SPEC_LAUNCH_NT
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

// The spectra of a resident (snum, tnum) radargram on ctx->stream.  columns: the sequences are the traces (n = snum, tnum of
// them), else the rows (n = tnum, snum of them).  SPEC_MEAN: d_out gets n doubles; SPEC_PGRAM (columns only): d_out gets the
// (n / 2 + 1, tnum) image.  window: n host doubles or null.  The caller holds g_sp's lock and has bound it to ctx.
static int spec_run(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, bool columns, int mode, const double *window, double scale,
                    void *d_out)
{
    const int n = columns ? snum : tnum;
    const long long rows = columns ? tnum : snum;
    const SpecRoute R = spec_route(n, rows);
    IMPDAR_ARG_CHECK(R.ok, "spectrum: no route for %lld rows of length %d", rows, n);
    const bool f32 = dtype == IMPDAR_F32;
    const bool rowbuf = columns || R.kind == SPEC_ROCFFT;
    int rc;
    if (rowbuf) IMPDAR_HIP_CHECK(g_sp.rows.ensure(R.rowbuf_doubles * sizeof(double)));
    if (columns) {
        rc = f32 ? spec_transpose<float, double>(d_data, g_sp.rows.p, snum, tnum, ctx->stream)
                 : spec_transpose<double, double>(d_data, g_sp.rows.p, snum, tnum, ctx->stream);
        if (rc) return rc;
    } else if (rowbuf) {
        const size_t count = R.rowbuf_doubles;
        const unsigned blocks = (unsigned)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
        if (f32) hipLaunchKernelGGL(spec_widen_kernel<float>, dim3(blocks), dim3(256), 0, ctx->stream, (const float *)d_data, g_sp.rows.as<double>(), count);
        else hipLaunchKernelGGL(spec_widen_kernel<double>, dim3(blocks), dim3(256), 0, ctx->stream, (const double *)d_data, g_sp.rows.as<double>(), count);
        IMPDAR_HIP_CHECK(hipGetLastError());
    }
    const double *d_win = nullptr;
    if (mode == SPEC_PGRAM && window) {
        const void *dev[1];
        rc = impdar_upload_tables(ctx, g_sp.win, {{window, (size_t)n * sizeof(double)}}, dev);
        if (rc) return rc;
        d_win = (const double *)dev[0];
    }
    double *sums;           // where the powers go: the partial sums, or the periodogram before its transpose
    if (mode == SPEC_PGRAM) {
        IMPDAR_HIP_CHECK(g_sp.image.ensure(R.image_doubles * sizeof(double)));
        sums = g_sp.image.as<double>();
    } else {
        IMPDAR_HIP_CHECK(g_sp.partial.ensure(R.partial_doubles * sizeof(double)));
        sums = g_sp.partial.as<double>();
    }
    if (R.kind != SPEC_ROCFFT) {
        if (rowbuf) rc = spec_launch_rows<double>(ctx, R, mode, g_sp.rows.p, d_win, scale, sums);
        else if (f32) rc = spec_launch_rows<float>(ctx, R, mode, d_data, d_win, scale, sums);
        else rc = spec_launch_rows<double>(ctx, R, mode, d_data, d_win, scale, sums);
        if (rc) return rc;
    } else {
        if (mode == SPEC_PGRAM) {
            hipLaunchKernelGGL(spec_prep_kernel, dim3((unsigned)rows), dim3(256), 0, ctx->stream, g_sp.rows.as<double>(), n, d_win);
            IMPDAR_HIP_CHECK(hipGetLastError());
        }
        IMPDAR_HIP_CHECK(g_sp.spec.ensure(R.spectrum_doubles * sizeof(double)));
        if (R.identity) {
            const size_t count = (size_t)rows;
            const unsigned blocks = (unsigned)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
            hipLaunchKernelGGL(spec_identity_kernel, dim3(blocks), dim3(256), 0, ctx->stream, g_sp.rows.as<double>(), g_sp.spec.as<OCp<double>>(), count);
            IMPDAR_HIP_CHECK(hipGetLastError());
        } else {
            if (g_sp.plan_n != n || g_sp.plan_rows != rows || !g_sp.plan.plan) {
                g_sp.plan_n = 0;
                rc = g_sp.plan.create(rocfft_transform_type_real_forward, true, false, (size_t)n, (size_t)rows, rocfft_array_type_real,
                                      rocfft_array_type_hermitian_interleaved, 1, (size_t)n, 1, (size_t)R.bins, 1.0, ctx->stream);
                if (rc) return rc;
                g_sp.plan_n = n;
                g_sp.plan_rows = rows;
            }
            rc = g_sp.plan.exec(g_sp.rows.p, g_sp.spec.p);
            if (rc) return rc;
        }
        const dim3 grid((unsigned)((R.bins + SPEC_POWER_THREADS - 1) / SPEC_POWER_THREADS), (unsigned)R.workgroups);
        if (mode == SPEC_PGRAM)
            hipLaunchKernelGGL(spec_power_kernel<true>, grid, dim3(SPEC_POWER_THREADS), 0, ctx->stream, g_sp.spec.as<OCp<double>>(), n, R.bins, rows,
                               R.rows_per_wg, scale, sums);
        else
            hipLaunchKernelGGL(spec_power_kernel<false>, grid, dim3(SPEC_POWER_THREADS), 0, ctx->stream, g_sp.spec.as<OCp<double>>(), n, R.bins, rows,
                               R.rows_per_wg, scale, sums);
        IMPDAR_HIP_CHECK(hipGetLastError());
    }
    if (mode == SPEC_PGRAM) return spec_transpose<double, double>(sums, d_out, tnum, R.bins, ctx->stream);
    hipLaunchKernelGGL(spec_reduce_kernel, dim3((unsigned)((R.bins + 255) / 256)), dim3(256), 0, ctx->stream, sums, R.workgroups, R.bins, n, (double)rows,
                       (double *)d_out);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

static int mean_spectrum_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int axis, const double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "impdar_mean_spectrum: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_mean_spectrum: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_mean_spectrum: empty radargram");
    IMPDAR_ARG_CHECK(axis == 0 || axis == 1, "impdar_mean_spectrum: axis must be 0 or 1, got %d", axis);
    return IMPDAR_OK;
}

static int periodogram_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, double scale, const void *out)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "impdar_periodogram: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_periodogram: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_periodogram: empty radargram");
    IMPDAR_ARG_CHECK(scale == scale && scale > 0.0 && scale < 1.0e300, "impdar_periodogram: scale %g", scale);
    return IMPDAR_OK;
}

extern "C" int impdar_mean_spectrum_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int axis, double *out)
{
    int rc = mean_spectrum_check(ctx, d_data, dtype, snum, tnum, axis, out);
    if (rc) return rc;
    const auto lock = g_sp.lock();
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_sp.bind(ctx);
    const size_t bytes = (size_t)(axis == 0 ? snum : tnum) * sizeof(double);
    IMPDAR_HIP_CHECK(g_sp.full.ensure(bytes));
    rc = spec_run(ctx, d_data, dtype, snum, tnum, axis == 0, SPEC_MEAN, nullptr, 1.0, g_sp.full.p);
    if (rc) return rc;
    impdar_ctx_note(ctx, "impdar_mean_spectrum_dev", "spec_rows_kernel");
    return impdar_download(ctx, out, g_sp.full.p, bytes, ctx->stream);
}

extern "C" int impdar_mean_spectrum(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int axis, double *out)
{
    int rc = mean_spectrum_check(ctx, data, dtype, snum, tnum, axis, out);
    if (rc) return rc;
    impdar_ctx_note(ctx, "impdar_mean_spectrum", "spec_rows_kernel");
    return g_sp.host_form(ctx, g_sp.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype), &g_sp.full, out,
                          (size_t)(axis == 0 ? snum : tnum) * sizeof(double),
                          [&](void *d_in, void *d_out) { return spec_run(ctx, d_in, dtype, snum, tnum, axis == 0, SPEC_MEAN, nullptr, 1.0, d_out); });
}

extern "C" int impdar_periodogram_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const double *window, double scale,
                                      void *d_out)
{
    int rc = periodogram_check(ctx, d_data, dtype, snum, tnum, scale, d_out);
    if (rc) return rc;
    const auto lock = g_sp.lock();
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_sp.bind(ctx);
    rc = spec_run(ctx, d_data, dtype, snum, tnum, true, SPEC_PGRAM, window, scale, d_out);
    if (rc) return rc;
    impdar_ctx_note(ctx, "impdar_periodogram_dev", "spec_rows_kernel");
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_periodogram(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *window, double scale, void *out)
{
    int rc = periodogram_check(ctx, data, dtype, snum, tnum, scale, out);
    if (rc) return rc;
    return g_sp.host_form(ctx, g_sp.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype), &g_sp.out, out,
                          (size_t)(snum / 2 + 1) * tnum * sizeof(double),
                          [&](void *d_in, void *d_out) { return impdar_periodogram_dev(ctx, d_in, dtype, snum, tnum, window, scale, d_out); });
}

extern "C" int impdar_spec_route_probe(int n, long long rows, int *out)
{
    IMPDAR_ARG_CHECK(out, "impdar_spec_route_probe: null argument");
    const SpecRoute R = spec_route(n, rows);
    IMPDAR_ARG_CHECK(R.ok, "impdar_spec_route_probe: no route for %lld rows of length %d", rows, n);
    out[0] = R.kind;
    out[1] = (int)R.workgroups;
    out[2] = (int)(R.rows_per_wg < 0x7fffffff ? R.rows_per_wg : 0x7fffffff);
    out[3] = (int)R.lds;
    return IMPDAR_OK;
}
