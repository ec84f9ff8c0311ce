// The processing steps that change the SAMPLE axis of a radargram, kept on the device so that a chain stays
// resident across them (reference src/impdar/lib/RadarData/_RadarDataProcessing.py):
//
//   * nmo (:64-193) and constant_sample_depth_spacing (:50-61): one scipy interp1d per trace in the reference, but
//     the abscissae are the same for every trace, so the whole step is a blend of two input ROWS per output row:
//       out[i, :] = (in[hi[i], :] - in[lo[i], :]) / den[i] * t[i] + in[lo[i], :]            (row_lerp_kernel)
//   * crop with a trace-wise pretrigger (:306-322) and elev_correct (:618-625): every trace moves up or down by
//     its own number of samples, NaN where nothing lands:
//       out[i, j] = in[i + shift[j], j]  where that row exists, NaN elsewhere                (col_shift_kernel)
//
// Both write float64 whatever the input (the reference allocates np.empty / np.zeros) and do nothing a copy does
// not, apart from the second row read of the blend: they are HBM-streaming kernels.  The file is compiled with
// -ffp-contract=off; the blend is in scipy's operation order (the difference in the data's own arithmetic,
// everything after it in fp64), as trace_lerp_kernel of preproc.hip.
#include "vecwidth.h"

#define VA_ROWS 8   // consecutive output rows per thread

// A thread owns V consecutive traces (one 16-byte load for float32 x 4 and float64 x 2) of VA_ROWS consecutive
// output rows.  The rows a row group reads are the same or neighbouring ones (a move-out stretches by a few per
// cent), so of its 2 * VA_ROWS row loads all but about VA_ROWS + 1 are repeats of a load the same thread has just
// issued.  The traffic MODEL (no counter run has checked it) is that those repeats hit in the CU's
// own cache, and that the one row two neighbouring row groups share -- blocks are numbered along the traces
// first, so they run at about the same time -- is served on the die the second time: input once, output once.
// V is chosen by the host so that tnum % V == 0: every row then starts on a multiple of the access width and no
// trace is left over; V = 1 serves every other trace count.
template <typename T, int V>
__global__ __launch_bounds__(256) void row_lerp_kernel(const T *__restrict__ x, double *__restrict__ out, int tnum,
                                                       int n_out, const int *__restrict__ lo, const int *__restrict__ hi,
                                                       const double *__restrict__ den, const double *__restrict__ t)
{
    typedef RwVec<T, V> In;
    typedef RwVec<double, V> Out;
    const int j = (blockIdx.x * 256 + threadIdx.x) * V;
    if (j >= tnum) return;
    const int i0 = blockIdx.y * VA_ROWS;
    In ylo[VA_ROWS], yhi[VA_ROWS];
#pragma unroll
    for (int u = 0; u < VA_ROWS; ++u) {
        const int i = i0 + u < n_out ? i0 + u : n_out - 1;   // uniform: the tables are read with scalar loads
        ylo[u] = *reinterpret_cast<const In *>(x + (size_t)lo[i] * tnum + j);
        yhi[u] = *reinterpret_cast<const In *>(x + (size_t)hi[i] * tnum + j);
    }
#pragma unroll
    for (int u = 0; u < VA_ROWS; ++u) {
        const int i = i0 + u;
        if (i < n_out) {
            const double dm = den[i], tm = t[i];
            Out o;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const double slope = (double)(T)(yhi[u].v[c] - ylo[u].v[c]) / dm;
                o.v[c] = slope * tm + (double)ylo[u].v[c];
            }
            *reinterpret_cast<Out *>(out + (size_t)i * tnum + j) = o;
        }
    }
}

// A thread owns V consecutive traces of VA_ROWS consecutive output rows.  Neighbouring traces read rows a few
// samples apart, so the loads of a wavefront fall into a few row segments; the stores are whole row segments
// (16 bytes per lane when tnum is even).
template <typename T, int V>
__global__ __launch_bounds__(256) void col_shift_kernel(const T *__restrict__ x, double *__restrict__ out, int snum,
                                                        int tnum, int n_out, const int *__restrict__ shift)
{
    typedef RwVec<double, V> Out;
    const int j = (blockIdx.x * 256 + threadIdx.x) * V;
    if (j >= tnum) return;
    const int i0 = blockIdx.y * VA_ROWS;
    int s[V];
#pragma unroll
    for (int c = 0; c < V; ++c) s[c] = shift[j + c];
    T y[VA_ROWS][V];
#pragma unroll
    for (int u = 0; u < VA_ROWS; ++u) {
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const long long r = (long long)i0 + u + s[c];
            y[u][c] = r >= 0 && r < snum ? x[(size_t)r * tnum + j + c] : (T)__builtin_nan("");
        }
    }
#pragma unroll
    for (int u = 0; u < VA_ROWS; ++u) {
        if (i0 + u < n_out) {
            Out o;
#pragma unroll
            for (int c = 0; c < V; ++c) o.v[c] = (double)y[u][c];
            *reinterpret_cast<Out *>(out + (size_t)(i0 + u) * tnum + j) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct VaxisBufs {
    DevBuf data, out, idx;   // staging of the host-buffer forms (input, result) and the per-row / per-trace tables
    void release()
    {
        data.release();
        out.release();
        idx.release();
    }
};
static StepScratch<VaxisBufs> g_va;

void impdar_vaxis_forget(impdar_ctx *ctx) { g_va.forget(ctx); }

template <typename T, int V>
static void row_lerp_launch(impdar_ctx *ctx, const void *d_data, double *d_out, int tnum, int n_out, const int *d_lo,
                            const int *d_hi, const double *d_den, const double *d_t)
{
    const dim3 grid(((tnum + V - 1) / V + 255) / 256, (n_out + VA_ROWS - 1) / VA_ROWS);
    hipLaunchKernelGGL((row_lerp_kernel<T, V>), grid, dim3(256), 0, ctx->stream, (const T *)d_data, d_out, tnum, n_out,
                       d_lo, d_hi, d_den, d_t);
}

static int row_lerp_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *lo, const int *hi,
                          const double *den, const double *t, int n_out, const double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && lo && hi && den && t && out, "impdar_row_lerp: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_row_lerp: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1 && n_out >= 0, "impdar_row_lerp: bad shape %d x %d -> %d rows", snum, tnum, n_out);
    IMPDAR_ARG_CHECK((size_t)n_out <= (size_t)65535 * VA_ROWS, "impdar_row_lerp: %d output rows (at most %d)", n_out,
                     65535 * VA_ROWS);
    for (int i = 0; i < n_out; ++i)
        IMPDAR_ARG_CHECK(lo[i] >= 0 && lo[i] < snum && hi[i] >= 0 && hi[i] < snum, "impdar_row_lerp: row index out of range at %d", i);
    return IMPDAR_OK;
}

extern "C" int impdar_row_lerp_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const int *lo,
                                   const int *hi, const double *den, const double *t, int n_out, double *d_out)
{
    const auto lock = g_va.lock();
    int rc = row_lerp_check(ctx, d_data, dtype, snum, tnum, lo, hi, den, t, n_out, d_out);
    if (rc) return rc;
    if (n_out == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_va.bind(ctx);
    const size_t ib = (size_t)n_out * sizeof(int), db = (size_t)n_out * sizeof(double);
    const void *d_tab[4];
    rc = impdar_upload_tables(ctx, g_va.idx, {{den, db}, {t, db}, {lo, ib}, {hi, ib}}, d_tab);
    if (rc) return rc;
    // 16-byte accesses need every row on a 16-byte boundary: the arrays themselves and the row pitch
    rw_dispatch(dtype, {d_data, d_out}, tnum, [&](auto ty, auto v) {
        row_lerp_launch<typename decltype(ty)::type, decltype(v)::value>(ctx, d_data, d_out, tnum, n_out, (const int *)d_tab[2],
                                                                         (const int *)d_tab[3], (const double *)d_tab[0],
                                                                         (const double *)d_tab[1]);
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

template <typename T, int V>
static void col_shift_launch(impdar_ctx *ctx, const void *d_data, double *d_out, int snum, int tnum, int n_out,
                             const int *d_shift)
{
    const dim3 grid(((tnum + V - 1) / V + 255) / 256, (n_out + VA_ROWS - 1) / VA_ROWS);
    hipLaunchKernelGGL((col_shift_kernel<T, V>), grid, dim3(256), 0, ctx->stream, (const T *)d_data, d_out, snum, tnum,
                       n_out, d_shift);
}

static int col_shift_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *shift, int n_out,
                           const double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && shift && out, "impdar_col_shift: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_col_shift: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1 && n_out >= 0, "impdar_col_shift: bad shape %d x %d -> %d rows", snum, tnum, n_out);
    IMPDAR_ARG_CHECK((size_t)n_out <= (size_t)65535 * VA_ROWS, "impdar_col_shift: %d output rows (at most %d)", n_out,
                     65535 * VA_ROWS);
    return IMPDAR_OK;
}

extern "C" int impdar_col_shift_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const int *shift,
                                    int n_out, double *d_out)
{
    const auto lock = g_va.lock();
    int rc = col_shift_check(ctx, d_data, dtype, snum, tnum, shift, n_out, d_out);
    if (rc) return rc;
    if (n_out == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_va.bind(ctx);
    const void *d_tab[1];
    rc = impdar_upload_tables(ctx, g_va.idx, {{shift, (size_t)tnum * sizeof(int)}}, d_tab);
    if (rc) return rc;
    // the loads are scalar: only the stores of the float64 output are vectors, two of them at the most
    rw_dispatch<2>(dtype, {d_out}, tnum, [&](auto t, auto v) {
        col_shift_launch<typename decltype(t)::type, decltype(v)::value>(ctx, d_data, d_out, snum, tnum, n_out, (const int *)d_tab[0]);
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer forms: the argument check, then StepScratch::host_form ----------------------------------

extern "C" int impdar_row_lerp(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *lo,
                               const int *hi, const double *den, const double *t, int n_out, double *out)
{
    const int rc = row_lerp_check(ctx, data, dtype, snum, tnum, lo, hi, den, t, n_out, out);
    if (rc) return rc;
    if (n_out == 0) return IMPDAR_OK;
    return g_va.host_form(ctx, g_va.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype), &g_va.out, out,
                          (size_t)n_out * tnum * sizeof(double), [&](void *d_in, void *d_out) {
                              return impdar_row_lerp_dev(ctx, d_in, dtype, snum, tnum, lo, hi, den, t, n_out, (double *)d_out);
                          });
}

extern "C" int impdar_col_shift(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *shift,
                                int n_out, double *out)
{
    const int rc = col_shift_check(ctx, data, dtype, snum, tnum, shift, n_out, out);
    if (rc) return rc;
    if (n_out == 0) return IMPDAR_OK;
    return g_va.host_form(ctx, g_va.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype), &g_va.out, out,
                          (size_t)n_out * tnum * sizeof(double), [&](void *d_in, void *d_out) {
                              return impdar_col_shift_dev(ctx, d_in, dtype, snum, tnum, shift, n_out, (double *)d_out);
                          });
}
