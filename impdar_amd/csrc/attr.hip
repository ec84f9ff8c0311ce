// Complex-trace attributes of a (snum, tnum) radargram where it lies: the quadrature trace, the envelope (reflection strength),
// the instantaneous phase and the instantaneous frequency, from the analytic signal z = x + i H[x] of every trace -- an
// extension: the reference has no Hilbert transform.  The contract and every refusal, route and scratch size are
// attr_route.h's; the kernels are attr_kernels.h.
//
//   own transforms   transpose in -> attr_rows_kernel (in place on the float64 rows) -> transpose back with the rounding
//   rocFFT           transpose in -> attr_flag_kernel -> plan forward -> attr_multiply_kernel -> plan inverse -> attr_global_kernel ->
//                    transpose back with the rounding.  The inverse plan carries no scale (rocFFT 1.0.36 refuses a scaled
//                    real-inverse plan at some even lengths, 16386 among them): the kernel after it multiplies by 1 / n, as the
//                    row kernel does.
//
// d_out may be d_data: the data are read once, by the first transpose.  Each call leaves a metrics line with its device time.
#include "common.h"
#include "fft.h"
#include "attr_kernels.h"

struct AttrBufs {
    DevBuf in, out, rows, spec, quad, flags;     // staging of the host form (2); float64 rows; rocFFT spectrum, quadrature, flags
    OwnTwiddles tw;
    FftPlan fwd, inv;
    int plan_n = 0;
    long long plan_rows = 0;
    void release()
    {
        for (DevBuf *b : {&in, &out, &rows, &spec, &quad, &flags, &tw.buf}) b->release();
        tw.nt = 0;
        fwd.release();
        inv.release();
        plan_n = 0;
        plan_rows = 0;
    }
};
static StepScratch<AttrBufs> g_at;

void impdar_attr_forget(impdar_ctx *ctx) { g_at.forget(ctx); }

template <typename TI, typename TO>
static int attr_transpose(const AttrRoute &A, const void *in, size_t in_pitch, void *out, size_t out_pitch, int rows, int cols, hipStream_t st)
{
    const long long tx = (cols + SPEC_TILE - 1) / SPEC_TILE, ty = (rows + SPEC_TILE - 1) / SPEC_TILE;
    IMPDAR_ARG_CHECK(tx * ty == A.tiles_x * A.tiles_y, "impdar_attr: %lld x %lld tiles are not the route's", tx, ty);
    hipLaunchKernelGGL((attr_transpose_kernel<TI, TO>), dim3((unsigned)(tx * ty)), dim3(256), 0, st, (const TI *)in, in_pitch, (TO *)out, out_pitch, rows,
                       cols, (int)tx);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

static int attr_launch_rows(impdar_ctx *ctx, const SpecRoute &R, int mode, int kind, int half, double tpd, double *rows)
{
    int rc = g_at.tw.ensure<double>(R.n, ctx->stream);
    if (rc) return rc;
    OwnMixedPlan pl;
    if (R.kind == SPEC_OWN_MIXED) IMPDAR_ARG_CHECK(own_mixed_plan_make(R.M, pl), "impdar_attr: no mixed-radix plan for %d", R.M);
    const OCp<double> *t = g_at.tw.buf.as<OCp<double>>();
#define ATTR_LAUNCH_NT(MIXED, MODE, NT)                                                                                           \
    do {                                                                                                                          \
        auto k = attr_rows_kernel<MIXED, MODE, NT>;                                                                               \
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.lds));           \
        hipLaunchKernelGGL(k, dim3((unsigned)R.workgroups), dim3(NT), R.lds, ctx->stream, rows, R.M, R.logm, pl, R.rows, R.rows_per_wg, t, kind, half, \
                           tpd);                                                                                                  \
    } while (0)
#define ATTR_LAUNCH_MODE(MIXED, MODE)                                                                                             \
    do {                                                                                                                          \
        if (R.threads == 1024) ATTR_LAUNCH_NT(MIXED, MODE, 1024);                                                                 \
        else if (R.threads == 512) ATTR_LAUNCH_NT(MIXED, MODE, 512);                                                              \
        else if (R.threads == 256) ATTR_LAUNCH_NT(MIXED, MODE, 256);                                                              \
        else ATTR_LAUNCH_NT(MIXED, MODE, 64);                                                                                     \
    } while (0)
#define ATTR_LAUNCH(MIXED)                                                                                                        \
    do {                                                                                                                          \
        if (mode == ATTR_MODE_SMOOTH) ATTR_LAUNCH_MODE(MIXED, ATTR_MODE_SMOOTH);                                                  \
        else if (mode == ATTR_MODE_FREQ) ATTR_LAUNCH_MODE(MIXED, ATTR_MODE_FREQ);                                                 \
        else ATTR_LAUNCH_MODE(MIXED, ATTR_MODE_POINT);                                                                            \
    } while (0)
    IMPDAR_ARG_CHECK(R.threads == 1024 || R.threads == 512 || R.threads == 256 || R.threads == 64, "impdar_attr: %d threads", R.threads);
    IMPDAR_ARG_CHECK((R.M + R.threads - 1) / R.threads <= attr_row_acc(R.threads), "impdar_attr: %d pairs on %d threads", R.M, R.threads);
    if (R.kind == SPEC_OWN_MIXED) ATTR_LAUNCH(true);
    else ATTR_LAUNCH(false);
#undef ATTR_LAUNCH
#undef ATTR_LAUNCH_MODE
#undef ATTR_LAUNCH_NT
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

// the rocFFT route on the float64 rows; *res and *res_pitch: where the attribute rows are
static int attr_launch_global(impdar_ctx *ctx, const AttrRoute &A, int mode, int kind, int half, double tpd, double **res, size_t *res_pitch)
{
    const SpecRoute &R = A.spec;
    const int n = R.n;
    const long long rows = R.rows;
    hipStream_t st = ctx->stream;
    IMPDAR_HIP_CHECK(g_at.spec.ensure(A.spectrum_doubles * sizeof(double)));
    IMPDAR_HIP_CHECK(g_at.quad.ensure(A.quad_doubles * sizeof(double)));
    IMPDAR_HIP_CHECK(g_at.flags.ensure(A.flag_ints * sizeof(int)));
    double *x = g_at.rows.as<double>(), *q = g_at.quad.as<double>(), *sp = g_at.spec.as<double>();
    hipLaunchKernelGGL(attr_flag_kernel, dim3((unsigned)rows), dim3(ATTR_GLOBAL_THREADS), 0, st, x, n, g_at.flags.as<int>());
    IMPDAR_HIP_CHECK(hipGetLastError());
    if (A.trivial) {
        IMPDAR_HIP_CHECK(hipMemsetAsync(q, 0, A.quad_doubles * sizeof(double), st));
    } else {
        if (g_at.plan_n != n || g_at.plan_rows != rows || !g_at.fwd.plan || !g_at.inv.plan) {
            g_at.plan_n = 0;
            int rc = g_at.fwd.create(rocfft_transform_type_real_forward, true, false, (size_t)n, (size_t)rows, rocfft_array_type_real,
                                     rocfft_array_type_hermitian_interleaved, 1, (size_t)n, 1, (size_t)R.bins, 1.0, st);
            if (rc) return rc;
            rc = g_at.inv.create(rocfft_transform_type_real_inverse, true, false, (size_t)n, (size_t)rows, rocfft_array_type_hermitian_interleaved,
                                 rocfft_array_type_real, 1, (size_t)R.bins, 1, (size_t)n, 1.0, st);
            if (rc) return rc;
            g_at.plan_n = n;
            g_at.plan_rows = rows;
        }
        int rc = g_at.fwd.exec(x, sp);
        if (rc) return rc;
        const size_t count = (size_t)rows * (size_t)R.bins;
        const unsigned blocks = (unsigned)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
        hipLaunchKernelGGL(attr_multiply_kernel, dim3(blocks), dim3(256), 0, st, g_at.spec.as<OCp<double>>(), n, R.bins, count);
        IMPDAR_HIP_CHECK(hipGetLastError());
        rc = g_at.inv.exec(sp, q);
        if (rc) return rc;
    }
    const size_t sp_pitch = 2 * (size_t)R.bins;
    *res = mode == ATTR_MODE_SMOOTH ? x : sp;
    *res_pitch = A.out_pitch;
    IMPDAR_ARG_CHECK(*res_pitch == (mode == ATTR_MODE_SMOOTH ? (size_t)n : sp_pitch), "impdar_attr: the route's pitch is not the launch's");
    const dim3 grid((unsigned)rows), block(ATTR_GLOBAL_THREADS);
    if (mode == ATTR_MODE_SMOOTH)
        hipLaunchKernelGGL(attr_global_kernel<ATTR_MODE_SMOOTH>, grid, block, 0, st, x, q, sp, sp_pitch, *res, *res_pitch, n, g_at.flags.as<int>(), kind, half, tpd);
    else if (mode == ATTR_MODE_FREQ)
        hipLaunchKernelGGL(attr_global_kernel<ATTR_MODE_FREQ>, grid, block, 0, st, x, q, sp, sp_pitch, *res, *res_pitch, n, g_at.flags.as<int>(), kind, half, tpd);
    else
        hipLaunchKernelGGL(attr_global_kernel<ATTR_MODE_POINT>, grid, block, 0, st, x, q, sp, sp_pitch, *res, *res_pitch, n, g_at.flags.as<int>(), kind, half, tpd);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

static int attr_check(impdar_ctx *ctx, const void *data, const void *out, int dtype, int snum, int tnum, int kind, int smooth, double dt)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "impdar_attr: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_attr: dtype must be float32 or float64");
    const char *why = attr_refusal(snum, tnum, kind, smooth, dt);
    IMPDAR_ARG_CHECK(!why, "impdar_attr: %s (snum %d, tnum %d, kind %d, smooth %d, dt %g)", why, snum, tnum, kind, smooth, dt);
    return IMPDAR_OK;
}

extern "C" int impdar_attr_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int kind, int smooth, double dt, void *d_out)
{
    const auto held = g_at.lock();
    int rc = attr_check(ctx, d_data, d_out, dtype, snum, tnum, kind, smooth, dt);
    if (rc) return rc;
    const AttrRoute A = attr_route(snum, tnum, kind, smooth);
    IMPDAR_ARG_CHECK(A.ok, "impdar_attr: no route for %d traces of %d samples", tnum, snum);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_at.bind(ctx);
    const bool f32 = dtype == IMPDAR_F32;
    const int mode = kind != ATTR_FREQUENCY ? ATTR_MODE_POINT : (smooth > 1 ? ATTR_MODE_SMOOTH : ATTR_MODE_FREQ), half = (smooth - 1) / 2;
    const double tpd = 6.283185307179586476925286766559 * dt;
    IMPDAR_HIP_CHECK(g_at.rows.ensure(A.rowbuf_doubles * sizeof(double)));
    impdar_ctx_note(ctx, "impdar_attr", A.label);
    if ((rc = impdar_ctx_tic(ctx))) return rc;
    rc = f32 ? attr_transpose<float, double>(A, d_data, (size_t)tnum, g_at.rows.p, (size_t)snum, snum, tnum, ctx->stream)
             : attr_transpose<double, double>(A, d_data, (size_t)tnum, g_at.rows.p, (size_t)snum, snum, tnum, ctx->stream);
    if (rc) return rc;
    double *res = g_at.rows.as<double>();
    size_t res_pitch = A.out_pitch;
    if (A.spec.kind != SPEC_ROCFFT) rc = attr_launch_rows(ctx, A.spec, mode, kind, half, tpd, res);
    else rc = attr_launch_global(ctx, A, mode, kind, half, tpd, &res, &res_pitch);
    if (rc) return rc;
    rc = f32 ? attr_transpose<double, float>(A, res, res_pitch, d_out, (size_t)tnum, tnum, snum, ctx->stream)
             : attr_transpose<double, double>(A, res, res_pitch, d_out, (size_t)tnum, tnum, snum, ctx->stream);
    if (rc) return rc;
    if ((rc = impdar_ctx_toc(ctx))) return rc;
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_attr(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int kind, int smooth, double dt, void *out)
{
    const int rc = attr_check(ctx, data, out, dtype, snum, tnum, kind, smooth, dt);
    if (rc) return rc;
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    return g_at.host_form(ctx, g_at.in, data, bytes, &g_at.out, out, bytes,
                          [&](void *d_in, void *d_out) { return impdar_attr_dev(ctx, d_in, dtype, snum, tnum, kind, smooth, dt, d_out); });
}

extern "C" int impdar_attr_route_probe(int snum, int tnum, int kind, int smooth, int *out)
{
    IMPDAR_ARG_CHECK(out, "impdar_attr_route_probe: null argument");
    const char *why = attr_refusal(snum, tnum, kind, smooth, 1.0);
    IMPDAR_ARG_CHECK(!why, "impdar_attr_route_probe: %s", why);
    const AttrRoute A = attr_route(snum, tnum, kind, smooth);
    IMPDAR_ARG_CHECK(A.ok, "impdar_attr_route_probe: no route for %d traces of %d samples", tnum, snum);
    out[0] = A.spec.kind;
    out[1] = A.spec.threads;
    out[2] = (int)A.spec.workgroups;
    out[3] = (int)(A.spec.rows_per_wg < 0x7fffffff ? A.spec.rows_per_wg : 0x7fffffff);
    out[4] = (int)A.spec.lds;
    out[5] = A.trivial;
    return IMPDAR_OK;
}
