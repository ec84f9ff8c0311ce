// Layer slopes of a (snum, tnum) radargram where it lies: the structure-tensor field (slope, dip, coherence or a tensor
// component) and the mean along the layers (dipsmooth) -- an extension: the reference has no slope field.  The contract, every
// refusal, block size and scratch size are slope_route.h's; the kernels are slope_kernels.h.
//
//   impdar_slope      row pass (products, Gaussian along the traces) -> three float64 planes -> column pass (Gaussian along the
//                     samples, eigen-analysis) -> the float64 field
//   impdar_dipsmooth  [the two passes at kind 0 into a scratch field, when no slope is given] -> gather; an in-place call gathers
//                     into a scratch copy that is then copied over the data
//
// Each call leaves a metrics line with its device time.
#include "vecwidth.h"
#include "slope_kernels.h"

struct SlopeBufs {
    DevBuf in, out, given, planes, field, copy, tables;     // staging of the host forms (3); scratch (3); the two weight tables
    double sz = -1.0, sx = -1.0;                            // the sigmas `tables` holds
    const double *wz = nullptr, *wx = nullptr;
    void release()
    {
        for (DevBuf *b : {&in, &out, &given, &planes, &field, &copy, &tables}) b->release();
        sz = sx = -1.0;
        wz = wx = nullptr;
    }
};
static StepScratch<SlopeBufs> g_sl;

void impdar_slope_forget(impdar_ctx *ctx) { g_sl.forget(ctx); }

// the weight tables of rule 4 on the device (kept while the sigmas stay)
static int slope_tables(impdar_ctx *ctx, double sigma_z, double sigma_x)
{
    if (g_sl.wz && g_sl.sz == sigma_z && g_sl.sx == sigma_x) return IMPDAR_OK;
    double wz[2 * SLOPE_MAX_R + 1], wx[2 * SLOPE_MAX_R + 1];
    int rz = 0, rx = 0;
    slope_weights(sigma_z, wz, &rz);
    slope_weights(sigma_x, wx, &rx);
    g_sl.wz = g_sl.wx = nullptr;
    const TableBlock blk[2] = {{wz, (size_t)(2 * rz + 1) * sizeof(double)}, {wx, (size_t)(2 * rx + 1) * sizeof(double)}};
    const void *dev[2] = {nullptr, nullptr};
    const int rc = impdar_upload_tables(ctx, g_sl.tables, blk, dev);
    if (rc) return rc;
    g_sl.wz = (const double *)dev[0];
    g_sl.wx = (const double *)dev[1];
    g_sl.sz = sigma_z;
    g_sl.sx = sigma_x;
    return IMPDAR_OK;
}

// the two passes, enqueued; the tables are up
static int slope_passes(impdar_ctx *ctx, const SlopeRoute &S, const void *d_data, int dtype, int snum, int tnum, int kind, double max_slope,
                        double *d_field)
{
    const size_t count = (size_t)snum * (size_t)tnum;
    double *pa = g_sl.planes.as<double>(), *pb = pa + count, *pc = pb + count;
    rw_typed(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(slope_row_kernel<T>, dim3((unsigned)S.row_blocks), dim3(SLOPE_ROW_TX), S.row_lds, ctx->stream, (const T *)d_data, snum, tnum,
                           S.rx, g_sl.wx, S.row_blocks_x, pa, pb, pc);
        return 0;
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(slope_col_kernel, dim3((unsigned)S.col_blocks), dim3(SLOPE_COL_THREADS), S.col_lds, ctx->stream, pa, pb, pc, snum, tnum, S.rz,
                       g_sl.wz, S.col_blocks_x, kind, max_slope, d_field);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

static int slope_check(impdar_ctx *ctx, const char *entry, const void *data, const void *out, int dtype, const char *why, int snum, int tnum)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "%s: null argument", entry);
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "%s: dtype must be float32 or float64", entry);
    IMPDAR_ARG_CHECK(!why, "%s: %s (snum %d, tnum %d)", entry, why, snum, tnum);
    return IMPDAR_OK;
}

extern "C" int impdar_slope_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int kind, double sigma_z, double sigma_x,
                                double max_slope, double *d_out)
{
    const auto held = g_sl.lock();
    int rc = slope_check(ctx, "impdar_slope", d_data, d_out, dtype, slope_refusal(snum, tnum, kind, sigma_z, sigma_x, max_slope), snum, tnum);
    if (rc) return rc;
    const SlopeRoute S = slope_route(snum, tnum, sigma_z, sigma_x, impdar_dtype_size(dtype));
    IMPDAR_ARG_CHECK(S.ok, "impdar_slope: no route for %d traces of %d samples", tnum, snum);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_sl.bind(ctx);
    IMPDAR_HIP_CHECK(g_sl.planes.ensure(S.plane_bytes));
    if ((rc = slope_tables(ctx, sigma_z, sigma_x))) return rc;
    impdar_ctx_note(ctx, "impdar_slope", "slope_row_kernel + slope_col_kernel");
    if ((rc = impdar_ctx_tic(ctx))) return rc;
    if ((rc = slope_passes(ctx, S, d_data, dtype, snum, tnum, kind, max_slope, d_out))) return rc;
    if ((rc = impdar_ctx_toc(ctx))) return rc;
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_dipsmooth_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int half, const double *d_slope,
                                    double sigma_z, double sigma_x, double max_slope, void *d_out)
{
    const auto held = g_sl.lock();
    int rc = slope_check(ctx, "impdar_dipsmooth", d_data, d_out, dtype,
                         dipsmooth_refusal(snum, tnum, half, d_slope != nullptr, sigma_z, sigma_x, max_slope), snum, tnum);
    if (rc) return rc;
    const bool own = d_slope == nullptr, in_place = d_out == d_data;
    const SlopeRoute S = slope_route(snum, tnum, own ? sigma_z : 0.0, own ? sigma_x : 0.0, impdar_dtype_size(dtype));
    IMPDAR_ARG_CHECK(S.ok, "impdar_dipsmooth: no route for %d traces of %d samples", tnum, snum);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_sl.bind(ctx);
    if (own) {
        IMPDAR_HIP_CHECK(g_sl.planes.ensure(S.plane_bytes));
        IMPDAR_HIP_CHECK(g_sl.field.ensure(S.field_bytes));
        if ((rc = slope_tables(ctx, sigma_z, sigma_x))) return rc;
    }
    if (in_place) IMPDAR_HIP_CHECK(g_sl.copy.ensure(S.inplace_bytes));
    impdar_ctx_note(ctx, "impdar_dipsmooth", own ? "slope_row_kernel + slope_col_kernel + slope_gather_kernel" : "slope_gather_kernel");
    if ((rc = impdar_ctx_tic(ctx))) return rc;
    if (own && (rc = slope_passes(ctx, S, d_data, dtype, snum, tnum, SLOPE_KIND_SLOPE, max_slope, g_sl.field.as<double>()))) return rc;
    const double *slope = own ? g_sl.field.as<double>() : d_slope;
    void *y = in_place ? g_sl.copy.p : d_out;
    rw_typed(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(slope_gather_kernel<T>, dim3((unsigned)S.gather_blocks), dim3(SLOPE_GATHER_THREADS), 0, ctx->stream, (const T *)d_data, slope,
                           snum, tnum, half, (T *)y);
        return 0;
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    if (in_place) IMPDAR_HIP_CHECK(hipMemcpyAsync(d_out, y, S.inplace_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = impdar_ctx_toc(ctx))) return rc;
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer forms: the argument check, then StepScratch::host_form ----------------------------------

extern "C" int impdar_slope(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int kind, double sigma_z, double sigma_x,
                            double max_slope, double *out)
{
    const int rc = slope_check(ctx, "impdar_slope", data, out, dtype, slope_refusal(snum, tnum, kind, sigma_z, sigma_x, max_slope), snum, tnum);
    if (rc) return rc;
    const size_t count = (size_t)snum * (size_t)tnum;
    return g_sl.host_form(ctx, g_sl.in, data, count * impdar_dtype_size(dtype), &g_sl.out, out, count * sizeof(double), [&](void *d_in, void *d_out) {
        return impdar_slope_dev(ctx, d_in, dtype, snum, tnum, kind, sigma_z, sigma_x, max_slope, (double *)d_out);
    });
}

extern "C" int impdar_dipsmooth(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int half, const double *slope, double sigma_z,
                                double sigma_x, double max_slope, void *out)
{
    const int rc = slope_check(ctx, "impdar_dipsmooth", data, out, dtype,
                               dipsmooth_refusal(snum, tnum, half, slope != nullptr, sigma_z, sigma_x, max_slope), snum, tnum);
    if (rc) return rc;
    const size_t count = (size_t)snum * (size_t)tnum, bytes = count * impdar_dtype_size(dtype);
    return g_sl.host_form(ctx, g_sl.in, data, bytes, &g_sl.out, out, bytes, [&](void *d_in, void *d_out) -> int {
        if (slope) {
            IMPDAR_HIP_CHECK(g_sl.given.ensure(count * sizeof(double)));
            IMPDAR_HIP_CHECK(hipMemcpyAsync(g_sl.given.p, slope, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        }
        return impdar_dipsmooth_dev(ctx, d_in, dtype, snum, tnum, half, slope ? g_sl.given.as<double>() : nullptr, sigma_z, sigma_x, max_slope, d_out);
    });
}

extern "C" int impdar_slope_route_probe(int snum, int tnum, double sigma_z, double sigma_x, int half, int *out)
{
    IMPDAR_ARG_CHECK(out, "impdar_slope_route_probe: null argument");
    const char *why = dipsmooth_refusal(snum, tnum, half, false, sigma_z, sigma_x, 1.0);
    IMPDAR_ARG_CHECK(!why, "impdar_slope_route_probe: %s", why);
    const SlopeRoute S = slope_route(snum, tnum, sigma_z, sigma_x, sizeof(double));
    IMPDAR_ARG_CHECK(S.ok, "impdar_slope_route_probe: no route for %d traces of %d samples", tnum, snum);
    const long long cap = 0x7fffffff, mb = (long long)((S.plane_bytes + S.field_bytes + S.inplace_bytes + ((size_t)1 << 20) - 1) >> 20);
    out[0] = S.rz;
    out[1] = S.rx;
    out[2] = SLOPE_ROW_TX;
    out[3] = (int)S.row_blocks;
    out[4] = (int)S.row_lds;
    out[5] = SLOPE_COL_THREADS;
    out[6] = (int)S.col_blocks;
    out[7] = (int)S.col_lds;
    out[8] = SLOPE_GATHER_THREADS;
    out[9] = (int)S.gather_blocks;
    out[10] = (int)(mb < cap ? mb : cap);
    return IMPDAR_OK;
}
