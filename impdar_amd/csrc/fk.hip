// f-k fan (dip) filter and f-k power spectrum of a (snum, tnum) radargram on gfx950 -- an extension: the reference has neither.
//
//   filter    y = Re ifft2(M * fft2(x)), M the real fan weight of fk_weight.h (apparent velocities va_lo <= |w| / |kx| <= va_hi,
//             cosine tapers in slowness, either dip side or both, pass or reject), shape and dtype of x
//   spectrum  P[j][i] = |fft2(x)[j][i]|^2 for the snum / 2 + 1 rows w >= 0, columns in fftshift order, float64, not normalised
//
// The transforms are Stolt's (stolt_stages.h), on the plan Stolt caches: the forward half with the tapers off leaves the spectrum
// as [kx >= 0][all w], [w >= 0][kx] or [kx][w >= 0] (stolt_route.h); the fan kernel of that layout (fk_kernels.h) stands where
// the Stolt stretch stands, one read and one write of the half spectrum; the inverse chain of the route brings the snum rows
// back.  At odd snum (rocFFT only) Stolt's inverse is one row short and a 2-D real inverse of snum rows is kept beside it
// (fk_route.h).  The transforms run in the data's precision, the weight in float64 from the float64 axes.
#include "fk_kernels.h"
#include "fk_route.h"
#include "stolt_stages.h"
#include <limits>

static inline unsigned fk_rows_grid(int rows) { return (unsigned)std::min(std::max(rows, 1), 65535); }
// The grid of a fan kernel on a layout of `rows` rows of `cols` complex numbers: 16 bytes per lane along a row, and about
// FK_FAN_BLOCKS workgroups in all, which stride over the rows.
constexpr int FK_FAN_BLOCKS = 4096;
template <typename T> static dim3 fk_fan_grid(int rows, int cols)
{
    const int per = FK_FAN_THREADS * fk_fan_vec<T>();
    const int gx = (cols + per - 1) / per;
    return dim3((unsigned)gx, (unsigned)std::min(std::max(rows, 1), std::max(FK_FAN_BLOCKS / gx, 1)));
}

// fan == nullptr: the spectrum into d_out ([m][tnum] float64); else the filtered radargram ([snum][tnum] of T; d_out may be d_data)
template <typename T>
static int fk_run(impdar_ctx *ctx, StoltPlan &pl, const void *d_data, int snum, int tnum, const double *kx, const double *ws,
                  const FkFan *fan, void *d_out)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();      // the front's tapers off
    const bool dbl = sizeof(T) == 8;
    StoltCall c;
    int rc;
    const int builds = pl.builds;
    if ((rc = stolt_prepare<T>(ctx, pl, snum, tnum, kx, ws, nan, nan, c))) return rc;
    hipStream_t st = ctx->stream;
    const int m = c.m;
    const FkRoute fr = fk_route(snum, tnum, kx, StoltKnobs::from_env());
    const bool odd = fan && fr.own_inverse_plan;
    bool planned = pl.builds != builds;
    if (odd) {
        if (!pl.fk_inv.plan || !(pl.fk_inv_key == pl.key)) {
            if ((rc = pl.fk_inv.create2d(rocfft_transform_type_real_inverse, dbl, false, snum, tnum, rocfft_array_type_hermitian_interleaved,
                                         rocfft_array_type_real, m, snum, 1.0 / ((double)snum * tnum), st)))
                return rc;
            pl.fk_inv_key = pl.key;
            planned = true;
        }
        IMPDAR_HIP_CHECK(pl.Y.ensure((size_t)tnum * snum * sizeof(T)));
    }
    if ((rc = impdar_ctx_tic(ctx))) return rc;
    if ((rc = stolt_front<T>(ctx, pl, c, d_data))) return rc;
    const double *dkx = pl.d_kx.as<double>(), *dws = pl.d_ws.as<double>();
    Cx<T> *F = pl.F.as<Cx<T>>(), *K = pl.K.as<Cx<T>>();
    if ((rc = impdar_ctx_ktic(ctx))) return rc;
    if (!fan) {
        double *P = (double *)d_out;
        if (c.route == STOLT_OWN_ROWS)
            hipLaunchKernelGGL((fk_power_t<T, true>), dim3((snum + 63) / 64, (c.hs + 63) / 64), dim3(256), 0, st, K, P, c.hs, snum, m, snum, tnum);
        else if (c.use_own)
            hipLaunchKernelGGL((fk_power_wkx<T>), dim3((tnum + 255) / 256, fk_rows_grid(m)), dim3(256), 0, st, K, P, m, tnum);
        else
            hipLaunchKernelGGL((fk_power_t<T, false>), dim3((m + 63) / 64, (tnum + 63) / 64), dim3(256), 0, st, F, P, tnum, m, m, snum, tnum);
        if ((rc = impdar_ctx_ktoc(ctx))) return rc;
    } else if (c.route == STOLT_OWN_ROWS) {      // K [kx >= 0][w] -> F
        hipLaunchKernelGGL((fk_fan_rows<T>), fk_fan_grid<T>(c.hs, snum), dim3(FK_FAN_THREADS), 0, st, K, F, dkx, dws, c.hs, snum, tnum, *fan);
        if ((rc = impdar_ctx_ktoc(ctx))) return rc;
        if ((rc = stolt_inverse_rows<T>(pl, c, 1, F, K, (T *)d_out, st))) return rc;
    } else if (c.use_own) {                      // K [w][kx] -> F
        hipLaunchKernelGGL((fk_fan_wkx<T>), fk_fan_grid<T>(m, tnum), dim3(FK_FAN_THREADS), 0, st, K, F, dkx, dws, m, snum, tnum, *fan);
        if ((rc = impdar_ctx_ktoc(ctx))) return rc;
        if ((rc = stolt_inverse_wkx<T>(pl, c, 1, F, K, (T *)d_out, st))) return rc;
    } else {                                     // F [kx][w] -> K
        hipLaunchKernelGGL((fk_fan_kxw<T>), fk_fan_grid<T>(tnum, m), dim3(FK_FAN_THREADS), 0, st, F, K, dkx, dws, m, snum, tnum, *fan);
        if ((rc = impdar_ctx_ktoc(ctx))) return rc;
        if (odd) {
            if ((rc = pl.fk_inv.exec(pl.K.p, pl.Y.p))) return rc;
            hipLaunchKernelGGL((stolt_transpose_back<T>), dim3((tnum + 63) / 64, (snum + 63) / 64), dim3(256), 0, st, pl.Y.as<T>(), (T *)d_out,
                               snum, tnum);
        } else if ((rc = stolt_inverse_rocfft<T>(pl, c, (T *)d_out, st))) {
            return rc;
        }
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    impdar_trace("fk: all kernels enqueued");
    ctx->m_entry = fan ? "impdar_fk_fan" : "impdar_fk_power";
    ctx->m_kernel = fk_kernel_label(c, !fan);
    ctx->m_kernel_ms = -1.f;
    // "planned": this call made plans or buffers; "plans_built": how often the shared plan was made anew in this process so far
    snprintf(ctx->m_extra, sizeof ctx->m_extra, "\"planned\": %d, \"plans_built\": %d", planned ? 1 : 0, pl.builds);
    return impdar_ctx_toc(ctx);
}

static int fk_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const double *kx, const double *ws, const FkFan *fan,
                  void *d_out)
{
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(g_stolt_mu);
    ImpdarBusy busy(t_stolt_busy);
    if (!g_stolt_plan) g_stolt_plan = new StoltPlan();
    auto run = dtype == IMPDAR_F32 ? fk_run<float> : fk_run<double>;
    const int rc = run(ctx, *g_stolt_plan, d_data, snum, tnum, kx, ws, fan, d_out);
    if (rc) return rc;
    // kx / ws were staged from caller memory: complete before returning
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return impdar_ctx_mark_produced(ctx);
}

static int fk_fan_args(int dtype, int snum, int tnum, double va_lo, double va_hi, double taper, int mode, int dip)
{
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    const char *why = fk_fan_refusal(snum, tnum, va_lo, va_hi, taper, mode, dip);
    IMPDAR_ARG_CHECK(!why, "impdar_fk_fan: %s (snum %d, tnum %d, va_lo %g, va_hi %g, taper %g, mode %d, dip %d)", why, snum, tnum, va_lo,
                     va_hi, taper, mode, dip);
    return IMPDAR_OK;
}

extern "C" int impdar_fk_fan_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const double *kx, const double *ws,
                                 double va_lo, double va_hi, double taper, int mode, int dip, void *d_out)
{
    IMPDAR_ARG_CHECK(ctx && d_data && d_out && kx && ws, "null argument");
    const int rc = fk_fan_args(dtype, snum, tnum, va_lo, va_hi, taper, mode, dip);
    if (rc) return rc;
    const FkFan fan = fk_fan_make(va_lo, va_hi, taper, mode, dip);
    return fk_dev(ctx, d_data, dtype, snum, tnum, kx, ws, &fan, d_out);
}

// The host forms: upload, the resident form, download.
static int fk_host(const char *entry, impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *kx, const double *ws,
                   const FkFan *fan, void *out)
{
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t inb = (size_t)snum * tnum * impdar_dtype_size(dtype);
    const size_t outb = fan ? inb : (size_t)(snum / 2 + 1) * tnum * 8;
    impdar_ctx_pinned_prefetch(ctx, std::min(outb, IMPDAR_STAGE_RING_BYTES));
    CallArrays a{ctx};
    int rc = a.alloc(inb, outb);
    if (rc) return rc;
    if (hipMemcpyAsync(a.din, data, inb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        impdar_set_error("%s: upload failed: %s", entry, hipGetErrorString(hipGetLastError()));
        return IMPDAR_ERR_HIP;
    }
    if ((rc = fk_dev(ctx, a.din, dtype, snum, tnum, kx, ws, fan, a.dout))) return rc;
    return impdar_download(ctx, out, a.dout, outb, ctx->stream);
}

extern "C" int impdar_fk_fan(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *kx, const double *ws,
                             double va_lo, double va_hi, double taper, int mode, int dip, void *out)
{
    IMPDAR_ARG_CHECK(ctx && data && out && kx && ws, "null argument");
    const int rc = fk_fan_args(dtype, snum, tnum, va_lo, va_hi, taper, mode, dip);
    if (rc) return rc;
    const FkFan fan = fk_fan_make(va_lo, va_hi, taper, mode, dip);
    return fk_host("impdar_fk_fan", ctx, data, dtype, snum, tnum, kx, ws, &fan, out);
}

static int fk_power_args(int dtype, int snum, int tnum)
{
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    IMPDAR_ARG_CHECK(snum >= 2 && tnum >= 2, "impdar_fk_power: need snum >= 2 and tnum >= 2 (got %d, %d)", snum, tnum);
    return IMPDAR_OK;
}

extern "C" int impdar_fk_power_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const double *kx, const double *ws,
                                   void *d_out)
{
    IMPDAR_ARG_CHECK(ctx && d_data && d_out && kx && ws, "null argument");
    const int rc = fk_power_args(dtype, snum, tnum);
    if (rc) return rc;
    return fk_dev(ctx, d_data, dtype, snum, tnum, kx, ws, nullptr, d_out);
}

extern "C" int impdar_fk_power(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *kx, const double *ws,
                               double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && out && kx && ws, "null argument");
    const int rc = fk_power_args(dtype, snum, tnum);
    if (rc) return rc;
    return fk_host("impdar_fk_power", ctx, data, dtype, snum, tnum, kx, ws, nullptr, out);
}
