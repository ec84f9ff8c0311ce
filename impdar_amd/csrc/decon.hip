// Predictive (gapped, Wiener-Levinson) deconvolution and the autocorrelogram of a (snum, tnum) radargram on gfx950 -- an
// extension: the reference has neither.  The contract is decon_core.h, the kernels are decon_kernels.h, and every refusal and
// launch argument is decon_route.h's.
//
//   impdar_decon   autocorrelation (one read of the radargram) -> lag table [lags][tnum] -> the recursion per trace (or, design
//                  'mean', the table summed over the live traces and one recursion) -> operators [oplen][tnum] -> apply (one
//                  read and one write of the radargram; d_out may be d_data)
//   impdar_acorr   the autocorrelation kernel straight into the caller's (maxlag + 1, tnum) float64 array, then the division
//
// Each call leaves a metrics line with the device time and the times of its stages ("acorr_ms", "solve_ms", "apply_ms").
#include "common.h"
#include "decon_kernels.h"

struct DeconBufs {
    DevBuf in, out, scratch, opout;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void release()
    {
        in.release();
        out.release();
        scratch.release();
        opout.release();
        for (hipEvent_t &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
};
static StepScratch<DeconBufs> g_dc;

void impdar_decon_forget(impdar_ctx *ctx) { g_dc.forget(ctx); }

static int dc_mark(impdar_ctx *ctx, int k)
{
    if (!g_dc.ev[k]) IMPDAR_HIP_CHECK(hipEventCreate(&g_dc.ev[k]));
    IMPDAR_HIP_CHECK(hipEventRecord(g_dc.ev[k], ctx->stream));
    return IMPDAR_OK;
}

// the stream is drained and the stages' times go into the metrics line
static int dc_stage_times(impdar_ctx *ctx, int stages)
{
    static const char *const names[3] = {"acorr_ms", "solve_ms", "apply_ms"};
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    size_t used = 0;
    for (int k = 0; k < stages; ++k) {
        float ms = 0.f;
        IMPDAR_HIP_CHECK(hipEventElapsedTime(&ms, g_dc.ev[k], g_dc.ev[k + 1]));
        const int w = snprintf(ctx->m_extra + used, sizeof ctx->m_extra - used, "%s\"%s\": %.4f", k ? ", " : "", names[k], ms);
        if (w > 0) used += (size_t)w;
    }
    return IMPDAR_OK;
}

static int dc_launch_acorr(impdar_ctx *ctx, const DeconPlan &P, const void *d_data, int dtype, int tnum, int s0, int s1, double *d_lag)
{
    rw_dispatch(dtype, {d_data}, tnum, [&](auto t, auto v) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL((decon_acorr_kernel<T, decltype(v)::value>), dim3((unsigned)P.groups, (unsigned)P.lag_chunks), dim3(DECON_THREADS),
                           P.acorr_lds, ctx->stream, (const T *)d_data, tnum, s0, s1, P.lags, d_lag);
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

static int decon_check(impdar_ctx *ctx, const void *data, const void *out, int dtype, int snum, int tnum, int s0, int s1, int oplen, int gap,
                       double prewhiten, int design)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "impdar_decon: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_decon: dtype must be float32 or float64");
    const char *why = decon_refusal(snum, tnum, s0, s1, oplen, gap, prewhiten, design);
    IMPDAR_ARG_CHECK(!why, "impdar_decon: %s (snum %d, tnum %d, window [%d, %d), oplen %d, gap %d, prewhiten %g, design %d)", why, snum, tnum, s0,
                     s1, oplen, gap, prewhiten, design);
    return IMPDAR_OK;
}

extern "C" int impdar_decon_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int s0, int s1, int oplen, int gap,
                                double prewhiten, int design, void *d_out, double *d_op)
{
    const auto held = g_dc.lock();
    int rc = decon_check(ctx, d_data, d_out, dtype, snum, tnum, s0, s1, oplen, gap, prewhiten, design);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_dc.bind(ctx);
    const DeconPlan P = decon_plan(snum, tnum, s0, s1, oplen, gap, design);
    IMPDAR_HIP_CHECK(g_dc.scratch.ensure(P.scratch_bytes));
    char *sc = g_dc.scratch.as<char>();
    double *lag = reinterpret_cast<double *>(sc), *op = reinterpret_cast<double *>(sc + P.off_op);
    double *part = reinterpret_cast<double *>(sc + P.off_mean), *R = part + (size_t)P.mean_blocks * P.nlags, *mop = R + P.nlags;
    int *dead = reinterpret_cast<int *>(sc + P.off_dead);
    const bool mean = design == DECON_MEAN;
    const double eps = prewhiten / 100.0;
    hipStream_t st = ctx->stream;
    impdar_ctx_note(ctx, "impdar_decon", P.label);
    if ((rc = impdar_ctx_tic(ctx))) return rc;
    if ((rc = dc_mark(ctx, 0))) return rc;
    if ((rc = dc_launch_acorr(ctx, P, d_data, dtype, tnum, s0, s1, lag))) return rc;
    if ((rc = dc_mark(ctx, 1))) return rc;
    if (mean) {
        hipLaunchKernelGGL(decon_mean_block_kernel, dim3((unsigned)P.mean_blocks), dim3(DECON_MEAN_BLOCK), 0, st, lag, tnum, P.nlags, part, dead);
        hipLaunchKernelGGL(decon_mean_sum_kernel, dim3(1), dim3(256), 0, st, part, P.mean_blocks, P.nlags, R);
        hipLaunchKernelGGL(decon_solve_kernel, dim3((unsigned)P.solve_groups), dim3(64), P.solve_lds, st, R, 1, 1, P.lags, oplen, gap, eps, mop, 1,
                           dead + tnum);
    } else {
        hipLaunchKernelGGL(decon_solve_kernel, dim3((unsigned)P.solve_groups), dim3(64), P.solve_lds, st, lag, tnum, tnum, P.lags, oplen, gap, eps, op,
                           tnum, dead);
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    if ((rc = dc_mark(ctx, 2))) return rc;
    rw_dispatch(dtype, {d_data, d_out}, tnum, [&](auto t, auto v) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL((decon_apply_kernel<T, decltype(v)::value>), dim3((unsigned)P.groups), dim3(DECON_THREADS), P.apply_lds, st,
                           (const T *)d_data, (T *)d_out, snum, tnum, oplen, gap, mean ? mop : op, mean ? 0 : tnum, dead,
                           mean ? dead + tnum : (const int *)nullptr);
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    if (d_op && mean)
        hipLaunchKernelGGL(decon_mean_spread_kernel, dim3((unsigned)((tnum + 255) / 256)), dim3(256), 0, st, mop, dead, oplen, tnum, d_op);
    else if (d_op)
        IMPDAR_HIP_CHECK(hipMemcpyAsync(d_op, op, (size_t)oplen * tnum * sizeof(double), hipMemcpyDeviceToDevice, st));
    IMPDAR_HIP_CHECK(hipGetLastError());
    if ((rc = dc_mark(ctx, 3))) return rc;
    if ((rc = impdar_ctx_toc(ctx))) return rc;
    if ((rc = dc_stage_times(ctx, 3))) return rc;
    return impdar_ctx_mark_produced(ctx);
}

static int acorr_check(impdar_ctx *ctx, const void *data, const void *out, int dtype, int snum, int tnum, int s0, int s1, int maxlag)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "impdar_acorr: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_acorr: dtype must be float32 or float64");
    const char *why = acorr_refusal(snum, tnum, s0, s1, maxlag);
    IMPDAR_ARG_CHECK(!why, "impdar_acorr: %s (snum %d, tnum %d, window [%d, %d), maxlag %d)", why, snum, tnum, s0, s1, maxlag);
    return IMPDAR_OK;
}

extern "C" int impdar_acorr_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int s0, int s1, int maxlag, int normalize,
                                double *d_out)
{
    const auto held = g_dc.lock();
    int rc = acorr_check(ctx, d_data, d_out, dtype, snum, tnum, s0, s1, maxlag);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_dc.bind(ctx);
    const DeconPlan P = acorr_plan(snum, tnum, s0, s1, maxlag);
    impdar_ctx_note(ctx, "impdar_acorr", P.label);
    if ((rc = impdar_ctx_tic(ctx))) return rc;
    if ((rc = dc_mark(ctx, 0))) return rc;
    if ((rc = dc_launch_acorr(ctx, P, d_data, dtype, tnum, s0, s1, d_out))) return rc;
    if (normalize) hipLaunchKernelGGL(decon_norm_kernel, dim3((unsigned)((tnum + 255) / 256)), dim3(256), 0, ctx->stream, d_out, P.nlags, tnum);
    IMPDAR_HIP_CHECK(hipGetLastError());
    if ((rc = dc_mark(ctx, 1))) return rc;
    if ((rc = impdar_ctx_toc(ctx))) return rc;
    if ((rc = dc_stage_times(ctx, 1))) return rc;
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer forms: the argument check, then StepScratch::host_form ----------------------------------

extern "C" int impdar_decon(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int s0, int s1, int oplen, int gap,
                            double prewhiten, int design, void *out, double *op)
{
    int rc = decon_check(ctx, data, out, dtype, snum, tnum, s0, s1, oplen, gap, prewhiten, design);
    if (rc) return rc;
    const auto held = g_dc.lock();
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype), opb = (size_t)oplen * tnum * sizeof(double);
    rc = g_dc.host_form(ctx, g_dc.in, data, bytes, &g_dc.out, out, bytes, [&](void *d_in, void *d_out) -> int {
        if (op) IMPDAR_HIP_CHECK(g_dc.opout.ensure(opb));
        return impdar_decon_dev(ctx, d_in, dtype, snum, tnum, s0, s1, oplen, gap, prewhiten, design, d_out, op ? g_dc.opout.as<double>() : nullptr);
    });
    if (rc || !op) return rc;
    IMPDAR_HIP_CHECK(hipMemcpy(op, g_dc.opout.p, opb, hipMemcpyDeviceToHost));
    return IMPDAR_OK;
}

extern "C" int impdar_acorr(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int s0, int s1, int maxlag, int normalize,
                            double *out)
{
    const int rc = acorr_check(ctx, data, out, dtype, snum, tnum, s0, s1, maxlag);
    if (rc) return rc;
    return g_dc.host_form(ctx, g_dc.in, data, (size_t)snum * tnum * impdar_dtype_size(dtype), &g_dc.out, out,
                          (size_t)(maxlag + 1) * tnum * sizeof(double), [&](void *d_in, void *d_out) {
                              return impdar_acorr_dev(ctx, d_in, dtype, snum, tnum, s0, s1, maxlag, normalize, (double *)d_out);
                          });
}
