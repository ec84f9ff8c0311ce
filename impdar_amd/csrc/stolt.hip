// Stolt f-k migration on gfx950: rocFFT transforms + hand-written taper /
// transpose / Stolt-stretch kernels.
//
// Behaviour restated from src/impdar/lib/migrationlib/mig_python.py:126-208:
//   :152-157  linear edge taper, product cast back to the data dtype
//   :159      FK = rfft2(data, axes=(1,0))  (real FFT over time, complex over traces)
//   :171-190  KK[zj,xi] = FK interpolated linearly along omega at
//             w' = (v/2) sqrt(kz^2+kx^2), clamped to the last knot; only rows
//             zj < snum//2 are written
//   :192-200  obliquity scaling kz/sqrt(kx^2+kz^2), KK[0,0] = 0
//   :202      irfft2(KK, axes=(1,0)) -> 2*(snum//2) rows
//
// Device layout is trace-major: X[tnum][snum] real, F[tnum][m] complex with
// m = snum/2+1, so the real transforms and the omega-interpolation run along
// the contiguous axis and the trace transform is a strided batched C2C.
//
// The kernels are in stolt_kernels.h; what a call decides on the host (knob, route, sizes, plan key, scan batches, metrics
// string) in stolt_route.h; the cached plan and the stages the f-k filter (fk.hip) shares in stolt_stages.h.
#include "fft.h"
#include "own_fft.h"
#include "stolt_kernels.h"
#include "stolt_route.h"
#include "stolt_stages.h"
#include <mutex>

std::mutex g_stolt_mu;
StoltPlan *g_stolt_plan = nullptr;            // last-used plan (sizes repeat across calls)

// called by impdar_ctx_destroy: a cached plan must not outlive the stream it was created on
// impdar_release_caches: out of device memory somewhere -- drop the cached plan unless a Stolt call is using it
thread_local bool t_stolt_busy = false;
void impdar_stolt_trim()
{
    if (t_stolt_busy) return;
    std::unique_lock<std::mutex> lk(g_stolt_mu, std::try_to_lock);
    if (lk.owns_lock() && g_stolt_plan) {
        delete g_stolt_plan;
        g_stolt_plan = nullptr;
    }
}

void impdar_stolt_forget(const impdar_ctx *ctx)
{
    std::lock_guard<std::mutex> lk(g_stolt_mu);
    if (g_stolt_plan && g_stolt_plan->key.owner == ctx) {
        delete g_stolt_plan;
        g_stolt_plan = nullptr;
    }
}

template <typename T> static int stolt_back(impdar_ctx *ctx, StoltPlan &pl, const StoltCall &c, double vel, void *d_out)
{
    const int snum = c.snum, tnum = c.tnum, m = c.m, nz = c.nz;
    hipStream_t st = ctx->stream;
    const double *dkx = pl.d_kx.as<double>(), *dws = pl.d_ws.as<double>();
    Cx<T> *F = pl.F.as<Cx<T>>(), *K = pl.K.as<Cx<T>>();
    int rc;
    if (c.route == STOLT_OWN_ROWS) {
        hipLaunchKernelGGL((stolt_stretch_rows<T>), dim3((nz + 1 + 255) / 256, c.hs), dim3(256), 0, st, K, F, dkx, dws, m, nz, snum, vel);
        if ((rc = stolt_inverse_rows<T>(pl, c, 1, F, K, (T *)d_out, st))) return rc;
    } else if (c.use_own) {      // K [w][kx] -> F [w][kx]
        hipLaunchKernelGGL((stolt_stretch_t<T>), dim3((tnum + 255) / 256, m), dim3(256), 0, st, K, F, dkx, dws, m, nz, tnum, vel);
        if ((rc = stolt_inverse_wkx<T>(pl, c, 1, F, K, (T *)d_out, st))) return rc;
    } else {
        hipLaunchKernelGGL((stolt_stretch<T>), dim3((m + 255) / 256, tnum), dim3(256), 0, st, F, K, dkx, dws, m, nz, tnum, vel);
        if ((rc = stolt_inverse_rocfft<T>(pl, c, (T *)d_out, st))) return rc;
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

template <typename T>
static int stolt_run(impdar_ctx *ctx, StoltPlan &pl, const void *d_data, int snum, int tnum, const double *kx,
                     const double *ws, double vel, double htaper, double vtaper, void *d_out)
{
    StoltCall c;
    int rc;
    if ((rc = stolt_prepare<T>(ctx, pl, snum, tnum, kx, ws, htaper, vtaper, c))) return rc;
    if ((rc = impdar_ctx_tic(ctx))) return rc;
    if ((rc = stolt_front<T>(ctx, pl, c, d_data))) return rc;
    if ((rc = stolt_back<T>(ctx, pl, c, vel, d_out))) return rc;
    impdar_trace(c.route == STOLT_OWN_ROWS ? "stolt: all kernels enqueued (traces first)" : "stolt: all kernels enqueued");
    ctx->m_entry = "impdar_stolt";
    ctx->m_kernel = stolt_kernel_label(c, false);
    ctx->m_kernel_ms = -1.f;
    ctx->ktimed = false;
    ctx->m_extra[0] = 0;
    return impdar_ctx_toc(ctx);
}

// The velocity scan: the front once, then the back half for nv velocities in batches of B, every image reduced to its rows' focus
// sums where it lies.  On the own transforms a batch is ONE stretch launch (grid z = velocity) and the inverse passes of a single
// call with B times the rows, on [B][rows][len] buffers (stolt_inverse_rows / _wkx).  On rocFFT the single call's back half runs
// once per velocity.
template <typename T>
static int stolt_scan_run(impdar_ctx *ctx, StoltPlan &pl, const void *d_data, int snum, int tnum, const double *kx, const double *ws,
                          const double *vels, int nv, double htaper, double vtaper, int t0, int t1, int max_batch, double *sums,
                          int keep, void *d_keep)
{
    StoltCall c;
    int rc;
    if ((rc = stolt_prepare<T>(ctx, pl, snum, tnum, kx, ws, htaper, vtaper, c))) return rc;
    const int m = c.m, nz = c.nz, nout = c.nout;
    hipStream_t st = ctx->stream;
    const StoltScanPlan sp = stolt_scan_plan(c, sizeof(T), nv, max_batch);
    const size_t plane = sp.plane, iplane = sp.iplane;
    const int B = sp.B;
    if (plane) {
        IMPDAR_HIP_CHECK(pl.S1.ensure((size_t)B * plane * 2 * sizeof(T)));
        IMPDAR_HIP_CHECK(pl.S2.ensure((size_t)B * plane * 2 * sizeof(T)));
    }
    IMPDAR_HIP_CHECK(pl.img.ensure(std::max((size_t)B * iplane, (size_t)1) * sizeof(T)));
    IMPDAR_HIP_CHECK(pl.d_vels.ensure((size_t)nv * 8));
    IMPDAR_HIP_CHECK(pl.d_sums.ensure(std::max((size_t)nv * nout * 3, (size_t)1) * 8));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_vels.p, vels, (size_t)nv * 8, hipMemcpyHostToDevice, st));
    if ((rc = impdar_ctx_tic(ctx))) return rc;
    if ((rc = stolt_front<T>(ctx, pl, c, d_data))) return rc;
    const double *dkx = pl.d_kx.as<double>(), *dws = pl.d_ws.as<double>();
    pl.scan_batches = 0;
    const size_t nev = 4 * (size_t)sp.batches;
    while (pl.scan_ev.size() < nev) {
        hipEvent_t e;
        IMPDAR_HIP_CHECK(hipEventCreate(&e));
        pl.scan_ev.push_back(e);
    }
    for (int b0 = 0; b0 < nv; b0 += B) {
        const int nb = std::min(B, nv - b0);
        hipEvent_t *ev = pl.scan_ev.data() + 4 * (size_t)(b0 / B);
        IMPDAR_HIP_CHECK(hipEventRecord(ev[0], st));
        const double *dv = pl.d_vels.as<double>() + b0;
        Cx<T> *S1 = pl.S1.as<Cx<T>>(), *S2 = pl.S2.as<Cx<T>>();
        T *img = pl.img.as<T>();
        if (!c.use_own) {
            IMPDAR_HIP_CHECK(hipEventRecord(ev[1], st));          // (the stretch is not timed apart from rocFFT's passes)
            for (int b = 0; b < nb; ++b)
                if ((rc = stolt_back<T>(ctx, pl, c, vels[b0 + b], img + (size_t)b * iplane))) return rc;
        } else if (c.route == STOLT_OWN_ROWS) {
            hipLaunchKernelGGL((stolt_stretch_scan_rows<T>), dim3((nz + 1 + 255) / 256, c.hs, nb), dim3(256), 0, st, pl.K.as<Cx<T>>(), S1, dkx,
                               dws, dv, m, nz, snum, plane);
            IMPDAR_HIP_CHECK(hipEventRecord(ev[1], st));
            if ((rc = stolt_inverse_rows<T>(pl, c, nb, S1, S2, img, st))) return rc;
        } else {
            hipLaunchKernelGGL((stolt_stretch_scan_t<T>), dim3((tnum + 255) / 256, m, nb), dim3(256), 0, st, pl.K.as<Cx<T>>(), S1, dkx, dws,
                               dv, m, nz, tnum, plane);
            IMPDAR_HIP_CHECK(hipEventRecord(ev[1], st));
            if ((rc = stolt_inverse_wkx<T>(pl, c, nb, S1, S2, img, st))) return rc;
        }
        IMPDAR_HIP_CHECK(hipEventRecord(ev[2], st));
        if (nout > 0)
            hipLaunchKernelGGL((stolt_focus_rows<T>), dim3(nout, nb), dim3(256), 0, st, img, pl.d_sums.as<double>() + (size_t)b0 * nout * 3,
                               nout, tnum, t0, t1);
        IMPDAR_HIP_CHECK(hipGetLastError());
        IMPDAR_HIP_CHECK(hipEventRecord(ev[3], st));
        ++pl.scan_batches;
        if (keep >= b0 && keep < b0 + nb && iplane)
            IMPDAR_HIP_CHECK(hipMemcpyAsync(d_keep, img + (size_t)(keep - b0) * iplane, iplane * sizeof(T), hipMemcpyDeviceToDevice, st));
    }
    impdar_trace("stolt scan: all kernels enqueued (%d velocities, batches of %d)", nv, B);
    ctx->m_entry = "impdar_stolt_scan";
    ctx->m_kernel = stolt_kernel_label(c, true);
    ctx->m_kernel_ms = -1.f;
    ctx->ktimed = false;
    snprintf(ctx->m_extra, sizeof ctx->m_extra, "\"B\": %d, \"nv\": %d", B, nv);
    if ((rc = impdar_ctx_toc(ctx))) return rc;
    IMPDAR_HIP_CHECK(hipMemcpyAsync(sums, pl.d_sums.p, (size_t)nv * nout * 3 * 8, hipMemcpyDeviceToHost, st));
    return IMPDAR_OK;
}

extern "C" int impdar_stolt_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const double *kx,
                                const double *ws, double vel, double htaper, double vtaper, void *d_out)
{
    IMPDAR_ARG_CHECK(ctx && d_data && d_out && kx && ws, "null argument");
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    IMPDAR_ARG_CHECK(snum >= 2 && tnum >= 1, "need snum >= 2 and tnum >= 1 (got %d, %d)", snum, tnum);
    IMPDAR_ARG_CHECK(vel > 0, "vel must be positive");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(g_stolt_mu);
    ImpdarBusy busy(t_stolt_busy);
    if (!g_stolt_plan) g_stolt_plan = new StoltPlan();
    auto run = dtype == IMPDAR_F32 ? stolt_run<float> : stolt_run<double>;
    int rc = run(ctx, *g_stolt_plan, d_data, snum, tnum, kx, ws, vel, htaper, vtaper, d_out);
    if (rc) return rc;
    // kx/ws were staged from caller memory: complete before returning
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    impdar_trace("stolt: device work complete");
    return impdar_ctx_mark_produced(ctx);
}

// The upload of a host entry point (`entry`) into the first of its call's two arrays.
static int stolt_upload(const char *entry, impdar_ctx *ctx, const CallArrays &a, const void *data, size_t inb)
{
    if (hipMemcpyAsync(a.din, data, inb, hipMemcpyHostToDevice, ctx->stream) == hipSuccess) return IMPDAR_OK;
    impdar_set_error("%s: upload failed: %s", entry, hipGetErrorString(hipGetLastError()));
    return IMPDAR_ERR_HIP;
}

extern "C" int impdar_stolt(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *kx,
                            const double *ws, double vel, double htaper, double vtaper, void *out)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "null argument");
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    IMPDAR_ARG_CHECK(snum >= 2 && tnum >= 1, "need snum >= 2 and tnum >= 1 (got %d, %d)", snum, tnum);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t esz = impdar_dtype_size(dtype);
    const size_t inb = (size_t)snum * tnum * esz, outb = (size_t)(2 * (snum / 2)) * tnum * esz;
    impdar_trace("impdar_stolt: enter (%d x %d)", snum, tnum);
    impdar_ctx_pinned_prefetch(ctx, std::min(outb, IMPDAR_STAGE_RING_BYTES));       // the download's staging ring, pinned while the call works
    CallArrays a{ctx};
    int rc = a.alloc(inb, outb ? outb : 8);
    if (rc == IMPDAR_OK) rc = stolt_upload("impdar_stolt", ctx, a, data, inb);
    impdar_trace("impdar_stolt: upload enqueued");
    if (rc == IMPDAR_OK) rc = impdar_stolt_dev(ctx, a.din, dtype, snum, tnum, kx, ws, vel, htaper, vtaper, a.dout);
    if (rc == IMPDAR_OK) rc = impdar_download(ctx, out, a.dout, outb, ctx->stream);
    impdar_trace("impdar_stolt: downloaded");
    return rc;
}

static int stolt_scan_args(int dtype, int snum, int tnum, const double *vels, int nv, int t0, int t1, int max_batch, int keep)
{
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    IMPDAR_ARG_CHECK(snum >= 2 && tnum >= 1, "need snum >= 2 and tnum >= 1 (got %d, %d)", snum, tnum);
    IMPDAR_ARG_CHECK(nv >= 1, "need at least one velocity (got %d)", nv);
    for (int b = 0; b < nv; ++b)
        IMPDAR_ARG_CHECK(vels[b] > 0 && vels[b] <= 1.7976931348623157e308, "vels[%d] must be positive and finite", b);
    IMPDAR_ARG_CHECK(0 <= t0 && t0 < t1 && t1 <= tnum, "the trace window must satisfy 0 <= t0 < t1 <= tnum (got %d, %d)", t0, t1);
    IMPDAR_ARG_CHECK(max_batch >= 0, "max_batch must be 0 (auto) or positive");
    IMPDAR_ARG_CHECK(keep >= -1 && keep < nv, "keep must be -1 or the index of a velocity (got %d of %d)", keep, nv);
    return IMPDAR_OK;
}

extern "C" int impdar_stolt_scan_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const double *kx,
                                     const double *ws, const double *vels, int nv, double htaper, double vtaper, int t0, int t1,
                                     int max_batch, double *sums, int keep, void *d_keep)
{
    IMPDAR_ARG_CHECK(ctx && d_data && kx && ws && vels && sums, "null argument");
    int rc = stolt_scan_args(dtype, snum, tnum, vels, nv, t0, t1, max_batch, keep);
    if (rc) return rc;
    IMPDAR_ARG_CHECK(keep < 0 || d_keep, "keep >= 0 needs an array for the image");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(g_stolt_mu);
    ImpdarBusy busy(t_stolt_busy);
    if (!g_stolt_plan) g_stolt_plan = new StoltPlan();
    auto run = dtype == IMPDAR_F32 ? stolt_scan_run<float> : stolt_scan_run<double>;
    rc = run(ctx, *g_stolt_plan, d_data, snum, tnum, kx, ws, vels, nv, htaper, vtaper, t0, t1, max_batch, sums, keep, d_keep);
    if (rc) return rc;
    // kx / ws / vels were staged from caller memory and the sums are on their way to it: complete before returning
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    {
        // the stages' device times, summed over the batches, after "B" and "nv" in the metrics line
        float stage[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < g_stolt_plan->scan_batches; ++i)
            for (int k = 0; k < 3; ++k) {
                float ms = 0.f;
                IMPDAR_HIP_CHECK(hipEventElapsedTime(&ms, g_stolt_plan->scan_ev[4 * i + k], g_stolt_plan->scan_ev[4 * i + k + 1]));
                stage[k] += ms;
            }
        const size_t used = strlen(ctx->m_extra);
        snprintf(ctx->m_extra + used, sizeof ctx->m_extra - used, ", \"stretch_ms\": %.4f, \"inverse_ms\": %.4f, \"focus_ms\": %.4f", stage[0],
                 stage[1], stage[2]);
    }
    impdar_trace("stolt scan: device work complete");
    return keep >= 0 ? impdar_ctx_mark_produced(ctx) : IMPDAR_OK;
}

extern "C" int impdar_stolt_scan(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *kx,
                                 const double *ws, const double *vels, int nv, double htaper, double vtaper, int t0, int t1,
                                 int max_batch, double *sums, int keep, void *keep_out)
{
    IMPDAR_ARG_CHECK(ctx && data && kx && ws && vels && sums, "null argument");
    int rc = stolt_scan_args(dtype, snum, tnum, vels, nv, t0, t1, max_batch, keep);
    if (rc) return rc;
    IMPDAR_ARG_CHECK(keep < 0 || keep_out, "keep >= 0 needs an array for the image");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t esz = impdar_dtype_size(dtype);
    const size_t inb = (size_t)snum * tnum * esz, outb = (size_t)(2 * (snum / 2)) * tnum * esz;
    // one upload for all velocities; nothing comes back but the sums unless an image is asked for
    CallArrays a{ctx};
    rc = a.alloc(inb, keep >= 0 ? (outb ? outb : 8) : 0);
    if (rc == IMPDAR_OK) rc = stolt_upload("impdar_stolt_scan", ctx, a, data, inb);
    if (rc == IMPDAR_OK)
        rc = impdar_stolt_scan_dev(ctx, a.din, dtype, snum, tnum, kx, ws, vels, nv, htaper, vtaper, t0, t1, max_batch, sums, keep, a.dout);
    if (rc == IMPDAR_OK && keep >= 0) rc = impdar_download(ctx, keep_out, a.dout, outb, ctx->stream);
    return rc;
}
