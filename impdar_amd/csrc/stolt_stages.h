// The cached plan of the Stolt path and the stages of a call on it, shared by the units that run them: stolt.hip (migration,
// velocity scan) and fk.hip (fan filter, f-k spectrum).  One plan per process, behind one mutex: a chain fk -> stolt at one size
// plans once.
#pragma once
#include "fft.h"
#include "own_fft.h"
#include "stolt_kernels.h"
#include "stolt_route.h"
#include <mutex>

struct StoltPlan {
    // power-of-two sizes run on the library's own row transforms (own_fft.h) and need no rocFFT plan
    OwnTwiddles tw_time, tw_trace;
    // what the plans and buffers were made for; they live on the device and stream of key.owner (an impdar_ctx)
    StoltPlanKey key;
    FftPlan r2c, c2c_f, c2c_b, c2r;     // separate passes (IMPDAR_STOLT_FFT=1d)
    FftPlan fwd2d, inv2d;               // the same two pairs as 2-D real transforms (default)
    DevBuf X, F, K, Y, d_kx, d_ws;      // (Y: the rocFFT routes alone)
    DevBuf d_taper;                     // [tnum + snum] float64 taper weights (the transform over the traces taken first)
    std::vector<double> h_taper;        // ... on the host (alive until the next call: async copy), and what they were made from
    double taper_h = -1.0, taper_v = -1.0;
    // the velocity scan (impdar_stolt_scan): the spectra of one batch of velocities, twice (a transpose is out of place), their
    // images, the velocities and the focus sums; they go with the plan (impdar_stolt_trim / _forget delete it)
    DevBuf S1, S2, img, d_vels, d_sums;
    // four events per batch of the last scan (before the stretch, after it, after the inverse passes, after the reduction): the
    // stage times of the metrics line
    std::vector<hipEvent_t> scan_ev;
    int scan_batches = 0;
    // the fan filter at odd snum (fk.hip): a 2-D real inverse of snum rows beside inv2d's 2 (snum / 2), and the key it was made under
    FftPlan fk_inv;
    StoltPlanKey fk_inv_key;
    // how often this plan's key changed (plans and buffers made anew): the f-k entries put it into their metrics line
    int builds = 0;
    void release_scan()
    {
        S1.release(); S2.release(); img.release(); d_vels.release(); d_sums.release();
        for (hipEvent_t e : scan_ev) (void)hipEventDestroy(e);
        scan_ev.clear();
        scan_batches = 0;
    }
    ~StoltPlan() { release_scan(); }
};

// defined in stolt.hip
extern std::mutex g_stolt_mu;
extern StoltPlan *g_stolt_plan;             // last-used plan (sizes repeat across calls)
extern thread_local bool t_stolt_busy;

// The shape of a call and its taper.
struct StoltCall : StoltShape {
    int do_taper;
    double htaper, vtaper;
};

// A call in three stages, shared by the single migration (stolt_run), the velocity scan (stolt_scan_run) and the f-k entries:
//   stolt_prepare  plans, buffers and twiddles for the size; kx and ws to the device
//   stolt_front    everything that does not depend on the velocity: taper, forward transforms; the spectrum is left in
//                  pl.K (own transforms: [kx >= 0][w] on the rows route, [w][kx] on the other) or pl.F (rocFFT: [kx][w])
//   stolt_back     (stolt.hip) stretch at one velocity, inverse transforms, the image into d_out (pl.F and pl.K are overwritten on the own routes)
template <typename T>
static int stolt_prepare(impdar_ctx *ctx, StoltPlan &pl, int snum, int tnum, const double *kx, const double *ws, double htaper,
                         double vtaper, StoltCall &c)
{
    hipStream_t st = ctx->stream;
    const bool dbl = sizeof(T) == 8;
    const StoltKnobs knobs = StoltKnobs::from_env();
    static_cast<StoltShape &>(c) = stolt_shape(dbl ? IMPDAR_F64 : IMPDAR_F32, snum, tnum, stolt_route(snum, tnum, kx, knobs));
    const int m = c.m, nout = c.nout;
    const StoltPlanKey key{ctx, c.dtype, snum, tnum, knobs.use2d, knobs.no_own, c.route};
    if (!(pl.key == key)) {
        pl.key.dtype = -1;                   // (no plan of any call until this one's are made)
        ++pl.builds;
        pl.h_taper.clear();
        if (pl.key.owner != ctx) {           // another device / stream: drop everything bound to the old one
            pl.X.release(); pl.F.release(); pl.K.release(); pl.Y.release(); pl.d_kx.release(); pl.d_ws.release(); pl.d_taper.release();
            pl.release_scan();
            pl.key.owner = ctx;
        }
        int rc;
        // rfft2(axes=(1,0)) (:159) = real transform over time (contiguous here), complex over the traces (rows);
        // irfft2 (:202) = complex inverse over the traces, then C2R over time.  rocFFT's 2-D real plans do
        // exactly these two passes each, with its own blocked column kernels instead of a strided batch.
        if (key.use2d && !c.use_own) {
            // (asking rocFFT for the spectrum frequency-major -- its layout before the plan's last transpose -- removes two
            // transposes but makes it pick slower kernels: 0.76 ms against 0.37 ms at 4096 x 4096 float32, round 2)
            if ((rc = impdar_parallel_plans(ctx->device, {
                     [&] { return pl.fwd2d.create2d(rocfft_transform_type_real_forward, dbl, false, snum, tnum, rocfft_array_type_real,
                                                    rocfft_array_type_hermitian_interleaved, snum, m, 1.0, st); },
                     [&] { return pl.inv2d.create2d(rocfft_transform_type_real_inverse, dbl, false, nout, tnum,
                                                    rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, m, nout,
                                                    1.0 / ((double)nout * tnum), st); }})))
                return rc;
        }
        if (!key.use2d) {
            // (round 3 built these four beside the 2-D pair on every new size: four run-time compilations nobody ran)
            if ((rc = pl.r2c.create(rocfft_transform_type_real_forward, dbl, false, snum, tnum, rocfft_array_type_real,
                                    rocfft_array_type_hermitian_interleaved, 1, snum, 1, m, 1.0, st)))
                return rc;
            if ((rc = pl.c2c_f.create(rocfft_transform_type_complex_forward, dbl, true, tnum, m,
                                      rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, m, 1,
                                      m, 1, 1.0, st)))
                return rc;
            if ((rc = pl.c2c_b.create(rocfft_transform_type_complex_inverse, dbl, true, tnum, m,
                                      rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, m, 1,
                                      m, 1, 1.0 / tnum, st)))
                return rc;
            if ((rc = pl.c2r.create(rocfft_transform_type_real_inverse, dbl, false, nout, tnum,
                                    rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, 1, m, 1, nout,
                                    1.0 / nout, st)))
                return rc;
        }
        IMPDAR_HIP_CHECK(pl.X.ensure(c.x_elems * sizeof(T)));
        IMPDAR_HIP_CHECK(pl.F.ensure(c.spec_elems * 2 * sizeof(T)));
        IMPDAR_HIP_CHECK(pl.K.ensure(c.spec_elems * 2 * sizeof(T)));
        // (the own routes write the real images over the spent spectrum: stolt_inverse_wkx)
        if (!c.use_own) IMPDAR_HIP_CHECK(pl.Y.ensure(c.y_elems * sizeof(T)));
        IMPDAR_HIP_CHECK(pl.d_kx.ensure((size_t)tnum * 8));
        IMPDAR_HIP_CHECK(pl.d_ws.ensure((size_t)m * 8));
        impdar_trace("stolt: plans and buffers ready");
        pl.key = key;
    }
    if (c.use_own) {
        impdar_trace("stolt: transforms on the library's own row kernels");
        int rc;
        if ((rc = pl.tw_time.ensure<T>(snum, st)) || (rc = pl.tw_trace.ensure<T>(tnum, st))) return rc;
    }
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_kx.p, kx, (size_t)tnum * 8, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_ws.p, ws, (size_t)m * 8, hipMemcpyHostToDevice, st));
    c.do_taper = !(htaper != htaper);             // NaN = caller already tapered (integer dtypes)
    c.htaper = htaper;
    c.vtaper = vtaper;
    return IMPDAR_OK;
}

template <typename T> static int stolt_front(impdar_ctx *ctx, StoltPlan &pl, const StoltCall &c, const void *d_data)
{
    const int snum = c.snum, tnum = c.tnum, m = c.m, do_taper = c.do_taper;
    const double htaper = c.htaper, vtaper = c.vtaper;
    const bool use_own = c.use_own;
    hipStream_t st = ctx->stream;
    // Round 6, power-of-two sizes: the transform over the TRACES first, on the radargram's own rows with the taper applied on load,
    // wavenumbers k = 0 .. tnum/2 only -- R2C over x -> [snum][hs]; transpose -> [hs][snum]; C2C over time; the stretch along the rows
    // (both signs of the frequency: stolt_stretch_rows); C2C back over time; transpose -> [snum][hs]; C2R over x straight into the
    // output: seven passes instead of ten (no transposes of the real arrays at either end, two half-size transposes instead of two
    // whole ones)
    const bool use_rows = c.route == STOLT_OWN_ROWS;
    if (use_rows && do_taper && !(pl.h_taper.size() == (size_t)tnum + snum && pl.taper_h == htaper && pl.taper_v == vtaper && pl.d_taper.p)) {
        std::vector<double> &taps = pl.h_taper;
        taps.resize((size_t)tnum + snum);
        for (int j = 0; j < tnum; ++j) taps[j] = impdar_taper_w(j, tnum, htaper);
        for (int i = 0; i < snum; ++i) taps[(size_t)tnum + i] = impdar_taper_w(i, snum, vtaper);
        IMPDAR_HIP_CHECK(pl.d_taper.ensure(taps.size() * 8));
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_taper.p, taps.data(), taps.size() * 8, hipMemcpyHostToDevice, st));
        pl.taper_h = htaper;
        pl.taper_v = vtaper;
    }
    int rc;
    if (use_rows) {
        const int hs = c.hs;
        const double *th = do_taper ? pl.d_taper.as<double>() : nullptr, *tv = do_taper ? th + tnum : nullptr;
        if ((rc = own_fft_launch<T>(OWN_R2C, tnum, (size_t)snum, d_data, pl.F.p, (size_t)tnum, (size_t)hs, 1.0, pl.tw_trace, st, th, tv, 1))) return rc;
        own_launch_transpose<T>(pl.F.p, pl.K.p, snum, hs, st);
        if ((rc = own_fft_launch<T>(OWN_C2C_FWD, snum, (size_t)hs, pl.K.p, pl.K.p, (size_t)snum, (size_t)snum, 1.0, pl.tw_time, st))) return rc;
        return IMPDAR_OK;
    }
    dim3 tgrid((tnum + 63) / 64, (snum + 63) / 64);
    hipLaunchKernelGGL((stolt_taper_transpose<T>), tgrid, dim3(256), 0, st, (const T *)d_data, pl.X.as<T>(), snum, tnum,
                       htaper, vtaper, do_taper);
    if (use_own) {
        // the four 1-D passes of the "1d" form on the library's own row kernels: real-to-complex over time (rows of X), over
        // the traces on contiguous rows of the transposed spectrum (K is free until the stretch writes it)
        if ((rc = own_fft_launch<T>(OWN_R2C, snum, (size_t)tnum, pl.X.p, pl.F.p, (size_t)snum, (size_t)m, 1.0, pl.tw_time, st))) return rc;
        own_launch_transpose<T>(pl.F.p, pl.K.p, tnum, m, st);
        if ((rc = own_fft_launch<T>(OWN_C2C_FWD, tnum, (size_t)m, pl.K.p, pl.K.p, (size_t)tnum, (size_t)tnum, 1.0, pl.tw_trace, st))) return rc;
    } else if (pl.key.use2d) {
        if ((rc = pl.fwd2d.exec(pl.X.p, pl.F.p))) return rc;
    } else {
        if ((rc = pl.r2c.exec(pl.X.p, pl.F.p))) return rc;
        if ((rc = pl.c2c_f.exec(pl.F.p, nullptr))) return rc;
    }
    return IMPDAR_OK;
}

// The inverse passes of the own routes behind the stretch, for nb velocities at once: A holds the nb stretched spectra, plane after
// plane, S takes their transposes, the images go to out [nb][nout][tnum].  They are the passes of one velocity with nb times the
// rows (a workgroup per row, the kernel chosen by the length alone: the same bits as nb calls with nb = 1); the transposes run
// plane by plane.
//   rows: A [nb][hs][snum] -- C2C back over time; transpose -> S [nb][snum][hs]; C2R over x straight into out
template <typename T>
static int stolt_inverse_rows(StoltPlan &pl, const StoltCall &c, int nb, Cx<T> *A, Cx<T> *S, T *out, hipStream_t st)
{
    const int snum = c.snum, tnum = c.tnum, hs = c.hs;
    const size_t plane = (size_t)hs * snum;
    int rc;
    if ((rc = own_fft_launch<T>(OWN_C2C_INV, snum, (size_t)nb * hs, A, A, (size_t)snum, (size_t)snum, 1.0 / snum, pl.tw_time, st))) return rc;
    for (int b = 0; b < nb; ++b) own_launch_transpose<T>(A + (size_t)b * plane, S + (size_t)b * plane, hs, snum, st);
    return own_fft_launch<T>(OWN_C2R, tnum, (size_t)nb * snum, S, out, (size_t)hs, (size_t)tnum, 1.0 / tnum, pl.tw_trace, st);
}
//   [w][kx]: A [nb][m][tnum] -- C2C back over the traces; transpose -> S [nb][tnum][m]; C2R over time; transpose of the reals into out
template <typename T>
static int stolt_inverse_wkx(StoltPlan &pl, const StoltCall &c, int nb, Cx<T> *A, Cx<T> *S, T *out, hipStream_t st)
{
    const int tnum = c.tnum, m = c.m, nout = c.nout;
    const size_t plane = (size_t)m * tnum, iplane = (size_t)nout * tnum;
    int rc;
    if ((rc = own_fft_launch<T>(OWN_C2C_INV, tnum, (size_t)nb * m, A, A, (size_t)tnum, (size_t)tnum, 1.0 / tnum, pl.tw_trace, st))) return rc;
    for (int b = 0; b < nb; ++b) own_launch_transpose<T>(A + (size_t)b * plane, S + (size_t)b * plane, m, tnum, st);
    // ([nb][tnum][m] is nb * tnum rows of m)
    hipLaunchKernelGGL((stolt_fix_hermitian<T>), dim3((nb * tnum + 255) / 256), dim3(256), 0, st, S, m, nb * tnum);
    // the real images before their transposes go where the spectra were: nout <= 2 m - 2 reals per row of m complex
    T *Yt = reinterpret_cast<T *>(A);
    if ((rc = own_fft_launch<T>(OWN_C2R, nout, (size_t)nb * tnum, S, Yt, (size_t)m, (size_t)nout, 1.0 / nout, pl.tw_time, st))) return rc;
    dim3 bgrid((tnum + 63) / 64, (nout + 63) / 64);
    for (int b = 0; b < nb; ++b)
        hipLaunchKernelGGL((stolt_transpose_back<T>), bgrid, dim3(256), 0, st, Yt + (size_t)b * iplane, out + (size_t)b * iplane, nout, tnum);
    return IMPDAR_OK;
}
//   rocFFT: pl.K [kx][w] -- the 2-D real inverse (or its two passes, "1d") into pl.Y [tnum][nout]; transpose of the reals into out
template <typename T> static int stolt_inverse_rocfft(StoltPlan &pl, const StoltCall &c, T *out, hipStream_t st)
{
    const int tnum = c.tnum, m = c.m, nout = c.nout;
    int rc;
    if (pl.key.use2d) {
        if ((rc = pl.inv2d.exec(pl.K.p, pl.Y.p))) return rc;
    } else {
        if ((rc = pl.c2c_b.exec(pl.K.p, nullptr))) return rc;
        hipLaunchKernelGGL((stolt_fix_hermitian<T>), dim3((tnum + 255) / 256), dim3(256), 0, st, pl.K.as<Cx<T>>(), m, tnum);
        if ((rc = pl.c2r.exec(pl.K.p, pl.Y.p))) return rc;
    }
    dim3 bgrid((tnum + 63) / 64, (nout + 63) / 64);
    hipLaunchKernelGGL((stolt_transpose_back<T>), bgrid, dim3(256), 0, st, pl.Y.as<T>(), out, nout, tnum);
    return IMPDAR_OK;
}
