// The horizontal frequency filters (reference src/impdar/lib/RadarData/_RadarDataFiltering.py:138-350:
// horizontal_band_pass, highpass, lowpass): scipy.signal.filtfilt(b, a, data, axis=1) of a Butterworth design,
// along the trace axis, float64 out.  Odd extension by padlen = 3 * ncoef samples in the data's own arithmetic,
// steady-state initial conditions zi * x0, forward pass, backward pass from zi * y0, rows [padlen, padlen + tnum).
//
// The recurrence runs along the axis that is contiguous in memory and every step depends on the one before, so
// each row is one serial chain of 2 * tnum + 3 * padlen steps (the backward pass stops at the first kept sample)
// in SciPy's own operation order (_lfilter.c.in, compiled with -ffp-contract=off):
//   y = z[0] + b[0]*x;  z[n] = z[n+1] + x*b[n+1] - y*a[n+1];  z[last] = x*b[last] - y*a[last].
// A transfer-function filter with low corners goes through large transient growth of its state, so neither a
// chunked evaluation with carried state nor second-order sections reproduce filtfilt(b, a): the
// parallelism comes from the rows only.  The delays of one row are spread over the lanes of the row's group and
// neighbours are fetched with DPP moves before anything is updated (FiltLane of filtfilt_core.h, the recurrence
// this file shares with the vertical band pass); a wavefront walks 64 / G rows side by side.  G = 4 lanes (one
// quad) when the filter has at most 4 delays, else 8 (two DPP hops for the broadcast of z[0], but half the
// delays per lane): measured in DESIGN.md 4.7.
//
// Memory side: the samples of a row are contiguous, so the wavefront reads a (rows x HP_CH) tile with plain
// element loads, 64 consecutive elements per instruction (two or more full row segments), and stages it
// through LDS; the loads of the next tile are in flight while the current one is filtered.  A step reads its
// sample from LDS (all lanes of a row read the same address: a broadcast).  The outputs stay in registers,
// packed as lane q holding step G * k + q, and are stored at the top of the next chunk, in front of the
// next prefetch, so a whole chunk of filtering separates every store and load from the wait that retires it.
#include "filtfilt_core.h"

#define HP_MAX_COEF 17   // 16 delays: K = 2 per lane at 8 lanes per row
#define HP_CH 32         // samples per chunk

// HP_CH steps on the samples of an LDS tile row (read forward or backward); lane q keeps step G*k + q in held[k]
template <int G, int K, bool REV>
__device__ __forceinline__ void hp_chunk_steps(FiltLane<G, K> &f, const double *tr, double (&held)[HP_CH / G], int q)
{
#pragma unroll
    for (int s = 0; s < HP_CH; ++s) {
        const double y = f.step(tr[REV ? HP_CH - 1 - s : s]);
        held[s / G] = q == s % G ? y : held[s / G];
    }
}

template <int G> struct HpTile {
    static constexpr int RPW = 64 / G;             // rows per wavefront
    static constexpr int LD = HP_CH + 1;           // LDS row stride in doubles: rows fall on distinct banks
    static constexpr int NE = RPW * HP_CH / 64;    // tile elements each lane loads
};

// forward pass over the extended rows; Y is (snum, tnum + 2*pad) fp64
template <typename T, int G, int K>
__global__ __launch_bounds__(64) void hp_forward_kernel(const T *__restrict__ x, double *__restrict__ Y, int snum,
                                                        int tnum, int pad, int nc, FiltCoefs<HP_MAX_COEF> c)
{
    using P = HpTile<G>;
    __shared__ double tile[2][P::RPW * P::LD];
    const int lane = threadIdx.x, g = lane / G, q = lane % G;
    const int row0 = blockIdx.x * P::RPW;
    const int L = tnum + 2 * pad;
    const size_t ldy = (size_t)L;
    // loading: element e of this lane is column (e*64 + lane) % HP_CH of tile row (e*64 + lane) / HP_CH
    const T *src[P::NE];
#pragma unroll
    for (int e = 0; e < P::NE; ++e) {
        const int r = row0 + (e * 64 + lane) / HP_CH;
        src[e] = x + (size_t)(r < snum ? r : snum - 1) * tnum;
    }
    const int lcol = lane % HP_CH;
    T nx[P::NE];
#pragma unroll
    for (int e = 0; e < P::NE; ++e) nx[e] = filt_odd_ext(src[e], lcol, tnum, pad, 1);
#pragma unroll
    for (int e = 0; e < P::NE; ++e) tile[0][((e * 64 + lane) / HP_CH) * P::LD + lcol] = (double)nx[e];
    __syncthreads();
    const int row = row0 + g;
    const bool live = row < snum;
    double *yr = Y + (size_t)(live ? row : 0) * ldy;
    FiltLane<G, K> f;
    f.init(c, q, nc, tile[0][g * P::LD]);
    double held[HP_CH / G];
#pragma unroll
    for (int k = 0; k < HP_CH / G; ++k) held[k] = 0.0;
    int buf = 0;
    for (int i0 = 0; i0 < L; i0 += HP_CH, buf ^= 1) {
        if (i0 > 0 && live) {
#pragma unroll
            for (int k = 0; k < HP_CH / G; ++k) {
                const int i = i0 - HP_CH + G * k + q;
                if (i < L) yr[i] = held[k];
            }
        }
        const int n0 = i0 + HP_CH;   // first sample of the next chunk (uniform)
        if (n0 < L) {
            if (n0 >= pad && n0 + HP_CH <= pad + tnum) {
#pragma unroll
                for (int e = 0; e < P::NE; ++e) nx[e] = src[e][n0 - pad + lcol];
            } else {
#pragma unroll
                for (int e = 0; e < P::NE; ++e) nx[e] = filt_odd_ext(src[e], n0 + lcol, tnum, pad, 1);
            }
        }
        hp_chunk_steps<G, K, false>(f, &tile[buf][g * P::LD], held, q);
        if (n0 < L) {
#pragma unroll
            for (int e = 0; e < P::NE; ++e) tile[buf ^ 1][((e * 64 + lane) / HP_CH) * P::LD + lcol] = (double)nx[e];
        }
        __syncthreads();
    }
    if (live) {
        const int i0 = (L - 1) / HP_CH * HP_CH;   // the last chunk
#pragma unroll
        for (int k = 0; k < HP_CH / G; ++k) {
            const int i = i0 + G * k + q;
            if (i < L) yr[i] = held[k];
        }
    }
}

// backward pass: filters each extended row of Y from its end down to position pad and writes positions
// [pad, pad + tnum) to `out` (snum x tnum float64; may be the input of the forward pass)
template <int G, int K>
__global__ __launch_bounds__(64) void hp_backward_kernel(const double *__restrict__ Y, double *__restrict__ out,
                                                         int snum, int tnum, int pad, int nc, FiltCoefs<HP_MAX_COEF> c)
{
    using P = HpTile<G>;
    __shared__ double tile[2][P::RPW * P::LD];
    const int lane = threadIdx.x, g = lane / G, q = lane % G;
    const int row0 = blockIdx.x * P::RPW;
    const int L = tnum + 2 * pad;
    const double *src[P::NE];
#pragma unroll
    for (int e = 0; e < P::NE; ++e) {
        const int r = row0 + (e * 64 + lane) / HP_CH;
        src[e] = Y + (size_t)(r < snum ? r : snum - 1) * L;
    }
    const int lcol = lane % HP_CH;
    // tile column j holds position P0 - (HP_CH - 1) + j of the chunk that starts (backwards) at P0
    double nx[P::NE];
    int p = L - 1 - (HP_CH - 1) + lcol;
#pragma unroll
    for (int e = 0; e < P::NE; ++e) nx[e] = src[e][p > 0 ? p : 0];
#pragma unroll
    for (int e = 0; e < P::NE; ++e) tile[0][((e * 64 + lane) / HP_CH) * P::LD + lcol] = nx[e];
    __syncthreads();
    const int row = row0 + g;
    const bool live = row < snum;
    double *orow = out + (size_t)(live ? row : 0) * tnum;
    FiltLane<G, K> f;
    f.init(c, q, nc, tile[0][g * P::LD + HP_CH - 1]);
    double held[HP_CH / G];
#pragma unroll
    for (int k = 0; k < HP_CH / G; ++k) held[k] = 0.0;
    int buf = 0, held_p = -1;
    for (int P0 = L - 1; P0 >= pad; P0 -= HP_CH, buf ^= 1) {
        if (held_p >= 0 && live) {
#pragma unroll
            for (int k = 0; k < HP_CH / G; ++k) {
                const int j = held_p - (G * k + q) - pad;
                if (j >= 0 && j < tnum) orow[j] = held[k];
            }
        }
        const int n0 = P0 - HP_CH;   // first (highest) position of the next chunk (uniform)
        if (n0 >= pad) {
            p = n0 - (HP_CH - 1) + lcol;
#pragma unroll
            for (int e = 0; e < P::NE; ++e) nx[e] = src[e][p > 0 ? p : 0];
        }
        hp_chunk_steps<G, K, true>(f, &tile[buf][g * P::LD], held, q);
        held_p = P0;
        if (n0 >= pad) {
#pragma unroll
            for (int e = 0; e < P::NE; ++e) tile[buf ^ 1][((e * 64 + lane) / HP_CH) * P::LD + lcol] = nx[e];
        }
        __syncthreads();
    }
    if (live && held_p >= 0) {
#pragma unroll
        for (int k = 0; k < HP_CH / G; ++k) {
            const int j = held_p - (G * k + q) - pad;
            if (j >= 0 && j < tnum) orow[j] = held[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct HpassBufs {
    DevBuf y, in, out;   // the fp64 forward pass (reused across calls); staging of the host-buffer form
    void release()
    {
        y.release();
        in.release();
        out.release();
    }
};
static StepScratch<HpassBufs> g_hp;

void impdar_hpass_forget(impdar_ctx *ctx) { g_hp.forget(ctx); }

template <typename T, int G, int K>
static void hp_launch(impdar_ctx *ctx, const T *x, double *Y, double *out, int snum, int tnum, int pad, int nc,
                      const FiltCoefs<HP_MAX_COEF> &c)
{
    const int nb = (snum + HpTile<G>::RPW - 1) / HpTile<G>::RPW;
    hipLaunchKernelGGL((hp_forward_kernel<T, G, K>), dim3(nb), dim3(64), 0, ctx->stream, x, Y, snum, tnum, pad, nc, c);
    hipLaunchKernelGGL((hp_backward_kernel<G, K>), dim3(nb), dim3(64), 0, ctx->stream, Y, out, snum, tnum, pad, nc, c);
}

template <typename T>
static void hp_dispatch(impdar_ctx *ctx, const T *x, double *Y, double *out, int snum, int tnum, int pad, int nc,
                        const FiltCoefs<HP_MAX_COEF> &c)
{
    static_assert(HP_MAX_COEF - 1 <= 2 * 8, "at most 2 delays per lane at 8 lanes per row");
    const int nd = nc - 1;   // delays
    if (nd <= 4) hp_launch<T, 4, 1>(ctx, x, Y, out, snum, tnum, pad, nc, c);
    else if (nd <= 8) hp_launch<T, 8, 1>(ctx, x, Y, out, snum, tnum, pad, nc, c);
    else hp_launch<T, 8, 2>(ctx, x, Y, out, snum, tnum, pad, nc, c);
}

static int hfiltfilt_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *b, const double *a,
                           int ncoef, const double *zi, const double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && b && a && zi && out, "impdar_hfiltfilt: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_hfiltfilt: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(ncoef >= 2 && ncoef <= HP_MAX_COEF, "impdar_hfiltfilt: %d filter coefficients (2..%d supported)",
                     ncoef, HP_MAX_COEF);
    IMPDAR_ARG_CHECK(a[0] != 0.0, "impdar_hfiltfilt: a[0] is zero");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_hfiltfilt: empty radargram");
    const int pad = 3 * ncoef;
    // scipy.signal.filtfilt's own guard and message
    IMPDAR_ARG_CHECK(tnum > pad, "The length of the input vector x must be greater than padlen, which is %d.", pad);
    IMPDAR_ARG_CHECK((long long)snum * (tnum + 2 * pad) < (1LL << 40), "impdar_hfiltfilt: radargram too large");
    return IMPDAR_OK;
}

extern "C" int impdar_hfiltfilt_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const double *b,
                                    const double *a, int ncoef, const double *zi, double *d_out)
{
    const auto lock = g_hp.lock();
    const int rc = hfiltfilt_check(ctx, d_data, dtype, snum, tnum, b, a, ncoef, zi, d_out);
    if (rc) return rc;
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F64 || d_out != d_data, "impdar_hfiltfilt: float32 input needs a separate output");
    const int pad = 3 * ncoef;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    const FiltCoefs<HP_MAX_COEF> c = filt_coefs<HP_MAX_COEF>(b, a, zi, ncoef);
    g_hp.bind(ctx);
    IMPDAR_HIP_CHECK(g_hp.y.ensure((size_t)snum * (tnum + 2 * pad) * sizeof(double)));
    if (dtype == IMPDAR_F32)
        hp_dispatch(ctx, (const float *)d_data, g_hp.y.as<double>(), d_out, snum, tnum, pad, ncoef, c);
    else
        hp_dispatch(ctx, (const double *)d_data, g_hp.y.as<double>(), d_out, snum, tnum, pad, ncoef, c);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer form: the argument check, then StepScratch::host_form (float64 runs in place) -------------

extern "C" int impdar_hfiltfilt(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *b,
                                const double *a, int ncoef, const double *zi, double *out)
{
    const int rc = hfiltfilt_check(ctx, data, dtype, snum, tnum, b, a, ncoef, zi, out);
    if (rc) return rc;
    const size_t ne = (size_t)snum * tnum;
    return g_hp.host_form(ctx, g_hp.in, data, ne * impdar_dtype_size(dtype), dtype == IMPDAR_F32 ? &g_hp.out : nullptr, out,
                          ne * sizeof(double), [&](void *d_in, void *d_out) {
                              return impdar_hfiltfilt_dev(ctx, d_in, dtype, snum, tnum, b, a, ncoef, zi, (double *)d_out);
                          });
}
