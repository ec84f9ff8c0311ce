// The time-offset search of kinematic GPS control (the reference's gpslib.kinematic_gps_control with guess_offset,
// src/impdar/lib/gpslib.py:420-427): for every candidate offset the GPS track, its times shifted by the candidate, is
// interpolated to the trace times, and the candidate's score is the Pearson correlation of the interpolated latitude with the
// radar's own plus that of the longitudes.
//
// The interpolation is SciPy's interp1d(kind='linear') as the reference calls it, restated from its source:
//   extrapolate == 0  np.interp (interp1d._call_linear_np): the bracket x[j] <= t < x[j + 1] by bisection, y[j] where
//                     t == x[j] or j is the last fix, else slope (t - x[j]) + y[j] with NumPy's NaN fallback from the other
//                     knot; a trace outside [x[0], x[ngps - 1]] is counted and takes no part (the reference raises there);
//   extrapolate == 1  interp1d._call_linear: idx = searchsorted(x, t, 'left') clipped to [1, ngps - 1], then
//                     ((y_hi - y_lo) / (x_hi - x_lo)) (t - x_lo) + y_lo.
// x[k] = (gps_t[k] + search[c]) + base is computed where it is needed, in that order, in float64; the unit builds with
// -ffp-contract=off, so every product and sum above is rounded as NumPy rounds it and the probe rows are SciPy's bits.
//
// One workgroup of GPS_THREADS threads per candidate, trace j on thread j % GPS_THREADS in rising order.  Two passes, each
// interpolating again (cheaper than storing ncand x tnum values): the sums and pair counts, then -- the means subtracted --
// the centred sums.  A pass ends in a butterfly over each wave and the waves' partials added in wave order: the order of
// the additions is a function of the trace index alone, no atomics, and two calls give the same bits.
#include "common.h"
#include "gps_route.h"

struct GpsArgs {
    const double *gt, *glat, *glon;       // [ngps]
    const double *t, *lat, *lon;          // [tnum]
    const double *search;                 // [ncand]
    double *cc;                           // [ncand]
    long long *nout;                      // [ncand]
    double *probe_lat, *probe_lon;        // [tnum]
    long long ngps, tnum, probe;
    double base;
};

// the interpolated latitude and longitude at trace time t for the shift s; returns whether t lies outside the record
template <bool EXTRAP>
__device__ __forceinline__ bool gps_interp(const GpsArgs &A, double s, double t, double &la, double &lo)
{
    const double nan = __builtin_nan("");
    const long long n = A.ngps;
#define GPS_X(k) ((A.gt[k] + s) + A.base)
    if (EXTRAP) {
        // the first k with x[k] >= t (a NaN t compares false everywhere: 0, and its result is NaN whatever the bracket)
        long long a = 0, b = n;
        while (a < b) {
            const long long mid = a + ((b - a) >> 1);
            if (GPS_X(mid) < t) a = mid + 1;
            else b = mid;
        }
        const long long hi = a < 1 ? 1 : (a > n - 1 ? n - 1 : a), lw = hi - 1;
        const double x_lo = GPS_X(lw), x_hi = GPS_X(hi);
        const double dx = x_hi - x_lo, dt = t - x_lo;
        la = ((A.glat[hi] - A.glat[lw]) / dx) * dt + A.glat[lw];
        lo = ((A.glon[hi] - A.glon[lw]) / dx) * dt + A.glon[lw];
        return false;
    }
    if (t != t) {
        la = lo = t;
        return false;
    }
    if (t < GPS_X(0) || t > GPS_X(n - 1)) {
        la = lo = nan;
        return true;
    }
    // the last j with x[j] <= t
    long long a = 0, b = n;
    while (a < b) {
        const long long mid = a + ((b - a) >> 1);
        if (GPS_X(mid) <= t) a = mid + 1;
        else b = mid;
    }
    const long long j = a - 1;
    const double xj = GPS_X(j);
    if (j == n - 1 || xj == t) {
        la = A.glat[j];
        lo = A.glon[j];
        return false;
    }
    const double xn = GPS_X(j + 1);
    const double dx = xn - xj, dt = t - xj;
    const double *ys[2] = {A.glat, A.glon};
    double r[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const double y0 = ys[q][j], y1 = ys[q][j + 1];
        const double slope = (y1 - y0) / dx;
        double v = slope * dt + y0;
        if (v != v) {
            v = slope * (t - xn) + y1;
            if (v != v && y0 == y1) v = y0;
        }
        r[q] = v;
    }
    la = r[0];
    lo = r[1];
    return false;
#undef GPS_X
}

// v[0 .. N) summed over the workgroup, the total in every thread: a butterfly over each wave, then the waves in their order
template <int N> __device__ __forceinline__ void gps_block_sum(double (&v)[N], double (*part)[N])
{
#pragma unroll
    for (int q = 0; q < N; ++q)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off);
    const int wave = threadIdx.x >> 6;
    __syncthreads();                    // (the partials of the pass before have been read)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) part[wave][q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) {
        double s = part[0][q];
        for (int w = 1; w < GPS_WAVES; ++w) s += part[w][q];
        v[q] = s;
    }
}

// np.corrcoef's off-diagonal term from the centred sums of n pairs
__device__ __forceinline__ double gps_pearson(double n, double sxy, double sxx, double syy)
{
    if (!(n >= 2.0) || sxx == 0.0 || syy == 0.0) return __builtin_nan("");
    const double r = sxy / sqrt(sxx * syy);           // (a NaN or Inf among the pairs: NaN, as in NumPy)
    return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
}

template <bool EXTRAP> __global__ __launch_bounds__(GPS_THREADS) void gps_cc_kernel(const GpsArgs A)
{
    __shared__ double part[GPS_WAVES][7];
    const long long c = blockIdx.x;
    const double s = A.search[c];
    const bool probe = c == A.probe;
    // pass 1: sums and counts of the pairs where neither value is NaN, latitude and longitude masked separately
    double p[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // sum lat_i, sum lat, pairs; the same of the longitudes; traces outside
    for (long long j = threadIdx.x; j < A.tnum; j += GPS_THREADS) {
        double la, lo;
        const bool outside = gps_interp<EXTRAP>(A, s, A.t[j], la, lo);
        if (probe) {
            A.probe_lat[j] = la;
            A.probe_lon[j] = lo;
        }
        if (outside) {
            p[6] += 1.0;
            continue;
        }
        const double rla = A.lat[j], rlo = A.lon[j];
        if (la == la && rla == rla) {
            p[0] += la;
            p[1] += rla;
            p[2] += 1.0;
        }
        if (lo == lo && rlo == rlo) {
            p[3] += lo;
            p[4] += rlo;
            p[5] += 1.0;
        }
    }
    gps_block_sum<7>(p, part);
    const double mla = p[0] / p[2], mrla = p[1] / p[2], mlo = p[3] / p[5], mrlo = p[4] / p[5];
    // pass 2: the centred sums
    double q[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // dxdy, dx^2, dy^2 of the latitudes, of the longitudes, (spare)
    for (long long j = threadIdx.x; j < A.tnum; j += GPS_THREADS) {
        double la, lo;
        if (gps_interp<EXTRAP>(A, s, A.t[j], la, lo)) continue;
        const double rla = A.lat[j], rlo = A.lon[j];
        if (la == la && rla == rla) {
            const double dx = la - mla, dy = rla - mrla;
            q[0] += dx * dy;
            q[1] += dx * dx;
            q[2] += dy * dy;
        }
        if (lo == lo && rlo == rlo) {
            const double dx = lo - mlo, dy = rlo - mrlo;
            q[3] += dx * dy;
            q[4] += dx * dx;
            q[5] += dy * dy;
        }
    }
    gps_block_sum<7>(q, part);
    if (threadIdx.x == 0) {
        A.cc[c] = gps_pearson(p[2], q[0], q[1], q[2]) + gps_pearson(p[5], q[3], q[4], q[5]);
        A.nout[c] = (long long)p[6];
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct GpsBufs {
    DevBuf in, out;
    void release()
    {
        in.release();
        out.release();
    }
};
static StepScratch<GpsBufs> g_gps;

void impdar_gpstrack_forget(impdar_ctx *ctx) { g_gps.forget(ctx); }

extern "C" int impdar_gps_cc_plan(long long ngps, long long tnum, long long ncand, int extrapolate, long long *scratch_bytes)
{
    const GpsRoute R = gps_route(ngps, tnum, ncand, extrapolate);
    IMPDAR_ARG_CHECK(R.ok, "impdar_gps_cc: %s (ngps %lld, tnum %lld, ncand %lld)", R.why, ngps, tnum, ncand);
    if (scratch_bytes) *scratch_bytes = R.scratch_bytes;
    return IMPDAR_OK;
}

extern "C" int impdar_gps_cc(impdar_ctx *ctx, const double *gps_t, const double *gps_lat, const double *gps_lon, long long ngps,
                             const double *t, const double *lat, const double *lon, long long tnum, double base, const double *search,
                             long long ncand, int extrapolate, double *cc, long long *nout, long long probe, double *probe_lat,
                             double *probe_lon)
{
    IMPDAR_ARG_CHECK(ctx && gps_t && gps_lat && gps_lon && t && lat && lon && search && cc && nout, "impdar_gps_cc: null argument");
    const GpsRoute R = gps_route(ngps, tnum, ncand, extrapolate);
    IMPDAR_ARG_CHECK(R.ok, "impdar_gps_cc: %s (ngps %lld, tnum %lld, ncand %lld)", R.why, ngps, tnum, ncand);
    IMPDAR_ARG_CHECK(gps_probe_ok(probe, ncand), "impdar_gps_cc: probe %lld of %lld candidates", probe, ncand);
    IMPDAR_ARG_CHECK(probe < 0 || (probe_lat && probe_lon), "impdar_gps_cc: a probe needs both of its rows");
    const long long bad = gps_times_bad(gps_t, ngps);
    IMPDAR_ARG_CHECK(!bad, "impdar_gps_cc: gps_t[%lld] is NaN or below the fix before it", bad - 1);

    const auto held = g_gps.lock();
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_gps.bind(ctx);
    const size_t gb = (size_t)ngps * sizeof(double), tb = (size_t)tnum * sizeof(double), cb = (size_t)ncand * sizeof(double);
    const void *dev[7];
    int rc = impdar_upload_tables(ctx, g_gps.in, {{gps_t, gb}, {gps_lat, gb}, {gps_lon, gb}, {t, tb}, {lat, tb}, {lon, tb}, {search, cb}}, dev);
    if (rc) return rc;
    const size_t off_nout = impdar_round16(cb), off_pla = off_nout + impdar_round16(cb), off_plo = off_pla + impdar_round16(tb);
    const size_t out_bytes = off_plo + impdar_round16(tb);
    IMPDAR_HIP_CHECK(g_gps.out.ensure(out_bytes));
    char *o = g_gps.out.as<char>();
    GpsArgs A;
    A.gt = (const double *)dev[0];
    A.glat = (const double *)dev[1];
    A.glon = (const double *)dev[2];
    A.t = (const double *)dev[3];
    A.lat = (const double *)dev[4];
    A.lon = (const double *)dev[5];
    A.search = (const double *)dev[6];
    A.cc = reinterpret_cast<double *>(o);
    A.nout = reinterpret_cast<long long *>(o + off_nout);
    A.probe_lat = reinterpret_cast<double *>(o + off_pla);
    A.probe_lon = reinterpret_cast<double *>(o + off_plo);
    A.ngps = ngps;
    A.tnum = tnum;
    A.probe = probe < 0 ? -1 : probe;
    A.base = base;
    impdar_ctx_note(ctx, "impdar_gps_cc", "gps_cc_kernel");
    rc = impdar_ctx_ktic(ctx);          // the search kernel alone: impdar_ctx_last_kernel_ms
    if (rc) return rc;
    if (extrapolate) hipLaunchKernelGGL(gps_cc_kernel<true>, dim3((unsigned)R.workgroups), dim3(R.threads), 0, ctx->stream, A);
    else hipLaunchKernelGGL(gps_cc_kernel<false>, dim3((unsigned)R.workgroups), dim3(R.threads), 0, ctx->stream, A);
    IMPDAR_HIP_CHECK(hipGetLastError());
    rc = impdar_ctx_ktoc(ctx);
    if (rc) return rc;
    const size_t back = probe < 0 ? off_pla : out_bytes;
    std::vector<char> host(back);
    IMPDAR_HIP_CHECK(hipMemcpyAsync(host.data(), o, back, hipMemcpyDeviceToHost, ctx->stream));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    memcpy(cc, host.data(), cb);
    memcpy(nout, host.data() + off_nout, cb);
    if (probe >= 0) {
        memcpy(probe_lat, host.data() + off_pla, tb);
        memcpy(probe_lon, host.data() + off_plo, tb);
    }
    return IMPDAR_OK;
}
