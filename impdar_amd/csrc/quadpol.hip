// The quad-polarised ApRES chain on the device (reference src/impdar/lib/ApresData/_QuadPolProcessing.py):
//
//   * rotation (:87-99): the four measured vectors shh, shv, svh, svv (n) rotated through n_thetas azimuths
//       into HH, HV, VH, VV (n, n_thetas); cos^2, sin cos and sin^2 of every azimuth are the host's.
//                                                                                          (qp_rotate_kernel)
//   * hhvv coherence (:153-165, coherence() of _TimeDiffProcessing.py:45-48): for output (row j, column i)
//         c = S(HH conj(VV)) / sqrt(S|HH|^2 S|VV|^2),  S over rows [max(0, j - nrange), min(n - 1, j + nrange))
//                                                       and columns [i - ntheta, i + ntheta)
//       Radar power falls by decades along range, so a window sum that is a DIFFERENCE of running sums loses
//       the window to the rounding of everything above it (1e-9 on a profile that decays three decades, where
//       the reference is at 1e-15).  Every sum here is therefore made of additions alone:
//         qp_box_kernel     the three products HH conj(VV), |HH|^2, |VV|^2 summed over the 2 ntheta columns of the
//                           window, in column order, per (row, output column): 4 doubles, `QpSum`;
//         qp_block_kernel   those summed over aligned blocks of `bk` rows, in row order;
//         qp_window_kernel  a window = the rows before its first whole block + its whole blocks + the rows after
//                           its last one, in row order, at most 2 nrange / bk + 2 (bk - 1) additions; the quotient.
//       The columns are taken as given (a padded array: output column i is input column i + ntheta, and there are
//       ncols - 2 ntheta of them) or periodic over ncols (the reference's hstack of the last and first ntheta
//       columns, never materialised).  Both add the same numbers in the same order.
//   * phase gradient (:199-216): dphi/dz = (R dI/dz - I dR/dz) / (R^2 + I^2) with numpy.gradient's edge-order-1
//       differences along range (the rule of impdar_kirchhoff's coefficients); R, I optionally through the
//       library's own filtfilt first (the reference's lowpass).                       (qp_split_kernel, qp_grad_kernel)
//   * cross-polarised extinction axis (:225-272, power_anomaly :303-319, lowpass :323-355): per row of HV the azimuth
//       inside a window of columns at which the low-passed power anomaly is least.
//         qp_anomaly_kernel  P = 10 log10(HV^2), complex as NumPy forms it (the square, clog, the two products with
//                            log10(e), the complex product with 10 + 0j), minus the row's nanmean; one wavefront per
//                            row.  The mean skips every element with a NaN in either part, as numpy.nanmean does, and
//                            its sum has one order whatever the grid or the entry point: lane l adds columns l, l + 64,
//                            l + 128 ... in that order, then the 64 lane sums meet in a butterfly over lane distances
//                            32, 16, 8, 4, 2, 1.  The quotient is NumPy's complex / (count + 0j).  Output: ONE (n, 2 m)
//                            float64 array, row j = the m real parts then the m imaginary parts, so that a single
//                            impdar_filtfilt_dev call over 2 m columns filters both (no qp_split_kernel pass).
//         impdar_filtfilt_dev  the library's own filtfilt along range, bit for bit SciPy's;
//         qp_argmin_kernel   numpy.argmin of complex values over columns [c0, c1): the first element with a NaN in
//                            either part, else the least (real, imag) in lexicographic order, ties to the lowest
//                            column; one wavefront per row, int32 out (the column itself, c0 included).
//   * gather (:174, :220, :266-270): out[j] = image[j, idx[j]] of a complex128 or float64 (n, m) image.
//                                                                                          (qp_gather_kernel)
//
// All data is complex128 as interleaved (re, im) doubles, row-major.  Compiled with -ffp-contract=off.
#include <cmath>
#include <limits>
#include "common.h"

#define QP_BLOCK 256
#define QP_MAX_BK 64

struct __attribute__((aligned(32))) QpSum {
    double pr, pi, a, b;   // S(HH conj(VV)) real and imaginary, S|HH|^2, S|VV|^2
};

__device__ __forceinline__ void qp_add(QpSum &s, const QpSum &t)
{
    s.pr += t.pr;
    s.pi += t.pi;
    s.a += t.a;
    s.b += t.b;
}

__global__ __launch_bounds__(QP_BLOCK) void qp_rotate_kernel(const double2 *__restrict__ shh, const double2 *__restrict__ shv,
                                                             const double2 *__restrict__ svh, const double2 *__restrict__ svv,
                                                             const double *__restrict__ c2, const double *__restrict__ sc,
                                                             const double *__restrict__ s2, double2 *__restrict__ HH,
                                                             double2 *__restrict__ HV, double2 *__restrict__ VH,
                                                             double2 *__restrict__ VV, int n, int nth)
{
    const size_t idx = (size_t)blockIdx.x * QP_BLOCK + threadIdx.x;
    if (idx >= (size_t)n * nth) return;
    const int j = (int)(idx / nth), i = (int)(idx % nth);
    const double2 hh = shh[j], hv = shv[j], vh = svh[j], vv = svv[j];
    const double c = c2[i], m = sc[i], s = s2[i];
    const double2 cross = make_double2(vh.x + hv.x, vh.y + hv.y), co = make_double2(vv.x - hh.x, vv.y - hh.y);
    HH[idx] = make_double2(hh.x * c + cross.x * m + vv.x * s, hh.y * c + cross.y * m + vv.y * s);
    HV[idx] = make_double2(hv.x * c + co.x * m - vh.x * s, hv.y * c + co.y * m - vh.y * s);
    VH[idx] = make_double2(vh.x * c + co.x * m - hv.x * s, vh.y * c + co.y * m - hv.y * s);
    VV[idx] = make_double2(vv.x * c - cross.x * m + hh.x * s, vv.y * c - cross.y * m + hh.y * s);
}

// one thread per (row, output column); neighbouring threads read neighbouring columns of the same row
__global__ __launch_bounds__(QP_BLOCK) void qp_box_kernel(const double2 *__restrict__ HH, const double2 *__restrict__ VV,
                                                          QpSum *__restrict__ box, int n, int ncols, int nout, int ntheta,
                                                          int wrap)
{
    const size_t idx = (size_t)blockIdx.x * QP_BLOCK + threadIdx.x;
    if (idx >= (size_t)n * nout) return;
    const int j = (int)(idx / nout), i = (int)(idx % nout);
    const double2 *h = HH + (size_t)j * ncols, *v = VV + (size_t)j * ncols;
    // as given: input columns [i, i + 2 ntheta); periodic: [i - ntheta, i + ntheta) mod ncols, from a column in [0, ncols)
    int c = wrap ? ((i - ntheta) % ncols + ncols) % ncols : i;
    QpSum s = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 2 * ntheta; ++k) {
        const double2 x = h[c], y = v[c];
        s.pr += x.x * y.x + x.y * y.y;
        s.pi += x.y * y.x - x.x * y.y;
        s.a += x.x * x.x + x.y * x.y;
        s.b += y.x * y.x + y.y * y.y;
        if (++c == ncols) c = 0;   // (as given never gets here: i + 2 ntheta <= ncols)
    }
    box[idx] = s;
}

// one thread per (block of bk rows, output column): rows [b bk, min(n, (b + 1) bk))
__global__ __launch_bounds__(QP_BLOCK) void qp_block_kernel(const QpSum *__restrict__ box, QpSum *__restrict__ blk, int n,
                                                            int nout, int bk, int nblk)
{
    const size_t idx = (size_t)blockIdx.x * QP_BLOCK + threadIdx.x;
    if (idx >= (size_t)nblk * nout) return;
    const int b = (int)(idx / nout), i = (int)(idx % nout);
    const int r0 = b * bk, r1 = r0 + bk < n ? r0 + bk : n;
    QpSum s = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int r = r0; r < r1; ++r) qp_add(s, box[(size_t)r * nout + i]);   // (loads ahead, additions in row order)
    blk[idx] = s;
}

__global__ __launch_bounds__(QP_BLOCK) void qp_window_kernel(const QpSum *__restrict__ box, const QpSum *__restrict__ blk,
                                                             double2 *__restrict__ out, int n, int nout, int nrange, int bk)
{
    const size_t idx = (size_t)blockIdx.x * QP_BLOCK + threadIdx.x;
    if (idx >= (size_t)n * nout) return;
    const int j = (int)(idx / nout), i = (int)(idx % nout);
    const int lo = j - nrange > 0 ? j - nrange : 0;
    const int hi = (long long)j + nrange < n - 1 ? j + nrange : n - 1;   // half-open: the last row is in no window
    // whole blocks [b0, b1) lie inside [lo, hi); without one the window is summed row by row
    int b0 = (lo + bk - 1) / bk, b1 = hi / bk;
    int e0 = b0 * bk, e1 = b1 * bk;
    if (b0 >= b1) b0 = b1 = 0, e0 = e1 = hi;
    QpSum s = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int r = lo; r < e0; ++r) qp_add(s, box[(size_t)r * nout + i]);
#pragma unroll 4
    for (int b = b0; b < b1; ++b) qp_add(s, blk[(size_t)b * nout + i]);
#pragma unroll 4
    for (int r = e1; r < hi; ++r) qp_add(s, box[(size_t)r * nout + i]);
    const double den = sqrt(s.a * s.b);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    // NumPy's complex / real with a zero divisor: NaN in both parts whatever the numerator
    out[idx] = den == 0.0 ? make_double2(nan, nan) : make_double2(s.pr / den, s.pi / den);
}

__global__ __launch_bounds__(QP_BLOCK) void qp_split_kernel(const double2 *__restrict__ c, double *__restrict__ re,
                                                            double *__restrict__ im, size_t count)
{
    const size_t idx = (size_t)blockIdx.x * QP_BLOCK + threadIdx.x;
    if (idx >= count) return;
    const double2 z = c[idx];
    re[idx] = z.x;
    im[idx] = z.y;
}

// numpy.gradient(f, x, axis=0), edge order 1, of column i at row j; f[k * ld] is row k
__device__ __forceinline__ double qp_gradient(const double *f, size_t ld, int j, int n, int uniform, double h,
                                              const double *ga, const double *gb, const double *gc)
{
    if (j == 0) return (f[ld] - f[0]) / (uniform ? h : ga[0]);
    if (j == n - 1) return (f[(size_t)(n - 1) * ld] - f[(size_t)(n - 2) * ld]) / (uniform ? h : ga[n - 1]);
    const double fm = f[(size_t)(j - 1) * ld], f0 = f[(size_t)j * ld], fp = f[(size_t)(j + 1) * ld];
    if (uniform) return (fp - fm) / (2.0 * h);
    return ga[j] * fm + gb[j] * f0 + gc[j] * fp;
}

// R and I are (n, m) with `step` doubles between neighbouring columns: 2 for the interleaved chhvv, 1 for the split
// and filtered pair
__global__ __launch_bounds__(QP_BLOCK) void qp_grad_kernel(const double *__restrict__ R, const double *__restrict__ I, int step,
                                                           double *__restrict__ out, int n, int m, int uniform, double h,
                                                           const double *__restrict__ ga, const double *__restrict__ gb,
                                                           const double *__restrict__ gc)
{
    const size_t idx = (size_t)blockIdx.x * QP_BLOCK + threadIdx.x;
    if (idx >= (size_t)n * m) return;
    const int j = (int)(idx / m), i = (int)(idx % m);
    const size_t ld = (size_t)m * step;
    const double *r = R + (size_t)i * step, *q = I + (size_t)i * step;
    const double dr = qp_gradient(r, ld, j, n, uniform, h, ga, gb, gc), di = qp_gradient(q, ld, j, n, uniform, h, ga, gb, gc);
    const double rv = r[(size_t)j * ld], iv = q[(size_t)j * ld];
    out[idx] = (rv * di - iv * dr) / (rv * rv + iv * iv);
}


// ---- cross-polarised extinction axis ---------------------------------------------------------------------------

#define QP_WAVE 64
#define QP_ROWS_PER_BLOCK (QP_BLOCK / QP_WAVE)

// 10. * numpy.log10(z ** 2.) of one complex128 element, operation by operation
__device__ __forceinline__ double2 qp_power(const double2 z)
{
    const double log10e = 0.434294481903251827651;
    const double sr = z.x * z.x - z.y * z.y, si = z.x * z.y + z.y * z.x;
    const double lr = log(hypot(sr, si)) * log10e, li = atan2(si, sr) * log10e;
    // (10 + 0j) * (lr + li j): a zero element (lr = -inf) leaves NaN in the imaginary part
    return make_double2(10.0 * lr - 0.0 * li, 10.0 * li + 0.0 * lr);
}

// one wavefront per row; pa is (n, 2 m): m real parts, then m imaginary parts
__global__ __launch_bounds__(QP_BLOCK) void qp_anomaly_kernel(const double2 *__restrict__ HV, double *__restrict__ pa, int n, int m)
{
    const int lane = threadIdx.x & (QP_WAVE - 1);
    const size_t row = (size_t)blockIdx.x * QP_ROWS_PER_BLOCK + (threadIdx.x / QP_WAVE);
    if (row >= (size_t)n) return;   // (a whole wavefront at a time)
    const double2 *src = HV + row * m;
    double *re = pa + row * 2 * m, *im = re + m;
    double sr = 0.0, si = 0.0;
    int cnt = 0;
    for (int c = lane; c < m; c += QP_WAVE) {
        const double2 p = qp_power(src[c]);
        re[c] = p.x;
        im[c] = p.y;
        const bool skip = isnan(p.x) || isnan(p.y);   // numpy.nanmean: the element becomes 0 and is not counted
        sr += skip ? 0.0 : p.x;
        si += skip ? 0.0 : p.y;
        cnt += skip ? 0 : 1;
    }
#pragma unroll
    for (int d = QP_WAVE / 2; d >= 1; d >>= 1) {
        sr += __shfl_xor(sr, d, QP_WAVE);
        si += __shfl_xor(si, d, QP_WAVE);
        cnt += __shfl_xor(cnt, d, QP_WAVE);
    }
    // NumPy's complex quotient by (cnt + 0j): ratio 0 / cnt = 0, scale 1 / cnt; 0 / 0 is NaN in both parts
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double mr = nan, mi = nan;
    if (cnt > 0) {
        const double scl = 1.0 / (double)cnt;
        mr = (sr + si * 0.0) * scl;
        mi = (si - sr * 0.0) * scl;
    }
    for (int c = lane; c < m; c += QP_WAVE) {   // (every lane reads back what it wrote itself)
        re[c] -= mr;
        im[c] -= mi;
    }
}

struct QpPick {
    double re, im;
    int idx, nan;   // idx < 0: nothing yet
};

// numpy.argmin's order on complex values: a NaN before everything, then (real, imag), then the lower column
__device__ __forceinline__ bool qp_before(const QpPick &a, const QpPick &b)
{
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    if (a.nan != b.nan) return a.nan != 0;
    if (!a.nan) {
        if (a.re != b.re) return a.re < b.re;
        if (a.im != b.im) return a.im < b.im;
    }
    return a.idx < b.idx;
}

// one wavefront per row of the (n, 2 m) filtered anomaly; columns [c0, c1), 0 <= c0 < c1 <= m
__global__ __launch_bounds__(QP_BLOCK) void qp_argmin_kernel(const double *__restrict__ pa, int *__restrict__ out, int n, int m,
                                                             int c0, int c1)
{
    const int lane = threadIdx.x & (QP_WAVE - 1);
    const size_t row = (size_t)blockIdx.x * QP_ROWS_PER_BLOCK + (threadIdx.x / QP_WAVE);
    if (row >= (size_t)n) return;
    const double *re = pa + row * 2 * m, *im = re + m;
    QpPick best = {0.0, 0.0, -1, 0};
    for (int c = c0 + lane; c < c1; c += QP_WAVE) {
        QpPick p = {re[c], im[c], c, 0};
        p.nan = (isnan(p.re) || isnan(p.im)) ? 1 : 0;
        if (qp_before(p, best)) best = p;
    }
#pragma unroll
    for (int d = QP_WAVE / 2; d >= 1; d >>= 1) {
        QpPick o;
        o.re = __shfl_xor(best.re, d, QP_WAVE);
        o.im = __shfl_xor(best.im, d, QP_WAVE);
        o.idx = __shfl_xor(best.idx, d, QP_WAVE);
        o.nan = __shfl_xor(best.nan, d, QP_WAVE);
        if (qp_before(o, best)) best = o;
    }
    if (lane == 0) out[row] = best.idx;
}

// out[j] = image[j, idx[j]]; `step` doubles per element (2: complex128).  An index outside [0, m) gives NaN.
__global__ __launch_bounds__(QP_BLOCK) void qp_gather_kernel(const double *__restrict__ image, const int *__restrict__ idx,
                                                             double *__restrict__ out, int n, int m, int step)
{
    const size_t j = (size_t)blockIdx.x * QP_BLOCK + threadIdx.x;
    if (j >= (size_t)n) return;
    const int i = idx[j];
    const bool ok = i >= 0 && i < m;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int k = 0; k < step; ++k) out[j * step + k] = ok ? image[(j * m + i) * step + k] : nan;
}

// ------------------------------------------------------------------------------------------------ host side

struct QpBufs {
    DevBuf in[4], out[4], tab, box, blk, re, im, idx;   // staging of the host-buffer forms, host tables, window sums, R and I, indices
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // stage boundaries of the last find_cpe (impdar_qp_find_cpe_last_ms)
    bool ev_set = false;
    void release()
    {
        for (hipEvent_t &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        ev_set = false;
        idx.release();
        for (DevBuf &b : in) b.release();
        for (DevBuf &b : out) b.release();
        tab.release();
        box.release();
        blk.release();
        re.release();
        im.release();
    }
};
static StepScratch<QpBufs> g_qp;

void impdar_quadpol_forget(impdar_ctx *ctx) { g_qp.forget(ctx); }

static inline dim3 qp_grid(size_t count) { return dim3((unsigned)((count + QP_BLOCK - 1) / QP_BLOCK)); }

// rows per block of partial sums: the power of two next to sqrt(nrange), where whole blocks and edge rows cost the same
static int qp_block_rows(int nrange)
{
    int bk = 4;
    while (bk < QP_MAX_BK && bk * bk < nrange) bk *= 2;
    return bk;
}

static int rotate_check(impdar_ctx *ctx, const void *shh, const void *shv, const void *svh, const void *svv, int n,
                        const double *c2, const double *sc, const double *s2, int n_thetas, const void *HH, const void *HV,
                        const void *VH, const void *VV)
{
    IMPDAR_ARG_CHECK(ctx && shh && shv && svh && svv && c2 && sc && s2 && HH && HV && VH && VV, "impdar_qp_rotate: null argument");
    IMPDAR_ARG_CHECK(n >= 1 && n_thetas >= 1, "impdar_qp_rotate: %d range bins and %d azimuths", n, n_thetas);
    IMPDAR_ARG_CHECK((size_t)n * n_thetas <= (size_t)1 << 36, "impdar_qp_rotate: %d x %d is too large", n, n_thetas);
    return IMPDAR_OK;
}

extern "C" int impdar_qp_rotate_dev(impdar_ctx *ctx, const double *d_shh, const double *d_shv, const double *d_svh,
                                    const double *d_svv, int n, const double *cos2, const double *sincos, const double *sin2,
                                    int n_thetas, double *d_HH, double *d_HV, double *d_VH, double *d_VV)
{
    const auto lock = g_qp.lock();
    int rc = rotate_check(ctx, d_shh, d_shv, d_svh, d_svv, n, cos2, sincos, sin2, n_thetas, d_HH, d_HV, d_VH, d_VV);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_qp.bind(ctx);
    const size_t tb = (size_t)n_thetas * sizeof(double);
    const void *d_tab[3];
    rc = impdar_upload_tables(ctx, g_qp.tab, {{cos2, tb}, {sincos, tb}, {sin2, tb}}, d_tab);
    if (rc) return rc;
    hipLaunchKernelGGL(qp_rotate_kernel, qp_grid((size_t)n * n_thetas), dim3(QP_BLOCK), 0, ctx->stream, (const double2 *)d_shh,
                       (const double2 *)d_shv, (const double2 *)d_svh, (const double2 *)d_svv, (const double *)d_tab[0],
                       (const double *)d_tab[1], (const double *)d_tab[2], (double2 *)d_HH, (double2 *)d_HV, (double2 *)d_VH,
                       (double2 *)d_VV, n, n_thetas);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

static int coherence_check(const char *who, const void *HH, const void *VV, int n, int ncols, int nrange, int ntheta, int wrap,
                           const void *out)
{
    IMPDAR_ARG_CHECK(HH && VV && out, "%s: null argument", who);
    IMPDAR_ARG_CHECK(n >= 1 && ncols >= 1, "%s: %d range bins and %d azimuth bins", who, n, ncols);
    IMPDAR_ARG_CHECK(nrange >= 1, "%s: nrange = %d leaves an empty window along range", who, nrange);
    IMPDAR_ARG_CHECK(ntheta >= 1, "%s: ntheta = %d leaves an empty window along azimuth", who, ntheta);
    if (wrap)
        IMPDAR_ARG_CHECK(ntheta <= ncols, "%s: ntheta = %d is wider than the %d azimuths it wraps around", who, ntheta, ncols);
    else
        IMPDAR_ARG_CHECK(ncols - 2 * (long long)ntheta >= 1, "%s: %d azimuth bins hold no column between two pads of ntheta = %d", who,
                         ncols, ntheta);
    IMPDAR_ARG_CHECK((size_t)n * ncols <= (size_t)1 << 34, "%s: %d x %d is too large", who, n, ncols);
    return IMPDAR_OK;
}

extern "C" int impdar_qp_coherence_dev(impdar_ctx *ctx, const double *d_HH, const double *d_VV, int n, int ncols, int nrange,
                                       int ntheta, int wrap, double *d_chhvv)
{
    const auto lock = g_qp.lock();
    IMPDAR_ARG_CHECK(ctx, "impdar_qp_coherence: null context");
    const int rc = coherence_check("impdar_qp_coherence", d_HH, d_VV, n, ncols, nrange, ntheta, wrap, d_chhvv);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_qp.bind(ctx);
    const int nout = wrap ? ncols : ncols - 2 * ntheta;
    const int bk = qp_block_rows(nrange), nblk = (n + bk - 1) / bk;
    IMPDAR_HIP_CHECK(g_qp.box.ensure((size_t)n * nout * sizeof(QpSum)));
    IMPDAR_HIP_CHECK(g_qp.blk.ensure((size_t)nblk * nout * sizeof(QpSum)));
    hipLaunchKernelGGL(qp_box_kernel, qp_grid((size_t)n * nout), dim3(QP_BLOCK), 0, ctx->stream, (const double2 *)d_HH,
                       (const double2 *)d_VV, g_qp.box.as<QpSum>(), n, ncols, nout, ntheta, wrap ? 1 : 0);
    hipLaunchKernelGGL(qp_block_kernel, qp_grid((size_t)nblk * nout), dim3(QP_BLOCK), 0, ctx->stream, g_qp.box.as<QpSum>(),
                       g_qp.blk.as<QpSum>(), n, nout, bk, nblk);
    hipLaunchKernelGGL(qp_window_kernel, qp_grid((size_t)n * nout), dim3(QP_BLOCK), 0, ctx->stream, g_qp.box.as<QpSum>(),
                       g_qp.blk.as<QpSum>(), (double2 *)d_chhvv, n, nout, nrange, bk);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

static int gradient_check(impdar_ctx *ctx, const void *chhvv, int n, int m, int uniform, double h, const double *ga,
                          const double *gb, const double *gc, const double *b, const double *a, int ncoef, const double *zi,
                          const void *out)
{
    IMPDAR_ARG_CHECK(ctx && chhvv && out, "impdar_qp_phase_gradient: null argument");
    IMPDAR_ARG_CHECK(n >= 2 && m >= 1, "impdar_qp_phase_gradient: %d range bins (a gradient needs 2) and %d azimuths", n, m);
    IMPDAR_ARG_CHECK(uniform ? h != 0.0 : (ga && gb && gc), "impdar_qp_phase_gradient: no gradient coefficients");
    IMPDAR_ARG_CHECK(!b || (a && zi && ncoef >= 2), "impdar_qp_phase_gradient: a filter needs b, a and zi");
    IMPDAR_ARG_CHECK((size_t)n * m <= (size_t)1 << 34, "impdar_qp_phase_gradient: %d x %d is too large", n, m);
    return IMPDAR_OK;
}

extern "C" int impdar_qp_phase_gradient_dev(impdar_ctx *ctx, const double *d_chhvv, int n, int m, int grad_uniform, double grad_h,
                                            const double *ga, const double *gb, const double *gc, const double *b,
                                            const double *a, int ncoef, const double *zi, double *d_dphi_dz)
{
    const auto lock = g_qp.lock();
    int rc = gradient_check(ctx, d_chhvv, n, m, grad_uniform, grad_h, ga, gb, gc, b, a, ncoef, zi, d_dphi_dz);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_qp.bind(ctx);
    const void *d_tab[3] = {nullptr, nullptr, nullptr};
    if (!grad_uniform) {
        const size_t tb = (size_t)n * sizeof(double);
        rc = impdar_upload_tables(ctx, g_qp.tab, {{ga, tb}, {gb, tb}, {gc, tb}}, d_tab);
        if (rc) return rc;
    }
    const size_t count = (size_t)n * m;
    const double *R = d_chhvv, *I = d_chhvv + 1;
    int step = 2;
    if (b) {
        IMPDAR_HIP_CHECK(g_qp.re.ensure(count * sizeof(double)));
        IMPDAR_HIP_CHECK(g_qp.im.ensure(count * sizeof(double)));
        hipLaunchKernelGGL(qp_split_kernel, qp_grid(count), dim3(QP_BLOCK), 0, ctx->stream, (const double2 *)d_chhvv,
                           g_qp.re.as<double>(), g_qp.im.as<double>(), count);
        IMPDAR_HIP_CHECK(hipGetLastError());
        // the band-pass step's filtfilt, along range: bit for bit SciPy's
        rc = impdar_filtfilt_dev(ctx, g_qp.re.p, IMPDAR_F64, n, m, b, a, ncoef, zi);
        if (rc) return rc;
        rc = impdar_filtfilt_dev(ctx, g_qp.im.p, IMPDAR_F64, n, m, b, a, ncoef, zi);
        if (rc) return rc;
        R = g_qp.re.as<double>(), I = g_qp.im.as<double>(), step = 1;
    }
    hipLaunchKernelGGL(qp_grad_kernel, qp_grid(count), dim3(QP_BLOCK), 0, ctx->stream, R, I, step, d_dphi_dz, n, m,
                       grad_uniform ? 1 : 0, grad_h, (const double *)d_tab[0], (const double *)d_tab[1], (const double *)d_tab[2]);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}


// ---- cross-polarised extinction axis ---------------------------------------------------------------------------

static inline dim3 qp_row_grid(int n) { return dim3((unsigned)(((size_t)n + QP_ROWS_PER_BLOCK - 1) / QP_ROWS_PER_BLOCK)); }

static int anomaly_check(const char *who, impdar_ctx *ctx, const void *HV, int n, int m, const void *pa)
{
    IMPDAR_ARG_CHECK(ctx && HV && pa, "%s: null argument", who);
    IMPDAR_ARG_CHECK(HV != pa, "%s: the anomaly cannot be written over the image", who);
    IMPDAR_ARG_CHECK(n >= 1 && m >= 1, "%s: %d range bins and %d azimuths", who, n, m);
    IMPDAR_ARG_CHECK((size_t)n * m <= (size_t)1 << 34, "%s: %d x %d is too large", who, n, m);
    return IMPDAR_OK;
}

extern "C" int impdar_qp_power_anomaly_dev(impdar_ctx *ctx, const double *d_HV, int n, int m, double *d_pa)
{
    const auto lock = g_qp.lock();
    const int rc = anomaly_check("impdar_qp_power_anomaly", ctx, d_HV, n, m, d_pa);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_qp.bind(ctx);
    hipLaunchKernelGGL(qp_anomaly_kernel, qp_row_grid(n), dim3(QP_BLOCK), 0, ctx->stream, (const double2 *)d_HV, d_pa, n, m);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

static int find_cpe_check(impdar_ctx *ctx, const void *HV, int n, int m, const double *b, const double *a, int ncoef,
                          const double *zi, int idx_start, int idx_stop, const void *cpe_idxs, const void *pa)
{
    IMPDAR_ARG_CHECK(cpe_idxs, "impdar_qp_find_cpe: null argument");
    const int rc = anomaly_check("impdar_qp_find_cpe", ctx, HV, n, m, cpe_idxs);
    if (rc) return rc;
    IMPDAR_ARG_CHECK(pa != HV, "impdar_qp_find_cpe: the anomaly cannot be written over the image");
    IMPDAR_ARG_CHECK(b && a && zi && ncoef >= 2, "impdar_qp_find_cpe: the filter needs b, a and zi");
    IMPDAR_ARG_CHECK(0 <= idx_start && idx_start < idx_stop && idx_stop <= m,
                     "impdar_qp_find_cpe: columns [%d, %d) are no window of %d azimuths", idx_start, idx_stop, m);
    return IMPDAR_OK;
}

static int qp_mark(impdar_ctx *ctx, int k)
{
    if (!g_qp.ev[k]) IMPDAR_HIP_CHECK(hipEventCreate(&g_qp.ev[k]));
    IMPDAR_HIP_CHECK(hipEventRecord(g_qp.ev[k], ctx->stream));
    return IMPDAR_OK;
}

extern "C" int impdar_qp_find_cpe_dev(impdar_ctx *ctx, const double *d_HV, int n, int m, const double *b, const double *a,
                                      int ncoef, const double *zi, int idx_start, int idx_stop, int *d_cpe_idxs, double *d_pa)
{
    const auto lock = g_qp.lock();
    int rc = find_cpe_check(ctx, d_HV, n, m, b, a, ncoef, zi, idx_start, idx_stop, d_cpe_idxs, d_pa);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_qp.bind(ctx);
    if (!d_pa) {
        IMPDAR_HIP_CHECK(g_qp.re.ensure((size_t)n * m * 2 * sizeof(double)));
        d_pa = g_qp.re.as<double>();
    }
    g_qp.ev_set = false;
    if ((rc = qp_mark(ctx, 0))) return rc;
    hipLaunchKernelGGL(qp_anomaly_kernel, qp_row_grid(n), dim3(QP_BLOCK), 0, ctx->stream, (const double2 *)d_HV, d_pa, n, m);
    IMPDAR_HIP_CHECK(hipGetLastError());
    if ((rc = qp_mark(ctx, 1))) return rc;
    // real and imaginary parts side by side: one filtfilt along range over 2 m columns, bit for bit SciPy's
    rc = impdar_filtfilt_dev(ctx, d_pa, IMPDAR_F64, n, 2 * m, b, a, ncoef, zi);
    if (rc) return rc;
    if ((rc = qp_mark(ctx, 2))) return rc;
    hipLaunchKernelGGL(qp_argmin_kernel, qp_row_grid(n), dim3(QP_BLOCK), 0, ctx->stream, (const double *)d_pa, d_cpe_idxs, n, m,
                       idx_start, idx_stop);
    IMPDAR_HIP_CHECK(hipGetLastError());
    if ((rc = qp_mark(ctx, 3))) return rc;
    g_qp.ev_set = true;
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_qp_find_cpe_last_ms(impdar_ctx *ctx, float *anomaly_ms, float *filter_ms, float *argmin_ms)
{
    const auto lock = g_qp.lock();
    IMPDAR_ARG_CHECK(ctx && anomaly_ms && filter_ms && argmin_ms, "impdar_qp_find_cpe_last_ms: null argument");
    IMPDAR_ARG_CHECK(g_qp.owner == ctx && g_qp.ev_set, "no find_cpe has run on this context");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    IMPDAR_HIP_CHECK(hipEventSynchronize(g_qp.ev[3]));
    float *out[3] = {anomaly_ms, filter_ms, argmin_ms};
    for (int k = 0; k < 3; ++k) IMPDAR_HIP_CHECK(hipEventElapsedTime(out[k], g_qp.ev[k], g_qp.ev[k + 1]));
    return IMPDAR_OK;
}

static int gather_check(impdar_ctx *ctx, const void *image, int n, int m, const void *idx, const void *out)
{
    IMPDAR_ARG_CHECK(ctx && image && idx && out, "impdar_qp_cpe_gather: null argument");
    IMPDAR_ARG_CHECK(image != out, "impdar_qp_cpe_gather: the result cannot be written over the image");
    IMPDAR_ARG_CHECK(n >= 1 && m >= 1, "impdar_qp_cpe_gather: %d range bins and %d azimuths", n, m);
    IMPDAR_ARG_CHECK((size_t)n * m <= (size_t)1 << 34, "impdar_qp_cpe_gather: %d x %d is too large", n, m);
    return IMPDAR_OK;
}

extern "C" int impdar_qp_cpe_gather_dev(impdar_ctx *ctx, const double *d_image, int is_complex, int n, int m, const int *d_idx,
                                        double *d_out)
{
    const auto lock = g_qp.lock();
    const int rc = gather_check(ctx, d_image, n, m, d_idx, d_out);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_qp.bind(ctx);
    hipLaunchKernelGGL(qp_gather_kernel, qp_grid((size_t)n), dim3(QP_BLOCK), 0, ctx->stream, d_image, d_idx, d_out, n, m,
                       is_complex ? 2 : 1);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer forms ---------------------------------------------------------------------------------------

extern "C" int impdar_qp_rotate(impdar_ctx *ctx, const double *shh, const double *shv, const double *svh, const double *svv, int n,
                                const double *cos2, const double *sincos, const double *sin2, int n_thetas, double *HH, double *HV,
                                double *VH, double *VV)
{
    int rc = rotate_check(ctx, shh, shv, svh, svv, n, cos2, sincos, sin2, n_thetas, HH, HV, VH, VV);
    if (rc) return rc;
    const auto held = g_qp.lock();
    const double *src[4] = {shh, shv, svh, svv};
    double *dst[4] = {HH, HV, VH, VV};
    const size_t bytes = (size_t)n * n_thetas * 16;
    for (int k = 0; k < 4; ++k) {
        rc = g_qp.stage_in(ctx, g_qp.in[k], src[k], (size_t)n * 16);
        if (rc) return rc;
        IMPDAR_HIP_CHECK(g_qp.out[k].ensure(bytes));
    }
    rc = impdar_qp_rotate_dev(ctx, g_qp.in[0].as<double>(), g_qp.in[1].as<double>(), g_qp.in[2].as<double>(),
                              g_qp.in[3].as<double>(), n, cos2, sincos, sin2, n_thetas, g_qp.out[0].as<double>(),
                              g_qp.out[1].as<double>(), g_qp.out[2].as<double>(), g_qp.out[3].as<double>());
    for (int k = 0; k < 4 && !rc; ++k) rc = impdar_download(ctx, dst[k], g_qp.out[k].p, bytes, ctx->stream);
    return rc;
}

extern "C" int impdar_qp_coherence(impdar_ctx *ctx, const double *HH, const double *VV, int n, int ncols, int nrange, int ntheta,
                                   int wrap, double *chhvv)
{
    IMPDAR_ARG_CHECK(ctx, "impdar_qp_coherence: null context");
    int rc = coherence_check("impdar_qp_coherence", HH, VV, n, ncols, nrange, ntheta, wrap, chhvv);
    if (rc) return rc;
    const auto held = g_qp.lock();
    const size_t bytes = (size_t)n * ncols * 16, bytes_out = (size_t)n * (wrap ? ncols : ncols - 2 * ntheta) * 16;
    rc = g_qp.stage_in(ctx, g_qp.in[0], HH, bytes);
    if (!rc) rc = g_qp.stage_in(ctx, g_qp.in[1], VV, bytes);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(g_qp.out[0].ensure(bytes_out));
    rc = impdar_qp_coherence_dev(ctx, g_qp.in[0].as<double>(), g_qp.in[1].as<double>(), n, ncols, nrange, ntheta, wrap,
                                 g_qp.out[0].as<double>());
    if (rc) return rc;
    return impdar_download(ctx, chhvv, g_qp.out[0].p, bytes_out, ctx->stream);
}

extern "C" int impdar_qp_phase_gradient(impdar_ctx *ctx, const double *chhvv, int n, int m, int grad_uniform, double grad_h,
                                        const double *ga, const double *gb, const double *gc, const double *b, const double *a,
                                        int ncoef, const double *zi, double *dphi_dz)
{
    const int rc = gradient_check(ctx, chhvv, n, m, grad_uniform, grad_h, ga, gb, gc, b, a, ncoef, zi, dphi_dz);
    if (rc) return rc;
    return g_qp.host_form(ctx, g_qp.in[0], chhvv, (size_t)n * m * 16, &g_qp.out[0], dphi_dz, (size_t)n * m * 8,
                          [&](void *d_in, void *d_out) {
                              return impdar_qp_phase_gradient_dev(ctx, (const double *)d_in, n, m, grad_uniform, grad_h, ga, gb, gc,
                                                                  b, a, ncoef, zi, (double *)d_out);
                          });
}


extern "C" int impdar_qp_power_anomaly(impdar_ctx *ctx, const double *HV, int n, int m, double *pa)
{
    const int rc = anomaly_check("impdar_qp_power_anomaly", ctx, HV, n, m, pa);
    if (rc) return rc;
    return g_qp.host_form(ctx, g_qp.in[0], HV, (size_t)n * m * 16, &g_qp.out[0], pa, (size_t)n * m * 16,
                          [&](void *d_in, void *d_out) { return impdar_qp_power_anomaly_dev(ctx, (const double *)d_in, n, m, (double *)d_out); });
}

extern "C" int impdar_qp_find_cpe(impdar_ctx *ctx, const double *HV, int n, int m, const double *b, const double *a, int ncoef,
                                  const double *zi, int idx_start, int idx_stop, int *cpe_idxs, double *pa)
{
    int rc = find_cpe_check(ctx, HV, n, m, b, a, ncoef, zi, idx_start, idx_stop, cpe_idxs, pa);
    if (rc) return rc;
    const auto held = g_qp.lock();
    const size_t bytes = (size_t)n * m * 16;
    rc = g_qp.stage_in(ctx, g_qp.in[0], HV, bytes);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(g_qp.out[0].ensure(bytes));
    IMPDAR_HIP_CHECK(g_qp.idx.ensure((size_t)n * sizeof(int)));
    rc = impdar_qp_find_cpe_dev(ctx, g_qp.in[0].as<double>(), n, m, b, a, ncoef, zi, idx_start, idx_stop, g_qp.idx.as<int>(),
                                g_qp.out[0].as<double>());
    if (rc) return rc;
    rc = impdar_download(ctx, cpe_idxs, g_qp.idx.p, (size_t)n * sizeof(int), ctx->stream);
    if (rc || !pa) return rc;
    return impdar_download(ctx, pa, g_qp.out[0].p, bytes, ctx->stream);
}

extern "C" int impdar_qp_cpe_gather(impdar_ctx *ctx, const double *image, int is_complex, int n, int m, const int *idx, double *out)
{
    int rc = gather_check(ctx, image, n, m, idx, out);
    if (rc) return rc;
    const auto held = g_qp.lock();
    const size_t es = is_complex ? 16 : 8;
    rc = g_qp.stage_in(ctx, g_qp.in[0], image, (size_t)n * m * es);
    if (!rc) rc = g_qp.stage_in(ctx, g_qp.idx, idx, (size_t)n * sizeof(int));
    if (rc) return rc;
    IMPDAR_HIP_CHECK(g_qp.out[0].ensure((size_t)n * es));
    rc = impdar_qp_cpe_gather_dev(ctx, g_qp.in[0].as<double>(), is_complex, n, m, g_qp.idx.as<int>(), g_qp.out[0].as<double>());
    if (rc) return rc;
    return impdar_download(ctx, out, g_qp.out[0].p, (size_t)n * es, ctx->stream);
}

// ---- the reference's native hook (src/impdar/lib/ApresData/coherence.h:13) -----------------------------------
// The arrays are the padded ones of _QuadPolProcessing.py:127-136: columns ntheta ... azimuth_bins - ntheta - 1 of
// chhvv are written, the pads are the caller's.  Device 0, a context of its own that lives as long as the process.

static impdar_ctx *g_qp_hook_ctx = nullptr;
static std::mutex g_qp_hook_mu;

extern "C" void coherence2d(double *chhvv, double *HH, double *VV, int nrange, int ntheta, int range_bins, int azimuth_bins)
{
    const int c0 = ntheta > 0 ? ntheta : 0;
    const long long c1 = (long long)azimuth_bins - c0;   // the written columns are [c0, c1)
    auto fail = [&](const char *why) {
        fprintf(stderr, "impdar coherence2d: %s -- chhvv filled with NaN\n", why);
        if (!chhvv || range_bins < 1) return;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int j = 0; j < range_bins; ++j)
            for (long long i = c0; i < c1; ++i) {
                chhvv[2 * ((size_t)j * azimuth_bins + i)] = nan;
                chhvv[2 * ((size_t)j * azimuth_bins + i) + 1] = nan;
            }
    };
    // everything that needs no device is refused before one is touched
    if (coherence_check("coherence2d", HH, VV, range_bins, azimuth_bins, nrange, ntheta, 0, chhvv)) return fail(impdar_last_error());
    std::lock_guard<std::mutex> lk(g_qp_hook_mu);
    if (!g_qp_hook_ctx && impdar_ctx_create(0, &g_qp_hook_ctx) != IMPDAR_OK) {
        g_qp_hook_ctx = nullptr;
        return fail(impdar_last_error());
    }
    const int nout = azimuth_bins - 2 * ntheta;
    std::vector<double> packed;
    try {
        packed.resize((size_t)range_bins * nout * 2);
    } catch (const std::bad_alloc &) {
        return fail("out of host memory");
    }
    if (impdar_qp_coherence(g_qp_hook_ctx, HH, VV, range_bins, azimuth_bins, nrange, ntheta, 0, packed.data()) != IMPDAR_OK) {
        (void)hipGetLastError();
        return fail(impdar_last_error());
    }
    for (int j = 0; j < range_bins; ++j)
        memcpy(chhvv + 2 * ((size_t)j * azimuth_bins + ntheta), packed.data() + 2 * (size_t)j * nout, (size_t)nout * 16);
}
