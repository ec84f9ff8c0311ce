// ApRES range conversion, stacking and phase difference on the device (reference
// src/impdar/lib/ApresData/_ApresDataProcessing.py:24-123 and :191-222, _TimeDiffProcessing.py:27-93):
//
//   * range conversion: `rows` = bnum cnum chirps of `snum` real samples, pad factor p, N = p snum, nf = floor(N / 2)
//       frequencies of which the first n <= nf are kept.  In chunks of rows, so that the scratch stays bounded:
//         ar_prep_kernel   one workgroup per chirp: the row's sum in float64 (a partial sum per thread, then a tree
//                          over the workgroup), the mean subtracted, the window applied, the real row of length N
//                          written with its zero padding;
//         rocFFT           a double-precision real-to-complex plan of length N batched over the chunk (FftPlan of
//                          fft.h; the library's own row transforms end at 8192 complex points, an instrument's row is
//                          2 x 40001), kept per (N, batch) while the context stays the same;
//         ar_post_kernel   one thread per (row, bin k < nf): spec = X[k] mul (1 / div) -- NumPy divides a complex
//                          array by a real scalar as a product with its reciprocal --, data = comp[k] spec,
//                          Rfine[k] = atan2(im, re) / den[k], or (lambdac atan2(im, re)) / den[k] in phase2range's
//                          first-order branch.  spec and data are stored for k < n, Rfine for all nf bins (the
//                          reference crops Rfine on its first axis, not along range).
//   * stacking: ap_stack_kernel, the mean over `m` consecutive rows of a (rows, snum) float64 or complex128 array: per
//       output sample a sum in row order, then NumPy's own last step -- a division by m for real data, a product
//       with 1 / m for complex data (its complex division by (m + 0j)).  Bit for bit numpy.mean(x, axis=1) of the
//       (groups, m, snum) view for snum >= 2; at snum = 1 the m-axis is contiguous, NumPy sums it pairwise and differs
//       from the row-order sum from m = 8 on.
//   * phase difference: window i covers samples [i step, i step + 2 (win / 2)) of two complex128 vectors;
//       co[i] = S(s1 conj(s2)) / sqrt(S|s1|^2 S|s2|^2), every S a plain sum in sample order of the lanes' parts (no
//       running differences); 0 / 0 is NaN in both parts.  ap_phase_diff_thread_kernel gives a window to a thread
//       (neighbouring threads read windows `step` samples apart: the same cache lines) up to AP_PD_THREAD_MAX
//       terms, ap_phase_diff_wave_kernel gives it to a wavefront above that.
//   * decode (load_apres.py:391-395): ap_decode_kernel, a burst's uint16 / uint32 counts to float64 volts, bit for bit
//       NumPy's expression; the counts go up as they are, in pieces, the kernel of one piece under the copy of the
//       next (impdar_apres_decode_dev at the end of this file).
//
// Everything is float64 / complex128 (interleaved (re, im) doubles), row-major.  Compiled with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <memory>
#include "common.h"
#include "fft.h"

#define AP_BLOCK 256
#define AP_WAVE 64
#define AP_PD_THREAD_MAX 64                         // terms of a window that one thread still sums alone
#define AP_SCRATCH_BYTES ((size_t)256 << 20)        // padded rows + spectra of one chunk, the library's choice of chunk
#define AP_MAX_PLANS 4
#define AP_DEC_VEC 8                                // counts per thread in the body of the decode
#define AP_DEC_PIECE_BYTES ((size_t)8 << 20)        // counts of one upload piece, the library's choice

__global__ __launch_bounds__(AP_BLOCK) void ar_prep_kernel(const double *__restrict__ raw, const double *__restrict__ win,
                                                           double *__restrict__ pad, int snum, int N)
{
    __shared__ double part[AP_BLOCK];
    const double *x = raw + (size_t)blockIdx.x * snum;
    double *y = pad + (size_t)blockIdx.x * N;
    double s = 0.0;
    for (int k = threadIdx.x; k < snum; k += AP_BLOCK) s += x[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = AP_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    const double mean = part[0] / (double)snum;
    for (int k = threadIdx.x; k < N; k += AP_BLOCK) y[k] = k < snum ? (x[k] - mean) * win[k] : 0.0;
}

// X: (chunk, N / 2 + 1) spectra of rows row0 ... row0 + chunk - 1; spec, data: (rows, n); rfine: (rows, nf)
__global__ __launch_bounds__(AP_BLOCK) void ar_post_kernel(const double2 *__restrict__ X, const double2 *__restrict__ comp,
                                                           const double *__restrict__ den, double2 *__restrict__ spec,
                                                           double2 *__restrict__ data, double *__restrict__ rfine, int chunk,
                                                           int nh, int nf, int n, size_t row0, double mul, double rdiv,
                                                           int first_order, double lambdac)
{
    const size_t idx = (size_t)blockIdx.x * AP_BLOCK + threadIdx.x;
    if (idx >= (size_t)chunk * nf) return;
    const int r = (int)(idx / nf), k = (int)(idx % nf);
    const double2 x = X[(size_t)r * nh + k];
    const double2 s = make_double2(x.x * mul * rdiv, x.y * mul * rdiv);
    const double2 c = comp[k];
    const double2 d = make_double2(c.x * s.x - c.y * s.y, c.x * s.y + c.y * s.x);
    const double phi = atan2(d.y, d.x);
    const size_t row = row0 + r;
    rfine[row * nf + k] = first_order ? lambdac * phi / den[k] : phi / den[k];
    if (k < n) {
        spec[row * n + k] = s;
        data[row * n + k] = d;
    }
}

// in: (rows, width) doubles, width = snum or 2 snum; out[g, j] = mean of rows g m ... g m + m - 1 of column j
__global__ __launch_bounds__(AP_BLOCK) void ap_stack_kernel(const double *__restrict__ in, double *__restrict__ out, int width,
                                                            int groups, int m, int reciprocal)
{
    const size_t idx = (size_t)blockIdx.x * AP_BLOCK + threadIdx.x;
    if (idx >= (size_t)groups * width) return;
    const size_t g = idx / width, j = idx % width;
    const double *x = in + g * m * width + j;
    double s = 0.0;
#pragma unroll 4
    for (int i = 0; i < m; ++i) s += x[(size_t)i * width];   // (loads ahead, additions in row order)
    out[idx] = reciprocal ? s * (1.0 / (double)m) : s / (double)m;
}

struct ApSum {
    double pr, pi, a, b;   // S(s1 conj(s2)) real and imaginary, S|s1|^2, S|s2|^2
};

__device__ __forceinline__ void ap_term(ApSum &s, const double2 x, const double2 y)
{
    s.pr += x.x * y.x + x.y * y.y;
    s.pi += x.y * y.x - x.x * y.y;
    s.a += x.x * x.x + x.y * x.y;
    s.b += y.x * y.x + y.y * y.y;
}

__device__ __forceinline__ double2 ap_quotient(const ApSum &s)
{
    const double den = sqrt(s.a * s.b);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (den == 0.0) return make_double2(nan, nan);   // NumPy's complex / real with a zero divisor
    const double scl = 1.0 / den;
    return make_double2(s.pr * scl, s.pi * scl);
}

__global__ __launch_bounds__(AP_BLOCK) void ap_phase_diff_thread_kernel(const double2 *__restrict__ s1, const double2 *__restrict__ s2,
                                                                        double2 *__restrict__ co, int nwin, int terms, int step)
{
    const size_t i = (size_t)blockIdx.x * AP_BLOCK + threadIdx.x;
    if (i >= (size_t)nwin) return;
    const size_t lo = i * step;
    ApSum s = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < terms; ++k) ap_term(s, s1[lo + k], s2[lo + k]);
    co[i] = ap_quotient(s);
}

// one wavefront per window: lane l sums terms l, l + 64, ... in order, then the 64 partial sums fold pairwise
__global__ __launch_bounds__(AP_BLOCK) void ap_phase_diff_wave_kernel(const double2 *__restrict__ s1, const double2 *__restrict__ s2,
                                                                      double2 *__restrict__ co, int nwin, int terms, int step)
{
    const int lane = threadIdx.x % AP_WAVE;
    const size_t i = (size_t)blockIdx.x * (AP_BLOCK / AP_WAVE) + threadIdx.x / AP_WAVE;
    if (i >= (size_t)nwin) return;   // (a whole wavefront leaves together)
    const size_t lo = i * step;
    ApSum s = {0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < terms; k += AP_WAVE) ap_term(s, s1[lo + k], s2[lo + k]);
    for (int off = AP_WAVE / 2; off > 0; off >>= 1) {
        s.pr += __shfl_down(s.pr, off, AP_WAVE);
        s.pi += __shfl_down(s.pi, off, AP_WAVE);
        s.a += __shfl_down(s.a, off, AP_WAVE);
        s.b += __shfl_down(s.b, off, AP_WAVE);
    }
    if (lane == 0) co[i] = ap_quotient(s);
}

// The instrument's counts as volts: (double)c * 2.5 / 65536., then / divisor where the burst is a sum of chirps -- NumPy's
// `counts.astype(float) * 2.5 / 2**16.` and `/= n` (load_apres.py:391-395), operation for operation.  c 2.5 is exact (c has at
// most 32 bits, 2.5 two), / 65536 moves the exponent, and the last division is IEEE's, correctly rounded here as there.
template <typename T> __device__ __forceinline__ double ap_volts(T c, double divisor, int divide)
{
    const double v = (double)c * 2.5 / 65536.0;
    return divide ? v / divisor : v;
}

// One flat run of n counts.  `head` < 8 elements bring in + head to a 16-byte and out + head to a 64-byte boundary (the
// caller places the counts so that both hold at once); from there a thread takes AP_DEC_VEC counts in one (uint16) or
// two (uint32) 16-byte loads and writes them as four 16-byte stores.  The first block also does the head and the
// (n - head) % 8 elements of the tail, one element per thread.
template <typename T>
__global__ __launch_bounds__(AP_BLOCK) void ap_decode_kernel(const T *__restrict__ in, double *__restrict__ out, size_t n,
                                                             unsigned head, double divisor, int divide)
{
    const size_t body = (n - head) / AP_DEC_VEC;
    const size_t v = (size_t)blockIdx.x * AP_BLOCK + threadIdx.x;
    if (v < body) {
        union {
            uint4 q[sizeof(T) * AP_DEC_VEC / 16];
            T c[AP_DEC_VEC];
        } u;
        const T(&c)[AP_DEC_VEC] = u.c;
        const uint4 *src = reinterpret_cast<const uint4 *>(in + head + v * AP_DEC_VEC);
#pragma unroll
        for (unsigned q = 0; q < sizeof(u.q) / 16; ++q) u.q[q] = src[q];
        double2 *dst = reinterpret_cast<double2 *>(out + head + v * AP_DEC_VEC);
#pragma unroll
        for (int j = 0; j < AP_DEC_VEC / 2; ++j)
            dst[j] = make_double2(ap_volts(c[2 * j], divisor, divide), ap_volts(c[2 * j + 1], divisor, divide));
    }
    if (blockIdx.x == 0 && threadIdx.x < AP_DEC_VEC) {
        const size_t t = threadIdx.x, tail = head + body * AP_DEC_VEC + t;
        if (t < head) out[t] = ap_volts(in[t], divisor, divide);
        if (tail < n) out[tail] = ap_volts(in[tail], divisor, divide);
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct ApPlan {
    size_t N = 0, batch = 0;
    FftPlan fft;
};

struct ApBufs {
    DevBuf in[2], out[3], tab, pad, spec;          // staging of the host-buffer forms, host tables, one chunk's rows and spectra
    std::vector<std::unique_ptr<ApPlan>> plans;    // real-to-complex plans per (N, batch), oldest first
    std::vector<hipEvent_t> ev;                    // stage boundaries of the last range conversion (impdar_apres_range_last_ms)
    size_t ev_used = 0;
    DevBuf cnt;                                    // the decode's two slots of counts
    hipEvent_t dec_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // slot s uploaded: s, decoded: 2 + s; a call's start: 4
    void release()
    {
        for (DevBuf &b : in) b.release();
        for (DevBuf &b : out) b.release();
        tab.release();
        pad.release();
        spec.release();
        plans.clear();
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
        ev_used = 0;
        cnt.release();
        for (hipEvent_t &e : dec_ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
};
static StepScratch<ApBufs> g_ap;

void impdar_apres_forget(impdar_ctx *ctx) { g_ap.forget(ctx); }

static inline dim3 ap_grid(size_t count) { return dim3((unsigned)((count + AP_BLOCK - 1) / AP_BLOCK)); }

static int ap_plan(impdar_ctx *ctx, size_t N, size_t batch, FftPlan **out)
{
    for (auto &pl : g_ap.plans)
        if (pl->N == N && pl->batch == batch) {
            *out = &pl->fft;
            return IMPDAR_OK;
        }
    if (g_ap.plans.size() >= AP_MAX_PLANS) {
        IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the oldest plan's last transform may still be running
        g_ap.plans.erase(g_ap.plans.begin());
    }
    std::unique_ptr<ApPlan> pl(new ApPlan());
    pl->N = N;
    pl->batch = batch;
    const int rc = pl->fft.create(rocfft_transform_type_real_forward, true, false, N, batch, rocfft_array_type_real,
                                  rocfft_array_type_hermitian_interleaved, 1, N, 1, N / 2 + 1, 1.0, ctx->stream);
    if (rc) return rc;
    g_ap.plans.push_back(std::move(pl));
    *out = &g_ap.plans.back()->fft;
    return IMPDAR_OK;
}

static int ap_mark(impdar_ctx *ctx)
{
    if (g_ap.ev_used == g_ap.ev.size()) {
        hipEvent_t e = nullptr;
        IMPDAR_HIP_CHECK(hipEventCreate(&e));
        g_ap.ev.push_back(e);
    }
    IMPDAR_HIP_CHECK(hipEventRecord(g_ap.ev[g_ap.ev_used++], ctx->stream));
    return IMPDAR_OK;
}

static int range_check(impdar_ctx *ctx, const void *raw, int rows, int snum, int p, int n, const double *win, const double *comp,
                       const double *den, double scale_mul, double scale_div, int chunk, const void *spec, const void *data,
                       const void *rfine)
{
    IMPDAR_ARG_CHECK(ctx && raw && win && comp && den && rfine, "impdar_apres_range: null argument");
    IMPDAR_ARG_CHECK(rows >= 1, "impdar_apres_range: %d chirps", rows);
    IMPDAR_ARG_CHECK(snum >= 2, "impdar_apres_range: %d samples per chirp (a chirp needs 2)", snum);
    IMPDAR_ARG_CHECK(p >= 1, "impdar_apres_range: pad factor %d", p);
    IMPDAR_ARG_CHECK((long long)p * snum <= (1LL << 27), "impdar_apres_range: a padded chirp of %d x %d samples is too long", p, snum);
    const int nf = (int)(((long long)p * snum) / 2);
    IMPDAR_ARG_CHECK(n >= 0 && n <= nf, "impdar_apres_range: %d bins kept of the %d that pad factor %d recovers from %d samples", n,
                     nf, p, snum);
    IMPDAR_ARG_CHECK(n == 0 || (spec && data), "impdar_apres_range: null argument");
    IMPDAR_ARG_CHECK(chunk >= 0, "impdar_apres_range: a chunk of %d chirps", chunk);
    IMPDAR_ARG_CHECK(scale_mul == scale_mul && scale_div == scale_div && scale_div != 0.0,
                     "impdar_apres_range: scale %g / %g", scale_mul, scale_div);
    IMPDAR_ARG_CHECK((size_t)rows * nf <= (size_t)1 << 36, "impdar_apres_range: %d x %d is too large", rows, nf);
    return IMPDAR_OK;
}

extern "C" int impdar_apres_range_dev(impdar_ctx *ctx, const double *d_raw, int rows, int snum, int p, int n, const double *win,
                                      const double *comp, const double *den, double scale_mul, double scale_div,
                                      int first_order, double lambdac, int chunk, double *d_spec, double *d_data, double *d_rfine)
{
    const auto lock = g_ap.lock();
    int rc = range_check(ctx, d_raw, rows, snum, p, n, win, comp, den, scale_mul, scale_div, chunk, d_spec, d_data, d_rfine);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_ap.bind(ctx);
    const size_t N = (size_t)p * snum, nh = N / 2 + 1;
    const int nf = (int)(N / 2);
    if (chunk == 0) {
        // as many rows as the scratch budget holds, then evened out so that every chunk runs the same plan
        const size_t most = std::max<size_t>(1, AP_SCRATCH_BYTES / (N * 8 + nh * 16));
        const size_t pieces = ((size_t)rows + most - 1) / most;
        chunk = (int)(((size_t)rows + pieces - 1) / pieces);
    }
    if (chunk > rows) chunk = rows;
    const void *d_tab[3];
    rc = impdar_upload_tables(ctx, g_ap.tab, {{win, (size_t)snum * 8}, {comp, (size_t)nf * 16}, {den, (size_t)nf * 8}}, d_tab);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(g_ap.pad.ensure((size_t)chunk * N * 8));
    IMPDAR_HIP_CHECK(g_ap.spec.ensure((size_t)chunk * nh * 16));
    g_ap.ev_used = 0;
    rc = ap_mark(ctx);
    if (rc) return rc;
    for (int r0 = 0; r0 < rows; r0 += chunk) {
        const int now = rows - r0 < chunk ? rows - r0 : chunk;
        FftPlan *plan = nullptr;
        rc = ap_plan(ctx, N, (size_t)now, &plan);
        if (rc) return rc;
        hipLaunchKernelGGL(ar_prep_kernel, dim3((unsigned)now), dim3(AP_BLOCK), 0, ctx->stream, d_raw + (size_t)r0 * snum,
                           (const double *)d_tab[0], g_ap.pad.as<double>(), snum, (int)N);
        IMPDAR_HIP_CHECK(hipGetLastError());
        if ((rc = ap_mark(ctx))) return rc;
        if ((rc = plan->exec(g_ap.pad.p, g_ap.spec.p))) return rc;
        if ((rc = ap_mark(ctx))) return rc;
        hipLaunchKernelGGL(ar_post_kernel, ap_grid((size_t)now * nf), dim3(AP_BLOCK), 0, ctx->stream, g_ap.spec.as<double2>(),
                           (const double2 *)d_tab[1], (const double *)d_tab[2], (double2 *)d_spec, (double2 *)d_data, d_rfine, now,
                           (int)nh, nf, n, (size_t)r0, scale_mul, 1.0 / scale_div, first_order ? 1 : 0, lambdac);
        IMPDAR_HIP_CHECK(hipGetLastError());
        if ((rc = ap_mark(ctx))) return rc;
    }
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_apres_range_last_ms(impdar_ctx *ctx, float *prep_ms, float *fft_ms, float *post_ms)
{
    const auto lock = g_ap.lock();
    IMPDAR_ARG_CHECK(ctx && prep_ms && fft_ms && post_ms, "impdar_apres_range_last_ms: null argument");
    IMPDAR_ARG_CHECK(g_ap.owner == ctx && g_ap.ev_used >= 4, "no range conversion has run on this context");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    IMPDAR_HIP_CHECK(hipEventSynchronize(g_ap.ev[g_ap.ev_used - 1]));
    float sum[3] = {0.f, 0.f, 0.f};
    for (size_t e = 0; e + 1 < g_ap.ev_used; ++e) {
        float ms = 0.f;
        IMPDAR_HIP_CHECK(hipEventElapsedTime(&ms, g_ap.ev[e], g_ap.ev[e + 1]));
        sum[e % 3] += ms;
    }
    *prep_ms = sum[0], *fft_ms = sum[1], *post_ms = sum[2];
    return IMPDAR_OK;
}

static int stack_check(impdar_ctx *ctx, const void *data, int rows, int snum, int groups, int m, const void *out)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "impdar_apres_stack: null argument");
    IMPDAR_ARG_CHECK(rows >= 1 && snum >= 1, "impdar_apres_stack: %d chirps of %d samples", rows, snum);
    IMPDAR_ARG_CHECK(groups >= 1 && m >= 1, "impdar_apres_stack: %d means over %d chirps", groups, m);
    IMPDAR_ARG_CHECK((long long)groups * m <= rows, "impdar_apres_stack: %d means over %d chirps need more than the %d there are",
                     groups, m, rows);
    IMPDAR_ARG_CHECK((size_t)rows * snum <= (size_t)1 << 36, "impdar_apres_stack: %d x %d is too large", rows, snum);
    return IMPDAR_OK;
}

extern "C" int impdar_apres_stack_dev(impdar_ctx *ctx, const double *d_data, int is_complex, int rows, int snum, int groups, int m,
                                      double *d_out)
{
    const auto lock = g_ap.lock();
    const int rc = stack_check(ctx, d_data, rows, snum, groups, m, d_out);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_ap.bind(ctx);
    const int width = is_complex ? 2 * snum : snum;
    hipLaunchKernelGGL(ap_stack_kernel, ap_grid((size_t)groups * width), dim3(AP_BLOCK), 0, ctx->stream, d_data, d_out, width,
                       groups, m, is_complex ? 1 : 0);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// windows of numpy.arange(win / 2, len - win / 2, step)
static long long ap_windows(int len, int win, int step)
{
    const long long h = win / 2, span = (long long)len - 2 * h;
    return span > 0 ? (span + step - 1) / step : 0;
}

static int phase_diff_check(impdar_ctx *ctx, const void *s1, const void *s2, int len, int win, int step, const void *co)
{
    IMPDAR_ARG_CHECK(ctx && s1 && s2, "impdar_apres_phase_diff: null argument");
    IMPDAR_ARG_CHECK(len >= 1, "impdar_apres_phase_diff: %d samples", len);
    IMPDAR_ARG_CHECK(win >= 0 && step >= 1, "impdar_apres_phase_diff: window %d, step %d", win, step);
    IMPDAR_ARG_CHECK(co || ap_windows(len, win, step) == 0, "impdar_apres_phase_diff: null argument");
    return IMPDAR_OK;
}

extern "C" int impdar_apres_phase_diff_dev(impdar_ctx *ctx, const double *d_s1, const double *d_s2, int len, int win, int step,
                                           double *d_co)
{
    const auto lock = g_ap.lock();
    const int rc = phase_diff_check(ctx, d_s1, d_s2, len, win, step, d_co);
    if (rc) return rc;
    const int nwin = (int)ap_windows(len, win, step), terms = 2 * (win / 2);
    if (nwin == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_ap.bind(ctx);
    // the last window ends at (nwin - 1) step + terms <= len: the first sample of window i is i step, and i step + win / 2 < len - win / 2
    if (terms <= AP_PD_THREAD_MAX)
        hipLaunchKernelGGL(ap_phase_diff_thread_kernel, ap_grid((size_t)nwin), dim3(AP_BLOCK), 0, ctx->stream, (const double2 *)d_s1,
                           (const double2 *)d_s2, (double2 *)d_co, nwin, terms, step);
    else
        hipLaunchKernelGGL(ap_phase_diff_wave_kernel, ap_grid((size_t)nwin * AP_WAVE), dim3(AP_BLOCK), 0, ctx->stream,
                           (const double2 *)d_s1, (const double2 *)d_s2, (double2 *)d_co, nwin, terms, step);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer forms ---------------------------------------------------------------------------------------

extern "C" int impdar_apres_range(impdar_ctx *ctx, const double *raw, int rows, int snum, int p, int n, const double *win,
                                  const double *comp, const double *den, double scale_mul, double scale_div, int first_order,
                                  double lambdac, int chunk, double *spec, double *data, double *rfine)
{
    int rc = range_check(ctx, raw, rows, snum, p, n, win, comp, den, scale_mul, scale_div, chunk, spec, data, rfine);
    if (rc) return rc;
    const auto held = g_ap.lock();
    const size_t nf = ((size_t)p * snum) / 2, kept = (size_t)rows * n * 16, fine = (size_t)rows * nf * 8;
    rc = g_ap.stage_in(ctx, g_ap.in[0], raw, (size_t)rows * snum * 8);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(g_ap.out[0].ensure(kept ? kept : 16));
    IMPDAR_HIP_CHECK(g_ap.out[1].ensure(kept ? kept : 16));
    IMPDAR_HIP_CHECK(g_ap.out[2].ensure(fine));
    rc = impdar_apres_range_dev(ctx, g_ap.in[0].as<double>(), rows, snum, p, n, win, comp, den, scale_mul, scale_div, first_order,
                                lambdac, chunk, g_ap.out[0].as<double>(), g_ap.out[1].as<double>(), g_ap.out[2].as<double>());
    if (!rc && kept) rc = impdar_download(ctx, spec, g_ap.out[0].p, kept, ctx->stream);
    if (!rc && kept) rc = impdar_download(ctx, data, g_ap.out[1].p, kept, ctx->stream);
    if (!rc) rc = impdar_download(ctx, rfine, g_ap.out[2].p, fine, ctx->stream);
    return rc;
}

extern "C" int impdar_apres_stack(impdar_ctx *ctx, const double *data, int is_complex, int rows, int snum, int groups, int m,
                                  double *out)
{
    const int rc = stack_check(ctx, data, rows, snum, groups, m, out);
    if (rc) return rc;
    const size_t el = is_complex ? 16 : 8;
    // only the rows that are read go up
    return g_ap.host_form(ctx, g_ap.in[0], data, (size_t)groups * m * snum * el, &g_ap.out[0], out, (size_t)groups * snum * el,
                          [&](void *d_in, void *d_out) {
                              return impdar_apres_stack_dev(ctx, (const double *)d_in, is_complex, rows, snum, groups, m,
                                                            (double *)d_out);
                          });
}

extern "C" int impdar_apres_phase_diff(impdar_ctx *ctx, const double *s1, const double *s2, int len, int win, int step, double *co)
{
    int rc = phase_diff_check(ctx, s1, s2, len, win, step, co);
    if (rc) return rc;
    const size_t nwin = (size_t)ap_windows(len, win, step);
    if (nwin == 0) return IMPDAR_OK;
    const auto held = g_ap.lock();
    rc = g_ap.stage_in(ctx, g_ap.in[0], s1, (size_t)len * 16);
    if (!rc) rc = g_ap.stage_in(ctx, g_ap.in[1], s2, (size_t)len * 16);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(g_ap.out[0].ensure(nwin * 16));
    rc = impdar_apres_phase_diff_dev(ctx, g_ap.in[0].as<double>(), g_ap.in[1].as<double>(), len, win, step, g_ap.out[0].as<double>());
    if (rc) return rc;
    return impdar_download(ctx, co, g_ap.out[0].p, nwin * 16, ctx->stream);
}

// ---- the instrument's counts to volts ----------------------------------------------------------------------------

static int decode_check(impdar_ctx *ctx, const void *counts, int kind, long long n, double divisor, const void *volts)
{
    IMPDAR_ARG_CHECK(ctx, "impdar_apres_decode: null context");
    IMPDAR_ARG_CHECK(n >= 0 && n <= (1LL << 36), "impdar_apres_decode: %lld counts", n);
    IMPDAR_ARG_CHECK(kind == 0 || kind == 1, "impdar_apres_decode: kind %d (0: uint16, 1: uint32)", kind);
    IMPDAR_ARG_CHECK(divisor > 0.0 && divisor <= 1.7976931348623157e308, "impdar_apres_decode: divisor %g", divisor);
    IMPDAR_ARG_CHECK(n == 0 || (counts && volts), "impdar_apres_decode: null argument");
    return IMPDAR_OK;
}

// Piece i of the counts: host memcpy into slot i % 2 of the context's pinned staging buffer (the counts sit at any
// byte offset of a file's image), a copy on the producer stream to slot i % 2 of g_ap.cnt, the kernel on the compute
// stream after it: the kernel of piece i runs under the copy of piece i + 1.  Inside its slot a piece starts as many
// elements past a 16-byte boundary as its first output element lies past a 64-byte one.
static int decode_pieces(impdar_ctx *ctx, const char *counts, char *stage, size_t el, size_t total, size_t piece, size_t slot,
                         double divisor, double *d_volts)
{
    const int divide = divisor != 1.0;
    int rk = IMPDAR_OK;
    size_t i = 0;
    for (size_t off = 0; off < total; off += piece, ++i) {
        const size_t now = std::min(piece, total - off), s = i & 1;
        double *out = d_volts + off;
        const size_t phase = ((uintptr_t)out / 8) % AP_DEC_VEC;
        const unsigned head = (unsigned)std::min<size_t>((AP_DEC_VEC - phase) % AP_DEC_VEC, now);
        char *d_in = g_ap.cnt.as<char>() + s * slot + phase * el;
        const char *src = counts + off * el;
        if (i >= 2) {
            IMPDAR_HIP_CHECK(hipEventSynchronize(g_ap.dec_ev[s]));                       // the pinned slot has gone up
            IMPDAR_HIP_CHECK(hipStreamWaitEvent(ctx->aux, g_ap.dec_ev[2 + s], 0));       // the device slot has been read
        }
        if (stage) {
            memcpy(stage + s * slot, src, now * el);
            src = stage + s * slot;
        }
        IMPDAR_HIP_CHECK(hipMemcpyAsync(d_in, src, now * el, hipMemcpyHostToDevice, ctx->aux));
        IMPDAR_HIP_CHECK(hipEventRecord(g_ap.dec_ev[s], ctx->aux));
        IMPDAR_HIP_CHECK(hipStreamWaitEvent(ctx->stream, g_ap.dec_ev[s], 0));
        const dim3 grid = ap_grid(std::max<size_t>((now - head) / AP_DEC_VEC, 1));
        if (i == 0 && (rk = impdar_ctx_ktic(ctx))) return rk;    // first kernel's start to last kernel's end: impdar_ctx_last_kernel_ms
        if (el == 4)
            hipLaunchKernelGGL(ap_decode_kernel<uint32_t>, grid, dim3(AP_BLOCK), 0, ctx->stream, (const uint32_t *)d_in, out, now, head,
                               divisor, divide);
        else
            hipLaunchKernelGGL(ap_decode_kernel<uint16_t>, grid, dim3(AP_BLOCK), 0, ctx->stream, (const uint16_t *)d_in, out, now, head,
                               divisor, divide);
        IMPDAR_HIP_CHECK(hipGetLastError());
        IMPDAR_HIP_CHECK(hipEventRecord(g_ap.dec_ev[2 + s], ctx->stream));
    }
    return impdar_ctx_ktoc(ctx);
}

// `piece` counts go up at a time, 0 for AP_DEC_PIECE_BYTES of them (the argument is for tests and for timing the kernel alone)
extern "C" int impdar_apres_decode_pieces_dev(impdar_ctx *ctx, const void *counts, int kind, long long n, double divisor,
                                              void *d_volts, long long piece_counts)
{
    const auto lock = g_ap.lock();
    const int rc = decode_check(ctx, counts, kind, n, divisor, d_volts);
    if (rc) return rc;
    IMPDAR_ARG_CHECK(((uintptr_t)d_volts & 7) == 0, "impdar_apres_decode: the output is not aligned to 8 bytes");
    IMPDAR_ARG_CHECK(piece_counts >= 0, "impdar_apres_decode: pieces of %lld counts", piece_counts);
    if (n == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_ap.bind(ctx);
    const size_t el = kind ? 4 : 2, total = (size_t)n;
    size_t piece = piece_counts ? (size_t)piece_counts : AP_DEC_PIECE_BYTES / el;
    piece = std::min(piece, total);
    piece = (piece + AP_DEC_VEC - 1) / AP_DEC_VEC * AP_DEC_VEC;          // every piece starts at the same phase of the output
    const size_t slot = ((piece + AP_DEC_VEC) * el + 255) & ~(size_t)255;
    IMPDAR_HIP_CHECK(g_ap.cnt.ensure(2 * slot));
    for (hipEvent_t &e : g_ap.dec_ev)
        if (!e) IMPDAR_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    std::lock_guard<std::mutex> pin(ctx->pinned_mu);
    char *stage = reinterpret_cast<char *>(impdar_ctx_pinned(ctx, 2 * slot));   // (null: straight from the caller's memory)
    // an earlier call's kernels may still read the slots
    IMPDAR_HIP_CHECK(hipEventRecord(g_ap.dec_ev[4], ctx->stream));
    IMPDAR_HIP_CHECK(hipStreamWaitEvent(ctx->aux, g_ap.dec_ev[4], 0));
    const int rp = decode_pieces(ctx, reinterpret_cast<const char *>(counts), stage, el, total, piece, slot, divisor,
                                 reinterpret_cast<double *>(d_volts));
    // Whatever became of the pieces, their copies leave the pinned slots and the caller's counts before pinned_mu is
    // released and this call returns: another call may overwrite or free that buffer.
    const hipError_t drained = hipStreamSynchronize(ctx->aux);
    if (rp) return rp;
    IMPDAR_HIP_CHECK(drained);
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_apres_decode_dev(impdar_ctx *ctx, const void *counts, int kind, long long n, double divisor, void *d_volts)
{
    return impdar_apres_decode_pieces_dev(ctx, counts, kind, n, divisor, d_volts, 0);
}

extern "C" int impdar_apres_decode(impdar_ctx *ctx, const void *counts, int kind, long long n, double divisor, double *volts)
{
    const int rc = decode_check(ctx, counts, kind, n, divisor, volts);
    if (rc || n == 0) return rc;
    const auto held = g_ap.lock();
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_ap.bind(ctx);
    IMPDAR_HIP_CHECK(g_ap.out[0].ensure((size_t)n * 8));
    const int rd = impdar_apres_decode_dev(ctx, counts, kind, n, divisor, g_ap.out[0].p);
    if (rd) return rd;
    return impdar_download(ctx, volts, g_ap.out[0].p, (size_t)n * 8, ctx->stream);
}
