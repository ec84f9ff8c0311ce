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
#include "fft.h"
#include "own_fft.h"
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <unistd.h>

static std::once_flag g_fft_once;
static int g_fft_rc = IMPDAR_OK;

int impdar_fft_global_setup()
{
    std::call_once(g_fft_once, [] {
        // rocFFT keeps the kernels of the plans it has built in a small user database; without one every new process
        // fetches them again from the 1.8 GB system database (0.25 s per plan with that file in the page cache, up to
        // 1.7 s from a cold disk: profiles/r05_first_call.txt) instead of 25 ms.  Where the user has not chosen a place
        // (ROCFFT_RTC_CACHE_PATH) and rocFFT's own default is not writable ($HOME on a batch node), give it one.
        if (!getenv("ROCFFT_RTC_CACHE_PATH")) {
            std::string dir;
            const char *xdg = getenv("XDG_CACHE_HOME"), *home = getenv("HOME");
            auto usable = [](const std::string &d) {
                if (d.empty()) return false;
                (void)mkdir(d.c_str(), 0700);
                return access(d.c_str(), W_OK | X_OK) == 0;
            };
            if (xdg && *xdg && usable(xdg)) dir = std::string(xdg) + "/impdar_amd";
            else if (home && *home && usable(std::string(home) + "/.cache")) dir = std::string(home) + "/.cache/impdar_amd";
            else dir = "/tmp/impdar_amd-" + std::to_string((long)getuid());
            if (usable(dir)) {
                const std::string path = dir + "/rocfft_kernel_cache.db";
                (void)setenv("ROCFFT_RTC_CACHE_PATH", path.c_str(), 0);
                impdar_trace("rocFFT user kernel cache: %s", path.c_str());
            }
        }
        impdar_trace("rocfft_setup: start");
        if (rocfft_setup() != rocfft_status_success) {
            g_fft_rc = IMPDAR_ERR_FFT;
        }
        impdar_trace("rocfft_setup: done");
    });
    if (g_fft_rc) impdar_set_error("rocfft_setup failed");
    return g_fft_rc;
}

std::mutex &impdar_fft_plan_mutex()
{
    static std::mutex mu;
    return mu;
}

// any: lengths 2^a 3^b 5^c 7^d too (impdar_fft_rows_any_dev)
static int fft_rows_dev(impdar_ctx *ctx, bool any, int mode, int dtype, int n, int batch, const void *d_in, void *d_out, double scale)
{
    IMPDAR_ARG_CHECK(ctx && d_in && d_out, "null argument");
    IMPDAR_ARG_CHECK(mode >= 0 && mode <= 4 && (dtype == IMPDAR_F32 || dtype == IMPDAR_F64) && batch >= 1, "bad mode / dtype / batch");
    const bool real = mode == OWN_R2C || mode == OWN_C2R;
    const int M = real ? n / 2 : n;
    const bool pow2 = n >= 2 && (n & (n - 1)) == 0 && own_fft_len_ok(M);
    if (any)
        IMPDAR_ARG_CHECK(pow2 || (n >= 2 && !(real && n % 2) && own_fft_mixed_len_ok(M)),
                         "length %d: the complex length must be 16 .. 8192 with no prime factor above 7 (a real length even)", n);
    else
        IMPDAR_ARG_CHECK(pow2, "length %d is not a power of two in range", n);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    OwnTwiddles tw;
    int rc;
    const size_t cin = mode == OWN_R2C ? (size_t)n : (mode == OWN_C2R ? (size_t)M + 1 : (size_t)n);
    const size_t cout = mode == OWN_R2C ? (size_t)M + 1 : (size_t)n;
    if (dtype == IMPDAR_F32) {
        if ((rc = tw.ensure<float>(n, ctx->stream))) return rc;
        rc = own_fft_launch<float>(mode, n, (size_t)batch, d_in, d_out, cin, cout, scale, tw, ctx->stream);
    } else {
        if ((rc = tw.ensure<double>(n, ctx->stream))) return rc;
        rc = own_fft_launch<double>(mode, n, (size_t)batch, d_in, d_out, cin, cout, scale, tw, ctx->stream);
    }
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));         // (the table is this call's)
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_fft_rows_dev(impdar_ctx *ctx, int mode, int dtype, int n, int batch, const void *d_in, void *d_out, double scale)
{
    return fft_rows_dev(ctx, false, mode, dtype, n, batch, d_in, d_out, scale);
}

extern "C" int impdar_fft_rows_any_dev(impdar_ctx *ctx, int mode, int dtype, int n, int batch, const void *d_in, void *d_out, double scale)
{
    return fft_rows_dev(ctx, true, mode, dtype, n, batch, d_in, d_out, scale);
}

template <typename T> struct Cx { T x, y; };

// (snum,tnum) row-major -> tapered, transposed X[tnum][snum]
template <typename T>
__global__ __launch_bounds__(256) void stolt_taper_transpose(const T *__restrict__ in, T *__restrict__ X, int snum,
                                                             int tnum, double htaper, double vtaper, int do_taper)
{
    __shared__ T tile[64][65];
    const int k0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    // the trace weight is the thread's own for all of its rows; the 64 sample weights of the tile are computed once
    // (two float64 divisions per element were most of this kernel's time)
    __shared__ double wrow[64];
    if (threadIdx.x < 64) wrow[threadIdx.x] = impdar_taper_w(min(k0 + (int)threadIdx.x, snum - 1), snum, vtaper);
    const double h = impdar_taper_w(min(j0 + tx, tnum - 1), tnum, htaper);
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, j = j0 + tx;
        T v = 0;
        if (k < snum && j < tnum) {
            v = in[(size_t)k * tnum + j];
            if (do_taper) v = (T)(((double)v * h) * wrow[r]);      // (data*H)*V then astype(dtype), :157
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, k = k0 + tx;
        if (j < tnum && k < snum) X[(size_t)j * snum + k] = tile[tx][r];
    }
}

// Y[tnum][nout] -> out (nout,tnum) row-major
template <typename T>
__global__ __launch_bounds__(256) void stolt_transpose_back(const T *__restrict__ Y, T *__restrict__ out, int nout,
                                                            int tnum)
{
    __shared__ T tile[64][65];
    const int k0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, k = k0 + tx;
        tile[r][tx] = (j < tnum && k < nout) ? Y[(size_t)j * nout + k] : (T)0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, j = j0 + tx;
        if (k < nout && j < tnum) out[(size_t)k * tnum + j] = tile[tx][r];
    }
}

// The Stolt stretch of one output point (zj, |kx|): between which knots of the frequency axis it interpolates, with which
// weight, and its obliquity factor.  The one statement of this arithmetic: every stretch kernel below calls it.
struct StoltKnot {
    int i0;
    double w, sc;
};
__device__ __forceinline__ StoltKnot stolt_knot(const double *__restrict__ ws, double kxi, int zj, int m, double vel)
{
    const double kz = ws[zj] * 2.0 / vel;                       // :180
    const double kk = sqrt(kz * kz + kxi * kxi);                // :188 and :196 (kx^2 + kz^2: the same sum)
    double wq = vel / 2.0 * kk;
    const double wlast = ws[m - 1];
    if (wq > wlast) wq = wlast;                                 // FITPACK clamps to the last knot
    const double dw = ws[1] - ws[0];
    int i0 = (int)floor(wq / dw);
    i0 = min(max(i0, 0), m - 2);
    while (i0 > 0 && ws[i0] > wq) --i0;
    while (i0 < m - 2 && ws[i0 + 1] <= wq) ++i0;
    StoltKnot k;
    k.i0 = i0;
    k.w = (wq - ws[i0]) / (ws[i0 + 1] - ws[i0]);
    k.sc = kz / kk;                                             // :196
    return k;
}
// the interpolated value is stored into the (complex64/128) array, then scaled in place in double and rounded again (:190, :198)
template <typename T> __device__ __forceinline__ Cx<T> stolt_mix(const Cx<T> a, const Cx<T> b, const StoltKnot k)
{
    const T re = (T)((1.0 - k.w) * (double)a.x + k.w * (double)b.x);
    const T im = (T)((1.0 - k.w) * (double)a.y + k.w * (double)b.y);
    Cx<T> o;
    o.x = (T)((double)re * k.sc);
    o.y = (T)((double)im * k.sc);
    return o;
}

// Stolt stretch + obliquity.  One thread per (xi, zj); zj is the fast index so
// loads of F[xi][i0], F[xi][i0+1] walk monotonically along a contiguous row.
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch(const Cx<T> *__restrict__ F, Cx<T> *__restrict__ K,
                                                     const double *__restrict__ kx, const double *__restrict__ ws,
                                                     int m, int nz, int tnum, double vel)
{
    const int zj = blockIdx.x * 256 + threadIdx.x;
    const int xi = blockIdx.y;
    if (zj >= m) return;
    Cx<T> o;
    o.x = 0;
    o.y = 0;
    if (zj < nz) {
        const StoltKnot k = stolt_knot(ws, kx[xi], zj, m, vel);
        o = stolt_mix<T>(F[(size_t)xi * m + k.i0], F[(size_t)xi * m + k.i0 + 1], k);
        if (zj == 0 && xi == 0) {                                   // :200
            o.x = 0;
            o.y = 0;
        }
    }
    K[(size_t)xi * m + zj] = o;
}

// The same on the spectrum as the own transforms leave it after the pass over the traces: frequency-major, F[w][kx].  One
// thread per (zj, xi) with xi the fast index: the two rows a wavenumber interpolates between move slowly with xi (kk grows
// with |kx|), so neighbouring lanes read neighbouring words of the same or the next row -- no transposes around the stretch.
template <typename T>
__device__ __forceinline__ void stolt_point_t(const Cx<T> *__restrict__ F, Cx<T> *__restrict__ K, const double *__restrict__ kx,
                                              const double *__restrict__ ws, int m, int nz, int tnum, double vel, int xi, int zj)
{
    Cx<T> o;
    o.x = 0;
    o.y = 0;
    if (zj < nz) {
        const StoltKnot k = stolt_knot(ws, kx[xi], zj, m, vel);
        o = stolt_mix<T>(F[(size_t)k.i0 * tnum + xi], F[(size_t)(k.i0 + 1) * tnum + xi], k);
        if (zj == 0 && xi == 0) {                                   // :200
            o.x = 0;
            o.y = 0;
        }
    }
    K[(size_t)zj * tnum + xi] = o;
}
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch_t(const Cx<T> *__restrict__ F, Cx<T> *__restrict__ K,
                                                       const double *__restrict__ kx, const double *__restrict__ ws,
                                                       int m, int nz, int tnum, double vel)
{
    const int xi = blockIdx.x * 256 + threadIdx.x;
    if (xi >= tnum) return;
    stolt_point_t<T>(F, K, kx, ws, m, nz, tnum, vel, xi, blockIdx.y);
}

// The same on the spectrum as [kx >= 0][all frequencies] (round 6: the transform over the traces taken first, on the radargram's own
// rows; rows k = 0 .. tnum/2 of snum complex numbers in FFT order).  irfft2 (:202) extends KK Hermitian-wise, KK[-w][kx] =
// conj KK[w][-kx], and conj FK[i][-kx] = FK[-i][kx] for a real radargram: the negative-frequency half of row kx is the same
// interpolation, with the same weights (they depend on |kx| only), between the mirrored knots of the SAME row.  One thread per
// (kx, zj), zj the fast index; the zero-frequency and Nyquist rows of KK are zero (kz = 0 scales the first to zero, :196; KK[:nz]
// alone is filled, :190), so numpy's dropping of their imaginary parts has nothing to drop.
template <typename T>
__device__ __forceinline__ void stolt_point_rows(const Cx<T> *__restrict__ B, Cx<T> *__restrict__ K, const double *__restrict__ kx,
                                                 const double *__restrict__ ws, int m, int nz, int snum, double vel, int xi, int zj)
{
    const Cx<T> *row = B + (size_t)xi * snum;
    Cx<T> *orow = K + (size_t)xi * snum;
    Cx<T> o, om;
    o.x = o.y = om.x = om.y = 0;
    if (zj < nz) {
        const StoltKnot k = stolt_knot(ws, kx[xi], zj, m, vel);
        o = stolt_mix<T>(row[k.i0], row[k.i0 + 1], k);
        if (zj > 0) om = stolt_mix<T>(row[k.i0 == 0 ? 0 : snum - k.i0], row[snum - k.i0 - 1], k);
        if (zj == 0 && xi == 0) {                                   // :200
            o.x = 0;
            o.y = 0;
        }
    }
    orow[zj] = o;                                                   // (zj = nz: the Nyquist row, zero)
    if (zj > 0 && zj < nz) orow[snum - zj] = om;
}
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch_rows(const Cx<T> *__restrict__ B, Cx<T> *__restrict__ K,
                                                          const double *__restrict__ kx, const double *__restrict__ ws,
                                                          int m, int nz, int snum, double vel)
{
    const int zj = blockIdx.x * 256 + threadIdx.x;
    if (zj > nz) return;
    stolt_point_rows<T>(B, K, kx, ws, m, nz, snum, vel, blockIdx.y, zj);
}

// The velocity scan's stretch (impdar_stolt_scan): ONE spectrum, as the forward half of a call leaves it, stretched at nb velocities
// into nb spectra [nb][plane].  Grid z is the velocity and the slowest index of the dispatch: a plane's blocks walk the shared
// spectrum front to back like a single call's, and the next plane re-reads it one plane of output later (the
// reuse distance is spectrum + one plane, inside the 256 MiB Infinity Cache up to 4096 x 4096 float32; small sizes stay in L2).
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch_scan_rows(const Cx<T> *__restrict__ B, Cx<T> *__restrict__ K,
                                                               const double *__restrict__ kx, const double *__restrict__ ws,
                                                               const double *__restrict__ vels, int m, int nz, int snum, size_t plane)
{
    const int zj = blockIdx.x * 256 + threadIdx.x;
    if (zj > nz) return;
    stolt_point_rows<T>(B, K + (size_t)blockIdx.z * plane, kx, ws, m, nz, snum, vels[blockIdx.z], blockIdx.y, zj);
}
template <typename T>
__global__ __launch_bounds__(256) void stolt_stretch_scan_t(const Cx<T> *__restrict__ F, Cx<T> *__restrict__ K,
                                                            const double *__restrict__ kx, const double *__restrict__ ws,
                                                            const double *__restrict__ vels, int m, int nz, int tnum, size_t plane)
{
    const int xi = blockIdx.x * 256 + threadIdx.x;
    if (xi >= tnum) return;
    stolt_point_t<T>(F, K + (size_t)blockIdx.z * plane, kx, ws, m, nz, tnum, vels[blockIdx.z], xi, blockIdx.y);
}

// Focus measures of the scan's images Y[nb][nout][tnum]: sum |x|, sum x^2, sum x^4 (x^4 = (x^2)^2) over the traces t0 <= j < t1
// of every row, in float64 -> sums[b][k][3].  One workgroup per (row, velocity).  The order of the additions is a function of the
// trace index alone -- the V = 16 / sizeof(T) traces of group g = j / V go to thread g % 256 in rising order, then a butterfly
// over the wave, then the four waves' partials in wave order -- so a row's sums do not depend on where its image lies in the
// batch, and two calls give the same bits.  A whole group inside the window is one 16-byte load where the row is 16-byte
// aligned; heads, tails and unaligned rows load the same traces one by one.  NaN and Inf propagate as in NumPy.
template <typename T>
__global__ __launch_bounds__(256) void stolt_focus_rows(const T *__restrict__ Y, double *__restrict__ sums, int nout, int tnum,
                                                        int t0, int t1)
{
    constexpr int V = 16 / sizeof(T);
    struct alignas(16) Vec { T v[V]; };
    const T *row = Y + ((size_t)blockIdx.y * nout + blockIdx.x) * tnum;
    const bool aligned = (reinterpret_cast<size_t>(row) & 15) == 0;
    double s1 = 0.0, s2 = 0.0, s4 = 0.0;
    for (int g = t0 / V + (int)threadIdx.x; g * V < t1; g += 256) {
        const int j = g * V;
        const bool whole = j >= t0 && j + V <= t1;
        Vec q;
        if (whole && aligned) {
            q = *reinterpret_cast<const Vec *>(row + j);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) q.v[e] = (j + e >= t0 && j + e < t1) ? row[j + e] : (T)0;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (whole || (j + e >= t0 && j + e < t1)) {
                const double x = (double)q.v[e];
                const double x2 = x * x;
                s1 += fabs(x);
                s2 += x2;
                s4 += x2 * x2;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
        s4 += __shfl_xor(s4, off);
    }
    __shared__ double part[4][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = s1;
        part[wave][1] = s2;
        part[wave][2] = s4;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = part[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) s += part[w][threadIdx.x];
        sums[((size_t)blockIdx.y * nout + blockIdx.x) * 3 + threadIdx.x] = s;
    }
}

// C2R ignores the imaginary part of the DC and Nyquist bins (numpy irfft):
// clear them so any Hermitian-assuming backend agrees.
template <typename T>
__global__ void stolt_fix_hermitian(Cx<T> *K, int m, int tnum)
{
    const int xi = blockIdx.x * 256 + threadIdx.x;
    if (xi >= tnum) return;
    K[(size_t)xi * m].y = 0;
    K[(size_t)xi * m + m - 1].y = 0;
}

struct StoltPlan {
    // power-of-two sizes run on the library's own row transforms (own_fft.h) and need no rocFFT plan
    bool plans_ready = false;
    int own_calls = 0;
    OwnTwiddles tw_time, tw_trace;
    int dtype = -1, snum = 0, tnum = 0;
    const impdar_ctx *owner = nullptr;   // plans and buffers live on this context's device and stream
    FftPlan r2c, c2c_f, c2c_b, c2r;     // separate passes (IMPDAR_STOLT_FFT=1d)
    FftPlan fwd2d, inv2d;               // the same two pairs as 2-D real transforms (default)
    bool use2d = true, no_own = false;
    int route = -1;                     // StoltRoute of the call the plans and buffers were made for
    DevBuf X, F, K, Y, d_kx, d_ws;
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
    void release_scan()
    {
        S1.release(); S2.release(); img.release(); d_vels.release(); d_sums.release();
        for (hipEvent_t e : scan_ev) (void)hipEventDestroy(e);
        scan_ev.clear();
        scan_batches = 0;
    }
    ~StoltPlan() { release_scan(); }
};

static std::mutex g_stolt_mu;
static StoltPlan *g_stolt_plan = nullptr;     // last-used plan (sizes repeat across calls)

// called by impdar_ctx_destroy: a cached plan must not outlive the stream it was created on
// impdar_release_caches: out of device memory somewhere -- drop the cached plan unless a Stolt call is using it
static thread_local bool t_stolt_busy = false;
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
    if (g_stolt_plan && g_stolt_plan->owner == ctx) {
        delete g_stolt_plan;
        g_stolt_plan = nullptr;
    }
}

// Which transforms a call runs on.  Both forms of the own transforms need snum even.
//   rows ("traces first", seven passes): R2C / C2R over the traces (complex length tnum / 2) and C2C of snum over time, on the
//     wavenumbers k = 0 .. tnum / 2 alone, which holds the other half through kx[k] == -kx[tnum - k]; tnum >= 64
//   [w][kx] (ten passes): R2C / C2R over time (complex length snum / 2), C2C of tnum over the traces; tnum may be odd
// Power-of-two sizes keep the gate they had (the [w][kx] lengths decide, the rows form where snum fits too).  Any other size
// takes the own transforms where the mixed-radix kernel has the lengths of a form (own_fft_mixed_plan.h), the rows form first --
// by default only where rocFFT would compile kernels at run time (a length above 1024); IMPDAR_STOLT_FFT=mixed: wherever
// the lengths allow.
enum StoltRoute { STOLT_ROCFFT = 0, STOLT_OWN_WKX = 1, STOLT_OWN_ROWS = 2 };
static inline bool stolt_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
static StoltRoute stolt_route(int snum, int tnum, const double *kx, bool want_mixed)
{
    if (snum % 2) return STOLT_ROCFFT;
    if (stolt_pow2(snum) && stolt_pow2(tnum)) {
        if (!(own_fft_len_ok(snum / 2) && own_fft_len_ok(tnum))) return STOLT_ROCFFT;
        return own_fft_len_ok(snum) && tnum >= 64 ? STOLT_OWN_ROWS : STOLT_OWN_WKX;
    }
    if (!(want_mixed || snum > 1024 || tnum > 1024)) return STOLT_ROCFFT;
    auto len_ok = [](int M) { return own_fft_len_ok(M) || own_fft_mixed_len_ok(M); };
    if (tnum % 2 == 0 && tnum >= 64 && len_ok(tnum / 2) && len_ok(snum)) {
        bool antisym = true;
        for (int k = 1; k < tnum / 2 && antisym; ++k) antisym = kx[k] == -kx[tnum - k];
        if (antisym) return STOLT_OWN_ROWS;
    }
    return len_ok(snum / 2) && len_ok(tnum) ? STOLT_OWN_WKX : STOLT_ROCFFT;
}

// What the stages of one call share: the sizes, the route and what follows from it.
struct StoltCall {
    int snum, tnum, m, nz, nout;
    StoltRoute route;
    bool use_own, mixed;    // mixed: a transform of the call runs on the mixed-radix kernel (the metrics line says so)
    int do_taper;
    double htaper, vtaper;
};

// A call in three stages, shared by the single migration (stolt_run) and the velocity scan (stolt_scan_run):
//   stolt_prepare  plans, buffers and twiddles for the size; kx and ws to the device
//   stolt_front    everything that does not depend on the velocity: taper, forward transforms; the spectrum is left in
//                  pl.K (own transforms: [kx >= 0][w] on the rows route, [w][kx] on the other) or pl.F (rocFFT: [kx][w])
//   stolt_back     stretch at one velocity, inverse transforms, the image into d_out (pl.K is overwritten on the own routes)
template <typename T>
static int stolt_prepare(impdar_ctx *ctx, StoltPlan &pl, int snum, int tnum, const double *kx, const double *ws, double htaper,
                         double vtaper, StoltCall &c)
{
    const int m = snum / 2 + 1, nout = 2 * (snum / 2);
    hipStream_t st = ctx->stream;
    const bool dbl = sizeof(T) == 8;
    bool want2d = true, no_own = false, want_mixed = false;
    {
        // tuning knob: "1d" = four 1-D rocFFT passes; "rocfft" = rocFFT's 2-D real plans also where the own transforms apply;
        // "own" = the default, spelled out (tests that pin one implementation); "mixed" = the own mixed-radix transforms at
        // every size they take, not only where rocFFT has kernels to compile
        const char *e = getenv("IMPDAR_STOLT_FFT");
        want2d = !(e && !strcmp(e, "1d"));
        no_own = e && !strcmp(e, "rocfft");
        want_mixed = e && !strcmp(e, "mixed");
    }
    // power-of-two sizes run on the library's own row transforms (own_fft.h), every call: 0.35 ms at 4096^2 against 0.37 on
    // rocFFT's 2-D plans (round 5: the stretch on the frequency-major spectrum, two transposes fewer), nothing compiled at
    // run time, no plan to make (rocFFT: 0.3-3 s per process for lengths above 1024)
    const StoltRoute route = want2d && !no_own ? stolt_route(snum, tnum, kx, want_mixed) : STOLT_ROCFFT;
    const bool own_ok = route != STOLT_ROCFFT;
    if (pl.owner != ctx || pl.dtype != (dbl ? IMPDAR_F64 : IMPDAR_F32) || pl.snum != snum || pl.tnum != tnum || pl.use2d != want2d || pl.no_own != no_own ||
        pl.route != route) {
        pl.own_calls = 0;
        pl.plans_ready = false;
        pl.dtype = -1;
        pl.h_taper.clear();
        if (pl.owner != ctx) {               // another device / stream: drop everything bound to the old one
            pl.X.release(); pl.F.release(); pl.K.release(); pl.Y.release(); pl.d_kx.release(); pl.d_ws.release(); pl.d_taper.release();
            pl.release_scan();
            pl.owner = ctx;
        }
        int rc;
        pl.use2d = want2d;
        pl.no_own = no_own;
        pl.route = route;
        // rfft2(axes=(1,0)) (:159) = real transform over time (contiguous here), complex over the traces (rows);
        // irfft2 (:202) = complex inverse over the traces, then C2R over time.  rocFFT's 2-D real plans do
        // exactly these two passes each, with its own blocked column kernels instead of a strided batch.
        if (pl.use2d && !own_ok) {
            // (asking rocFFT for the spectrum frequency-major -- its layout before the plan's last transpose -- removes two
            // transposes but makes it pick slower kernels: 0.76 ms against 0.37 ms at 4096 x 4096 float32, round 2)
            if ((rc = impdar_parallel_plans(ctx->device, {
                     [&] { return pl.fwd2d.create2d(rocfft_transform_type_real_forward, dbl, false, snum, tnum, rocfft_array_type_real,
                                                    rocfft_array_type_hermitian_interleaved, snum, m, 1.0, st); },
                     [&] { return pl.inv2d.create2d(rocfft_transform_type_real_inverse, dbl, false, nout, tnum,
                                                    rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, m, nout,
                                                    1.0 / ((double)nout * tnum), st); }})))
                return rc;
            pl.plans_ready = true;
        }
        if (!pl.use2d) {
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
        IMPDAR_HIP_CHECK(pl.X.ensure((size_t)tnum * snum * sizeof(T)));
        // (the rows layout, below: [snum][tnum/2 + 1] and [tnum/2 + 1][snum] complex)
        const size_t spec = std::max((size_t)tnum * m, (size_t)snum * (tnum / 2 + 1));
        IMPDAR_HIP_CHECK(pl.F.ensure(spec * 2 * sizeof(T)));
        IMPDAR_HIP_CHECK(pl.K.ensure(spec * 2 * sizeof(T)));
        IMPDAR_HIP_CHECK(pl.Y.ensure((size_t)tnum * nout * sizeof(T)));
        IMPDAR_HIP_CHECK(pl.d_kx.ensure((size_t)tnum * 8));
        IMPDAR_HIP_CHECK(pl.d_ws.ensure((size_t)m * 8));
        impdar_trace("stolt: plans and buffers ready");
        pl.dtype = dbl ? IMPDAR_F64 : IMPDAR_F32;
        pl.snum = snum;
        pl.tnum = tnum;
    }
    const bool use_own = own_ok;
    if (use_own) {
        impdar_trace("stolt: transforms on the library's own row kernels");
        int rc;
        if ((rc = pl.tw_time.ensure<T>(snum, st)) || (rc = pl.tw_trace.ensure<T>(tnum, st))) return rc;
    }
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_kx.p, kx, (size_t)tnum * 8, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_ws.p, ws, (size_t)m * 8, hipMemcpyHostToDevice, st));
    c.snum = snum;
    c.tnum = tnum;
    c.m = m;
    c.nz = snum / 2;
    c.nout = nout;
    c.route = route;
    c.use_own = use_own;
    // (the metrics line says when a transform of the call ran on the mixed-radix kernel)
    c.mixed = use_own && !(stolt_pow2(snum) && stolt_pow2(tnum));
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
        const int hs = tnum / 2 + 1;
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
    } else if (pl.use2d) {
        if ((rc = pl.fwd2d.exec(pl.X.p, pl.F.p))) return rc;
    } else {
        if ((rc = pl.r2c.exec(pl.X.p, pl.F.p))) return rc;
        if ((rc = pl.c2c_f.exec(pl.F.p, nullptr))) return rc;
    }
    return IMPDAR_OK;
}

template <typename T> static int stolt_back(impdar_ctx *ctx, StoltPlan &pl, const StoltCall &c, double vel, void *d_out)
{
    const int snum = c.snum, tnum = c.tnum, m = c.m, nz = c.nz, nout = c.nout;
    const bool use_own = c.use_own;
    hipStream_t st = ctx->stream;
    int rc;
    if (c.route == STOLT_OWN_ROWS) {
        const int hs = tnum / 2 + 1;
        hipLaunchKernelGGL((stolt_stretch_rows<T>), dim3((nz + 1 + 255) / 256, hs), dim3(256), 0, st, pl.K.as<Cx<T>>(), pl.F.as<Cx<T>>(),
                           pl.d_kx.as<double>(), pl.d_ws.as<double>(), m, nz, snum, vel);
        if ((rc = own_fft_launch<T>(OWN_C2C_INV, snum, (size_t)hs, pl.F.p, pl.F.p, (size_t)snum, (size_t)snum, 1.0 / snum, pl.tw_time, st))) return rc;
        own_launch_transpose<T>(pl.F.p, pl.K.p, hs, snum, st);
        if ((rc = own_fft_launch<T>(OWN_C2R, tnum, (size_t)snum, pl.K.p, d_out, (size_t)hs, (size_t)tnum, 1.0 / tnum, pl.tw_trace, st))) return rc;
        IMPDAR_HIP_CHECK(hipGetLastError());
        return IMPDAR_OK;
    }
    if (use_own)      // K [w][kx] -> F [w][kx]
        hipLaunchKernelGGL((stolt_stretch_t<T>), dim3((tnum + 255) / 256, m), dim3(256), 0, st, pl.K.as<Cx<T>>(),
                           pl.F.as<Cx<T>>(), pl.d_kx.as<double>(), pl.d_ws.as<double>(), m, nz, tnum, vel);
    else
        hipLaunchKernelGGL((stolt_stretch<T>), dim3((m + 255) / 256, tnum), dim3(256), 0, st, pl.F.as<Cx<T>>(),
                           pl.K.as<Cx<T>>(), pl.d_kx.as<double>(), pl.d_ws.as<double>(), m, nz, tnum, vel);
    if (use_own) {
        if ((rc = own_fft_launch<T>(OWN_C2C_INV, tnum, (size_t)m, pl.F.p, pl.F.p, (size_t)tnum, (size_t)tnum, 1.0 / tnum, pl.tw_trace, st))) return rc;
        own_launch_transpose<T>(pl.F.p, pl.K.p, m, tnum, st);
        hipLaunchKernelGGL((stolt_fix_hermitian<T>), dim3((tnum + 255) / 256), dim3(256), 0, st, pl.K.as<Cx<T>>(), m, tnum);
        if ((rc = own_fft_launch<T>(OWN_C2R, nout, (size_t)tnum, pl.K.p, pl.Y.p, (size_t)m, (size_t)nout, 1.0 / nout, pl.tw_time, st))) return rc;
    } else if (pl.use2d) {
        if ((rc = pl.inv2d.exec(pl.K.p, pl.Y.p))) return rc;
    } else {
        if ((rc = pl.c2c_b.exec(pl.K.p, nullptr))) return rc;
        hipLaunchKernelGGL((stolt_fix_hermitian<T>), dim3((tnum + 255) / 256), dim3(256), 0, st, pl.K.as<Cx<T>>(), m, tnum);
        if ((rc = pl.c2r.exec(pl.K.p, pl.Y.p))) return rc;
    }
    dim3 bgrid((tnum + 63) / 64, (nout + 63) / 64);
    hipLaunchKernelGGL((stolt_transpose_back<T>), bgrid, dim3(256), 0, st, pl.Y.as<T>(), (T *)d_out, nout, tnum);
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
    const bool rows = c.route == STOLT_OWN_ROWS;
    impdar_trace(rows ? "stolt: all kernels enqueued (traces first)" : "stolt: all kernels enqueued");
    ctx->m_entry = "impdar_stolt";
    if (rows)
        ctx->m_kernel = c.mixed ? "stolt_stretch_rows (+ the library's own row transforms, traces first, mixed radix)"
                                : "stolt_stretch_rows (+ the library's own row transforms, traces first)";
    else
        ctx->m_kernel = c.use_own ? (c.mixed ? "stolt_stretch (+ the library's own row transforms, mixed radix)" : "stolt_stretch (+ the library's own row transforms)")
                                  : "stolt_stretch (+ rocFFT 2-D real transforms)";
    ctx->m_kernel_ms = -1.f;
    ctx->ktimed = false;
    ctx->m_extra[0] = 0;
    return impdar_ctx_toc(ctx);
}

// What one velocity of a scan batch may hold on the device, spectra and image together: the batch is as large as fits.
constexpr size_t STOLT_SCAN_BUDGET_BYTES = (size_t)2 << 30;
constexpr int STOLT_SCAN_MAX_BATCH = 1024;

// The velocity scan: the front once, then the back half for nv velocities in batches of B, every image reduced to its rows' focus
// sums where it lies.  On the own transforms a batch is ONE stretch launch (grid z = velocity) and the inverse passes of a single
// call with B times the rows, on [B][rows][len] buffers (a workgroup per row, the kernel chosen by the length alone: the same bits
// as B single calls); the transposes run plane by plane.  On rocFFT the single call's back half runs once per velocity.
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
    const bool rows = c.route == STOLT_OWN_ROWS;
    const int hs = tnum / 2 + 1;
    // one spectrum of the batch, in complex numbers: [hs][snum] on the rows route, [m][tnum] (then [tnum][m]) on the other
    const size_t plane = !c.use_own ? 0 : (rows ? (size_t)hs * snum : (size_t)m * tnum);
    const size_t iplane = (size_t)nout * tnum;
    const size_t per = 2 * plane * 2 * sizeof(T) + std::max(iplane, (size_t)1) * sizeof(T);
    int B = (int)std::min<size_t>(std::max<size_t>(STOLT_SCAN_BUDGET_BYTES / per, 1), (size_t)std::min(nv, STOLT_SCAN_MAX_BATCH));
    if (max_batch > 0) B = std::min(B, max_batch);
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
    const size_t nev = 4 * (size_t)((nv + B - 1) / B);
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
        } else if (rows) {
            hipLaunchKernelGGL((stolt_stretch_scan_rows<T>), dim3((nz + 1 + 255) / 256, hs, nb), dim3(256), 0, st, pl.K.as<Cx<T>>(), S1, dkx,
                               dws, dv, m, nz, snum, plane);
            IMPDAR_HIP_CHECK(hipEventRecord(ev[1], st));
            if ((rc = own_fft_launch<T>(OWN_C2C_INV, snum, (size_t)nb * hs, S1, S1, (size_t)snum, (size_t)snum, 1.0 / snum, pl.tw_time, st))) return rc;
            for (int b = 0; b < nb; ++b) own_launch_transpose<T>(S1 + (size_t)b * plane, S2 + (size_t)b * plane, hs, snum, st);
            if ((rc = own_fft_launch<T>(OWN_C2R, tnum, (size_t)nb * snum, S2, img, (size_t)hs, (size_t)tnum, 1.0 / tnum, pl.tw_trace, st))) return rc;
        } else {
            hipLaunchKernelGGL((stolt_stretch_scan_t<T>), dim3((tnum + 255) / 256, m, nb), dim3(256), 0, st, pl.K.as<Cx<T>>(), S1, dkx, dws,
                               dv, m, nz, tnum, plane);
            IMPDAR_HIP_CHECK(hipEventRecord(ev[1], st));
            if ((rc = own_fft_launch<T>(OWN_C2C_INV, tnum, (size_t)nb * m, S1, S1, (size_t)tnum, (size_t)tnum, 1.0 / tnum, pl.tw_trace, st))) return rc;
            for (int b = 0; b < nb; ++b) own_launch_transpose<T>(S1 + (size_t)b * plane, S2 + (size_t)b * plane, m, tnum, st);
            // ([nb][tnum][m] is nb * tnum rows of m: the single call's kernels with nb times the rows)
            hipLaunchKernelGGL((stolt_fix_hermitian<T>), dim3((nb * tnum + 255) / 256), dim3(256), 0, st, S2, m, nb * tnum);
            // the real images before their transposes go where the spectra were: nout <= 2 m - 2 reals per row of m complex
            T *Yt = reinterpret_cast<T *>(S1);
            if ((rc = own_fft_launch<T>(OWN_C2R, nout, (size_t)nb * tnum, S2, Yt, (size_t)m, (size_t)nout, 1.0 / nout, pl.tw_time, st))) return rc;
            dim3 bgrid((tnum + 63) / 64, (nout + 63) / 64);
            for (int b = 0; b < nb; ++b)
                hipLaunchKernelGGL((stolt_transpose_back<T>), bgrid, dim3(256), 0, st, Yt + (size_t)b * iplane, img + (size_t)b * iplane, nout, tnum);
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
    if (rows)
        ctx->m_kernel = c.mixed ? "stolt_stretch_scan_rows (+ the library's own row transforms, traces first, mixed radix)"
                                : "stolt_stretch_scan_rows (+ the library's own row transforms, traces first)";
    else
        ctx->m_kernel = c.use_own ? (c.mixed ? "stolt_stretch_scan_t (+ the library's own row transforms, mixed radix)"
                                             : "stolt_stretch_scan_t (+ the library's own row transforms)")
                                  : "stolt_stretch (+ rocFFT 2-D real transforms, one velocity at a time)";
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
    int rc = dtype == IMPDAR_F32
                 ? stolt_run<float>(ctx, *g_stolt_plan, d_data, snum, tnum, kx, ws, vel, htaper, vtaper, d_out)
                 : stolt_run<double>(ctx, *g_stolt_plan, d_data, snum, tnum, kx, ws, vel, htaper, vtaper, d_out);
    if (rc) return rc;
    // kx/ws were staged from caller memory: complete before returning
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    impdar_trace("stolt: device work complete");
    return impdar_ctx_mark_produced(ctx);
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
    // (the two device arrays of the call come from the cache of freed ones: no hipMalloc / hipFree per call)
    void *din = nullptr, *dout = nullptr;
    int rc = impdar_devcache_alloc(ctx->device, inb, &din);
    if (rc == IMPDAR_OK) rc = impdar_devcache_alloc(ctx->device, outb ? outb : 8, &dout);
    if (rc == IMPDAR_OK && hipMemcpyAsync(din, data, inb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        impdar_set_error("impdar_stolt: upload failed: %s", hipGetErrorString(hipGetLastError()));
        rc = IMPDAR_ERR_HIP;
    }
    impdar_trace("impdar_stolt: upload enqueued");
    if (rc == IMPDAR_OK) rc = impdar_stolt_dev(ctx, din, dtype, snum, tnum, kx, ws, vel, htaper, vtaper, dout);
    if (rc == IMPDAR_OK) rc = impdar_download(ctx, out, dout, outb, ctx->stream);
    impdar_trace("impdar_stolt: downloaded");
    (void)hipStreamSynchronize(ctx->stream);                  // (nothing in flight may still touch the arrays)
    impdar_devcache_free(din);
    impdar_devcache_free(dout);
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
    rc = dtype == IMPDAR_F32 ? stolt_scan_run<float>(ctx, *g_stolt_plan, d_data, snum, tnum, kx, ws, vels, nv, htaper, vtaper, t0, t1,
                                                     max_batch, sums, keep, d_keep)
                             : stolt_scan_run<double>(ctx, *g_stolt_plan, d_data, snum, tnum, kx, ws, vels, nv, htaper, vtaper, t0, t1,
                                                      max_batch, sums, keep, d_keep);
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
    void *din = nullptr, *dkeep = nullptr;
    rc = impdar_devcache_alloc(ctx->device, inb, &din);
    if (rc == IMPDAR_OK && keep >= 0) rc = impdar_devcache_alloc(ctx->device, outb ? outb : 8, &dkeep);
    if (rc == IMPDAR_OK && hipMemcpyAsync(din, data, inb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        impdar_set_error("impdar_stolt_scan: upload failed: %s", hipGetErrorString(hipGetLastError()));
        rc = IMPDAR_ERR_HIP;
    }
    if (rc == IMPDAR_OK)
        rc = impdar_stolt_scan_dev(ctx, din, dtype, snum, tnum, kx, ws, vels, nv, htaper, vtaper, t0, t1, max_batch, sums, keep, dkeep);
    if (rc == IMPDAR_OK && keep >= 0) rc = impdar_download(ctx, keep_out, dkeep, outb, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);                  // (nothing in flight may still touch the arrays)
    impdar_devcache_free(din);
    impdar_devcache_free(dkeep);
    return rc;
}
