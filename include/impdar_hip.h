/*
 * impdar_hip.h -- C ABI of the MI355X (gfx950) migration engine.
 *
 * This is the drop-in boundary for the migration hot path of dlilien/ImpDAR
 * (reference paths are relative to the ImpDAR source tree):
 *
 *   - the reference's only native hook of the migrations is
 *       src/impdar/lib/migrationlib/mig_cython.h:11   (mig_kirch_loop)
 *     bound by src/impdar/lib/migrationlib/_mig_cython.pyx:19-20 and selected
 *     in src/impdar/lib/migrationlib/__init__.py:16-19.  That exact symbol is
 *     exported below, and so is its other native hook,
 *       src/impdar/lib/ApresData/coherence.h:13       (coherence2d)
 *     bound by src/impdar/lib/ApresData/_coherence.pyx.
 *   - Stolt / phase-shift / T-K have no native hook in the reference; their
 *     boundary is the Python function (mig_python.py:126, :211, :290).  The
 *     impdar_* entry points below are what a ctypes binding of those
 *     functions calls.
 *
 * Conventions: plain pointers and sizes only.  All host buffers are
 * caller-owned, C-contiguous, row-major; radargrams have shape (snum, tnum)
 * (a row is one time sample across all traces).  Calls that take HOST buffers
 * are blocking.  Calls that take DEVICE pointers (the *_dev forms, impdar_dev_memset and the
 * impdar_kirch_prep / _allgather / _exchange / _migrate family) only enqueue work: they are ordered
 * among themselves on the device, and impdar_ctx_sync / any download waits for them.  Every call returns 0 on success or a negative
 * impdar_status, never throws or exits.  impdar_last_error() returns a
 * thread-local message for the last failing call.
 */
#ifndef IMPDAR_HIP_H
#define IMPDAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum impdar_status {
    IMPDAR_OK = 0,
    IMPDAR_ERR_ARG = -1,      /* bad argument (maps to ValueError in Python)  */
    IMPDAR_ERR_HIP = -2,      /* HIP runtime failure                           */
    IMPDAR_ERR_FFT = -3,      /* rocFFT failure                                */
    IMPDAR_ERR_COMM = -4,     /* RCCL failure                                  */
    IMPDAR_ERR_NODEV = -5,    /* no usable GPU                                 */
    IMPDAR_ERR_UNSUPPORTED = -6
} impdar_status;

typedef enum impdar_dtype { IMPDAR_F32 = 0, IMPDAR_F64 = 1 } impdar_dtype;

/* Kirchhoff kernel selection.  AUTO: F64 data -> EXACT, F32 data on a uniform
 * (dist, travel_time) grid -> FAST, otherwise EXACT. */
typedef enum impdar_kirch_mode {
    IMPDAR_KIRCH_AUTO = 0,
    IMPDAR_KIRCH_EXACT = 1,   /* per-pair fp64 index math, any geometry        */
    IMPDAR_KIRCH_FAST = 2     /* fp32 LDS-ring kernel, uniform grids only      */
} impdar_kirch_mode;

typedef struct impdar_ctx impdar_ctx;           /* device + stream + workspaces */
typedef struct impdar_kirch_plan impdar_kirch_plan;

/* ---- library / device ------------------------------------------------- */
const char *impdar_last_error(void);
int impdar_device_count(void);
int impdar_ctx_create(int device, impdar_ctx **out);
void impdar_ctx_destroy(impdar_ctx *ctx);
int impdar_ctx_sync(impdar_ctx *ctx);
/* device-side duration (HIP events on the compute stream, ms) of the kernels of the last impdar_stolt[_dev] /
 * impdar_phaseshift[_dev] call on this context; blocks until they have completed */
int impdar_ctx_last_ms(impdar_ctx *ctx, float *ms);
/* ... and of the frequency-sum kernels alone (the rotate-accumulate work of mig_python.py:396-487, without the
 * transforms and transposes around it) of the last impdar_phaseshift[_dev] call; after impdar_apres_decode[_dev] the
 * time from its first kernel's start to its last kernel's end */
int impdar_ctx_last_kernel_ms(impdar_ctx *ctx, float *ms);
/* One JSON object about the last migration entry point that ran on this context (impdar_kirchhoff, impdar_stolt,
 * impdar_phaseshift[_ffd], impdar_taper): {"entry", "kernel" (the kernel that did the sums), "device", "kernel_ms",
 * "device_ms", and per entry point e.g. "plan": "new" | "cached", "launches"}.  SURVEY.md section 5 "metrics": the
 * reference prints 'complete in N seconds' only (mig_python.py:121-122,206-207,285-286); the Python entry points add
 * sizes, traces per second and the device count and print the line on stderr when IMPDAR_METRICS is set. */
int impdar_ctx_last_metrics(impdar_ctx *ctx, char *json, size_t cap);
/* raw device-memory plumbing for resident data (bench, multi-GPU) */
int impdar_dev_alloc(impdar_ctx *ctx, size_t bytes, void **dptr);
int impdar_dev_free(impdar_ctx *ctx, void *dptr);
int impdar_dev_upload(impdar_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int impdar_dev_download(impdar_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int impdar_dev_memset(impdar_ctx *ctx, void *dst_dev, int value, size_t bytes);
/* device (float32 or float64, `n` elements) -> a float64 host array: what the reference's migrations hand back
 * whatever the input type (mig_python.py:118, :282).  Goes through the context's pinned staging buffer and
 * converts on several host threads (a single-threaded astype of a fresh 512 MB array costs more than the
 * phase-shift kernel that produced it). */
int impdar_dev_download_f64(impdar_ctx *ctx, double *dst_host, const void *src_dev, int dtype, size_t n);

/* ---- reference-compatible native hook ---------------------------------
 * Replaces mig_cython.h:11.  Same argument meaning as
 * mig_python.py:35 migrationKirchhoffLoop: writes migdata (snum x tnum,
 * row-major, float64) in place.  The reference prototype carries no `data`
 * pointer, so nearfield != 0 cannot be honoured through it (the reference's
 * own defect); it is rejected with a message on stderr and
 * migdata is left untouched.  Uses device 0. */
void mig_kirch_loop(double *migdata, int tnum, int snum, double *dist,
                    double *zs, double *zs2, double *tt_sec, double vel,
                    double *gradD, double max_travel_time, int nearfield);

/* ---- Kirchhoff (mig_python.py:35-123) ---------------------------------
 * One-shot host-buffer form: data (snum,tnum) of `dtype`; gradient
 * coefficients come from impdar's host shim (they restate numpy.gradient's
 * choice of the uniform / non-uniform formula, mig_python.py:93):
 *   grad_uniform != 0: interior (f[k+1]-f[k-1])/(2*grad_h), ends (f1-f0)/grad_h
 *   grad_uniform == 0: interior ga[k]*f[k-1]+gb[k]*f[k]+gc[k]*f[k+1],
 *                      ends (f[1]-f[0])/ga[0], (f[n-1]-f[n-2])/ga[n-1]
 * out is float64 (snum,tnum) like the reference's dat.data. */
int impdar_kirchhoff(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                     const double *dist_m, const double *tt_sec, double vel, int nearfield,
                     int grad_uniform, double grad_h, const double *ga, const double *gb,
                     const double *gc, int mode, double *out);

/* Resident / sharded form.  A plan owns the trace-major gradient image
 * GT[tnum_pad][snum] (and the data image for the near-field term), the
 * per-sample and per-offset tables and the launch geometry.
 *   prep     : gradient + transpose of the caller's LOCAL column block
 *              d_data (snum x nloc, row-major, leading dimension ld) into
 *              rows [jlo, jlo+nloc) of the image
 *   allgather: RCCL all-gather of the image rows across the communicator
 *              (equal blocks of tnum_pad/nranks traces per rank)
 *   migrate  : diffraction sum for output traces [xlo,xhi) into d_out
 *              (snum x (xhi-xlo), row-major, element type = plan dtype)
 * All of them are asynchronous; call impdar_ctx_sync to wait.  prep and allgather run on
 * the context's producer stream into one of two buffer sets, migrate on its compute stream,
 * so the prep/all-gather of the next radargram overlap the diffraction sum of the current
 * one; the first prep after a migrate starts a new radargram (switches buffer set).  prep waits
 * (on the device) for whatever the *_dev entry points and impdar_dev_memset have enqueued on the
 * compute stream before it, so a resident chain filter -> prep needs no host synchronisation;
 * impdar_dev_upload is blocking.  The IMPDAR_KIRCH_* plan knobs are read when the plan is created; prep and
 * migrate go by what the plan was created under. */
int impdar_kirch_plan_create(impdar_ctx *ctx, int dtype, int snum, int tnum,
                             const double *dist_m, const double *tt_sec, double vel,
                             int nearfield, int grad_uniform, double grad_h,
                             const double *ga, const double *gb, const double *gc,
                             int mode, int nranks, impdar_kirch_plan **out);
void impdar_kirch_plan_destroy(impdar_kirch_plan *plan);
int impdar_kirch_plan_mode(const impdar_kirch_plan *plan);      /* resolved mode */
int impdar_kirch_plan_tnum_pad(const impdar_kirch_plan *plan);
/* Position noise of the profile in units of the trace spacing: how far dist[j] - dist[xi] can be from (j - xi) dx
 * (deviation from the fitted grid + rounding of the largest |dist|).  The float64 kernels that weight a pair by its
 * trace offset (ring, tabulated) meet  max(1e-12, 0.1 xnoise)  of the image maximum against mig_python.py:44-60. */
double impdar_kirch_plan_xnoise(const impdar_kirch_plan *plan);
/* which diffraction-sum kernel the plan will launch */
typedef enum impdar_kirch_kernel {
    IMPDAR_KERNEL_EXACT_PAIR = 0,   /* per-pair fp64 arithmetic in the reference's order: any geometry            */
    IMPDAR_KERNEL_EXACT_TAB = 1,    /* fp64 picks/weights tabulated per (sample, |offset|), global-memory gather  */
    IMPDAR_KERNEL_DQUAD = 2,        /* float64 LDS ring (the float64 default on uniform grids)                    */
    IMPDAR_KERNEL_QUAD = 3,         /* float32 LDS ring, ds_read_b128 (the fast path)                             */
    IMPDAR_KERNEL_TAB = 4,          /* float32 LDS ring, trace-major, for steep moveout                           */
    IMPDAR_KERNEL_GEN = 5           /* float32, non-uniform (sorted) dist: picks computed per pair, LDS-staged     */
} impdar_kirch_kernel;
int impdar_kirch_plan_kernel(const impdar_kirch_plan *plan);
/* How the persistent ring kernels hand out their (chunk, tile) items, for every plan created after the call (process-wide;
 * the plans that impdar_kirchhoff and mig_kirch_loop keep are rebuilt when it changes).  It changes no bit of an image.
 *   order: 0 the library's choice by the launch, 1 chunk by chunk (longest first inside a chunk), 2 packed (one
 *          longest-first order across all chunks)
 *   gang : adjacent tiles of a chunk that go to one XCD together, 1, 2 or 4; 0 the library's choice
 * Anything else is IMPDAR_ERR_ARG and changes nothing. */
int impdar_kirch_queue_policy(int order, int gang);
/* The output window of the float32 ring kernel's tiles (far field), for every plan created after the call (process-wide, like
 * the queue policy above).
 *   window: 0 the library's choice, 1 the sliding window, 2 the quad-aligned window where the plan's ring holds its three
 *           further traces of moveout (elsewhere the plan keeps the sliding one)
 * The two differ by float32 rounding in the three columns left of every tile start (two partial sums added there) and in no
 * other bit.  Anything else is IMPDAR_ERR_ARG and changes nothing. */
int impdar_kirch_window_policy(int window);
/* which one the plan's kernel runs: 0 sliding, 1 quad-aligned */
int impdar_kirch_plan_window(const impdar_kirch_plan *plan);
int impdar_kirch_prep(impdar_kirch_plan *plan, const void *d_data, int ld, int jlo, int nloc);
int impdar_kirch_allgather(impdar_kirch_plan *plan);
/* Halo form of the exchange ("grouped ncclSend/ncclRecv of halos when H < shard"): this rank sends
 * image rows [slo[i], shi[i]) to rank speer[i] and receives rows [rlo[i], rhi[i]) from rank rpeer[i], all in one
 * RCCL group on the producer stream.  Ranges are whole 8-trace groups (multiples of 8 inside [0, tnum_pad)).
 * impdar_amd/parallel.py (plan_exchange) derives them from the output blocks and the aperture half width. */
int impdar_kirch_exchange(impdar_kirch_plan *plan, int nsend, const int *speer, const int *slo, const int *shi,
                          int nrecv, const int *rpeer, const int *rlo, const int *rhi);
int impdar_kirch_migrate(impdar_kirch_plan *plan, void *d_out, int xlo, int xhi);
/* HIP-event durations (ms) of the last prep / allgather / migrate enqueued on
 * the plan's stream; blocks until they have completed. */
int impdar_kirch_last_ms(impdar_kirch_plan *plan, float *prep_ms, float *gather_ms,
                         float *migrate_ms);
/* same for the step `back` steps before the last one (a step starts at each
 * impdar_kirch_prep; 64 steps of history are kept), so a timed loop can read
 * its per-step kernel durations after the loop without synchronising in it */
int impdar_kirch_history_ms(impdar_kirch_plan *plan, int back, float *prep_ms, float *gather_ms,
                            float *migrate_ms);
/* exact number of in-aperture (output sample, input trace) pairs for output
 * traces [xlo,xhi) under the plan's geometry (uniform grids only; -1 else) */
long long impdar_kirch_count_pairs(const impdar_kirch_plan *plan, int xlo, int xhi);

/* ---- Stolt f-k (mig_python.py:126-208) --------------------------------
 * data (snum,tnum) of dtype already tapered-cast by the caller? NO: the taper
 * (mig_python.py:152-157) runs on the device.  kx has tnum entries, ws has
 * snum/2+1 entries (host shim restates :161-168).  out has 2*(snum/2) rows,
 * same dtype as data.
 * Sizes with a length above 1024 whose lengths have no prime factor above 7 run on the library's own row transforms
 * (IMPDAR_STOLT_FFT=mixed: every such size).  Their "traces first" form keeps the wavenumbers k = 0 .. tnum/2 alone and
 * therefore needs kx[k] == -kx[tnum - k] exactly for 1 <= k < tnum/2 -- what 2 pi fftfreq(tnum, dx) gives; the host checks
 * it at sizes that are no power of two, and any other kx takes the form that keeps all wavenumbers (or rocFFT). */
int impdar_stolt(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                 const double *kx, const double *ws, double vel, double htaper,
                 double vtaper, void *out);
/* resident form used by bench/tests: d_data and d_out are device pointers */
int impdar_stolt_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum,
                     const double *kx, const double *ws, double vel, double htaper,
                     double vtaper, void *d_out);
/* Velocity scan: the Stolt image of the same radargram at each of vels[0 .. nv), none of them downloaded -- the taper and
 * the forward transforms run once, the stretch and the inverse transforms in batches of velocities (max_batch > 0 caps the
 * batch; 0: as many as fit the library's budget), and every image is reduced on the device to three focus sums per output
 * row over the traces t0 <= j < t1: sums[v][k] = { sum |x|, sum x^2, sum x^4 }, float64, [nv][2*(snum/2)][3] on the host.
 * The additions have a fixed order (no atomics): the same call gives the same bits, whatever max_batch.  Every image is
 * bit for bit what impdar_stolt_dev gives at that velocity; keep >= 0 copies the image of vels[keep] into d_keep
 * (2*(snum/2) x tnum of dtype), keep = -1: no image (d_keep may be NULL).  d_data is not modified.  ERR_ARG unless
 * nv >= 1, every velocity positive and finite, 0 <= t0 < t1 <= tnum and -1 <= keep < nv. */
int impdar_stolt_scan_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum,
                          const double *kx, const double *ws, const double *vels, int nv,
                          double htaper, double vtaper, int t0, int t1, int max_batch,
                          double *sums, int keep, void *d_keep);
/* host-buffer form: data is uploaded once; keep_out (host) receives the image of vels[keep] when keep >= 0 */
int impdar_stolt_scan(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                      const double *kx, const double *ws, const double *vels, int nv,
                      double htaper, double vtaper, int t0, int t1, int max_batch,
                      double *sums, int keep, void *keep_out);

/* ---- f-k fan (dip) filter and f-k spectrum (csrc/fk.hip; an extension) ----------
 * On the transforms and the cached plan of impdar_stolt (IMPDAR_STOLT_FFT chooses the route as there; a chain
 * fk -> stolt at one size plans once), with both tapers off.  kx: tnum wavenumbers in numpy.fft.fftfreq order; ws: the
 * snum/2 + 1 frequencies of numpy.fft.rfftfreq (the negative ones are their mirror).  snum, tnum >= 2, odd sizes included.
 * impdar_fk_fan: out = Re ifft2(M * fft2(data)), (snum, tnum) of dtype (d_out may be d_data), M real, per element:
 *   slowness p = 0 where |kx| == 0, else +inf where |w| == 0, else |kx| / |w|;
 *   E(p; pc, taper) = 1 for p <= pc (1 - taper) (tested first), 0 for p >= pc (1 + taper), a raised cosine between;
 *   W = E(p; 1/va_lo, taper) * (1 - E(p; 1/va_hi, taper)), a factor 1 for an edge that is NaN: apparent velocities
 *   va_lo <= |w| / |kx| <= va_hi pass;  dip 0: both sides, 1 (down_right: arrival time grows with distance) keeps
 *   w kx < 0, 2 (down_left) w kx > 0 -- elements with w kx == 0 or on a Nyquist row / column belong to both -- off the
 *   side W = 0;  mode 0 (pass): M = W, 1 (reject): M = 1 - W.  The weight is evaluated in float64 for both dtypes.
 *   ERR_ARG, before any device work: both edges NaN; an edge not finite and positive; taper outside [0, 1);
 *   (1/va_hi) (1 + taper) > (1/va_lo) (1 - taper); snum < 2 or tnum < 2; another dtype, mode or dip.
 * impdar_fk_power: out[j][i] = |fft2(data)[j][i]|^2 for the snum/2 + 1 rows w >= 0, the columns in fftshift order,
 *   not normalised: (snum/2 + 1, tnum) float64 whatever dtype (the transforms run in dtype).
 * Metrics: "kernel_ms" is the fan (or power) kernel alone; "planned": 1 when this call made plans or buffers. */
int impdar_fk_fan(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                  const double *kx, const double *ws, double va_lo, double va_hi, double taper,
                  int mode, int dip, void *out);
int impdar_fk_fan_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum,
                      const double *kx, const double *ws, double va_lo, double va_hi, double taper,
                      int mode, int dip, void *d_out);
int impdar_fk_power(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                    const double *kx, const double *ws, double *out);
int impdar_fk_power_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum,
                        const double *kx, const double *ws, void *d_out);

/* ---- predictive (gapped, Wiener-Levinson) deconvolution and the autocorrelogram (csrc/decon.hip; an extension) ----
 * The contract is csrc/decon_core.h; all arithmetic is float64 for both dtypes.  Per trace (column) x, over the design
 * window [s0, s1): r[l] = sum_k x[k] x[k + l]; the symmetric Toeplitz system c[|m - i|] a[i] = r[gap + m], m < oplen, with
 * c[0] = r[0] (1 + prewhiten / 100), by Levinson recursion; y[k] = x[k] - sum_i a[i] x[k - gap - i] over the whole trace
 * (samples before its start are zero), rounded to dtype.  gap = 1: spiking deconvolution.
 * design 0 (each): every trace its own operator; 1 (mean): one operator from the lags summed over the live traces, in a
 *   fixed order.  A trace whose r[0] is not finite or not > 0, or whose recursion loses a finite positive error power, is
 *   dead: it passes unchanged (NaN positions included) and its operator is zero.
 * impdar_decon: out is (snum, tnum) of dtype (d_out may be d_data: the result is the out-of-place one bit for bit);
 *   op: null, or (oplen, tnum) float64, the operator applied to every trace (a device array in the _dev form).
 * impdar_acorr: out[l][j] = r_j[l], l = 0 .. maxlag: (maxlag + 1, tnum) float64; normalize != 0 divides by r_j[0], a
 *   dead trace's column is NaN.
 * ERR_ARG, before any device work, with the reason of csrc/decon_route.h: oplen outside 1 .. 256; gap < 1; a window that
 *   is not 0 <= s0 < s1 <= snum; gap + oplen > s1 - s0; maxlag < 0 or >= s1 - s0; prewhiten negative or not finite;
 *   another design or dtype.
 * Metrics: "device_ms" and the stages "acorr_ms", "solve_ms", "apply_ms" (impdar_acorr: "acorr_ms"); the _dev forms
 *   return with the stream drained. */
int impdar_decon(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int s0, int s1,
                 int oplen, int gap, double prewhiten, int design, void *out, double *op);
int impdar_decon_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int s0, int s1,
                     int oplen, int gap, double prewhiten, int design, void *d_out, double *d_op);
int impdar_acorr(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int s0, int s1,
                 int maxlag, int normalize, double *out);
int impdar_acorr_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int s0, int s1,
                     int maxlag, int normalize, double *d_out);

/* ---- complex-trace attributes: envelope, instantaneous phase and frequency (csrc/attr.hip; an extension) ----
 * The contract is csrc/attr_route.h; all arithmetic is float64 for both dtypes.  Per trace (column) x of n = snum samples:
 * q = irfft(Y, n) with Y[k] = -i rfft(x)[k] for 0 < k < n / 2 (and k = (n - 1) / 2 of an odd n), Y[0] = 0, Y[n / 2] = 0 for
 * even n -- imag(scipy.signal.hilbert(x)); n <= 2 gives q = 0.  With z = x + i q:
 *   kind 0 quadrature q;  1 envelope hypot(x, q);  2 phase atan2(q, x) in radians;
 *   kind 3 frequency f[k] = arg(z[k + 1] conj z[k]) / (2 pi dt) in Hz, f[n - 1] = f[n - 2], 0 for n = 1; with smooth = W > 1
 *   (odd, at most 255) the mean of f over |j - k| <= (W - 1) / 2, clipped to the trace, weighted by x[j]^2 + q[j]^2 and summed
 *   with j rising, 0 where the weights sum to 0.  smooth = 1 leaves f as it is; dt is read for kind 3 alone.
 * out is (snum, tnum) of dtype, rounded once (d_out may be d_data: the result is the out-of-place one bit for bit).  A trace
 * with a sample that is not finite is NaN throughout, an all-zero trace gives zeros; both are decided by a reduction over
 * the trace, not by a transform.  No floating-point atomics: two calls give the same bits.
 * ERR_ARG, before any device work, with the reason of csrc/attr_route.h: an unknown kind; smooth even or outside 1 .. 255;
 *   smooth > 1 with a kind other than 3; dt not finite or not positive (kind 3); an empty radargram; another dtype.
 * impdar_attr_route_probe: what csrc/attr_route.h decides for tnum traces of snum samples: out[0] = 0 own power-of-two
 *   transform, 1 own mixed-radix transform, 2 rocFFT; out[1] threads of the row kernel; out[2] workgroups; out[3] traces
 *   per workgroup; out[4] bytes of LDS per workgroup; out[5] = 1 when no transform runs (n <= 2).  No device call.
 * Metrics: "device_ms"; the _dev form enqueues on the context's compute stream. */
int impdar_attr(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int kind, int smooth,
                double dt, void *out);
int impdar_attr_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int kind, int smooth,
                    double dt, void *d_out);
int impdar_attr_route_probe(int snum, int tnum, int kind, int smooth, int *out);

/* ---- layer slopes: structure-tensor dip field and dip-steered mean (csrc/slope.hip; an extension) ----
 * The contract is csrc/slope_route.h; all arithmetic is float64 for both dtypes; a sample that is not finite is read as NaN.
 * impdar_slope: gradients gz, gx in index units (np.gradient), the products gz gz, gz gx, gx gx smoothed by a separable
 *   Gaussian (sigma_x along the traces, then sigma_z along the samples; radius int(4 sigma + 0.5), clamped indices, sigma 0
 *   leaves the axis alone) into a, b, c; d = a - c, D = sqrt(d d + 4 b b).  out is a float64 (snum, tnum) field:
 *   kind 0 slope in samples per trace (-2b / (d + D) where d >= 0, -(D - d) / (2b) where d < 0, 0 where D = 0), clamped to
 *   +-max_slope;  1 dip atan2(-2b, d) / 2 in radians;  2 coherence D / (a + c) (0 where a + c is not positive);
 *   3, 4, 5: a, b, c.  A NaN in a, b or c gives NaN in kinds 0 .. 2.
 * impdar_dipsmooth: every sample becomes the mean over the traces j - half .. j + half inside the radargram of their linear
 *   interpolation at k + p i clamped to the trace, p the slope at the sample itself -- `slope` (float64, (snum, tnum); a
 *   device pointer in the _dev form) or, when that is null, kind 0 at (sigma_z, sigma_x, max_slope), which are not read
 *   otherwise.  A NaN p gives NaN.  out is (snum, tnum) of dtype, rounded once; d_out may be d_data (the same bits).
 * No floating-point atomics and one fixed order of every sum: two calls give the same bits.
 * ERR_ARG, before any device work, with the reason of csrc/slope_route.h: an unknown kind; a sigma not finite, negative or
 *   above 16; max_slope not finite or not positive; half outside 1 .. 32; an empty radargram; another dtype.
 * impdar_slope_route_probe: what csrc/slope_route.h decides: out[0], out[1] the radii r_z, r_x; out[2 .. 4] threads,
 *   workgroups and bytes of LDS of the row pass; out[5 .. 7] of the column pass; out[8], out[9] threads and workgroups of
 *   the gather; out[10] MiB of scratch of an in-place float64 dipsmooth with no slope given (the most).  No device call.
 * Metrics: "device_ms"; the _dev forms enqueue on the context's compute stream. */
int impdar_slope(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int kind, double sigma_z,
                 double sigma_x, double max_slope, double *out_f64);
int impdar_slope_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int kind, double sigma_z,
                     double sigma_x, double max_slope, double *d_out_f64);
int impdar_dipsmooth(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int half,
                     const double *slope_f64_or_null, double sigma_z, double sigma_x, double max_slope, void *out);
int impdar_dipsmooth_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int half,
                         const double *d_slope_f64_or_null, double sigma_z, double sigma_x, double max_slope, void *d_out);
int impdar_slope_route_probe(int snum, int tnum, double sigma_z, double sigma_x, int half, int *out);

/* ---- the library's own batched power-of-two row transforms (csrc/own_fft.h) ----
 * What the Stolt / phase-shift calls of power-of-two sizes run their transforms on (rocFFT compiles the kernels of
 * lengths above 1024 at run time: 0.25-3 s per plan, profiles/r05_first_call.txt).  numpy.fft conventions
 * (mig_python.py:159, 202, 270, 282), unnormalised, times `scale`.
 * mode 0: complex forward, 1: complex inverse -- d_in / d_out [batch][n] complex (d_out may be d_in);
 * mode 2: real forward -- d_in [batch][n] real, d_out [batch][n/2 + 1] complex;
 * mode 3: real inverse -- d_in [batch][n/2 + 1] complex, d_out [batch][n] real (imaginary parts of the first and last
 * entry are the caller's business: numpy.fft.irfft ignores them);
 * mode 4: complex inverse, real parts only -- d_in [batch][n] complex, d_out [batch][n] real (mig_python.py:282).
 * n a power of two; complex length (n, or n/2 for the real modes) 16 .. 8192.  dtype IMPDAR_F32 / IMPDAR_F64. */
int impdar_fft_rows_dev(impdar_ctx *ctx, int mode, int dtype, int n, int batch, const void *d_in, void *d_out, double scale);
/* The same at any length whose complex length (n, or n/2 for the real modes; a real n must be even) is 16 .. 8192 with
 * no prime factor above 7: a power of two runs as above, any other such length on the mixed-radix kernel
 * (csrc/own_fft_mixed.h) -- 10000 traces are real rows of 5000 complex numbers. */
int impdar_fft_rows_any_dev(impdar_ctx *ctx, int mode, int dtype, int n, int batch, const void *d_in, void *d_out, double scale);

/* ---- phase shift / Gazdag (mig_python.py:211-287, :361-493) ------------
 * vmig_len == 0: constant velocity `vconst`; vmig_len == snum: 1-D v(z).
 * kx has tnum entries, ws has nt entries (two-sided, :268), tt_us has snum
 * entries (microseconds).  out float64/float32 (snum,tnum) = dtype. */
int impdar_phaseshift(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                      int nt, const double *kx, const double *ws, double dt,
                      const double *tt_us, double vconst, const double *vmig, int vmig_len,
                      double htaper, double vtaper, void *out);

/* resident form: d_data and d_out are device arrays of `dtype` (snum, tnum) */
int impdar_phaseshift_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum,
                          int nt, const double *kx, const double *ws, double dt,
                          const double *tt_us, double vconst, const double *vmig, int vmig_len,
                          double htaper, double vtaper, void *d_out);
/* Phase shift sharded over the wavenumbers (every k is independent in phaseShift, mig_python.py:396-487):
 * a rank calls, on the whole radargram resident on its device,
 *   impdar_phaseshift_tk_dev      -> d_tk [nk][snum] complex: TK (already / snum, :492) of wavenumbers [k0, k0 + nk)
 *   impdar_ps_alltoall_dev        -> d_t2 [tnum][tw] complex: all wavenumbers, its own depth rows (grouped RCCL
 *                                    send/recv; tau_edges / k_edges: nranks + 1 slab edges, the same on every rank)
 *   impdar_phaseshift_finish_dev  -> d_out (tw, tnum) real: ifft over k, real part (:282)
 * (d_tk holds the rows TK[k] themselves.  impdar_phaseshift / impdar_phaseshift_dev, which only need the real part of the inverse
 * transform, may sum rows k and tnum - k as their Hermitian combination (TK[k] + conj TK[tnum - k]) / 2 -- one transform for two
 * rows, csrc/ps_nufft.h, ps_series.h; the image is the same.) */
int impdar_phaseshift_tk_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int nt,
                             const double *kx, const double *ws, double dt, const double *tt_us, double vconst,
                             const double *vmig, int vmig_len, double htaper, double vtaper, int k0, int nk, void *d_tk);
int impdar_ps_alltoall_dev(impdar_ctx *ctx, const void *d_tk, int dtype, int snum, int tnum, int nranks, int rank,
                           const int *tau_edges, const int *k_edges, void *d_t2);
int impdar_phaseshift_finish_dev(impdar_ctx *ctx, void *d_t2, int dtype, int tw, int tnum, void *d_out);

/* ---- phase shift, 2-D v(x,z): Fourier finite-difference branch ----------
 * Replaces the `hasattr(vmig[itau], "__len__")` path of phaseShift
 * (mig_python.py:428-432, 448-487) with fourierFiniteDiff (:496-525) and the
 * stencil of Sp_Matr (:528-540), behind migrationPhaseShift (:211-287).
 * float64 only.  data/out: host (snum, tnum) row-major; vmig2d: host
 * (snum, tnum) migration velocities (getVelocityProfile's 3-column output);
 * kx (tnum), ws (nt) as for impdar_phaseshift; dx_mean = mean(trace_int).
 * The (tau, omega) nest is one serial chain in the reference (a single
 * FFX_last); it is executed in that order. */
int impdar_phaseshift_ffd(impdar_ctx *ctx, const double *data, int snum, int tnum, int nt,
                          const double *kx, const double *ws, double dt, const double *tt_us,
                          const double *vmig2d, double dx_mean, double htaper, double vtaper,
                          double *out);

/* ---- taper only (what mtype='tk' does, mig_python.py:330-335) ---------- */
int impdar_taper(impdar_ctx *ctx, void *data_inout, int dtype, int snum, int tnum,
                 double htaper, double vtaper);

/* ---- processing steps in front of a migration ----------
 * The `_dev` forms take device pointers and run on the context's compute
 * stream without synchronising it, so a radargram can stay resident from the
 * first filter to the migrated image; the plain forms take host buffers.
 *
 * impdar_filtfilt: RadarData.vertical_band_pass with an IIR design
 * (_RadarDataFiltering.py:527-535) = scipy.signal.filtfilt(b, a, data, axis=0)
 * cast back to the data's dtype, in place.  b, a: `ncoef` (2..33)
 * coefficients each; zi: ncoef-1 steady-state initial conditions
 * (scipy.signal.lfilter_zi).  Fails with scipy's message when
 * snum <= 3*ncoef.
 * impdar_fir_shift: the FIR branch (:536-540): rows [0, snum-order) become
 * lfilter(taps, 1, data)[order:], the last `order` = ntaps-1 rows are left.
 * impdar_trace_lerp: the data part of RadarData.constant_space
 * (_RadarDataProcessing.py:549-553): out[k, m] = (data[k, hi[m]] -
 * data[k, lo[m]]) / den[m] * t[m] + data[k, lo[m]] (scipy interp1d's slope
 * form), out float64 (snum, n_new); lo/hi/den/t are host arrays. */
int impdar_filtfilt(impdar_ctx *ctx, void *data_inout, int dtype, int snum, int tnum,
                    const double *b, const double *a, int ncoef, const double *zi);
int impdar_filtfilt_dev(impdar_ctx *ctx, void *d_data_inout, int dtype, int snum, int tnum,
                        const double *b, const double *a, int ncoef, const double *zi);
int impdar_fir_shift(impdar_ctx *ctx, void *data_inout, int dtype, int snum, int tnum,
                     const double *taps, int ntaps);
int impdar_fir_shift_dev(impdar_ctx *ctx, void *d_data_inout, int dtype, int snum, int tnum,
                         const double *taps, int ntaps);
int impdar_trace_lerp(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                      const int *lo, const int *hi, const double *den, const double *t,
                      int n_new, double *out);
int impdar_trace_lerp_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum,
                          const int *lo, const int *hi, const double *den, const double *t,
                          int n_new, double *d_out);

/* impdar_hfilt: RadarData.horizontalfilt (_RadarDataFiltering.py:93-135),
 * in place: row t loses (T)((T)mean(data[t, lo:hi]) * scale[t]) in the
 * data's own arithmetic (T = float32 or float64; the mean is summed in
 * fp64).  lo/hi are the clamped trace bounds, 0 <= lo < hi <= tnum; scale:
 * snum host doubles (the taper exp(-tt*0.05) / exp(-tt[0]*0.05)).
 * impdar_ahfilt: RadarData.adaptivehfilt (:19-90), in place: trace i loses
 * scale[t] * filtfilt([.25]*4, 1, mean(data[:, lo[i]:hi[i]], -1)), the
 * difference taken in fp64 and stored in the data's dtype; the mean of an
 * empty window (lo[i] == hi[i]) is NaN.  lo, hi: tnum host ints with
 * 0 <= lo[i] <= hi[i] <= tnum; scale: snum host doubles.  Fails with
 * scipy's message when snum <= 12 (filtfilt's padlen).  Run time does not
 * depend on the window sizes. */
int impdar_hfilt(impdar_ctx *ctx, void *data_inout, int dtype, int snum, int tnum,
                 int lo, int hi, const double *scale);
int impdar_hfilt_dev(impdar_ctx *ctx, void *d_data_inout, int dtype, int snum, int tnum,
                     int lo, int hi, const double *scale);
int impdar_ahfilt(impdar_ctx *ctx, void *data_inout, int dtype, int snum, int tnum,
                  const int *lo, const int *hi, const double *scale);
int impdar_ahfilt_dev(impdar_ctx *ctx, void *d_data_inout, int dtype, int snum, int tnum,
                      const int *lo, const int *hi, const double *scale);
/* impdar_winavg: RadarData.winavg_hfilt (:353-440), in place: trace i loses
 * scale[t] * (T)mean(data[:, lo[i]:hi[i]], -1), the difference taken in fp64
 * and stored in the data's dtype; no vertical smoothing, so any snum.  lo, hi,
 * scale as for impdar_ahfilt. */
int impdar_winavg(impdar_ctx *ctx, void *data_inout, int dtype, int snum, int tnum,
                  const int *lo, const int *hi, const double *scale);
int impdar_winavg_dev(impdar_ctx *ctx, void *d_data_inout, int dtype, int snum, int tnum,
                      const int *lo, const int *hi, const double *scale);

/* impdar_wiener: RadarData.denoise(ftype='wiener') (_RadarDataFiltering.py:552-587) =
 * scipy.signal.wiener(data, mysize=(vert_win, hor_win), noise): box means and
 * variances over the window (zero padding, always divided by the full
 * vert_win * hor_win; output i covers inputs i - w/2 .. i + (w-1)/2), noise =
 * mean(lVar) when noise_given == 0, out = lVar < noise ? lMean
 * : (x - lMean) * (1 - noise / lVar) + lMean.  Input float32 or float64 (float32
 * squares rounded to float32, as the reference squares in the data's dtype);
 * output: snum x tnum float64 (host buffer / device array).  *noise_used (may be
 * null) receives the noise applied.  An output whose window holds a non-finite
 * value is NaN (with an estimated noise every output is).  Fails with
 * IMPDAR_ERR_ARG ("Could not compute variance, specify noise for denoise") when
 * the estimated noise is exactly 0.  Bitwise repeatable; run time does not
 * depend on the window size.
 * impdar_median: scipy.ndimage.median_filter(data, size=(vert_win, hor_win)),
 * mode 'reflect', rank N/2 of N = vert_win * hor_win, into a separate buffer of
 * the input's dtype (float32 or float64).  Windows >= 1 in both axes, any size. */
int impdar_wiener(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int vert_win, int hor_win,
                  double noise, int noise_given, double *out, double *noise_used);
int impdar_wiener_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int vert_win, int hor_win,
                      double noise, int noise_given, double *d_out, double *noise_used);
int impdar_median(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int vert_win, int hor_win,
                  void *out);
int impdar_median_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int vert_win, int hor_win,
                      void *d_out);

/* impdar_hfiltfilt: scipy.signal.filtfilt(b, a, data, axis=1) along the trace axis
 * of a (snum, tnum) radargram: the reference's horizontal_band_pass, highpass and
 * lowpass (_RadarDataFiltering.py:138-350).  ncoef = len(b) = len(a), 2..17; zi
 * (ncoef - 1 values) = scipy.signal.lfilter_zi(b, a).  Odd extension by
 * padlen = 3 * ncoef samples computed in the input's arithmetic, initial state
 * zi * x0, forward pass, backward pass from zi * y0, all in fp64 in SciPy's
 * operation order.  Input float32 or float64; output snum x tnum float64 (host
 * buffer / device array), which may be the input itself when it is float64.  Each
 * row is filtered on its own (a NaN stays in its row).  Fails with IMPDAR_ERR_ARG
 * ("The length of the input vector x must be greater than padlen, which is N.")
 * when tnum <= padlen.  The fp64 forward pass, snum x (tnum + 2 * padlen), is
 * scratch the context keeps for the next call. */
int impdar_hfiltfilt(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *b,
                     const double *a, int ncoef, const double *zi, double *out);
int impdar_hfiltfilt_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const double *b,
                         const double *a, int ncoef, const double *zi, double *d_out);

/* ---- steps that change the sample axis (csrc/vaxis.hip) ------------------
 * impdar_row_lerp: the data part of RadarData.nmo and
 * constant_sample_depth_spacing (_RadarDataProcessing.py:50-61, :164-170): the
 * per-trace interp1d with abscissae shared by all traces, as a blend of rows:
 * out[i, :] = (data[hi[i], :] - data[lo[i], :]) / den[i] * t[i] + data[lo[i], :]
 * (the difference in the data's own arithmetic, the rest in fp64), out float64
 * (n_out, tnum); lo/hi/den/t are host arrays of n_out entries, 0 <= lo, hi < snum.
 * impdar_col_shift: RadarData.crop with a trace-wise pretrigger (:306-322,
 * shift = the trigger samples, n_out = snum - min(shift)) and elev_correct
 * (:618-625, shift = -top_inds, n_out = snum + max_samp):
 * out[i, j] = data[i + shift[j], j] where 0 <= i + shift[j] < snum, NaN
 * elsewhere; out float64 (n_out, tnum); shift: tnum host ints.
 * Input float32 or float64.  A scalar crop is a row range: impdar_cast_dev
 * with equal dtypes from the first kept row. */
int impdar_row_lerp(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                    const int *lo, const int *hi, const double *den, const double *t,
                    int n_out, double *out);
int impdar_row_lerp_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum,
                        const int *lo, const int *hi, const double *den, const double *t,
                        int n_out, double *d_out);
int impdar_col_shift(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                     const int *shift, int n_out, double *out);
int impdar_col_shift_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum,
                         const int *shift, int n_out, double *d_out);

/* ---- gains (csrc/gain.hip) -------------------------------------------------
 * impdar_rangegain: RadarData.rangegain (_RadarDataProcessing.py:456-471), in
 * place: data[i, j] = (T)((double)data[i, j] * gain[i]) for i >= start[j]
 * (NumPy's in-place product of float32 data and a float64 gain).  gain: snum
 * host doubles (travel_time * slope); start: tnum host ints, the first row of
 * each trace that is multiplied (snum or more: none).
 * impdar_agc: RadarData.agc (:474-496), in place: row i is multiplied by
 * (T)(scaling / m_i), m_i the largest |data| of rows [max(0, i - half),
 * min(i + half, snum)) (half = window // 2 >= 1), NaN if one of them holds a
 * NaN, 1e-6 where it is 0.  The window maximum is taken on the device.
 * impdar_row_absmax: the row maxima alone, max |data[i, :]| (NaN if the row
 * holds one) into snum host doubles: what agc needs of integer data, whose
 * truncated integer scale the host applies.
 * Input float32 or float64. */
int impdar_rangegain(impdar_ctx *ctx, void *data_inout, int dtype, int snum, int tnum,
                     const double *gain, const int *start);
int impdar_rangegain_dev(impdar_ctx *ctx, void *d_data_inout, int dtype, int snum, int tnum,
                         const double *gain, const int *start);
int impdar_agc(impdar_ctx *ctx, void *data_inout, int dtype, int snum, int tnum, int half, double scaling);
int impdar_agc_dev(impdar_ctx *ctx, void *d_data_inout, int dtype, int snum, int tnum, int half, double scaling);
int impdar_row_absmax(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, double *rowmax);

/* ---- steps that change the trace axis (csrc/taxis.hip) --------------------
 * impdar_restack: the data part of RadarData.restack (:405-453):
 * out[s, j] = mean(data[s, j * traces : (j + 1) * traces]) for j < tnum / traces
 * (a remainder is dropped), summed in fp64 in trace order; out float64
 * (snum, tnum / traces); traces odd.
 * impdar_reverse_dev: RadarData.reverse (:20-47) on a resident array, in place:
 * every row reversed (np.fliplr).
 * impdar_hcrop_dev: RadarData.hcrop (:340-402) on a resident array: traces
 * [lo, hi) of every row into d_out, (snum, hi - lo) of the same dtype.
 * On host arrays reverse and hcrop are a view and a slice and need no call.
 * Input float32 or float64. */
int impdar_restack(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int traces, double *out);
int impdar_restack_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int traces, double *d_out);
int impdar_reverse_dev(impdar_ctx *ctx, void *d_data_inout, int dtype, int snum, int tnum);
int impdar_hcrop_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int lo, int hi, void *d_out);

/* ---- layer picking (csrc/pick.hip) ------------------------------------------
 * The reference's picker (src/impdar/lib/picklib.py) and its continuity index
 * (src/impdar/lib/analysis/continuity_index.py) on a (snum, tnum) radargram,
 * float32 or float64.  The *_dev forms take a resident array; picks, outcomes
 * and the index always come back into host arrays.
 * The packet rule (picklib.packet_pick:139-199) with the pick parameters
 * plength, FWW, scst (PickParameters.freq_update) and pol (1 or -1): the packet
 * is trace[slice(trunc(mid - plength / 2.), trunc(mid + plength / 2.))]; a pick
 * is {top, centre, bottom, NaN, power}.  Outcomes: 0 picked, 1 packet shorter
 * than scst + FWW (the reference's 'frequency is too high' ValueError), 2 / 3
 * an empty argmax / argmin slice (NumPy's ValueError).
 * impdar_auto_pick: picklib.auto_pick (:51-93).  Seed k starts at row
 * seed_snum[k] of trace seed_tnum[k] (0 <= seed_tnum[k] < tnum), walks to trace
 * 0 and then from seed_tnum[k] + 1 to tnum - 1, each midpoint (top + bottom) // 2
 * of the pick before.  out: (nseeds, 5, tnum) host doubles; status: (nseeds, 2)
 * host ints, {outcome, trace} of the first pick that failed in the reference's
 * order (left walk first), {0, -1} if none did.  A walk stops where it fails;
 * what it did not reach is NaN.
 * impdar_pick_guided: picklib.pick (:16-48) on traces t0 ... t0 + n - 1, trace
 * t0 + i around row mid[i].  out: (5, n) host doubles, NaN where a pick failed;
 * status: {outcome, trace} of the first failing trace, {0, -1} if none.
 * impdar_continuity: continuity_index (:27-81).  s, b: tnum host ints, the
 * bounds of slice(surface, bed).indices(snum), or -1 for a NaN pick; cut_mode 1
 * takes int(len * cutoff_ratio) rows off both ends (none left when that is 0, as
 * the reference's p_ext[cut:-cut]).  out: tnum host doubles. */
int impdar_auto_pick(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int nseeds,
                     const int *seed_snum, const int *seed_tnum, int plength, int FWW, int scst, int pol,
                     double *out, int *status);
int impdar_auto_pick_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int nseeds,
                         const int *seed_snum, const int *seed_tnum, int plength, int FWW, int scst, int pol,
                         double *out, int *status);
int impdar_pick_guided(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int t0, int n,
                       const int *mid, int plength, int FWW, int scst, int pol, double *out, int *status);
int impdar_pick_guided_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int t0, int n,
                           const int *mid, int plength, int FWW, int scst, int pol, double *out, int *status);
int impdar_continuity(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *s,
                      const int *b, int cut_mode, double cutoff_ratio, double *out);
int impdar_continuity_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const int *s,
                          const int *b, int cut_mode, double cutoff_ratio, double *out);

/* ---- spectra (csrc/spectrum.hip) ---------------------------------------------
 * Diagnostics of a (snum, tnum) radargram, float32 or float64, host (no suffix)
 * or resident (_dev).  Data of either dtype is widened to float64 on load;
 * transforms, powers and sums run in float64 and the results are float64.
 * Sums are formed in a fixed order without atomics: two calls on the same data
 * give the same bits.  Any snum, tnum >= 1.
 * impdar_mean_spectrum: src/impdar/lib/plot.py:310-312 (axis 0) and :346-347
 * (axis 1): out[k] = mean over the other axis of |fft(data, axis)[k]|^2, the
 * unnormalised forward transform, k in numpy.fft.fftfreq order.  out: snum
 * (axis 0) or tnum (axis 1) host doubles in both forms, the upper half filled
 * by out[n - k] = out[k] (exact for real data).
 * impdar_periodogram: plot.py:654-674, scipy.signal.periodogram of every trace:
 * the trace's mean is subtracted, sample j multiplied by window[j] (snum host
 * doubles; null: a boxcar), and out[k, t] = |rfft|^2 * scale, doubled for every
 * k except 0 and, for even snum, snum / 2.  The caller derives `scale` from the
 * window and the sampling rate (1 / sum(w)^2 or 1 / (fs sum(w^2))).  out:
 * (snum / 2 + 1, tnum) float64, host for the host form, device for _dev (which
 * enqueues on the context's compute stream and returns without waiting).
 * impdar_spec_route_probe: what csrc/spec_route.h decides for `rows` sequences
 * of length n: out[0] = 0 own power-of-two transform, 1 own mixed-radix
 * transform, 2 rocFFT; out[1] workgroups; out[2] rows per workgroup; out[3]
 * bytes of LDS per workgroup.  No device call. */
int impdar_mean_spectrum(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int axis, double *out);
int impdar_mean_spectrum_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int axis, double *out);
int impdar_periodogram(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const double *window,
                       double scale, void *out);
int impdar_periodogram_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const double *window,
                           double scale, void *d_out);
int impdar_spec_route_probe(int n, long long rows, int *out);

/* ---- quad-polarised ApRES (csrc/quadpol.hip) --------------------------------
 * The reference's second native hook (src/impdar/lib/ApresData/coherence.h:13,
 * called at _QuadPolProcessing.py:139-146): the hhvv coherence of two padded
 * (range_bins, azimuth_bins) complex128 images, written into columns
 * ntheta ... azimuth_bins - ntheta - 1 of chhvv; the other columns are left as
 * they are.  Pointers are to (re, im) pairs of doubles, layout-compatible with
 * `double complex`.  Host arrays, device 0.  On anything it cannot do (no GPU,
 * a size below 1, a null pointer, no memory) those columns come back NaN and
 * one line goes to stderr. */
void coherence2d(double *chhvv, double *HH, double *VV, int nrange, int ntheta,
                 int range_bins, int azimuth_bins);

/* All arrays complex128 as interleaved (re, im) doubles, row-major.
 * impdar_qp_rotate: _QuadPolProcessing.py:87-99.  shh, shv, svh, svv: n values;
 * cos2, sincos, sin2: n_thetas host doubles, cos^2, sin cos and sin^2 of every
 * azimuth; HH, HV, VH, VV: (n, n_thetas).
 * impdar_qp_coherence: (:153-165)  chhvv[j, i] = S(HH conj(VV)) /
 * sqrt(S|HH|^2 S|VV|^2), S over rows [max(0, j - nrange), min(n - 1, j + nrange))
 * and columns [i - ntheta, i + ntheta) of the (n, ncols) images; a zero
 * denominator gives NaN in both parts.  wrap != 0: the columns are periodic
 * over ncols and chhvv is (n, ncols); wrap == 0: the images are already padded,
 * chhvv is (n, ncols - 2 ntheta) and its column i is centred on input column
 * i + ntheta.  Every window sum is made of additions only (no differences of
 * running sums).  nrange >= 1, 1 <= ntheta, and ntheta <= ncols (wrap) or
 * 2 ntheta < ncols (as given).
 * impdar_qp_phase_gradient: (:199-216)  dphi_dz = (R dI - I dR) / (R^2 + I^2),
 * R, I the parts of the (n, m) chhvv, dR, dI their numpy.gradient along the
 * rows with impdar_kirchhoff's coefficients (grad_uniform, grad_h, ga, gb, gc);
 * dphi_dz is (n, m) float64.  With b != NULL, R and I first go through
 * impdar_filtfilt (b, a, zi of ncoef coefficients) along the rows: the
 * reference's lowpass.
 * impdar_qp_power_anomaly: (:303-319)  pa = 10 log10(HV^2) - nanmean over each
 * row, complex arithmetic as NumPy does it (a zero element gives -inf + NaN j
 * and, like every element with a NaN in either part, is left out of the mean).
 * HV: (n, m) complex128.  pa: ONE (n, 2 m) float64 array, row j holding the m
 * real parts and then the m imaginary parts, the layout impdar_filtfilt_dev
 * filters in a single call.  The row sum has one order whatever the entry
 * point: lane l of a 64-lane wavefront adds columns l, l + 64, ... in turn, the
 * lane sums meet in a butterfly over distances 32, 16, 8, 4, 2, 1.
 * impdar_qp_find_cpe: (:225-272)  that anomaly, impdar_filtfilt (b, a, zi of
 * ncoef coefficients) along the rows, then per row numpy.argmin of the complex
 * values in columns [idx_start, idx_stop): the first element with a NaN in
 * either part, else the least in (real, imag) order, ties to the lowest
 * column.  cpe_idxs: n int32 column numbers (idx_start is included).  pa, when
 * not NULL, receives the filtered anomaly in the (n, 2 m) layout.
 * 0 <= idx_start < idx_stop <= m; n <= 3 ncoef fails with scipy's message.
 * impdar_qp_find_cpe_last_ms: device time of the three stages of the last
 * find_cpe on this context (waits for it).
 * impdar_qp_cpe_gather: out[j] = image[j, idx[j]] of an (n, m) float64 or
 * (is_complex != 0) complex128 image; idx: n int32.  An index outside [0, m)
 * gives NaN.
 * The *_dev forms take device arrays (the tables stay host arrays), enqueue on
 * the context's compute stream and return without waiting for it. */
int impdar_qp_rotate(impdar_ctx *ctx, const double *shh, const double *shv, const double *svh, const double *svv, int n,
                     const double *cos2, const double *sincos, const double *sin2, int n_thetas,
                     double *HH, double *HV, double *VH, double *VV);
int impdar_qp_rotate_dev(impdar_ctx *ctx, const double *d_shh, const double *d_shv, const double *d_svh,
                         const double *d_svv, int n, const double *cos2, const double *sincos, const double *sin2,
                         int n_thetas, double *d_HH, double *d_HV, double *d_VH, double *d_VV);
int impdar_qp_coherence(impdar_ctx *ctx, const double *HH, const double *VV, int n, int ncols, int nrange, int ntheta,
                        int wrap, double *chhvv);
int impdar_qp_coherence_dev(impdar_ctx *ctx, const double *d_HH, const double *d_VV, int n, int ncols, int nrange,
                            int ntheta, int wrap, double *d_chhvv);
int impdar_qp_phase_gradient(impdar_ctx *ctx, const double *chhvv, int n, int m, int grad_uniform, double grad_h,
                             const double *ga, const double *gb, const double *gc, const double *b, const double *a,
                             int ncoef, const double *zi, double *dphi_dz);
int impdar_qp_phase_gradient_dev(impdar_ctx *ctx, const double *d_chhvv, int n, int m, int grad_uniform, double grad_h,
                                 const double *ga, const double *gb, const double *gc, const double *b, const double *a,
                                 int ncoef, const double *zi, double *d_dphi_dz);
int impdar_qp_power_anomaly(impdar_ctx *ctx, const double *HV, int n, int m, double *pa);
int impdar_qp_power_anomaly_dev(impdar_ctx *ctx, const double *d_HV, int n, int m, double *d_pa);
int impdar_qp_find_cpe(impdar_ctx *ctx, const double *HV, int n, int m, const double *b, const double *a, int ncoef,
                       const double *zi, int idx_start, int idx_stop, int *cpe_idxs, double *pa);
int impdar_qp_find_cpe_dev(impdar_ctx *ctx, const double *d_HV, int n, int m, const double *b, const double *a, int ncoef,
                           const double *zi, int idx_start, int idx_stop, int *d_cpe_idxs, double *d_pa);
int impdar_qp_find_cpe_last_ms(impdar_ctx *ctx, float *anomaly_ms, float *filter_ms, float *argmin_ms);
int impdar_qp_cpe_gather(impdar_ctx *ctx, const double *image, int is_complex, int n, int m, const int *idx, double *out);
int impdar_qp_cpe_gather_dev(impdar_ctx *ctx, const double *d_image, int is_complex, int n, int m, const int *d_idx,
                             double *d_out);

/* ---- ApRES range conversion, stacking, phase difference (csrc/apres.hip) ----
 * Everything float64 / complex128 (interleaved (re, im) doubles), row-major.
 * impdar_apres_range: _ApresDataProcessing.py:84-113 for `rows` = bnum cnum
 * chirps of `snum` real samples: de-mean, window, real transform of length
 * N = p snum, nf = N / 2 (rounded down) bins of which the first n are kept:
 *   spec[r, k] = X[r, k] scale_mul (1 / scale_div)                   k < n
 *   data[r, k] = comp[k] spec[r, k]                                  k < n
 *   Rfine[r, k] = atan2(im, re of data) / den[k]                     k < nf
 * or, with first_order != 0, (lambdac atan2(im, re)) / den[k] (phase2range's
 * first-order branch with den[k] = 4 pi; lambdac is not read otherwise).
 * win: snum, comp: nf complex, den: nf host values.  spec, data: (rows, n);
 * Rfine: (rows, nf).  n == 0 writes Rfine alone (spec and data may be null).
 * The chirps are transformed `chunk` at a time, 0 for the library's choice
 * (256 MiB of scratch); the results do not depend on it.
 * snum < 2, p < 1, n > nf, a null table are IMPDAR_ERR_ARG before any device work.
 * impdar_apres_range_last_ms: device time of the three stages of the last
 * range conversion on this context, summed over its chunks (waits for it).
 * impdar_apres_stack: (:191-222) out[g, j] = mean of rows g m ... g m + m - 1
 * of the (rows, snum) array `data`, float64 or (is_complex != 0) complex128,
 * g < groups, groups m <= rows: a sum in row order, then numpy.mean's last
 * step (a division by m; for complex data a product with 1 / m).
 * impdar_apres_phase_diff: _TimeDiffProcessing.py:75-91.  co[i] = S(s1 conj(s2))
 * / sqrt(S|s1|^2 S|s2|^2), S over samples [i step, i step + 2 (win / 2)) of two
 * complex128 vectors of `len` samples, i < ceil((len - 2 (win / 2)) / step)
 * (none when that is not positive); a zero denominator gives NaN in both
 * parts.  Sums are additions only.
 * The *_dev forms take device arrays (the tables stay host arrays), enqueue on
 * the context's compute stream and return without waiting for it. */
int impdar_apres_range(impdar_ctx *ctx, const double *raw, int rows, int snum, int p, int n, const double *win,
                       const double *comp, const double *den, double scale_mul, double scale_div, int first_order,
                       double lambdac, int chunk, double *spec, double *data, double *rfine);
int impdar_apres_range_dev(impdar_ctx *ctx, const double *d_raw, int rows, int snum, int p, int n, const double *win,
                           const double *comp, const double *den, double scale_mul, double scale_div, int first_order,
                           double lambdac, int chunk, double *d_spec, double *d_data, double *d_rfine);
int impdar_apres_range_last_ms(impdar_ctx *ctx, float *prep_ms, float *fft_ms, float *post_ms);
int impdar_apres_stack(impdar_ctx *ctx, const double *data, int is_complex, int rows, int snum, int groups, int m,
                       double *out);
int impdar_apres_stack_dev(impdar_ctx *ctx, const double *d_data, int is_complex, int rows, int snum, int groups, int m,
                           double *d_out);
int impdar_apres_phase_diff(impdar_ctx *ctx, const double *s1, const double *s2, int len, int win, int step, double *co);
int impdar_apres_phase_diff_dev(impdar_ctx *ctx, const double *d_s1, const double *d_s2, int len, int win, int step,
                                double *d_co);

/* ---- an ApRES burst's counts to volts (csrc/apres.hip) ----
 * load_apres.py:391-395: volts[i] = (double)counts[i] * 2.5 / 65536., then
 * / divisor unless divisor == 1 (the reference's n_subbursts n_attenuators of
 * an averaged burst).  counts: `n` little-endian elements in HOST memory at
 * any byte offset (a file's image as it was read), uint16 (kind 0) or uint32
 * (kind 1, Average=2).  One flat run: rows do not matter.  Bit for bit NumPy's
 * expression: the product is exact, / 65536 moves the exponent, the last
 * division is IEEE's, and nothing is a reciprocal product.
 * The counts go up as they are, 2 (4) bytes per sample, in pieces through two
 * slots of the context's pinned staging buffer; the kernel of one piece runs
 * under the copy of the next.  impdar_apres_decode writes host memory and
 * waits; impdar_apres_decode_dev writes `n` doubles of an 8-byte aligned
 * device array -- the (rows, snum) chirps impdar_apres_range_dev reads -- and
 * returns once the counts have left the host (the last kernels still run on
 * the compute stream).  impdar_ctx_last_kernel_ms after either gives the time
 * from the first kernel's start to the last one's end: the kernel alone when
 * the counts went up in one piece.
 * n < 0, another kind, a null pointer with n > 0, a divisor that is not
 * finite and positive are IMPDAR_ERR_ARG before any device work; n == 0
 * succeeds and touches nothing.  Not here: Average=1 (the reference cannot read
 * it either), formats 2-4 of the burst header.
 * impdar_apres_decode_pieces_dev: impdar_apres_decode_dev with `piece_counts`
 * counts going up at a time (rounded up to a multiple of 8), 0 for the
 * library's choice, 8 MiB of counts: for tests, and for timing the kernel
 * alone.  The result does not depend on it. */
int impdar_apres_decode(impdar_ctx *ctx, const void *counts_host, int kind, long long n, double divisor, double *volts_host);
int impdar_apres_decode_dev(impdar_ctx *ctx, const void *counts_host, int kind, long long n, double divisor, void *d_volts);
int impdar_apres_decode_pieces_dev(impdar_ctx *ctx, const void *counts_host, int kind, long long n, double divisor,
                                   void *d_volts, long long piece_counts);

/* ---- instrument files decoded in HBM (csrc/rawload.hip, csrc/rawload_route.h) ----
 * A raw buffer of `nbytes` bytes -- a GSSI .DZT, pulseEKKO .DT1, RAMAC .rd3 or
 * Tek .DAT file as it is on disk -- holds `tnum` little-endian records: record
 * t starts at byte base + t * stride, its `snum` samples of `in_kind` at byte
 * `head` of it (unsigned counts are the same bits as signed: I16 / I32).  With
 * v[s, t] = sample s of record t, the native result of `op` is
 *   NONE       v;
 *   GSSI_TOP   rows 0 and 1 take row 2's values (load_gssi.py:210-211); I16, I32;
 *   TEK_BIAS   v - 512 in int16, wrapping (load_tek.py:73-74); I16;
 *   PE_DEMEAN  v minus np.nanmean of the trace's first min(100, snum) samples
 *              (load_pulse_ekko.py:238-239), bit for bit: the mean in NumPy's
 *              summation order in float64, the difference in float64, stored
 *              as NumPy stores it into int16 (truncated through int32, low 16
 *              bits) or float32 (to nearest even); I16, F32.
 * out_kind NATIVE keeps int16 / int32 / float32, F32 and F64 convert the native
 * value as astype does.  out: (snum, tnum) row-major of that type in device
 * memory, aligned to its element.
 * impdar_rawload_plan: the check alone, *out_bytes = snum * tnum * sizeof(out);
 * it needs no context and no device.  IMPDAR_ERR_ARG: snum or tnum < 1, a
 * negative size, head + snum * elem > stride, base + (tnum - 1) * stride +
 * head + snum * elem > nbytes, GSSI_TOP with snum < 3, any product that
 * overflows 64 bits.  IMPDAR_ERR_UNSUPPORTED: an op / kind pair not listed.
 * No kernel runs on a descriptor the plan rejects.
 * impdar_rawload_dev: raw bytes already in HBM (any byte alignment); enqueues on
 * the compute stream and returns.  impdar_rawload: host bytes, uploaded as they
 * are into scratch the context keeps, decoded by the same kernels; returns
 * when the bytes have left the host and the result is complete.
 * impdar_ctx_last_kernel_ms after either gives the decode kernels alone. */
enum { IMPDAR_RAW_I16 = 0, IMPDAR_RAW_I32 = 1, IMPDAR_RAW_F32 = 2 };
enum { IMPDAR_RAW_NONE = 0, IMPDAR_RAW_GSSI_TOP = 1, IMPDAR_RAW_TEK_BIAS = 2, IMPDAR_RAW_PE_DEMEAN = 3 };
enum { IMPDAR_RAW_OUT_NATIVE = 0, IMPDAR_RAW_OUT_F32 = 1, IMPDAR_RAW_OUT_F64 = 2 };
int impdar_rawload_plan(long long nbytes, long long base, long long stride, long long head, int snum, int tnum, int in_kind,
                        int op, int out_kind, long long *out_bytes);
int impdar_rawload_dev(impdar_ctx *ctx, const void *d_raw, long long nbytes, long long base, long long stride, long long head,
                       int snum, int tnum, int in_kind, int op, int out_kind, void *d_out);
int impdar_rawload(impdar_ctx *ctx, const void *raw_host, long long nbytes, long long base, long long stride, long long head,
                   int snum, int tnum, int in_kind, int op, int out_kind, void *d_out);

/* ---- the time-offset search of kinematic GPS control (csrc/gpstrack.hip, csrc/gps_route.h) ----
 * gpslib.py:420-427 of the reference for `ncand` candidate offsets at once.  All
 * arrays are HOST float64.  gps_t (non-decreasing, no NaN), gps_lat, gps_lon:
 * the `ngps` fixes; t, lat, lon: the `tnum` traces' decimal day, radar latitude
 * and radar longitude % 360.  For candidate c the fixes' times are
 *   x[k] = (gps_t[k] + search[c]) + base        (float64, in that order)
 * and the track is interpolated to every t[j] as SciPy's interp1d(kind='linear')
 * does it, bit for bit:
 *   extrapolate == 0  np.interp: bracket x[j] <= t < x[j+1]; y[j] where t == x[j]
 *     or j is the last fix, else slope (t - x[j]) + y[j] with NumPy's NaN
 *     fallback from the other knot.  A non-NaN t outside [x[0], x[ngps-1]] counts
 *     into nout[c] and takes no part in the sums (the reference raises there);
 *   extrapolate == 1  interp1d._call_linear: idx = searchsorted(x, t, 'left')
 *     clipped to [1, ngps-1], ((y_hi - y_lo) / (x_hi - x_lo)) (t - x_lo) + y_lo;
 *     nout[c] = 0.
 * Duplicate x give what IEEE gives.  cc[c] = r(lat_i, lat) + r(lon_i, lon), r
 * the Pearson correlation over the pairs where neither value is NaN (latitude and
 * longitude masked separately): means first, then sum dx dy / sqrt(sum dx^2
 * sum dy^2), clipped to [-1, 1]; fewer than 2 pairs or a zero variance: NaN.
 * float64 sums whose order depends on the trace index alone, no atomics: two calls
 * return the same bits.  probe = c >= 0 also writes candidate c's interpolated
 * latitude and longitude (tnum each, NaN where the trace was left out).
 * IMPDAR_ERR_ARG before any device work: ngps < 2, tnum < 1, ncand < 1, extrapolate
 * not 0 or 1, a decreasing or NaN gps_t, probe >= ncand, sizes whose products
 * overflow 64 bits or more candidates than a launch has workgroups (2^31 - 1).
 * impdar_gps_cc_plan: the checks on the sizes alone, *scratch_bytes = the device
 * bytes of the call; no context, no device.
 * impdar_ctx_last_kernel_ms after impdar_gps_cc gives the search kernel alone. */
int impdar_gps_cc_plan(long long ngps, long long tnum, long long ncand, int extrapolate, long long *scratch_bytes);
int impdar_gps_cc(impdar_ctx *ctx, const double *gps_t, const double *gps_lat, const double *gps_lon, long long ngps,
                  const double *t, const double *lat, const double *lon, long long tnum, double base, const double *search,
                  long long ncand, int extrapolate, double *cc, long long *nout, long long probe, double *probe_lat,
                  double *probe_lon);

/* ---- the window search of the attenuation methods 3 and 6b (csrc/attsearch.hip, csrc/att_route.h) ----
 * analysis/attenuation.py of the reference: attenuation_method3 (flavour 0, index
 * windows) and attenuation_method6b (flavour 1, depth windows) for `ncent` centres
 * in one launch.  All arrays are HOST; float64 throughout.  z, pc: the `n` NaN-free
 * (depth in km, 10 log10 corrected power) pairs -- of one pick in trace order
 * (flavour 0), or of the pooled picks sorted by z, non-decreasing (flavour 1).  ns:
 * the `nn` candidate rates, ns[j0] == 0.  A centre walks nested windows:
 *   flavour 0  centre b is trace tr = first + b; the window of width `win` is
 *     [tr - win/2, tr + win/2) (integer division), visited while win/2 <= tr and
 *     win/2 <= n - tr; then win += win_step.  win_init >= 2, win_step >= 1, both
 *     integers handed over as doubles;
 *   flavour 1  centre b is the depth d = centres[b]; the window is the contiguous
 *     range with |z - d| < win/2 evaluated in float64, visited while
 *     d - win/2 >= z[0] and d + win/2 <= z[n-1]; then win += win_step, a repeated
 *     float64 addition.
 * At each window, for every rate N = ns[j]: pa = pc + 2 z N and
 *   C[j] = |sum (z - mean z)(pa - mean pa) / (sqrt(sum (z - mean z)^2) sqrt(sum (pa - mean pa)^2))|;
 * Cm = min C; if Cm < cw and C[j0] > cw then Nh = max ns[C < cw] - min ns[C < cw]
 * (halved for flavour 1).  The walk ends when Nh <= nh_target (Nh starts at
 * nh_target + 1) or the next window leaves the record.  Per centre:
 *   code 0  idx = the j of the minimum of the last window visited;
 *   code 1  no window was visited (idx = -1);
 *   code 2  that minimum is attained by more than one rate (idx = the first);
 *   code 3  a window was empty or held a C that is NaN or Inf: the walk stopped
 *           there and the caller decides (NumPy's comparison rules are not restated);
 *   win = the width after the last increment (win_init for code 1).
 * The sums have a fixed order per window, no atomics: two calls return the same
 * bits.  probe = b >= 0 also writes the C rows of every window centre b visited
 * to probe_c (row-major, nn per row, at most probe_cap rows) and their number to
 * *probe_rows (which may exceed probe_cap).
 * IMPDAR_ERR_ARG before any device work: n, nn or ncent < 1, a flavour other than
 * 0 / 1, win_init < 2 or win_step < 1 or a fraction (flavour 0), a width or step
 * that is not positive and finite (flavour 1), j0 outside [0, nn), first < 0,
 * a decreasing, NaN or infinite z (flavour 1), a flavour 1 walk that could not end
 * -- win_step so small that 2 (z[n-1] - z[0]) + win_step / 2 == 2 (z[n-1] - z[0]), or
 * (z[n-1] - z[0]) / win_step above 2^20 --, probe >= ncent or probe_cap < 1 with a probe,
 * sizes whose products overflow 64 bits, more centres than a launch has
 * workgroups (2^31 - 1).
 * impdar_att_search_plan: the checks on the sizes alone, *scratch_bytes = the
 * device bytes of the call; no context, no device.
 * impdar_ctx_last_kernel_ms after impdar_att_search gives the search kernel alone. */
int impdar_att_search_plan(int flavour, long long n, long long nn, long long ncent, double win_init, double win_step,
                           long long probe, long long probe_cap, long long *scratch_bytes);
int impdar_att_search(impdar_ctx *ctx, int flavour, const double *z, const double *pc, long long n, const double *ns,
                      long long nn, long long j0, const double *centres, long long first, long long ncent, double win_init,
                      double win_step, double cw, double nh_target, long long *idx, double *win, int *code,
                      long long probe, double *probe_c, long long probe_cap, long long *probe_rows);

/* ---- what a plot reads from the radargram (csrc/display.hip) ----
 * data: (snum, tnum) float32 / float64, row-major; a window is rows [y0, y1),
 * traces [x0, x1) of it, 0 <= y0 <= y1 <= snum, 0 <= x0 <= x1 <= tnum.
 * impdar_order_stats: the neighbours of np.percentile's linear method.
 * counts[0] = N, the elements of the window; counts[1] = how many are NaN.
 * With n = N - counts[1] and, in float64, lo = floor((n - 1) (q[i] / 100)),
 * hi = min(lo + 1, n - 1): vals[2 i] and vals[2 i + 1] (of the data's dtype)
 * are the values of rank lo and hi among the window's n values that are no
 * NaN -- exactly, as a sort would place them (-0.0 and 0.0 count as equal).
 * 1 <= nq <= 8, 0 <= q[i] <= 100.  Where n == 0, or skip_nan == 0 and the
 * window holds a NaN, vals are NaN and the call succeeds: the counts say so.
 * Integer atomics only: two calls give the same bits.
 * impdar_flatten: out is (snum, x1 - x0) of the data's dtype,
 *   out[i, j] = data[i - shift[j], x0 + j]   where 0 <= i - shift[j] < snum,
 * NaN elsewhere and in every column with shift[j] == IMPDAR_FLATTEN_NONE
 * (plot.py:240-254 with shift = int(offset), NONE for a NaN offset).  shift:
 * x1 - x0 host values; x1 > x0.
 * impdar_window_dev: the window of a resident array into the dense
 * (y1 - y0, x1 - x0) host array `out`; waits for the copy.
 * The *_dev forms take device arrays; counts, vals, q and shift stay host
 * arrays.  impdar_order_stats_dev waits for its result; impdar_flatten_dev
 * enqueues on the context's compute stream and returns. */
#define IMPDAR_FLATTEN_NONE (-2147483647 - 1)
int impdar_order_stats(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int y0, int y1, int x0, int x1,
                       const double *q, int nq, int skip_nan, long long *counts, void *vals);
int impdar_order_stats_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int y0, int y1, int x0,
                           int x1, const double *q, int nq, int skip_nan, long long *counts, void *vals);
int impdar_flatten(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int x0, int x1, const int *shift,
                   void *out);
int impdar_flatten_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int x0, int x1,
                       const int *shift, void *d_out);
int impdar_window_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int y0, int y1, int x0, int x1,
                      void *out);

/* float32 <-> float64 conversion of a resident array of `n` elements (NumPy's astype, on the device) */
int impdar_cast_dev(impdar_ctx *ctx, const void *d_src, int src_dtype, void *d_dst, int dst_dtype, size_t n);

/* ---- communicator (RCCL over xGMI) ------------------------------------- */
#define IMPDAR_UNIQUE_ID_BYTES 128
int impdar_comm_unique_id(char id[IMPDAR_UNIQUE_ID_BYTES]);
int impdar_comm_init(impdar_ctx *ctx, const char id[IMPDAR_UNIQUE_ID_BYTES], int rank, int nranks);
int impdar_comm_rank(const impdar_ctx *ctx);
int impdar_comm_size(const impdar_ctx *ctx);
/* RCCL's own view of the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice / ncclGetVersion); any
 * pointer may be null */
int impdar_comm_info(const impdar_ctx *ctx, int *ranks, int *rank, int *device, int *version);
int impdar_comm_barrier(impdar_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* IMPDAR_HIP_H */
