// Shared host-side plumbing for the impdar HIP library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <string>
#include <vector>
#include "../../include/impdar_hip.h"

struct ncclComm;

struct impdar_ctx {
    int device = 0;
    hipStream_t stream = nullptr;   // compute stream (migration kernels, copies)
    hipStream_t aux = nullptr;      // producer stream: prep / table / all-gather of the NEXT radargram
    // RCCL communicator (null until impdar_comm_init)
    ncclComm *comm = nullptr;
    int rank = 0;
    int nranks = 1;
    // pinned host staging for the one-shot (host-buffer) entry points: device -> pinned at PCIe speed,
    // then pinned -> the caller's pageable buffer on several threads (first touch of a fresh result
    // array is a page fault per 4 KiB; the faults parallelise, a single D2H into it does not)
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    std::mutex pinned_mu;           // held for a whole staged download (the buffer may be re-allocated by the next one)
    // a staging buffer on its way: allocated by a thread of its own while the call that will need it plans, uploads and
    // computes (hipHostMalloc pins ~4.5 GB/s: 36 ms for the 164 MB of a config-3 image -- the largest term of a first call)
    std::thread pin_thread;
    void *pin_next = nullptr;
    size_t pin_next_bytes = 0;
    // last work enqueued on `stream` by a *_dev entry point that WRITES a caller-visible device array; consumers
    // on the producer stream (impdar_kirch_prep) wait for it
    hipEvent_t ev_produced = nullptr;
    bool produced = false;
    // device-side duration of the last Stolt / phase-shift call enqueued on `stream` (impdar_ctx_last_ms)
    hipEvent_t ev_tic = nullptr, ev_toc = nullptr;
    bool timed = false;
    // ... and of its dominant kernel alone (the frequency sum of a phase-shift call: impdar_ctx_last_kernel_ms)
    hipEvent_t ev_ktic = nullptr, ev_ktoc = nullptr;
    bool ktimed = false;
    // what the last migration entry point on this context did (impdar_ctx_last_metrics): its name, the kernel that did
    // the sums, that kernel's time when the entry point measured it itself (< 0: read ev_ktic / ev_ktoc), and further
    // "key": value pairs of JSON
    const char *m_entry = nullptr, *m_kernel = nullptr;
    float m_kernel_ms = -1.f;
    char m_extra[320] = "";
};

// "this entry point ran this kernel, nothing was timed, no further metrics"
static inline void impdar_ctx_note(impdar_ctx *ctx, const char *entry, const char *kernel)
{
    ctx->m_entry = entry;
    ctx->m_kernel = kernel;
    ctx->m_kernel_ms = -1.f;
    ctx->timed = ctx->ktimed = false;
    ctx->m_extra[0] = 0;
}

// The staging buffer of a download (download.hip) is a RING of at most 64 MB, not the whole image: pinning costs 0.22 ms
// per MB -- the 164 MB of a config-3 Kirchhoff image, the 268 MB of an 8192^2 float32 one (59 ms) were the largest term of
// a process's first call.  Pieces of <= 16 MB go round it, up to four DMAs in flight: the copy of a piece is enqueued as
// soon as the host threads have copied (or widened) the piece that held its room out of the ring.
// (same-box A/B of the steady call at config 3, ring 32 / 64 / 96 / 128 MB / whole image: 16.4 / 13.2 / 12.9 / 13.0 / 13.0 ms;
// the first call of a process: 52 ms with 64 MB, 66 ms with 96 MB -- more than the call can pin behind its plan
// before the first block is ready to leave.  64 MB.)
constexpr size_t IMPDAR_STAGE_RING_BYTES = (size_t)64 << 20;
// start allocating a pinned staging buffer of `bytes` unless the context has one (impdar_ctx_pinned adopts it)
void impdar_ctx_pinned_prefetch(impdar_ctx *ctx, size_t bytes);
// bracket the device work of one call on ctx->stream (read back by impdar_ctx_last_ms)
int impdar_ctx_tic(impdar_ctx *ctx);
int impdar_ctx_toc(impdar_ctx *ctx);
// bracket the dominant kernel(s) inside such a call (read back by impdar_ctx_last_kernel_ms)
int impdar_ctx_ktic(impdar_ctx *ctx);
int impdar_ctx_ktoc(impdar_ctx *ctx);

// record "everything enqueued on ctx->stream so far produces data a later call may read" (see impdar_kirch_prep)
int impdar_ctx_mark_produced(impdar_ctx *ctx);

// grow-only pinned staging buffer of the context; nullptr when the allocation fails (callers fall back to pageable
// memory).  Callers hold ctx->pinned_mu.
void *impdar_ctx_pinned(impdar_ctx *ctx, size_t bytes);
// the context is going away: its staging buffer, and one on its way, are freed
void impdar_ctx_pinned_release(impdar_ctx *ctx);
// device -> host through the staging ring and a threaded copy (below 1 MiB: a plain D2H); synchronises `st`
int impdar_download(impdar_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes, hipStream_t st);
// several output-trace blocks of one image, each after its own event, copies and host widening pipelined across blocks
// (one block with width == ld: a flat array)
int impdar_download_blocks_f64(impdar_ctx *ctx, double *dst_host, size_t ld, size_t rows, int dtype, int nblk,
                               const size_t *col0, const size_t *width, const void *const *src, const hipEvent_t *after,
                               hipStream_t st);

// device arrays of the one-shot calls, from a small cache of freed ones (api.hip); the caller of _free has synchronised their users
int impdar_devcache_alloc(int device, size_t bytes, void **dptr);
void impdar_devcache_free(void *p);

void impdar_set_error(const char *fmt, ...);
// IMPDAR_TRACE=1: one line on stderr per milestone of a call ("[impdar +12.3 ms] stolt: plans ready"), the time since the
// library's first trace point -- where a first call's time goes (profiles/r05_first_call.txt).  A no-op otherwise.
bool impdar_trace_on();
void impdar_trace(const char *fmt, ...);

#define IMPDAR_HIP_CHECK(expr)                                                        \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            impdar_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,            \
                             hipGetErrorString(_e));                                  \
            return IMPDAR_ERR_HIP;                                                    \
        }                                                                             \
    } while (0)

#define IMPDAR_ARG_CHECK(cond, ...)                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            impdar_set_error(__VA_ARGS__);                                            \
            return IMPDAR_ERR_ARG;                                                    \
        }                                                                             \
    } while (0)

static inline size_t impdar_dtype_size(int dtype) { return dtype == IMPDAR_F64 ? 8 : 4; }
static inline bool impdar_dtype_ok(int dtype) { return dtype == IMPDAR_F32 || dtype == IMPDAR_F64; }

// Drop what the entry points keep between calls -- the one-shot Kirchhoff plan with its images and staging copies
// (hundreds of MB at config 3), the mig_kirch_loop plan, the Stolt and phase-shift plans with their spectra (GBs at
// 8192^2) -- except what a call in progress on this thread's stack is using (their mutexes are only tried).  Called by
// DevBuf::ensure when hipMalloc reports out of memory, before it tries once more: a large call after a large call
// of another kind must not fail on memory that only a cache is holding.
void impdar_release_caches();
// "this thread is inside the entry point that owns cache X": its trim must not even try the (non-recursive) mutex
struct ImpdarBusy {
    bool &flag;
    explicit ImpdarBusy(bool &f) : flag(f) { flag = true; }
    ~ImpdarBusy() { flag = false; }
};

// RAII device buffer bound to a context's device.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, n);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            p = nullptr;
            // the trims destroy cached plans of other contexts and set THEIR device while doing so: come back to ours
            int dev = -1;
            const bool have_dev = hipGetDevice(&dev) == hipSuccess;
            impdar_release_caches();
            if (have_dev) (void)hipSetDevice(dev);
            e = hipMalloc(&p, n);
        }
        if (e == hipSuccess) bytes = n;
        else p = nullptr;
        return e;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// The two device arrays of a host entry point's call (impdar_stolt, impdar_stolt_scan, impdar_phaseshift), from the cache of freed
// ones (api.hip: no hipMalloc / hipFree per call).  The call uploads into din, runs, downloads from dout; the arrays go back
// when it returns, after a synchronisation: nothing in flight may still touch them.
struct CallArrays {
    impdar_ctx *ctx;
    void *din = nullptr, *dout = nullptr;
    // outb = 0: the call has no second array
    int alloc(size_t inb, size_t outb)
    {
        const int rc = impdar_devcache_alloc(ctx->device, inb, &din);
        return rc || !outb ? rc : impdar_devcache_alloc(ctx->device, outb, &dout);
    }
    ~CallArrays()
    {
        if (!din) return;                                 // (the call ended before it had one)
        (void)hipStreamSynchronize(ctx->stream);
        impdar_devcache_free(din);
        impdar_devcache_free(dout);
    }
};

// The small host tables of a step (gains, windows, row indices): `blk` blocks packed at 16-byte-rounded offsets of
// one device buffer, so a table of doubles stays aligned whatever precedes it.
struct TableBlock {
    const void *src;
    size_t bytes;
};
static inline size_t impdar_round16(size_t n) { return (n + 15) & ~(size_t)15; }

// One packed synchronous copy of the tables into `buf`, their device addresses into `dev`: the caller's host arrays
// are free to go away on return (the stream is drained first because the previous launch may still read `buf`).
template <int N> static int impdar_upload_tables(impdar_ctx *ctx, DevBuf &buf, const TableBlock (&blk)[N], const void *(&dev)[N])
{
    size_t total = 0;
    for (int k = 0; k < N; ++k) total += impdar_round16(blk[k].bytes);
    IMPDAR_HIP_CHECK(buf.ensure(total));
    std::vector<char> pack(total);
    size_t off = 0;
    for (int k = 0; k < N; ++k) {
        memcpy(pack.data() + off, blk[k].src, blk[k].bytes);
        dev[k] = buf.as<char>() + off;
        off += impdar_round16(blk[k].bytes);
    }
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    IMPDAR_HIP_CHECK(hipMemcpy(buf.p, pack.data(), total, hipMemcpyHostToDevice));
    return IMPDAR_OK;
}

// What a unit of processing steps (preproc.hip, hfilt.hip, denoise.hip, hpass.hip, vaxis.hip, gain.hip, taxis.hip,
// quadpol.hip, apres.hip, pick.hip, spectrum.hip, display.hip, rawload.hip, gpstrack.hip, attsearch.hip, decon.hip, attr.hip, slope.hip) keeps between calls: its buffers -- `Bufs`, with a release() that frees every one of them -- and the context they
// belong to.  One set per process and step: entry points of different contexts / threads take turns, each holding
// lock() from its argument check to its return (re-entrant because the host-buffer forms call the resident ones).
template <class Bufs> struct StepScratch : Bufs {
    impdar_ctx *owner = nullptr;
    std::recursive_mutex mu;
    std::unique_lock<std::recursive_mutex> lock() { return std::unique_lock<std::recursive_mutex>(mu); }
    // buffers live on the owner's device: a call on another context starts from none
    void bind(impdar_ctx *ctx)
    {
        if (owner != ctx) {
            Bufs::release();
            owner = ctx;
        }
    }
    // the context is going away (impdar_ctx_destroy)
    void forget(impdar_ctx *ctx)
    {
        const auto held = lock();
        if (owner == ctx) {
            Bufs::release();
            owner = nullptr;
        }
    }
    // a host-buffer entry point's upload of the caller's array into `buf` (one of Bufs), on the compute stream
    int stage_in(impdar_ctx *ctx, DevBuf &buf, const void *host, size_t bytes)
    {
        IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
        bind(ctx);
        IMPDAR_HIP_CHECK(buf.ensure(bytes));
        IMPDAR_HIP_CHECK(hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
        return IMPDAR_OK;
    }
    // The host-buffer form of a step, after its argument check: upload `bytes_in` of the caller's array into `in`,
    // run the resident form as run(d_in, d_out), download `bytes_out`.  With `out` the result is that second
    // staging buffer, ensured to hold bytes_out; without, the resident form works in place and d_out == d_in.
    template <class Run>
    int host_form(impdar_ctx *ctx, DevBuf &in, const void *host_in, size_t bytes_in, DevBuf *out, void *host_out,
                  size_t bytes_out, const Run &run)
    {
        const auto held = lock();
        int rc = stage_in(ctx, in, host_in, bytes_in);
        if (rc) return rc;
        if (out) IMPDAR_HIP_CHECK(out->ensure(bytes_out));
        DevBuf &res = out ? *out : in;
        rc = run(in.p, res.p);
        if (rc) return rc;
        return impdar_download(ctx, host_out, res.p, bytes_out, ctx->stream);
    }
};
