// Context, error channel and raw device-memory plumbing of the C ABI.
#include "common.h"
#include <algorithm>

static thread_local char g_err[1024] = "";

void impdar_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *impdar_last_error(void) { return g_err; }

#include <chrono>
bool impdar_trace_on()
{
    const char *e = getenv("IMPDAR_TRACE");          // read per call (a handful of trace points per migration)
    return e && atoi(e) != 0;
}
void impdar_trace(const char *fmt, ...)
{
    if (!impdar_trace_on()) return;
    static const auto t0 = std::chrono::steady_clock::now();
    static std::mutex mu;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    const double unix_s = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    std::lock_guard<std::mutex> lk(mu);
    fprintf(stderr, "[impdar +%9.2f ms, unix %.3f] %s\n", ms, unix_s, buf);
}

extern "C" int impdar_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

extern "C" int impdar_ctx_create(int device, impdar_ctx **out)
{
    IMPDAR_ARG_CHECK(out, "null output pointer");
    impdar_trace("ctx_create: enter");
    int n = impdar_device_count();
    if (n <= 0) {
        impdar_set_error("no HIP device visible (hipGetDeviceCount = %d)", n);
        return IMPDAR_ERR_NODEV;
    }
    IMPDAR_ARG_CHECK(device >= 0 && device < n, "device %d out of range [0,%d)", device, n);
    IMPDAR_HIP_CHECK(hipSetDevice(device));
    impdar_ctx *c = new impdar_ctx();
    c->device = device;
    // compute stream at the highest priority, producer stream at the lowest: the next
    // radargram's prep then fills the tail of the current diffraction sum instead of
    // competing with it for CUs
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    hipError_t e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->aux, hipStreamNonBlocking, prio_lo);
    if (e != hipSuccess) {
        delete c;
        impdar_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        return IMPDAR_ERR_HIP;
    }
    *out = c;
    impdar_trace("ctx_create: device %d set, two streams made", device);
    return IMPDAR_OK;
}

int impdar_ctx_mark_produced(impdar_ctx *ctx)
{
    if (!ctx->ev_produced) IMPDAR_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_produced, hipEventDisableTiming));
    IMPDAR_HIP_CHECK(hipEventRecord(ctx->ev_produced, ctx->stream));
    ctx->produced = true;
    return IMPDAR_OK;
}

int impdar_ctx_tic(impdar_ctx *ctx)
{
    if (!ctx->ev_tic) IMPDAR_HIP_CHECK(hipEventCreate(&ctx->ev_tic));
    if (!ctx->ev_toc) IMPDAR_HIP_CHECK(hipEventCreate(&ctx->ev_toc));
    ctx->timed = false;
    ctx->ktimed = false;
    IMPDAR_HIP_CHECK(hipEventRecord(ctx->ev_tic, ctx->stream));
    return IMPDAR_OK;
}

int impdar_ctx_ktic(impdar_ctx *ctx)
{
    if (!ctx->ev_ktic) IMPDAR_HIP_CHECK(hipEventCreate(&ctx->ev_ktic));
    if (!ctx->ev_ktoc) IMPDAR_HIP_CHECK(hipEventCreate(&ctx->ev_ktoc));
    ctx->ktimed = false;
    IMPDAR_HIP_CHECK(hipEventRecord(ctx->ev_ktic, ctx->stream));
    return IMPDAR_OK;
}

int impdar_ctx_ktoc(impdar_ctx *ctx)
{
    IMPDAR_HIP_CHECK(hipEventRecord(ctx->ev_ktoc, ctx->stream));
    ctx->ktimed = true;
    return IMPDAR_OK;
}

int impdar_ctx_toc(impdar_ctx *ctx)
{
    IMPDAR_HIP_CHECK(hipEventRecord(ctx->ev_toc, ctx->stream));
    ctx->timed = true;
    return IMPDAR_OK;
}

extern "C" int impdar_ctx_last_ms(impdar_ctx *ctx, float *ms)
{
    IMPDAR_ARG_CHECK(ctx && ms, "null context/pointer");
    IMPDAR_ARG_CHECK(ctx->timed, "no timed call (impdar_stolt_dev / impdar_phaseshift_dev) has run on this context");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    IMPDAR_HIP_CHECK(hipEventSynchronize(ctx->ev_toc));
    IMPDAR_HIP_CHECK(hipEventElapsedTime(ms, ctx->ev_tic, ctx->ev_toc));
    return IMPDAR_OK;
}

extern "C" int impdar_ctx_last_kernel_ms(impdar_ctx *ctx, float *ms)
{
    IMPDAR_ARG_CHECK(ctx && ms, "null context/pointer");
    IMPDAR_ARG_CHECK(ctx->ktimed, "the last timed call on this context bracketed no kernel (impdar_phaseshift[_dev] and impdar_apres_decode[_dev] do)");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    IMPDAR_HIP_CHECK(hipEventSynchronize(ctx->ev_ktoc));
    IMPDAR_HIP_CHECK(hipEventElapsedTime(ms, ctx->ev_ktic, ctx->ev_ktoc));
    return IMPDAR_OK;
}

// One JSON object about the last migration entry point that ran on this context ("emit a JSON
// line per run beside the print"; the reference only prints 'complete in N seconds', mig_python.py:121-122,206-207,
// 285-286).  The Python entry points add the sizes, traces per second and the device count and print the line on
// stderr when IMPDAR_METRICS is set.
extern "C" int impdar_ctx_last_metrics(impdar_ctx *ctx, char *json, size_t cap)
{
    IMPDAR_ARG_CHECK(ctx && json && cap > 0, "null context/buffer");
    IMPDAR_ARG_CHECK(ctx->m_entry, "no migration entry point has run on this context");
    float dev_ms = -1.f, k_ms = ctx->m_kernel_ms;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    if (ctx->timed && hipEventSynchronize(ctx->ev_toc) == hipSuccess) (void)hipEventElapsedTime(&dev_ms, ctx->ev_tic, ctx->ev_toc);
    if (k_ms < 0.f && ctx->ktimed && hipEventSynchronize(ctx->ev_ktoc) == hipSuccess)
        (void)hipEventElapsedTime(&k_ms, ctx->ev_ktic, ctx->ev_ktoc);
    (void)hipGetLastError();
    int n = snprintf(json, cap, "{\"entry\": \"%s\", \"kernel\": \"%s\", \"device\": %d", ctx->m_entry,
                     ctx->m_kernel ? ctx->m_kernel : "", ctx->device);
    if (n > 0 && (size_t)n < cap && k_ms >= 0.f) n += snprintf(json + n, cap - n, ", \"kernel_ms\": %.4f", k_ms);
    if (n > 0 && (size_t)n < cap && dev_ms >= 0.f) n += snprintf(json + n, cap - n, ", \"device_ms\": %.4f", dev_ms);
    if (n > 0 && (size_t)n < cap && ctx->m_extra[0]) n += snprintf(json + n, cap - n, ", %s", ctx->m_extra);
    if (n > 0 && (size_t)n < cap) n += snprintf(json + n, cap - n, "}");
    IMPDAR_ARG_CHECK(n > 0 && (size_t)n < cap, "buffer of %zu bytes is too small for the metrics object", cap);
    return IMPDAR_OK;
}

void impdar_comm_destroy(impdar_ctx *ctx);   // comm.hip

void impdar_stolt_forget(const impdar_ctx *ctx);   // stolt.hip
void impdar_ps_forget(const impdar_ctx *ctx);      // phaseshift.hip
void impdar_kirch_forget(const impdar_ctx *ctx);   // kirch_oneshot.hip
void impdar_preproc_forget(impdar_ctx *ctx);       // preproc.hip
void impdar_hfilt_forget(impdar_ctx *ctx);         // hfilt.hip
void impdar_denoise_forget(impdar_ctx *ctx);       // denoise.hip
void impdar_hpass_forget(impdar_ctx *ctx);         // hpass.hip
void impdar_vaxis_forget(impdar_ctx *ctx);         // vaxis.hip
void impdar_gain_forget(impdar_ctx *ctx);          // gain.hip
void impdar_taxis_forget(impdar_ctx *ctx);         // taxis.hip
void impdar_quadpol_forget(impdar_ctx *ctx);       // quadpol.hip
void impdar_apres_forget(impdar_ctx *ctx);         // apres.hip
void impdar_pick_forget(impdar_ctx *ctx);          // pick.hip
void impdar_spectrum_forget(impdar_ctx *ctx);      // spectrum.hip
void impdar_display_forget(impdar_ctx *ctx);       // display.hip
void impdar_rawload_forget(impdar_ctx *ctx);       // rawload.hip
void impdar_gpstrack_forget(impdar_ctx *ctx);      // gpstrack.hip
void impdar_attsearch_forget(impdar_ctx *ctx);     // attsearch.hip
void impdar_decon_forget(impdar_ctx *ctx);         // decon.hip
void impdar_attr_forget(impdar_ctx *ctx);          // attr.hip
void impdar_slope_forget(impdar_ctx *ctx);         // slope.hip

void impdar_kirch_trim();    // kirch_oneshot.hip
void impdar_stolt_trim();    // stolt.hip
void impdar_ps_trim();       // phaseshift.hip

void impdar_devcache_trim(int device);

void impdar_release_caches()
{
    impdar_kirch_trim();
    impdar_stolt_trim();
    impdar_ps_trim();
    impdar_devcache_trim(-1);
}

extern "C" void impdar_ctx_destroy(impdar_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->aux);
    (void)hipStreamSynchronize(ctx->stream);
    impdar_stolt_forget(ctx);
    impdar_ps_forget(ctx);
    impdar_kirch_forget(ctx);
    impdar_preproc_forget(ctx);
    impdar_hfilt_forget(ctx);
    impdar_denoise_forget(ctx);
    impdar_hpass_forget(ctx);
    impdar_vaxis_forget(ctx);
    impdar_gain_forget(ctx);
    impdar_taxis_forget(ctx);
    impdar_quadpol_forget(ctx);
    impdar_apres_forget(ctx);
    impdar_pick_forget(ctx);
    impdar_spectrum_forget(ctx);
    impdar_display_forget(ctx);
    impdar_rawload_forget(ctx);
    impdar_gpstrack_forget(ctx);
    impdar_attsearch_forget(ctx);
    impdar_decon_forget(ctx);
    impdar_attr_forget(ctx);
    impdar_slope_forget(ctx);
    impdar_devcache_trim(ctx->device);
    impdar_ctx_pinned_release(ctx);
    if (ctx->ev_produced) (void)hipEventDestroy(ctx->ev_produced);
    if (ctx->ev_tic) (void)hipEventDestroy(ctx->ev_tic);
    if (ctx->ev_toc) (void)hipEventDestroy(ctx->ev_toc);
    if (ctx->ev_ktic) (void)hipEventDestroy(ctx->ev_ktic);
    if (ctx->ev_ktoc) (void)hipEventDestroy(ctx->ev_ktoc);
    impdar_comm_destroy(ctx);
    (void)hipStreamDestroy(ctx->aux);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int impdar_ctx_sync(impdar_ctx *ctx)
{
    IMPDAR_ARG_CHECK(ctx, "null context");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->aux));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return IMPDAR_OK;
}

// Device arrays of the one-shot calls -- the radargram a call uploads, the image it downloads -- come from a small cache
// (round 6): hipMalloc + hipFree of a 64 ... 268 MB array were ~1.5 ms of every call through host arrays (a third of a Stolt
// call at 4096^2).  A freed array is kept (at most four, 2 GiB in total, per process) and handed to the next request of
// [its size / 1.25, its size]; impdar_release_caches and impdar_ctx_destroy empty it.  Everything a cached array was used
// for has been waited for before it went back (impdar_devcache_free synchronises the context's streams first).
struct DevCacheEntry {
    void *p;
    size_t bytes;
    int device;
    bool free_;
};
static std::mutex g_devcache_mu;
static std::vector<DevCacheEntry> g_devcache;                  // arrays handed out (free_ = false) and kept (free_ = true)
constexpr size_t DEVCACHE_MAX_BYTES = (size_t)2 << 30;
constexpr int DEVCACHE_MAX_KEPT = 4;

int impdar_devcache_alloc(int device, size_t bytes, void **dptr)
{
    if (bytes == 0) bytes = 8;
    {
        std::lock_guard<std::mutex> lk(g_devcache_mu);
        DevCacheEntry *best = nullptr;
        for (DevCacheEntry &e : g_devcache)
            if (e.free_ && e.device == device && e.bytes >= bytes && e.bytes <= bytes + bytes / 4 + ((size_t)1 << 20) && (!best || e.bytes < best->bytes)) best = &e;
        if (best) {
            best->free_ = false;
            *dptr = best->p;
            return IMPDAR_OK;
        }
    }
    DevBuf b;                                                   // (its ensure() retries after impdar_release_caches when memory is short)
    IMPDAR_HIP_CHECK(b.ensure(bytes));
    *dptr = b.p;
    b.p = nullptr;
    b.bytes = 0;
    std::lock_guard<std::mutex> lk(g_devcache_mu);
    g_devcache.push_back(DevCacheEntry{*dptr, bytes, device, false});
    return IMPDAR_OK;
}

// the caller has synchronised whatever used the array
void impdar_devcache_free(void *p)
{
    if (!p) return;
    void *drop[DEVCACHE_MAX_KEPT + 2] = {};
    int ndrop = 0;
    {
        std::lock_guard<std::mutex> lk(g_devcache_mu);
        size_t kept_bytes = 0;
        int kept = 0;
        bool found = false;
        for (DevCacheEntry &e : g_devcache) {
            if (e.p == p) {
                e.free_ = true;
                found = true;
            }
            if (e.free_) {
                kept_bytes += e.bytes;
                ++kept;
            }
        }
        if (!found) drop[ndrop++] = p;                           // (not one of ours: plain hipFree)
        // over the limits: the oldest kept arrays go
        for (size_t i = 0; i < g_devcache.size() && (kept > DEVCACHE_MAX_KEPT || kept_bytes > DEVCACHE_MAX_BYTES) && ndrop < DEVCACHE_MAX_KEPT + 2;) {
            if (g_devcache[i].free_) {
                drop[ndrop++] = g_devcache[i].p;
                kept_bytes -= g_devcache[i].bytes;
                --kept;
                g_devcache.erase(g_devcache.begin() + (long)i);
            } else {
                ++i;
            }
        }
    }
    for (int i = 0; i < ndrop; ++i) (void)hipFree(drop[i]);
}

// device < 0: every device
void impdar_devcache_trim(int device)
{
    std::vector<void *> drop;
    {
        std::lock_guard<std::mutex> lk(g_devcache_mu);
        for (size_t i = 0; i < g_devcache.size();) {
            if (g_devcache[i].free_ && (device < 0 || g_devcache[i].device == device)) {
                drop.push_back(g_devcache[i].p);
                g_devcache.erase(g_devcache.begin() + (long)i);
            } else {
                ++i;
            }
        }
    }
    for (void *p : drop) (void)hipFree(p);
}

extern "C" int impdar_dev_alloc(impdar_ctx *ctx, size_t bytes, void **dptr)
{
    IMPDAR_ARG_CHECK(ctx && dptr, "null context/pointer");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    return impdar_devcache_alloc(ctx->device, bytes, dptr);
}

extern "C" int impdar_dev_free(impdar_ctx *ctx, void *dptr)
{
    IMPDAR_ARG_CHECK(ctx, "null context");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->aux));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    impdar_devcache_free(dptr);
    return IMPDAR_OK;
}

extern "C" int impdar_dev_upload(impdar_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes)
{
    IMPDAR_ARG_CHECK(ctx && dst_dev && src_host, "null context/pointer");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    // an image that goes up usually comes down again, through the context's pinned staging buffer: have it pinned by a
    // thread of its own while the upload and the migration run (44 ms for the 256 MB of an 8192^2 float32 image when the
    // download has to do it itself: profiles/r05_first_call.txt)
    impdar_ctx_pinned_prefetch(ctx, std::min(bytes, IMPDAR_STAGE_RING_BYTES));
    // straight from pageable memory: the runtime's own staging pipeline reaches 17 GB/s here; copying into the
    // context's pinned buffer on host threads first was slower (9.8 -> 17 ms for 164 MB)
    IMPDAR_HIP_CHECK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return IMPDAR_OK;
}

extern "C" int impdar_dev_download(impdar_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes)
{
    IMPDAR_ARG_CHECK(ctx && dst_host && src_dev, "null context/pointer");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    // through the pinned staging buffer and a threaded copy: the destination is usually a fresh pageable array
    return impdar_download(ctx, dst_host, src_dev, bytes, ctx->stream);
}

extern "C" int impdar_dev_download_f64(impdar_ctx *ctx, double *dst_host, const void *src_dev, int dtype, size_t n)
{
    IMPDAR_ARG_CHECK(ctx && dst_host && src_dev, "impdar_dev_download_f64: null argument");
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "impdar_dev_download_f64: dtype must be float32 or float64");
    if (n == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    // one block of one row, as wide as the host array: a flat array
    const size_t col0 = 0;
    const hipEvent_t after = nullptr;
    return impdar_download_blocks_f64(ctx, dst_host, n, 1, dtype, 1, &col0, &n, &src_dev, &after, ctx->stream);
}

extern "C" int impdar_dev_memset(impdar_ctx *ctx, void *dst_dev, int value, size_t bytes)
{
    IMPDAR_ARG_CHECK(ctx && dst_dev, "null context/pointer");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    IMPDAR_HIP_CHECK(hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
    return impdar_ctx_mark_produced(ctx);
}
