// Device -> host transfers of the host-buffer entry points: the context's pinned staging buffer, the host worker
// threads, and the one staged download that every such entry point ends in.
#include "common.h"
#include "download_plan.h"
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <memory>
#include <new>
#include <unistd.h>

static void pinned_adopt(impdar_ctx *ctx)
{
    if (ctx->pin_thread.joinable()) ctx->pin_thread.join();
    if (ctx->pin_next) {
        if (ctx->pin_next_bytes > ctx->pinned_bytes) {
            if (ctx->pinned) (void)hipHostFree(ctx->pinned);
            ctx->pinned = ctx->pin_next;
            ctx->pinned_bytes = ctx->pin_next_bytes;
        } else {
            (void)hipHostFree(ctx->pin_next);
        }
        ctx->pin_next = nullptr;
        ctx->pin_next_bytes = 0;
    }
}

void impdar_ctx_pinned_prefetch(impdar_ctx *ctx, size_t bytes)
{
    std::lock_guard<std::mutex> lock(ctx->pinned_mu);
    if (bytes < ((size_t)1 << 20) || bytes <= ctx->pinned_bytes || bytes > ((size_t)1 << 30)) return;
    if (ctx->pin_thread.joinable()) {
        if (ctx->pin_next_bytes >= bytes) return;          // one on its way that will do
        pinned_adopt(ctx);
        if (bytes <= ctx->pinned_bytes) return;
    }
    ctx->pin_next_bytes = bytes;
    const int device = ctx->device;
    ctx->pin_thread = std::thread([ctx, device, bytes] {
        void *p = nullptr;
        impdar_trace("pinned prefetch thread: hipHostMalloc of %zu MB: start", bytes >> 20);
        if (hipSetDevice(device) != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
        }
        impdar_trace("pinned prefetch thread: done");
        ctx->pin_next = p;          // (read after the join)
    });
}

// (callers hold ctx->pinned_mu)
void *impdar_ctx_pinned(impdar_ctx *ctx, size_t bytes)
{
    if (bytes <= ctx->pinned_bytes) return ctx->pinned;      // (a larger one on its way is not waited for)
    pinned_adopt(ctx);
    if (bytes <= ctx->pinned_bytes) return ctx->pinned;
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = nullptr;
    ctx->pinned_bytes = 0;
    void *p = nullptr;
    impdar_trace("impdar_ctx_pinned: synchronous hipHostMalloc of %zu MB", bytes >> 20);
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    impdar_trace("impdar_ctx_pinned: done");
    ctx->pinned = p;
    ctx->pinned_bytes = bytes;
    return p;
}

void impdar_ctx_pinned_release(impdar_ctx *ctx)
{
    pinned_adopt(ctx);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = nullptr;
    ctx->pinned_bytes = 0;
}

// Host worker threads that live as long as the process: a parallel copy used to start and join 16 threads of its own
// -- 0.3-0.5 ms each time, which is why download pieces below 48 MB did not pay.  The pool is created on first use and never
// destroyed (its threads sleep on a condition variable; a static destructor that joined them would run at exit, in the order
// the runtime tears its own threads down).  One job at a time: callers hold ctx->pinned_mu or are the only caller.
struct ImpdarPool {
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::function<void(unsigned)> job;
    unsigned nthr = 0, generation = 0, pending = 0;
    std::mutex user_mu;                                     // one parallel_for at a time
    explicit ImpdarPool(unsigned n) : nthr(n)
    {
        for (unsigned t = 0; t < n; ++t)
            std::thread([this, t] {
                unsigned seen = 0;
                for (;;) {
                    std::function<void(unsigned)> f;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv_work.wait(lk, [&] { return generation != seen; });
                        seen = generation;
                        f = job;
                    }
                    f(t);
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        if (--pending == 0) cv_done.notify_all();
                    }
                }
            }).detach();
    }
    void run(const std::function<void(unsigned)> &f)
    {
        std::lock_guard<std::mutex> user(user_mu);
        {
            std::lock_guard<std::mutex> lk(mu);
            job = f;
            pending = nthr;
            ++generation;
        }
        cv_work.notify_all();
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
    }
};
static ImpdarPool *impdar_pool()
{
    // (leaked on purpose; a forked child has the pointer but none of the threads: it makes its own)
    static std::mutex mu;
    static ImpdarPool *pool = nullptr;
    static pid_t owner = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (!pool || owner != getpid()) {
        pool = new ImpdarPool(std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
        owner = getpid();
    }
    return pool;
}

// `n` items on the host worker threads: fn(begin, end)
template <typename F> static void impdar_parallel_for(size_t n, size_t align, F fn)
{
    ImpdarPool *pool = impdar_pool();
    const unsigned nthr = pool->nthr;
    if (n * 1 <= (size_t)nthr * align) {                   // (nothing to share out)
        fn(0, n);
        return;
    }
    pool->run([&](unsigned t) {
        const size_t a = (n * t / nthr) / align * align, b = t + 1 == nthr ? n : (n * (t + 1) / nthr) / align * align;
        if (b > a) fn(a, b);
    });
}

// One (rows x width) device array, contiguous, that lands in columns [col0, col0 + width) of a host array with `ld`
// elements per row, once `after` (null: nothing to wait for) has passed.  width == ld is a flat array.
struct DownloadBlock {
    const void *src;
    size_t rows, width, ld, col0;
    hipEvent_t after;
};

// elements [first, first + count) of block `b`, staged at `sp`, into the caller's array on the host threads
static void download_copy_out(const DownloadBlock &b, const char *sp, size_t first, size_t count, char *host_dst, size_t elem_in,
                              bool widen)
{
    const auto widen_run = [](char *dst, const char *src, size_t a, size_t e) {
        const float *f = reinterpret_cast<const float *>(src);
        double *d = reinterpret_cast<double *>(dst);
        for (size_t i = a; i < e; ++i) d[i] = (double)f[i];
    };
    const size_t elem_out = widen ? 8 : elem_in;
    if (b.width != b.ld) {
        // rows first / width .. of the block -> host rows of `ld` elements, columns col0 ..
        const size_t w = b.width, ld = b.ld, c0 = b.col0, r0 = first / w;
        impdar_parallel_for(count / w, 1, [=](size_t ra, size_t rb) {
            for (size_t r = ra; r < rb; ++r) {
                const char *src = sp + r * w * elem_in;
                char *dst = host_dst + ((r0 + r) * ld + c0) * elem_out;
                if (widen) widen_run(dst, src, 0, w);
                else memcpy(dst, src, w * elem_in);
            }
        });
    } else if (widen) {
        char *dst = host_dst + first * elem_out;
        impdar_parallel_for(count, 16, [=](size_t a, size_t e) { widen_run(dst, sp, a, e); });
    } else {
        char *dst = host_dst + first * elem_in;
        impdar_parallel_for(count * elem_in, 64, [=](size_t a, size_t e) { memcpy(dst + a, sp + a, e - a); });
    }
}

// Device -> pageable host memory in pieces (download_plan.h): every piece is DMA-ed into the staging ring as soon as the
// ring has room for it, and copied out (or widened float32 -> float64) on the host threads while the DMA of the pieces
// behind it is still running.  Synchronises `st`.
static int download_run(impdar_ctx *ctx, void *host_dst, const DownloadBlock *blk, int nblk, size_t elem_in, bool widen,
                        hipStream_t st)
{
    std::vector<DlBlock> shape(nblk);
    size_t total = 0;
    for (int i = 0; i < nblk; ++i) {
        shape[i] = DlBlock{blk[i].rows * blk[i].width, blk[i].width != blk[i].ld ? blk[i].width : 16};
        total += shape[i].count * elem_in;
    }
    const bool plain = nblk == 1 && blk[0].width == blk[0].ld && !widen;      // a contiguous copy
    if (total == 0 && !plain) return IMPDAR_OK;
    // one staged download per context at a time: the staging buffer is shared (and may be re-allocated) and
    // ctypes callers run without the GIL
    std::lock_guard<std::mutex> lock(ctx->pinned_mu);
    const size_t cap = std::min(total, IMPDAR_STAGE_RING_BYTES);
    char *stage = total >= ((size_t)1 << 20) ? reinterpret_cast<char *>(impdar_ctx_pinned(ctx, cap)) : nullptr;
    std::unique_ptr<char[]> heap;
    if (!stage) {
        if (plain) {
            if (blk[0].after) IMPDAR_HIP_CHECK(hipStreamWaitEvent(st, blk[0].after, 0));
            IMPDAR_HIP_CHECK(hipMemcpyAsync(host_dst, blk[0].src, total, hipMemcpyDeviceToHost, st));
            IMPDAR_HIP_CHECK(hipStreamSynchronize(st));
            return IMPDAR_OK;
        }
        heap.reset(new (std::nothrow) char[cap]);           // no pinned memory: the same ring in pageable memory
        stage = heap.get();
        if (!stage) {
            impdar_set_error("device -> host copy: no host memory for a staging ring of %zu bytes", cap);
            return IMPDAR_ERR_HIP;
        }
    }
    std::vector<DlPiece> pieces;
    if (download_plan(cap, elem_in, shape.data(), nblk, pieces) != DL_OK) {
        impdar_set_error("device -> host copy: a row does not fit the staging ring of %zu bytes", cap);
        return IMPDAR_ERR_ARG;
    }
    std::vector<size_t> off(pieces.size(), 0);              // where each piece lies in the ring
    std::vector<hipEvent_t> ev(pieces.size(), nullptr);     // ... and the event behind its copy
    DlRing ring(cap);
    size_t oldest = 0;                                      // the next piece to copy out
    const auto retire_oldest = [&]() {
        const DlPiece &q = pieces[oldest];
        if (hipEventSynchronize(ev[oldest]) != hipSuccess) return false;
        download_copy_out(blk[q.block], stage + off[oldest], q.first, q.count, reinterpret_cast<char *>(host_dst), elem_in, widen);
        ring.retire(q.bytes);
        ++oldest;
        return true;
    };
    bool ok = true;
    for (size_t k = 0; k < pieces.size() && ok; ++k) {
        const DlPiece &q = pieces[k];
        const DownloadBlock &b = blk[q.block];
        while (ok && !ring.place(q.bytes, &off[k])) ok = retire_oldest();      // (q.bytes <= cap: placed at the latest once none is live)
        ok = ok && hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) == hipSuccess &&
             (!b.after || q.first != 0 || hipStreamWaitEvent(st, b.after, 0) == hipSuccess) &&
             hipMemcpyAsync(stage + off[k], reinterpret_cast<const char *>(b.src) + q.first * elem_in, q.bytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipEventRecord(ev[k], st) == hipSuccess;
    }
    while (ok && oldest < pieces.size()) ok = retire_oldest();
    if (!ok) {
        // no DMA into the staging buffer may still be in flight when it is handed to the next caller
        (void)hipStreamSynchronize(st);
        impdar_set_error("device -> host copy failed: %s", hipGetErrorString(hipGetLastError()));
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return ok ? IMPDAR_OK : IMPDAR_ERR_HIP;
}

int impdar_download(impdar_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes, hipStream_t st)
{
    const DownloadBlock b{dev_src, 1, bytes, bytes, 0, nullptr};
    return download_run(ctx, host_dst, &b, 1, 1, false, st);
}

// Several (rows x width[i]) device blocks of `dtype` into columns [col0[i], col0[i] + width[i]) of ONE (rows x ld) float64
// host array, each as soon as `after[i]` (the event behind the kernel that produces it) has passed: the copies are
// enqueued on `st` as the ring takes them, and the host threads widen piece k while the DMA of piece k + 1 (of this block
// or the next) runs -- the pipelined one-shot Kirchhoff call's way out.  One block as wide as the host array is a flat
// array of rows * ld elements (impdar_dev_download_f64).
int impdar_download_blocks_f64(impdar_ctx *ctx, double *dst_host, size_t ld, size_t rows, int dtype, int nblk,
                               const size_t *col0, const size_t *width, const void *const *src, const hipEvent_t *after,
                               hipStream_t st)
{
    std::vector<DownloadBlock> blk(nblk);
    for (int i = 0; i < nblk; ++i) blk[i] = DownloadBlock{src[i], rows, width[i], ld, col0[i], after[i]};
    return download_run(ctx, dst_host, blk.data(), nblk, impdar_dtype_size(dtype), dtype == IMPDAR_F32, st);
}
