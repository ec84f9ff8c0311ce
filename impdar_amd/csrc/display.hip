// What a plot of the (snum, tnum) radargram reads from it, computed where it lies (the reference's plot_radargram and plot_traces,
// src/impdar/lib/plot.py:102-283, 368-445):
//   order statistics of a window -- np.percentile's two neighbours of every percentage, exact: a radix select on
//     order-preserving integer keys (display_route.h), DISP_DIGIT_BITS bits per pass, most significant first.  One pass streams the
//     window once: every element that is no NaN is counted in the histogram of each prefix it carries (ranks with equal prefixes
//     share one; the first pass has the empty prefix alone and counts the NaNs besides).  A workgroup counts in LDS and adds its
//     non-empty bins to the 64-bit histograms in memory, one integer atomic each.  The host moves every rank into its bin and
//     forms the next prefixes (disp_select_step).  float32: 4 passes, float64: 8.  Integer atomics only: two calls, same bits.
//   the flattened image -- out[i, j] = data[i - k[j], x0 + j] where that row exists, NaN elsewhere: a gather, one store pass.
//   a window into a dense host array -- a strided copy, no kernel.
#include <limits>
#include "common.h"
#include "display_route.h"
#include "vecwidth.h"

static_assert(DISP_THREADS == DISP_BINS, "a workgroup merges its histograms one thread per bin");

struct DispPass {
    unsigned long long prefix[DISP_MAX_RANKS];
    int ngroups, shift, first;
};

template <typename T> struct DispKey;
template <> struct DispKey<float> {
    typedef unsigned int type;
    static __device__ __forceinline__ type of(float v)
    {
        const unsigned int b = __float_as_uint(v);
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
};
template <> struct DispKey<double> {
    typedef unsigned long long type;
    static __device__ __forceinline__ type of(double v)
    {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }
};

// thread (tx, ty) of a workgroup: access tx of a row of `units`, rows ty, ty + stride ... (display_route.h's DispGrid)
struct DispThread {
    long long unit, row0, stride;
};
static __device__ __forceinline__ DispThread disp_thread(int log_tx)
{
    const int tx = threadIdx.x & ((1 << log_tx) - 1), ty = threadIdx.x >> log_tx, th = DISP_THREADS >> log_tx;
    return DispThread{(long long)blockIdx.x * (1 << log_tx) + tx, (long long)blockIdx.y * th + ty, (long long)gridDim.y * th};
}

// win: the window's first element; row r of it at win + r pitch, `units` accesses of V elements wide.  hist: DISP_HIST_WORDS
// counters, zero on entry.  The caller has checked the alignment of every access (rw_dispatch).
template <typename T, int V>
__global__ __launch_bounds__(DISP_THREADS) void disp_hist_kernel(const T *__restrict__ win, size_t pitch, long long rows, long long units, int log_tx,
                                                                 const DispPass P, unsigned long long *__restrict__ hist)
{
    typedef typename DispKey<T>::type K;
    __shared__ unsigned int lh[DISP_MAX_RANKS * DISP_BINS];
    __shared__ unsigned int lnan;
    const int tid = threadIdx.x;
    for (int g = 0; g < P.ngroups; ++g) lh[g * DISP_BINS + tid] = 0;
    if (tid == 0) lnan = 0;
    __syncthreads();
    const DispThread t = disp_thread(log_tx);
    unsigned int nan = 0;
    if (t.unit < units) {
        for (long long r = t.row0; r < rows; r += t.stride) {
            const RwVec<T, V> x = rw_load<T, V>(win + (size_t)r * pitch + (size_t)t.unit * V);
            if (P.first) {
                // equal digits of one access go out as one add
                int slot[V];
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    const T v = x.v[c];
                    slot[c] = v != v ? -1 : (int)((DispKey<T>::of(v) >> P.shift) & (DISP_BINS - 1));
                    nan += v != v;
                }
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    if (slot[c] < 0) continue;
                    unsigned int cnt = 1;
#pragma unroll
                    for (int d = c + 1; d < V; ++d)
                        if (slot[d] == slot[c]) {
                            ++cnt;
                            slot[d] = -1;
                        }
                    atomicAdd(&lh[slot[c]], cnt);
                }
            } else {
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    const T v = x.v[c];
                    if (v != v) continue;
                    const K key = DispKey<T>::of(v);
                    const unsigned long long head = (unsigned long long)(key >> P.shift) >> DISP_DIGIT_BITS;
                    const int digit = (int)((key >> P.shift) & (DISP_BINS - 1));
                    for (int g = 0; g < P.ngroups; ++g)
                        if (head == P.prefix[g]) atomicAdd(&lh[g * DISP_BINS + digit], 1u);
                }
            }
        }
    }
    if (nan) atomicAdd(&lnan, nan);
    __syncthreads();
    for (int g = 0; g < P.ngroups; ++g) {
        const unsigned int c = lh[g * DISP_BINS + tid];
        if (c) atomicAdd(&hist[g * DISP_BINS + tid], (unsigned long long)c);
    }
    if (tid == 0 && lnan) atomicAdd(&hist[DISP_HIST_WORDS - 1], (unsigned long long)lnan);
}

template <typename T, int V> static __device__ __forceinline__ void disp_store(T *p, const RwVec<T, V> &x)
{
    typedef T Native __attribute__((ext_vector_type(V)));
    Native n;
#pragma unroll
    for (int c = 0; c < V; ++c) n[c] = x.v[c];
    *reinterpret_cast<Native *>(p) = n;
}

// out: (snum, width) with width = units V; out[i, j] = data[i - shift[j], x0 + j] where 0 <= i - shift[j] < snum, NaN elsewhere and
// in every column whose shift is IMPDAR_FLATTEN_NONE
template <typename T, int V>
__global__ __launch_bounds__(DISP_THREADS) void disp_flatten_kernel(const T *__restrict__ data, size_t tnum, int snum, int x0, long long units, int log_tx,
                                                                    const int *__restrict__ shift, T *__restrict__ out)
{
    const DispThread t = disp_thread(log_tx);
    if (t.unit >= units) return;
    const size_t j0 = (size_t)t.unit * V, width = (size_t)units * V;
    int k[V];
#pragma unroll
    for (int c = 0; c < V; ++c) k[c] = shift[j0 + c];
    for (long long r = t.row0; r < snum; r += t.stride) {
        RwVec<T, V> o;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const long long src = r - (long long)k[c];
            const bool in = k[c] != IMPDAR_FLATTEN_NONE && src >= 0 && src < snum;
            o.v[c] = in ? data[(size_t)src * tnum + (size_t)x0 + j0 + c] : std::numeric_limits<T>::quiet_NaN();
        }
        disp_store<T, V>(out + (size_t)r * width + j0, o);
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct DispBufs {
    DevBuf data, hist, tab, out;        // staging of a host radargram, the counters of a pass, the shifts, the flattened image
    void release()
    {
        for (DevBuf *b : {&data, &hist, &tab, &out}) b->release();
    }
};
static StepScratch<DispBufs> g_dp;

void impdar_display_forget(impdar_ctx *ctx) { g_dp.forget(ctx); }

static int window_check(const char *who, impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int y0, int y1, int x0, int x1)
{
    IMPDAR_ARG_CHECK(ctx && data, "%s: null argument", who);
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "%s: dtype must be float32 or float64", who);
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "%s: empty radargram", who);
    IMPDAR_ARG_CHECK(0 <= y0 && y0 <= y1 && y1 <= snum, "%s: rows [%d, %d) of %d", who, y0, y1, snum);
    IMPDAR_ARG_CHECK(0 <= x0 && x0 <= x1 && x1 <= tnum, "%s: traces [%d, %d) of %d", who, x0, x1, tnum);
    return IMPDAR_OK;
}

static int order_stats_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int y0, int y1, int x0, int x1, const double *q, int nq,
                             const long long *counts, const void *vals)
{
    int rc = window_check("impdar_order_stats", ctx, data, dtype, snum, tnum, y0, y1, x0, x1);
    if (rc) return rc;
    IMPDAR_ARG_CHECK(q && counts && vals, "impdar_order_stats: null argument");
    IMPDAR_ARG_CHECK(nq >= 1 && nq <= DISP_MAX_Q, "impdar_order_stats: %d percentages (1 to %d)", nq, (int)DISP_MAX_Q);
    for (int i = 0; i < nq; ++i) IMPDAR_ARG_CHECK(q[i] >= 0.0 && q[i] <= 100.0, "impdar_order_stats: percentage %g is outside [0, 100]", q[i]);
    return IMPDAR_OK;
}

// The order statistics of rows [y0, y1), traces [x0, x1) of a resident radargram.  The caller holds g_dp's lock and has bound it.
static int order_stats_run(impdar_ctx *ctx, const void *d_data, int dtype, int tnum, int y0, int y1, int x0, int x1, const double *q, int nq,
                           int skip_nan, long long *counts, void *vals)
{
    const long long rows = y1 - y0, width = x1 - x0, N = rows * width;
    const bool f32 = dtype == IMPDAR_F32;
    for (int i = 0; i < 2 * nq; ++i) {
        if (f32) ((float *)vals)[i] = std::numeric_limits<float>::quiet_NaN();
        else ((double *)vals)[i] = std::numeric_limits<double>::quiet_NaN();
    }
    counts[0] = N;
    counts[1] = 0;
    if (N == 0) return IMPDAR_OK;
    const int bits = f32 ? 32 : 64;
    IMPDAR_HIP_CHECK(g_dp.hist.ensure(DISP_HIST_WORDS * sizeof(unsigned long long)));
    std::vector<uint64_t> hist(DISP_HIST_WORDS);
    DispSelect S;
    DispPass P;
    memset(&P, 0, sizeof(P));
    for (int p = 0; p < disp_passes(bits); ++p) {
        P.first = p == 0;
        P.shift = bits - DISP_DIGIT_BITS * (p + 1);
        P.ngroups = p == 0 ? 1 : S.ngroups;
        for (int g = 0; g < P.ngroups; ++g) P.prefix[g] = p == 0 ? 0 : S.prefix[g];
        IMPDAR_HIP_CHECK(hipMemsetAsync(g_dp.hist.p, 0, DISP_HIST_WORDS * sizeof(unsigned long long), ctx->stream));
        int rc = IMPDAR_OK;
        // every access of V elements is aligned when the array, the row pitch, the first trace and the width all are
        rw_dispatch(dtype, {d_data}, tnum | x0 | (int)width, [&](auto t, auto vw) {
            typedef typename decltype(t)::type T;
            constexpr int V = decltype(vw)::value;
            const DispGrid G = disp_grid(rows, width, V);
            if (!G.ok) {
                impdar_set_error("impdar_order_stats: a window of %lld x %lld is beyond the grid", rows, width);
                rc = IMPDAR_ERR_ARG;
                return;
            }
            const T *win = (const T *)d_data + (size_t)y0 * tnum + x0;
            hipLaunchKernelGGL((disp_hist_kernel<T, V>), dim3(G.grid_x, G.grid_y), dim3(DISP_THREADS), 0, ctx->stream, win, (size_t)tnum, rows, G.units,
                               G.log_tx, P, g_dp.hist.as<unsigned long long>());
        });
        if (rc) return rc;
        IMPDAR_HIP_CHECK(hipGetLastError());
        IMPDAR_HIP_CHECK(hipMemcpyAsync(hist.data(), g_dp.hist.p, DISP_HIST_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (p == 0) {
            // the counting is done: the ranks of np.percentile's linear method among the n values that are no NaN
            const long long nan = (long long)hist[DISP_HIST_WORDS - 1], n = N - nan;
            counts[1] = nan;
            if (n == 0 || (nan > 0 && !skip_nan)) return IMPDAR_OK;
            long long ranks[DISP_MAX_RANKS];
            for (int i = 0; i < nq; ++i) disp_ranks(n, q[i], &ranks[2 * i], &ranks[2 * i + 1]);
            disp_select_start(S, ranks, 2 * nq);
        }
        IMPDAR_ARG_CHECK(disp_select_step(S, hist.data()), "impdar_order_stats: pass %d counted fewer elements than the ranks ask for", p);
    }
    for (int i = 0; i < 2 * nq; ++i) {
        const uint64_t key = S.prefix[S.group[i]];
        if (f32) ((float *)vals)[i] = disp_unkey32((uint32_t)key);
        else ((double *)vals)[i] = disp_unkey64(key);
    }
    return IMPDAR_OK;
}

extern "C" int impdar_order_stats_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int y0, int y1, int x0, int x1,
                                      const double *q, int nq, int skip_nan, long long *counts, void *vals)
{
    int rc = order_stats_check(ctx, d_data, dtype, snum, tnum, y0, y1, x0, x1, q, nq, counts, vals);
    if (rc) return rc;
    const auto lock = g_dp.lock();
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_dp.bind(ctx);
    impdar_ctx_note(ctx, "impdar_order_stats_dev", "disp_hist_kernel");
    return order_stats_run(ctx, d_data, dtype, tnum, y0, y1, x0, x1, q, nq, skip_nan, counts, vals);
}

extern "C" int impdar_order_stats(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int y0, int y1, int x0, int x1, const double *q,
                                  int nq, int skip_nan, long long *counts, void *vals)
{
    int rc = order_stats_check(ctx, data, dtype, snum, tnum, y0, y1, x0, x1, q, nq, counts, vals);
    if (rc) return rc;
    const auto lock = g_dp.lock();
    // only the window's rows travel (none of an empty window, which order_stats_run reports without reading)
    const size_t row_bytes = (size_t)tnum * impdar_dtype_size(dtype);
    if (y1 > y0 && x1 > x0) rc = g_dp.stage_in(ctx, g_dp.data, (const char *)data + (size_t)y0 * row_bytes, (size_t)(y1 - y0) * row_bytes);
    if (rc) return rc;
    impdar_ctx_note(ctx, "impdar_order_stats", "disp_hist_kernel");
    return order_stats_run(ctx, g_dp.data.p, dtype, tnum, 0, y1 - y0, x0, x1, q, nq, skip_nan, counts, vals);
}

static int flatten_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int x0, int x1, const int *shift, const void *out)
{
    int rc = window_check("impdar_flatten", ctx, data, dtype, snum, tnum, 0, snum, x0, x1);
    if (rc) return rc;
    IMPDAR_ARG_CHECK(shift && out, "impdar_flatten: null argument");
    IMPDAR_ARG_CHECK(x1 > x0, "impdar_flatten: no traces in [%d, %d)", x0, x1);
    return IMPDAR_OK;
}

extern "C" int impdar_flatten_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int x0, int x1, const int *shift, void *d_out)
{
    int rc = flatten_check(ctx, d_data, dtype, snum, tnum, x0, x1, shift, d_out);
    if (rc) return rc;
    const auto lock = g_dp.lock();
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_dp.bind(ctx);
    const int width = x1 - x0;
    const void *d_tab[1];
    rc = impdar_upload_tables(ctx, g_dp.tab, {{shift, (size_t)width * sizeof(int)}}, d_tab);
    if (rc) return rc;
    // the stores are the vector accesses: the image's own pitch decides their width
    rw_dispatch(dtype, {d_out}, width, [&](auto t, auto vw) {
        typedef typename decltype(t)::type T;
        constexpr int V = decltype(vw)::value;
        const DispGrid G = disp_grid(snum, width, V);
        if (!G.ok) {
            impdar_set_error("impdar_flatten: %d x %d is beyond the grid", snum, width);
            rc = IMPDAR_ERR_ARG;
            return;
        }
        hipLaunchKernelGGL((disp_flatten_kernel<T, V>), dim3(G.grid_x, G.grid_y), dim3(DISP_THREADS), 0, ctx->stream, (const T *)d_data, (size_t)tnum, snum,
                           x0, G.units, G.log_tx, (const int *)d_tab[0], (T *)d_out);
    });
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipGetLastError());
    impdar_ctx_note(ctx, "impdar_flatten_dev", "disp_flatten_kernel");
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_flatten(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int x0, int x1, const int *shift, void *out)
{
    int rc = flatten_check(ctx, data, dtype, snum, tnum, x0, x1, shift, out);
    if (rc) return rc;
    const size_t es = impdar_dtype_size(dtype);
    return g_dp.host_form(ctx, g_dp.data, data, (size_t)snum * tnum * es, &g_dp.out, out, (size_t)snum * (x1 - x0) * es,
                          [&](void *d_in, void *d_out) { return impdar_flatten_dev(ctx, d_in, dtype, snum, tnum, x0, x1, shift, d_out); });
}

extern "C" int impdar_window_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int y0, int y1, int x0, int x1, void *out)
{
    int rc = window_check("impdar_window_dev", ctx, d_data, dtype, snum, tnum, y0, y1, x0, x1);
    if (rc) return rc;
    IMPDAR_ARG_CHECK(out, "impdar_window_dev: null argument");
    if (y1 == y0 || x1 == x0) return IMPDAR_OK;
    const size_t es = impdar_dtype_size(dtype), row = (size_t)(x1 - x0) * es;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    const char *src = (const char *)d_data + ((size_t)y0 * tnum + x0) * es;
    IMPDAR_HIP_CHECK(hipMemcpy2DAsync(out, row, src, (size_t)tnum * es, row, (size_t)(y1 - y0), hipMemcpyDeviceToHost, ctx->stream));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return IMPDAR_OK;
}
