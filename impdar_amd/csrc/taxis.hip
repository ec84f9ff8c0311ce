// The processing steps that change the TRACE axis of a radargram, kept on the device so that a chain stays resident
// across them (reference src/impdar/lib/RadarData/_RadarDataProcessing.py:20-47, 340-453):
//
//   * restack(traces): out[s, j] = mean(data[s, j * traces : (j + 1) * traces]) for the tnum / traces whole blocks,
//       float64 whatever the input (the reference fills np.zeros), summed in fp64 in trace order:
//         restack_kernel        a workgroup reads a run of whole blocks of one row into an LDS tile with the widest
//                               aligned loads the row allows, then one thread sums one block from LDS (`traces` is
//                               odd, so the lanes' strides fall on different banks) and stores its mean;
//         restack_long_kernel   blocks that do not fit the tile (thousands of traces): one workgroup per output,
//                               a strided fp64 sum reduced by shuffles and LDS;
//   * reverse(): the rows reversed in place, two 16-byte pieces swapped per thread            (reverse_kernel)
//   * hcrop(lim): traces [lo, hi) of every row into a new array of the same dtype: one strided device-to-device
//       copy (hipMemcpy2DAsync).
//
// reverse and hcrop move bits; restack is one fp64 sum and one division.  Data is (snum, tnum) row-major.  The file
// is compiled with -ffp-contract=off, like the rest of the library.
#include "rowwise.h"

#define TX_BLOCK 256
#define TX_MAX_BLOCKS 2048            // resident workgroups; further tiles / rows are reached by a grid stride
#define TX_TILE_BYTES 32768           // LDS tile of restack_kernel (five workgroups per CU)
#define TX_REV_ROWS 4                 // rows per thread and trip of reverse_kernel

// A tile is `nper` whole blocks of one row, inputs [first, first + n) of the array.  They are loaded from the last
// multiple of V at or below `first` (the row starts on one, so that is still inside the row) to the first at or
// above the end (at most the row's end), V elements per access, and land in LDS at the same offset from that
// point, so LDS accesses are as aligned as the global ones.
template <typename T, int V>
__global__ __launch_bounds__(TX_BLOCK) void restack_kernel(const T *__restrict__ x, double *__restrict__ out, int snum,
                                                           int tnum, int traces, int tnum_new, int nper)
{
    typedef RwVec<T, V> Vec;
    constexpr int CAP = TX_TILE_BYTES / sizeof(T);
    __shared__ Vec tile[CAP / V];
    T *lds = reinterpret_cast<T *>(tile);
    const int tiles_per_row = (tnum_new + nper - 1) / nper;
    const long long ntiles = (long long)snum * tiles_per_row;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int s = (int)(t / tiles_per_row);
        const int j0 = (int)(t % tiles_per_row) * nper;
        const int nb = tnum_new - j0 < nper ? tnum_new - j0 : nper;        // blocks of this tile
        const size_t first = (size_t)s * tnum + (size_t)j0 * traces;       // first input element
        const size_t base = first / V * V;
        const int off = (int)(first - base);
        const int nvec = (off + nb * traces + V - 1) / V;                  // (off + nper * traces + V - 1) / V <= CAP / V
        const Vec *src = reinterpret_cast<const Vec *>(x + base);
#pragma unroll 4
        for (int k = threadIdx.x; k < nvec; k += TX_BLOCK) tile[k] = src[k];
        __syncthreads();
        for (int b = threadIdx.x; b < nb; b += TX_BLOCK) {
            const T *p = lds + off + b * traces;
            double sum = 0.0;
            for (int k = 0; k < traces; ++k) sum += (double)p[k];
            out[(size_t)s * tnum_new + j0 + b] = sum / (double)traces;
        }
        __syncthreads();   // the tile is rewritten by the next trip
    }
}

template <typename T>
__global__ __launch_bounds__(TX_BLOCK) void restack_long_kernel(const T *__restrict__ x, double *__restrict__ out,
                                                                int snum, int tnum, int traces, int tnum_new)
{
    __shared__ double red[TX_BLOCK / 64];
    const long long nout = (long long)snum * tnum_new;
    for (long long o = blockIdx.x; o < nout; o += gridDim.x) {
        const int s = (int)(o / tnum_new), j = (int)(o % tnum_new);
        const T *p = x + (size_t)s * tnum + (size_t)j * traces;
        double sum = 0.0;
        for (int k = threadIdx.x; k < traces; k += TX_BLOCK) sum += (double)p[k];
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) sum += __shfl_xor(sum, w, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) out[o] = ((red[0] + red[1]) + (red[2] + red[3])) / (double)traces;
        __syncthreads();   // red is rewritten by the next trip
    }
}

template <typename T, int V> __device__ __forceinline__ RwVec<T, V> tx_flip(const RwVec<T, V> &a)
{
    RwVec<T, V> r;
#pragma unroll
    for (int c = 0; c < V; ++c) r.v[c] = a.v[V - 1 - c];
    return r;
}

// tnum % V == 0: a row is nvec pieces of V traces, and piece k changes places with piece nvec - 1 - k, each turned
// round.  A thread owns one such pair (the middle piece of an odd count is its own partner: both stores then write
// the same bits) in TX_REV_ROWS consecutive rows.
template <typename T, int V>
__global__ __launch_bounds__(TX_BLOCK) void reverse_kernel(T *__restrict__ x, int snum, int tnum)
{
    typedef RwVec<T, V> Vec;
    const int nvec = tnum / V;
    const int k = blockIdx.x * TX_BLOCK + threadIdx.x;
    if (k >= (nvec + 1) / 2) return;
    const int m = nvec - 1 - k;
    for (int i0 = blockIdx.y * TX_REV_ROWS; i0 < snum; i0 += gridDim.y * TX_REV_ROWS) {
        Vec a[TX_REV_ROWS], b[TX_REV_ROWS];
#pragma unroll
        for (int u = 0; u < TX_REV_ROWS; ++u) {
            const int i = i0 + u < snum ? i0 + u : snum - 1;
            const Vec *row = reinterpret_cast<const Vec *>(x + (size_t)i * tnum);
            a[u] = row[k];
            b[u] = row[m];
        }
#pragma unroll
        for (int u = 0; u < TX_REV_ROWS; ++u) {
            if (i0 + u < snum) {
                Vec *row = reinterpret_cast<Vec *>(x + (size_t)(i0 + u) * tnum);
                row[k] = tx_flip<T, V>(b[u]);
                row[m] = tx_flip<T, V>(a[u]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct TaxisBufs {
    DevBuf data, out;   // staging of the host-buffer form of restack (input, result)
    void release()
    {
        data.release();
        out.release();
    }
};
static StepScratch<TaxisBufs> g_tx;

void impdar_taxis_forget(impdar_ctx *ctx) { g_tx.forget(ctx); }

template <typename T, int V>
static void restack_launch(impdar_ctx *ctx, const void *d_data, double *d_out, int snum, int tnum, int traces, int tnum_new)
{
    const int cap = TX_TILE_BYTES / (int)sizeof(T);
    const int nper = (cap - 2 * (V - 1)) / traces;   // whole blocks per tile, with room for the aligned ends
    if (nper >= 1) {
        const long long ntiles = (long long)snum * ((tnum_new + nper - 1) / nper);
        const int nblk = ntiles < TX_MAX_BLOCKS ? (int)ntiles : TX_MAX_BLOCKS;
        hipLaunchKernelGGL((restack_kernel<T, V>), dim3(nblk), dim3(TX_BLOCK), 0, ctx->stream, (const T *)d_data, d_out,
                           snum, tnum, traces, tnum_new, nper);
    } else {
        const long long nout = (long long)snum * tnum_new;
        const int nblk = nout < TX_MAX_BLOCKS ? (int)nout : TX_MAX_BLOCKS;
        hipLaunchKernelGGL(restack_long_kernel<T>, dim3(nblk), dim3(TX_BLOCK), 0, ctx->stream, (const T *)d_data, d_out,
                           snum, tnum, traces, tnum_new);
    }
}

static int restack_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int traces, const double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "impdar_restack: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_restack: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_restack: empty radargram");
    IMPDAR_ARG_CHECK(traces >= 1 && traces % 2 == 1, "impdar_restack: %d traces per stack (an odd number, at least 1)", traces);
    return IMPDAR_OK;
}

extern "C" int impdar_restack_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int traces,
                                  double *d_out)
{
    const auto lock = g_tx.lock();
    const int rc = restack_check(ctx, d_data, dtype, snum, tnum, traces, d_out);
    if (rc) return rc;
    const int tnum_new = tnum / traces;
    if (tnum_new == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_tx.bind(ctx);
    rw_dispatch(dtype, {d_data}, tnum, [&](auto t, auto v) {
        restack_launch<typename decltype(t)::type, decltype(v)::value>(ctx, d_data, d_out, snum, tnum, traces, tnum_new);
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

template <typename T, int V> static void reverse_launch(impdar_ctx *ctx, void *d_data, int snum, int tnum)
{
    const int pairs = (tnum / V + 1) / 2;
    const int gx = (pairs + TX_BLOCK - 1) / TX_BLOCK;
    const int groups = (snum + TX_REV_ROWS - 1) / TX_REV_ROWS;
    const int cap = TX_MAX_BLOCKS / gx > 1 ? TX_MAX_BLOCKS / gx : 1;
    hipLaunchKernelGGL((reverse_kernel<T, V>), dim3(gx, groups < cap ? groups : cap), dim3(TX_BLOCK), 0, ctx->stream,
                       (T *)d_data, snum, tnum);
}

extern "C" int impdar_reverse_dev(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum)
{
    const auto lock = g_tx.lock();
    IMPDAR_ARG_CHECK(ctx && d_data, "impdar_reverse: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_reverse: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_reverse: empty radargram");
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    rw_dispatch(dtype, {d_data}, tnum, [&](auto t, auto v) {
        reverse_launch<typename decltype(t)::type, decltype(v)::value>(ctx, d_data, snum, tnum);
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_hcrop_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int lo, int hi,
                                void *d_out)
{
    IMPDAR_ARG_CHECK(ctx && d_data && d_out, "impdar_hcrop: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_hcrop: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_hcrop: empty radargram");
    IMPDAR_ARG_CHECK(lo >= 0 && lo <= hi && hi <= tnum, "impdar_hcrop: trace range [%d, %d) not inside [0, %d]", lo, hi, tnum);
    if (hi == lo) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t es = impdar_dtype_size(dtype), width = (size_t)(hi - lo) * es;
    IMPDAR_HIP_CHECK(hipMemcpy2DAsync(d_out, width, (const char *)d_data + (size_t)lo * es, (size_t)tnum * es, width,
                                      (size_t)snum, hipMemcpyDeviceToDevice, ctx->stream));
    return impdar_ctx_mark_produced(ctx);
}

// ---- host-buffer form: the argument check, then StepScratch::host_form -------------------------------------

extern "C" int impdar_restack(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int traces, double *out)
{
    const int rc = restack_check(ctx, data, dtype, snum, tnum, traces, out);
    if (rc) return rc;
    const int tnum_new = tnum / traces;
    if (tnum_new == 0) return IMPDAR_OK;
    return g_tx.host_form(ctx, g_tx.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype), &g_tx.out, out,
                          (size_t)snum * tnum_new * sizeof(double), [&](void *d_in, void *d_out) {
                              return impdar_restack_dev(ctx, d_in, dtype, snum, tnum, traces, (double *)d_out);
                          });
}
