// Instrument files as they are on disk, made into the (snum, tnum) sample-major radargram in HBM (reference
// src/impdar/lib/load/load_gssi.py, load_pulse_ekko.py, load_ramac.py, load_tek.py: trace-major integer or float records,
// decoded there one struct.unpack per trace).  One decode family described by a record descriptor (rawload_route.h), not
// one kernel per instrument:
//
//   rl_mean_kernel     PE_DEMEAN only: one thread per trace, np.nanmean of its first min(100, snum) samples bit for bit --
//                      NaN counts as 0 and leaves the count, the float64 sum runs in NumPy's order for a contiguous
//                      vector of n <= 128 (n < 8 sequential; else eight running sums over the first n - n % 8 samples,
//                      combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the last n % 8 added in order), sum / count;
//   rl_decode_kernel   64 samples x 64 traces per tile through LDS: a wave reads 64 consecutive samples of one record
//                      (coalesced along the record), the tile is turned in LDS (pitch 65 words: a column write of 32
//                      lanes touches 32 banks), a wave writes 64 consecutive traces of one output row.  The op and the
//                      conversion to the output type are applied on the way out, one rounding each, as NumPy's casts.
//
// Reads assume the element's own alignment at most (a pulseEKKO record is 128 + 2 snum bytes, a Tek record 2020); where
// even that fails (`aligned` == 0: a buffer or a base at an odd byte) a sample is put together from its bytes.  Byte
// offsets are 64-bit throughout.  The file is compiled with -ffp-contract=off, like the rest of the library.
#include <algorithm>
#include <cstdint>
#include <type_traits>
#include "common.h"
#include "rawload_route.h"

#define RL_TILE 64
#define RL_BLOCK 256
#define RL_MAX_BLOCKS 4096         // resident workgroups of either kernel; the tiles / traces beyond go round

template <typename Tin> __device__ __forceinline__ Tin rl_read(const unsigned char *p, int aligned)
{
    if (aligned) return *reinterpret_cast<const Tin *>(p);
    uint32_t bits = 0;
#pragma unroll
    for (int b = 0; b < (int)sizeof(Tin); ++b) bits |= (uint32_t)p[b] << (8 * b);
    if constexpr (sizeof(Tin) == 2) {
        return (Tin)(int16_t)(uint16_t)bits;
    } else if constexpr (std::is_same<Tin, float>::value) {
        return __uint_as_float(bits);
    } else {
        return (Tin)(int32_t)bits;
    }
}

template <typename Tin> __device__ __forceinline__ uint32_t rl_pack(Tin v)
{
    if constexpr (std::is_same<Tin, float>::value) return __float_as_uint(v);
    else return (uint32_t)(int32_t)v;
}

template <typename Tin> __device__ __forceinline__ Tin rl_unpack(uint32_t w)
{
    if constexpr (std::is_same<Tin, float>::value) return __uint_as_float(w);
    else return (Tin)(int32_t)w;
}

// the native value of `op` from sample v (and its trace's mean), then astype(Tout)
template <typename Tin, typename Tout> __device__ __forceinline__ Tout rl_finish(Tin v, int op, double mean)
{
    Tin nat = v;
    if constexpr (std::is_same<Tin, int16_t>::value) {
        if (op == IMPDAR_RAW_TEK_BIAS) nat = (int16_t)(uint16_t)((uint32_t)(int32_t)v - 512u);
        else if (op == IMPDAR_RAW_PE_DEMEAN) nat = (int16_t)(uint16_t)(uint32_t)(int32_t)((double)v - mean);   // |v - mean| < 2^17
    } else if constexpr (std::is_same<Tin, float>::value) {
        if (op == IMPDAR_RAW_PE_DEMEAN) nat = (float)((double)v - mean);
    }
    return (Tout)nat;
}

template <typename Tin>
__global__ __launch_bounds__(RL_BLOCK) void rl_mean_kernel(const unsigned char *__restrict__ raw, long long first, long long stride,
                                                           int snum, int tnum, int aligned, double *__restrict__ mean)
{
    const int n = snum < RAWLOAD_MEAN_WINDOW ? snum : RAWLOAD_MEAN_WINDOW;
    for (long long t = (long long)blockIdx.x * RL_BLOCK + threadIdx.x; t < tnum; t += (long long)gridDim.x * RL_BLOCK) {
        const unsigned char *rec = raw + first + t * stride;
        int count = 0;
        const auto at = [&](int i) {
            const double x = (double)rl_read<Tin>(rec + (size_t)i * sizeof(Tin), aligned);
            if (x != x) return 0.0;
            ++count;
            return x;
        };
        double res;
        if (n < 8) {
            res = 0.0;
            for (int i = 0; i < n; ++i) res += at(i);
        } else {
            double r[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = at(j);
            const int body = n - n % 8;
            for (int i = 8; i < body; i += 8) {
#pragma unroll
                for (int j = 0; j < 8; ++j) r[j] += at(i + j);
            }
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (int i = body; i < n; ++i) res += at(i);
        }
        mean[t] = res / (double)count;      // an all-NaN window: 0 / 0
    }
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(RL_BLOCK) void rl_decode_kernel(const unsigned char *__restrict__ raw, long long first, long long stride,
                                                             int snum, int tnum, int op, int aligned,
                                                             const double *__restrict__ mean, Tout *__restrict__ out,
                                                             long long tiles_t, long long ntiles)
{
    __shared__ uint32_t tile[RL_TILE][RL_TILE + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int PER_WAVE = RL_TILE / (RL_BLOCK / 64);
    for (long long it = blockIdx.x; it < ntiles; it += gridDim.x) {
        const long long s0 = (it / tiles_t) * RL_TILE, t0 = (it % tiles_t) * RL_TILE;
        // in: lane = sample of the tile, one record per step
        const long long s = s0 + lane;
        const long long src = (op == IMPDAR_RAW_GSSI_TOP && s < 2) ? 2 : s;
        if (s < snum) {
#pragma unroll 4
            for (int k = 0; k < PER_WAVE; ++k) {
                const int tl = wave * PER_WAVE + k;
                const long long t = t0 + tl;
                if (t < tnum) tile[lane][tl] = rl_pack<Tin>(rl_read<Tin>(raw + first + t * stride + src * (long long)sizeof(Tin), aligned));
            }
        }
        __syncthreads();
        // out: lane = trace of the tile, one output row per step
        const long long t = t0 + lane;
        if (t < tnum) {
            const double m = op == IMPDAR_RAW_PE_DEMEAN ? mean[t] : 0.0;
#pragma unroll 4
            for (int k = 0; k < PER_WAVE; ++k) {
                const int sl = wave * PER_WAVE + k;
                const long long so = s0 + sl;
                if (so < snum) out[(size_t)so * (size_t)tnum + (size_t)t] = rl_finish<Tin, Tout>(rl_unpack<Tin>(tile[sl][lane]), op, m);
            }
        }
        __syncthreads();   // the tile is rewritten for the next one
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct RawBufs {
    DevBuf raw, mean;   // the uploaded file of the host-buffer form, the trace means of PE_DEMEAN
    void release()
    {
        raw.release();
        mean.release();
    }
};
static StepScratch<RawBufs> g_rl;

void impdar_rawload_forget(impdar_ctx *ctx) { g_rl.forget(ctx); }

static RawloadDesc rl_desc(long long nbytes, long long base, long long stride, long long head, int snum, int tnum, int in_kind,
                           int op, int out_kind)
{
    RawloadDesc d;
    d.nbytes = nbytes;
    d.base = base;
    d.stride = stride;
    d.head = head;
    d.snum = snum;
    d.tnum = tnum;
    d.in_kind = in_kind;
    d.op = op;
    d.out_kind = out_kind;
    return d;
}

static int rl_check(const RawloadDesc &d, RawloadRoute &R)
{
    R = rawload_route(d);
    if (R.status != IMPDAR_OK) impdar_set_error("impdar_rawload: %s", R.why);
    return R.status;
}

extern "C" int impdar_rawload_plan(long long nbytes, long long base, long long stride, long long head, int snum, int tnum,
                                   int in_kind, int op, int out_kind, long long *out_bytes)
{
    RawloadRoute R;
    const int rc = rl_check(rl_desc(nbytes, base, stride, head, snum, tnum, in_kind, op, out_kind), R);
    if (out_bytes) *out_bytes = rc ? 0 : R.total_bytes;
    return rc;
}

template <typename Tin, typename Tout>
static void rl_launch(impdar_ctx *ctx, const RawloadDesc &d, const unsigned char *raw, int aligned, void *d_out)
{
    const long long first = d.base + d.head;
    if (d.op == IMPDAR_RAW_PE_DEMEAN) {
        const long long blocks = std::min<long long>(((long long)d.tnum + RL_BLOCK - 1) / RL_BLOCK, RL_MAX_BLOCKS);
        hipLaunchKernelGGL(rl_mean_kernel<Tin>, dim3((unsigned)blocks), dim3(RL_BLOCK), 0, ctx->stream, raw, first, d.stride, d.snum,
                           d.tnum, aligned, g_rl.mean.as<double>());
    }
    const long long tiles_t = ((long long)d.tnum + RL_TILE - 1) / RL_TILE, tiles_s = ((long long)d.snum + RL_TILE - 1) / RL_TILE;
    const long long ntiles = tiles_t * tiles_s;      // < 2^50: snum, tnum < 2^31
    const long long blocks = std::min<long long>(ntiles, RL_MAX_BLOCKS);
    hipLaunchKernelGGL((rl_decode_kernel<Tin, Tout>), dim3((unsigned)blocks), dim3(RL_BLOCK), 0, ctx->stream, raw, first, d.stride,
                       d.snum, d.tnum, d.op, aligned, g_rl.mean.as<double>(), reinterpret_cast<Tout *>(d_out), tiles_t, ntiles);
}

template <typename Tin> static void rl_launch_out(impdar_ctx *ctx, const RawloadDesc &d, const unsigned char *raw, int aligned, void *d_out)
{
    if (d.out_kind == IMPDAR_RAW_OUT_F64) rl_launch<Tin, double>(ctx, d, raw, aligned, d_out);
    else if (d.out_kind == IMPDAR_RAW_OUT_F32) rl_launch<Tin, float>(ctx, d, raw, aligned, d_out);
    else rl_launch<Tin, Tin>(ctx, d, raw, aligned, d_out);
}

// the decode of a checked descriptor on raw bytes in HBM; the caller holds g_rl's lock and has bound the context
static int rl_run(impdar_ctx *ctx, const RawloadDesc &d, const RawloadRoute &R, const void *d_raw, void *d_out)
{
    IMPDAR_ARG_CHECK(((uintptr_t)d_out % (uintptr_t)R.out_bytes) == 0, "impdar_rawload: the output is not aligned to its element");
    if (d.op == IMPDAR_RAW_PE_DEMEAN) IMPDAR_HIP_CHECK(g_rl.mean.ensure((size_t)d.tnum * sizeof(double)));
    const unsigned char *raw = reinterpret_cast<const unsigned char *>(d_raw);
    const uintptr_t el = (uintptr_t)R.in_bytes;
    const int aligned = ((uintptr_t)raw + (uintptr_t)d.base + (uintptr_t)d.head) % el == 0 && (uintptr_t)d.stride % el == 0;
    impdar_ctx_note(ctx, "impdar_rawload", "rl_decode_kernel");
    int rc = impdar_ctx_ktic(ctx);       // the decode kernels alone: impdar_ctx_last_kernel_ms
    if (rc) return rc;
    if (d.in_kind == IMPDAR_RAW_I16) rl_launch_out<int16_t>(ctx, d, raw, aligned, d_out);
    else if (d.in_kind == IMPDAR_RAW_I32) rl_launch_out<int32_t>(ctx, d, raw, aligned, d_out);
    else rl_launch_out<float>(ctx, d, raw, aligned, d_out);
    IMPDAR_HIP_CHECK(hipGetLastError());
    rc = impdar_ctx_ktoc(ctx);
    if (rc) return rc;
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_rawload_dev(impdar_ctx *ctx, const void *d_raw, long long nbytes, long long base, long long stride,
                                  long long head, int snum, int tnum, int in_kind, int op, int out_kind, void *d_out)
{
    const auto lock = g_rl.lock();
    IMPDAR_ARG_CHECK(ctx && d_raw && d_out, "impdar_rawload: null argument");
    const RawloadDesc d = rl_desc(nbytes, base, stride, head, snum, tnum, in_kind, op, out_kind);
    RawloadRoute R;
    const int rc = rl_check(d, R);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_rl.bind(ctx);
    return rl_run(ctx, d, R, d_raw, d_out);
}

extern "C" int impdar_rawload(impdar_ctx *ctx, const void *raw_host, long long nbytes, long long base, long long stride,
                              long long head, int snum, int tnum, int in_kind, int op, int out_kind, void *d_out)
{
    const auto lock = g_rl.lock();
    IMPDAR_ARG_CHECK(ctx && raw_host && d_out, "impdar_rawload: null argument");
    const RawloadDesc d = rl_desc(nbytes, base, stride, head, snum, tnum, in_kind, op, out_kind);
    RawloadRoute R;
    int rc = rl_check(d, R);
    if (rc) return rc;
    // the bytes the kernels read go up, at the offsets they have in the file (stage_in: one copy on the compute stream)
    rc = g_rl.stage_in(ctx, g_rl.raw, raw_host, (size_t)R.last_end);
    if (rc) return rc;
    rc = rl_run(ctx, d, R, g_rl.raw.p, d_out);
    if (rc) return rc;
    // the caller's bytes are free to go away on return
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return IMPDAR_OK;
}
