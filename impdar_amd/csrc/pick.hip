// Layer picking on a resident radargram (reference src/impdar/lib/picklib.py:16-199 and
// src/impdar/lib/analysis/continuity_index.py:27-81).  Data is (snum, tnum) row-major, float32 or float64.
//
//   * the packet rule (picklib.packet_pick): around a midpoint, the packet trace[slice(top, bot)] with
//       top = trunc(mid - plength / 2.), bot = trunc(mid + plength / 2.) and Python's slice semantics; in it the
//       centre peak c (argmax of pol * x over FWW samples from scst + 1), the opposite peaks t above and b below
//       (argmin over at most FWW samples) and the mean power of [t, b].  Every slice end is clipped to the packet's
//       length L as NumPy clips it; argmax / argmin take the first NaN, else the first extreme.  pk_rule states it
//       once, over a "window" that knows how to read packet sample k and how to reduce a range of them.
//   * pk_walk_kernel (picklib.auto_pick): the window of trace j + 1 is centred on the pick of trace j, so a seed is
//       a chain of tnum dependent steps.  One wave (a workgroup of 64) per seed and direction: the left wave picks
//       t0, t0 - 1 ... 0, the right one re-computes t0 and picks t0 + 1 ... tnum - 1.  The wave keeps a band of the
//       radargram in LDS -- `rows` rows around the current window by the PK_W traces of the 32-aligned trace chunk
//       it is in, loaded row-wise (a row segment is one 128- or 256-byte line) and stored trace-major with an odd
//       pitch, so the 64 lanes that stride a window read 64 banks -- and walks the chunk out of it: a step costs
//       LDS reads and cross-lane moves, not an HBM miss.  It restages when the next window is not wholly inside
//       the staged rows or the chunk is used up.  A plength above PK_STAGE_MAX cannot keep a margin around its
//       window in the 64 KiB a workgroup may hold and takes the same walk with the window read from global memory.
//       The three arg-reductions and the power sum are wave reductions by DPP row shifts and row broadcasts.
//   * pk_guided_kernel (picklib.pick): independent picks, one per trace, each with its own midpoint: adjacent
//       lanes take adjacent traces, every lane runs the rule serially over its own column.
//   * pk_continuity_kernel (continuity_index, Karlsson et al. 2012): per trace the mean |np.gradient(P)| of
//       P = 10 log10(x^2) over rows [s, b), optionally with int(len * ratio) rows off both ends; NaN when fewer than
//       10 rows remain or a P is not finite.  The square is rounded in the data's dtype (that is where the
//       reference's zeros and overflows come from), everything after it is fp64.  Adjacent lanes, adjacent traces.
//
// Outcome codes of a pick: 0 picked, 1 the packet is shorter than scst + FWW (the reference's 'frequency is too
// high' ValueError), 2 / 3 an empty argmax / argmin slice (NumPy's ValueError).
#include <climits>
#include "vecwidth.h"

#define PK_W 32            // traces of a staged band (one chunk of the trace axis)
#define PK_ROWS 254        // most rows of a band: 32 x 255 doubles are 65280 bytes of LDS
#define PK_MARGIN 32       // rows a band keeps on either side of the longest window it serves
#define PK_STAGE_MAX (PK_ROWS - 2 * PK_MARGIN)   // 190: the longest plength that walks out of LDS

#define PK_OK 0
#define PK_SHORT 1
#define PK_EMPTY_ARGMAX 2
#define PK_EMPTY_ARGMIN 3

// ------------------------------------------------------------------------------------------------ packet bounds
struct PkPacket {
    long long top;   // the reference's topsnum: what is added to t, c and b
    int start, len;  // the packet is rows [start, start + len) of the trace
};

__device__ __forceinline__ long long pk_slice_end(long long v, int snum)
{
    if (v < 0) {
        v += snum;
        return v < 0 ? 0 : v;
    }
    return v > snum ? snum : v;
}

__device__ __forceinline__ PkPacket pk_packet(long long mid, int plength, int snum)
{
    const double half = (double)plength / 2.;
    const double dtop = trunc((double)mid - half), dbot = trunc((double)mid + half);
    // a midpoint far outside the data cannot pick; keep the conversions in range
    const double lim = 4.0e18;
    const long long top = (long long)(dtop < -lim ? -lim : dtop > lim ? lim : dtop);
    const long long bot = (long long)(dbot < -lim ? -lim : dbot > lim ? lim : dbot);
    const long long a = pk_slice_end(top, snum), b = pk_slice_end(bot, snum);
    PkPacket p;
    p.top = top;
    p.start = (int)a;
    p.len = b > a ? (int)(b - a) : 0;
    return p;
}

// floor((a + b) / 2) of two row numbers, the reference's (pp[0] + pp[2]) // 2
__device__ __forceinline__ long long pk_next_mid(long long a, long long b)
{
    const long long s = a + b;
    return s >= 0 ? s / 2 : -((-s + 1) / 2);
}

// ------------------------------------------------------------------------------------------------ ordering
// An unsigned key that orders pol * x as np.argmax does: a NaN above everything, -0 equal to +0.
__device__ __forceinline__ unsigned long long pk_key(float v)
{
    if (v != v) return ~0ull;
    if (v == 0.f) v = 0.f;
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? (unsigned)~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long pk_key(double v)
{
    if (v != v) return ~0ull;
    if (v == 0.) v = 0.;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct PkBest {
    unsigned long long key;   // 0: nothing seen (no value maps to 0)
    unsigned idx;
};
__device__ __forceinline__ PkBest pk_none() { return PkBest{0ull, 0xffffffffu}; }
__device__ __forceinline__ PkBest pk_better(const PkBest &a, const PkBest &b)
{
    return (b.key > a.key || (b.key == a.key && b.idx < a.idx)) ? b : a;
}

// ------------------------------------------------------------------------------------------------ wave reductions
// One DPP move of the wave: lanes whose source does not exist, or whose row is masked out, get `idle`.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int pk_dpp(int idle, int v)
{
    return __builtin_amdgcn_update_dpp(idle, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ PkBest pk_dpp_best(const PkBest &x)
{
    PkBest y;
    const unsigned lo = (unsigned)pk_dpp<CTRL, ROW_MASK>(0, (int)(unsigned)x.key);
    const unsigned hi = (unsigned)pk_dpp<CTRL, ROW_MASK>(0, (int)(unsigned)(x.key >> 32));
    y.key = ((unsigned long long)hi << 32) | lo;
    y.idx = (unsigned)pk_dpp<CTRL, ROW_MASK>(-1, (int)x.idx);
    return y;
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double pk_dpp_f64(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = (unsigned)pk_dpp<CTRL, ROW_MASK>(0, (int)(unsigned)b);
    const unsigned hi = (unsigned)pk_dpp<CTRL, ROW_MASK>(0, (int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// row_shr:1, 2, 4, 8 leave a row's result in its lane 15; row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows
// 2 and 3 leave the wave's in lane 63.  All 64 lanes are active here.
__device__ __forceinline__ PkBest pk_wave_best(PkBest x)
{
    x = pk_better(x, pk_dpp_best<0x111, 0xf>(x));
    x = pk_better(x, pk_dpp_best<0x112, 0xf>(x));
    x = pk_better(x, pk_dpp_best<0x114, 0xf>(x));
    x = pk_better(x, pk_dpp_best<0x118, 0xf>(x));
    x = pk_better(x, pk_dpp_best<0x142, 0xa>(x));
    x = pk_better(x, pk_dpp_best<0x143, 0xc>(x));
    PkBest r;
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x.key, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x.key >> 32), 63);
    r.key = ((unsigned long long)hi << 32) | lo;
    r.idx = (unsigned)__builtin_amdgcn_readlane((int)x.idx, 63);
    return r;
}
__device__ __forceinline__ double pk_wave_sum(double x)
{
    x += pk_dpp_f64<0x111, 0xf>(x);
    x += pk_dpp_f64<0x112, 0xf>(x);
    x += pk_dpp_f64<0x114, 0xf>(x);
    x += pk_dpp_f64<0x118, 0xf>(x);
    x += pk_dpp_f64<0x142, 0xa>(x);
    x += pk_dpp_f64<0x143, 0xc>(x);
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 63);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ------------------------------------------------------------------------------------------------ windows
// A window reads packet sample k (0 <= k < len) and reduces ranges [lo, hi) of them, 0 <= lo < hi <= len:
//   argmax(lo, hi, pol)  index, from lo, of the first NaN of pol * x, else of its first maximum
//   sumsq(lo, hi)        sum of x * x, each square rounded in T, summed in fp64 (hi <= lo: 0)

// the whole wave on one packet: lanes stride the range; every result is the same in all lanes
template <typename T, bool STAGED> struct PkWaveWindow {
    const T *p;       // sample 0 of the packet: in the staged band (pitch 1) or in global memory (pitch tnum)
    size_t pitch;
    int lane;
    __device__ __forceinline__ T get(int k) const { return STAGED ? p[k] : p[(size_t)k * pitch]; }
    __device__ __forceinline__ int argmax(int lo, int hi, T pol) const
    {
        PkBest best = pk_none();
        for (int k = lo + lane; k < hi; k += 64) {
            const PkBest cand{pk_key(pol * get(k)), (unsigned)k};
            best = pk_better(best, cand);
        }
        return (int)pk_wave_best(best).idx - lo;
    }
    __device__ __forceinline__ double sumsq(int lo, int hi) const
    {
        double s = 0.;
        for (int k = lo + lane; k < hi; k += 64) {
            const T v = get(k);
            const T q = v * v;
            s += (double)q;
        }
        return pk_wave_sum(s);
    }
};

// one lane on its own packet in global memory
template <typename T> struct PkLaneWindow {
    const T *p;
    size_t pitch;
    __device__ __forceinline__ T get(int k) const { return p[(size_t)k * pitch]; }
    __device__ __forceinline__ int argmax(int lo, int hi, T pol) const
    {
        PkBest best = pk_none();
        for (int k = lo; k < hi; ++k) {
            const PkBest cand{pk_key(pol * get(k)), (unsigned)k};
            best = pk_better(best, cand);
        }
        return (int)best.idx - lo;
    }
    __device__ __forceinline__ double sumsq(int lo, int hi) const
    {
        double s = 0.;
        for (int k = lo; k < hi; ++k) {
            const T v = get(k);
            const T q = v * v;
            s += (double)q;
        }
        return s;
    }
};

struct PkParams {
    int plength, FWW, scst, pol;
};

struct PkPick {
    long long t, c, b;   // rows of the radargram (top added)
    double power;
};

__device__ __forceinline__ int pk_clip(long long v, int len) { return v < 0 ? 0 : v > len ? len : (int)v; }

// The packet rule.  `len` is the packet's length, `top` what the reference adds to its indices.
template <typename T, class Window>
__device__ __forceinline__ int pk_rule(const Window &w, long long top, int len, const PkParams &pp, PkPick &out)
{
    const long long plength = pp.plength, FWW = pp.FWW, scst = pp.scst;
    if (len < scst + FWW) return PK_SHORT;
    const T pol = (T)pp.pol;
    int lo = pk_clip(scst + 1, len), hi = pk_clip(scst + FWW + 1, len);
    if (lo >= hi) return PK_EMPTY_ARGMAX;
    const long long c = w.argmax(lo, hi, pol) + lo;

    long long t;
    if (c > FWW) {
        lo = pk_clip(c - FWW, len), hi = pk_clip(c, len);
        t = w.argmax(lo, hi, -pol) + lo;   // lo < hi: c <= len and FWW >= 1
    } else if (c <= 1) {
        t = 0;
    } else {
        t = w.argmax(0, pk_clip(c, len), -pol);
    }

    long long b;
    if (c + FWW < plength) {
        lo = pk_clip(c + 1, len), hi = pk_clip(c + FWW + 1, len);
        if (lo >= hi) return PK_EMPTY_ARGMIN;
        b = w.argmax(lo, hi, -pol) + lo;
    } else if (c >= plength - 1) {
        b = plength - 1;
    } else {
        lo = pk_clip(c + 1, len);
        if (lo >= len) return PK_EMPTY_ARGMIN;
        b = w.argmax(lo, len, -pol) + lo;
    }

    // the slice is clipped, the divisor is not; NumPy's quotient is in the data's dtype
    const double sum = w.sumsq(pk_clip(t, len), pk_clip(b + 1, len));
    out.power = (double)(T)(sum / (double)(b - t + 1));
    out.t = t + top;
    out.c = c + top;
    out.b = b + top;
    return PK_OK;
}

// ------------------------------------------------------------------------------------------------ auto_pick
// grid: 2 * nseeds workgroups of one wave; workgroup 2 s walks seed s to the left, 2 s + 1 to the right.
// out: (nseeds, 5, tnum) doubles, preset to NaN; stat: (nseeds, 2 directions, 2) ints {outcome, trace it stopped at
// or -1}.  `rows` is the band's row count (<= PK_ROWS, <= snum), its LDS pitch rows | 1.
template <typename T, bool STAGED>
__global__ __launch_bounds__(64) void pk_walk_kernel(const T *__restrict__ x, int snum, int tnum,
                                                     const int *__restrict__ seed_snum, const int *__restrict__ seed_tnum,
                                                     PkParams pp, int rows, double *__restrict__ out, int *__restrict__ stat)
{
    extern __shared__ __align__(16) unsigned char pk_lds[];
    T *band = reinterpret_cast<T *>(pk_lds);
    const int pitch = rows | 1;
    const int lane = threadIdx.x;
    const int seed = blockIdx.x >> 1, right = blockIdx.x & 1;
    const int t0 = seed_tnum[seed];
    long long mid = seed_snum[seed];
    double *o = out + (size_t)seed * 5 * tnum;

    int chunk = -1, r0 = 0;   // the staged band: traces [chunk * PK_W, ...), rows [r0, r0 + rows)
    int j = t0, code = PK_OK;
    for (;;) {
        const PkPacket pk = pk_packet(mid, pp.plength, snum);
        PkWaveWindow<T, STAGED> w;
        w.lane = lane;
        if (STAGED) {
            // a packet that will be refused for its length is not read, so it need not be staged
            if (pk.len >= pp.scst + pp.FWW && (j / PK_W != chunk || pk.start < r0 || pk.start + pk.len > r0 + rows)) {
                __syncthreads();   // the reads of the band that is being replaced
                chunk = j / PK_W;
                r0 = pk.start - (rows - pk.len) / 2;   // len <= min(plength, snum) <= rows
                r0 = r0 > snum - rows ? snum - rows : r0;
                r0 = r0 < 0 ? 0 : r0;
                const int col = chunk * PK_W + (lane & (PK_W - 1));
                if (col < tnum) {
                    const T *src = x + (size_t)r0 * tnum + col;
                    T *dst = band + (size_t)(lane & (PK_W - 1)) * pitch;
#pragma unroll 8
                    for (int r = lane / PK_W; r < rows; r += 64 / PK_W) dst[r] = src[(size_t)r * tnum];
                }
                __syncthreads();
            }
            w.p = band + (size_t)(j & (PK_W - 1)) * pitch + (pk.start - r0);
            w.pitch = 1;
        } else {
            w.p = x + (size_t)pk.start * tnum + j;
            w.pitch = (size_t)tnum;
        }
        PkPick res;
        code = pk_rule<T>(w, pk.top, pk.len, pp, res);
        if (code != PK_OK) break;
        if (lane == 0 && (!right || j != t0)) {
            o[j] = (double)res.t;
            o[(size_t)tnum + j] = (double)res.c;
            o[(size_t)2 * tnum + j] = (double)res.b;
            o[(size_t)4 * tnum + j] = res.power;   // row 3 stays NaN
        }
        mid = pk_next_mid(res.t, res.b);
        if (right) {
            if (j == tnum - 1) break;
            ++j;
        } else {
            if (j == 0) break;
            --j;
        }
    }
    if (lane == 0) {
        stat[blockIdx.x * 2] = code;
        stat[blockIdx.x * 2 + 1] = code == PK_OK ? -1 : j;
    }
}

// ------------------------------------------------------------------------------------------------ guided pick
// out: (5, n) doubles, preset to NaN; codes: n ints
template <typename T>
__global__ __launch_bounds__(64) void pk_guided_kernel(const T *__restrict__ x, int snum, int tnum, int t0, int n,
                                                       const int *__restrict__ mid, PkParams pp, double *__restrict__ out,
                                                       int *__restrict__ codes)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const PkPacket pk = pk_packet(mid[i], pp.plength, snum);
    PkLaneWindow<T> w;
    w.p = x + (size_t)pk.start * tnum + (t0 + i);   // start <= snum; nothing is read when len is 0
    w.pitch = (size_t)tnum;
    PkPick res;
    const int code = pk_rule<T>(w, pk.top, pk.len, pp, res);
    codes[i] = code;
    if (code != PK_OK) return;
    out[i] = (double)res.t;
    out[(size_t)n + i] = (double)res.c;
    out[(size_t)2 * n + i] = (double)res.b;
    out[(size_t)4 * n + i] = res.power;
}

// ------------------------------------------------------------------------------------------------ continuity index
// s, b: slice bounds per trace, 0 <= s, b <= snum, or -1 for a NaN pick
template <typename T>
__global__ __launch_bounds__(64) void pk_continuity_kernel(const T *__restrict__ x, int snum, int tnum,
                                                           const int *__restrict__ s, const int *__restrict__ b, int cut_mode,
                                                           double ratio, double *__restrict__ out)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= tnum) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double res = nan;
    const int sj = s[j], bj = b[j];
    if (sj >= 0 && bj >= 0) {
        int lo = sj, hi = bj > sj ? bj : sj;
        if (cut_mode) {
            const double want = (double)(hi - lo) * ratio;
            const int cut = want >= (double)(hi - lo) ? hi - lo : want <= 0. ? 0 : (int)want;
            // p_ext[cut:-cut] is empty for cut == 0 (and for a negative one, at the lengths that count); a cut that
            // meets in the middle leaves nothing as well
            if (cut <= 0 || 2 * (long long)cut >= hi - lo) hi = lo;
            else lo += cut, hi -= cut;
        }
        const int len = hi - lo;
        if (len >= 10) {
            const T *p = x + (size_t)lo * tnum + j;
            bool finite = true;
            double prev2 = 0., prev = 0., acc = 0.;
            for (int k = 0; k < len; ++k) {
                const T v = p[(size_t)k * tnum];
                const T q = v * v;
                finite = finite && q > (T)0 && q <= (sizeof(T) == 4 ? (T)3.4028234663852886e38 : (T)1.7976931348623157e308);
                const double P = 10. * log10((double)q);
                if (k == 1) acc += fabs(P - prev);                       // one-sided at the first row
                if (k >= 2) acc += fabs((P - prev2) / 2.);               // central at row k - 1
                if (k == len - 1) acc += fabs(P - prev);                 // one-sided at the last row
                prev2 = prev;
                prev = P;
            }
            if (finite) res = acc / (double)len;
        }
    }
    out[j] = res;
}

// ------------------------------------------------------------------------------------------------ host side

struct PickBufs {
    DevBuf data, tab, out, stat;   // staging of the host-buffer forms, the host tables, the picks, the outcomes
    void release()
    {
        data.release();
        tab.release();
        out.release();
        stat.release();
    }
};
static StepScratch<PickBufs> g_pk;

void impdar_pick_forget(impdar_ctx *ctx) { g_pk.forget(ctx); }

static int pk_params_check(const char *who, int plength, int FWW, int scst, int pol)
{
    IMPDAR_ARG_CHECK(plength >= 1 && FWW >= 1 && scst >= 0, "%s: plength %d, FWW %d, scst %d: need plength >= 1, FWW >= 1, scst >= 0",
                     who, plength, FWW, scst);
    IMPDAR_ARG_CHECK(FWW < (1 << 30) && scst < (1 << 30), "%s: FWW %d or scst %d is out of range", who, FWW, scst);
    IMPDAR_ARG_CHECK(pol == 1 || pol == -1, "%s: pol must be 1 or -1, got %d", who, pol);
    return IMPDAR_OK;
}

// rows of the staged band for a plength that is staged
static int pk_band_rows(int plength, int snum)
{
    int rows = 3 * plength > plength + 2 * PK_MARGIN ? 3 * plength : plength + 2 * PK_MARGIN;
    rows = rows < PK_ROWS ? rows : PK_ROWS;
    return rows < snum ? rows : snum;
}

static int auto_pick_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int nseeds, const int *seed_snum,
                           const int *seed_tnum, int plength, int FWW, int scst, int pol, const double *out, const int *status)
{
    IMPDAR_ARG_CHECK(ctx && data && seed_snum && seed_tnum && out && status, "impdar_auto_pick: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_auto_pick: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_auto_pick: empty radargram");
    IMPDAR_ARG_CHECK(nseeds >= 1 && nseeds <= (1 << 20), "impdar_auto_pick: %d seeds", nseeds);
    for (int k = 0; k < nseeds; ++k)
        IMPDAR_ARG_CHECK(seed_tnum[k] >= 0 && seed_tnum[k] < tnum, "impdar_auto_pick: seed %d starts at trace %d of %d", k,
                         seed_tnum[k], tnum);
    return pk_params_check("impdar_auto_pick", plength, FWW, scst, pol);
}

extern "C" int impdar_auto_pick_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int nseeds,
                                    const int *seed_snum, const int *seed_tnum, int plength, int FWW, int scst, int pol,
                                    double *out, int *status)
{
    const auto lock = g_pk.lock();
    int rc = auto_pick_check(ctx, d_data, dtype, snum, tnum, nseeds, seed_snum, seed_tnum, plength, FWW, scst, pol, out, status);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_pk.bind(ctx);
    const void *d_tab[2];
    rc = impdar_upload_tables(ctx, g_pk.tab, {{seed_snum, (size_t)nseeds * sizeof(int)}, {seed_tnum, (size_t)nseeds * sizeof(int)}},
                              d_tab);
    if (rc) return rc;
    const size_t out_bytes = (size_t)nseeds * 5 * tnum * sizeof(double), stat_bytes = (size_t)nseeds * 4 * sizeof(int);
    IMPDAR_HIP_CHECK(g_pk.out.ensure(out_bytes));
    IMPDAR_HIP_CHECK(g_pk.stat.ensure(stat_bytes));
    IMPDAR_HIP_CHECK(hipMemsetAsync(g_pk.out.p, 0xff, out_bytes, ctx->stream));   // all ones: a NaN
    IMPDAR_HIP_CHECK(hipMemsetAsync(g_pk.stat.p, 0, stat_bytes, ctx->stream));
    const PkParams pp{plength, FWW, scst, pol};
    const bool staged = plength <= PK_STAGE_MAX;
    const int rows = staged ? pk_band_rows(plength, snum) : 0;
    rw_typed(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        const size_t lds = staged ? (size_t)PK_W * (rows | 1) * sizeof(T) : 0;
        if (staged)
            hipLaunchKernelGGL((pk_walk_kernel<T, true>), dim3(2 * nseeds), dim3(64), lds, ctx->stream, (const T *)d_data, snum,
                               tnum, (const int *)d_tab[0], (const int *)d_tab[1], pp, rows, g_pk.out.as<double>(),
                               g_pk.stat.as<int>());
        else
            hipLaunchKernelGGL((pk_walk_kernel<T, false>), dim3(2 * nseeds), dim3(64), lds, ctx->stream, (const T *)d_data, snum,
                               tnum, (const int *)d_tab[0], (const int *)d_tab[1], pp, rows, g_pk.out.as<double>(),
                               g_pk.stat.as<int>());
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    std::vector<int> stat((size_t)nseeds * 4);
    IMPDAR_HIP_CHECK(hipMemcpyAsync(stat.data(), g_pk.stat.p, stat_bytes, hipMemcpyDeviceToHost, ctx->stream));
    rc = impdar_download(ctx, out, g_pk.out.p, out_bytes, ctx->stream);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // a seed's left walk comes before its right walk in the reference's loop
    for (int k = 0; k < nseeds; ++k) {
        const int *s = &stat[(size_t)k * 4];
        const int dir = s[0] != PK_OK ? 0 : 1;
        status[2 * k] = s[2 * dir];
        status[2 * k + 1] = s[2 * dir + 1];
    }
    return IMPDAR_OK;
}

static int pick_guided_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int t0, int n, const int *mid,
                             int plength, int FWW, int scst, int pol, const double *out, const int *status)
{
    IMPDAR_ARG_CHECK(ctx && data && mid && out && status, "impdar_pick_guided: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_pick_guided: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_pick_guided: empty radargram");
    IMPDAR_ARG_CHECK(t0 >= 0 && n >= 1 && n <= tnum - t0, "impdar_pick_guided: traces %d ... %d + %d of %d", t0, t0, n, tnum);
    return pk_params_check("impdar_pick_guided", plength, FWW, scst, pol);
}

extern "C" int impdar_pick_guided_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int t0, int n,
                                      const int *mid, int plength, int FWW, int scst, int pol, double *out, int *status)
{
    const auto lock = g_pk.lock();
    int rc = pick_guided_check(ctx, d_data, dtype, snum, tnum, t0, n, mid, plength, FWW, scst, pol, out, status);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_pk.bind(ctx);
    const void *d_tab[1];
    rc = impdar_upload_tables(ctx, g_pk.tab, {{mid, (size_t)n * sizeof(int)}}, d_tab);
    if (rc) return rc;
    const size_t out_bytes = (size_t)5 * n * sizeof(double), stat_bytes = (size_t)n * sizeof(int);
    IMPDAR_HIP_CHECK(g_pk.out.ensure(out_bytes));
    IMPDAR_HIP_CHECK(g_pk.stat.ensure(stat_bytes));
    IMPDAR_HIP_CHECK(hipMemsetAsync(g_pk.out.p, 0xff, out_bytes, ctx->stream));
    IMPDAR_HIP_CHECK(hipMemsetAsync(g_pk.stat.p, 0, stat_bytes, ctx->stream));
    const PkParams pp{plength, FWW, scst, pol};
    rw_typed(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(pk_guided_kernel<T>, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, (const T *)d_data, snum, tnum, t0, n,
                           (const int *)d_tab[0], pp, g_pk.out.as<double>(), g_pk.stat.as<int>());
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    std::vector<int> codes((size_t)n);
    IMPDAR_HIP_CHECK(hipMemcpyAsync(codes.data(), g_pk.stat.p, stat_bytes, hipMemcpyDeviceToHost, ctx->stream));
    rc = impdar_download(ctx, out, g_pk.out.p, out_bytes, ctx->stream);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    status[0] = PK_OK;
    status[1] = -1;
    for (int i = 0; i < n; ++i)
        if (codes[i] != PK_OK) {   // the reference's loop stops at its first failing trace
            status[0] = codes[i];
            status[1] = t0 + i;
            break;
        }
    return IMPDAR_OK;
}

static int continuity_check(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *s, const int *b,
                            int cut_mode, double ratio, const double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && s && b && out, "impdar_continuity: null argument");
    IMPDAR_ARG_CHECK(impdar_dtype_ok(dtype), "impdar_continuity: dtype must be float32 or float64");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "impdar_continuity: empty radargram");
    IMPDAR_ARG_CHECK(cut_mode == 0 || cut_mode == 1, "impdar_continuity: cut_mode must be 0 or 1");
    IMPDAR_ARG_CHECK(!cut_mode || (ratio == ratio && ratio > -1.0e9 && ratio < 1.0e9), "impdar_continuity: cutoff_ratio %g", ratio);
    for (int j = 0; j < tnum; ++j)
        IMPDAR_ARG_CHECK(s[j] >= -1 && s[j] <= snum && b[j] >= -1 && b[j] <= snum,
                         "impdar_continuity: trace %d has slice bounds %d, %d outside 0 ... %d", j, s[j], b[j], snum);
    return IMPDAR_OK;
}

extern "C" int impdar_continuity_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, const int *s,
                                     const int *b, int cut_mode, double cutoff_ratio, double *out)
{
    const auto lock = g_pk.lock();
    int rc = continuity_check(ctx, d_data, dtype, snum, tnum, s, b, cut_mode, cutoff_ratio, out);
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_pk.bind(ctx);
    const void *d_tab[2];
    rc = impdar_upload_tables(ctx, g_pk.tab, {{s, (size_t)tnum * sizeof(int)}, {b, (size_t)tnum * sizeof(int)}}, d_tab);
    if (rc) return rc;
    const size_t out_bytes = (size_t)tnum * sizeof(double);
    IMPDAR_HIP_CHECK(g_pk.out.ensure(out_bytes));
    rw_typed(dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(pk_continuity_kernel<T>, dim3((tnum + 63) / 64), dim3(64), 0, ctx->stream, (const T *)d_data, snum, tnum,
                           (const int *)d_tab[0], (const int *)d_tab[1], cut_mode, cutoff_ratio, g_pk.out.as<double>());
    });
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_download(ctx, out, g_pk.out.p, out_bytes, ctx->stream);
}

// ---- host-buffer forms: the argument check, the upload of the radargram, the resident form ----------------

extern "C" int impdar_auto_pick(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int nseeds, const int *seed_snum,
                                const int *seed_tnum, int plength, int FWW, int scst, int pol, double *out, int *status)
{
    int rc = auto_pick_check(ctx, data, dtype, snum, tnum, nseeds, seed_snum, seed_tnum, plength, FWW, scst, pol, out, status);
    if (rc) return rc;
    const auto lock = g_pk.lock();
    rc = g_pk.stage_in(ctx, g_pk.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype));
    if (rc) return rc;
    return impdar_auto_pick_dev(ctx, g_pk.data.p, dtype, snum, tnum, nseeds, seed_snum, seed_tnum, plength, FWW, scst, pol, out,
                                status);
}

extern "C" int impdar_pick_guided(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int t0, int n, const int *mid,
                                  int plength, int FWW, int scst, int pol, double *out, int *status)
{
    int rc = pick_guided_check(ctx, data, dtype, snum, tnum, t0, n, mid, plength, FWW, scst, pol, out, status);
    if (rc) return rc;
    const auto lock = g_pk.lock();
    rc = g_pk.stage_in(ctx, g_pk.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype));
    if (rc) return rc;
    return impdar_pick_guided_dev(ctx, g_pk.data.p, dtype, snum, tnum, t0, n, mid, plength, FWW, scst, pol, out, status);
}

extern "C" int impdar_continuity(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, const int *s, const int *b,
                                 int cut_mode, double cutoff_ratio, double *out)
{
    int rc = continuity_check(ctx, data, dtype, snum, tnum, s, b, cut_mode, cutoff_ratio, out);
    if (rc) return rc;
    const auto lock = g_pk.lock();
    rc = g_pk.stage_in(ctx, g_pk.data, data, (size_t)snum * tnum * impdar_dtype_size(dtype));
    if (rc) return rc;
    return impdar_continuity_dev(ctx, g_pk.data.p, dtype, snum, tnum, s, b, cut_mode, cutoff_ratio, out);
}
