// The growing-window search of the empirical attenuation methods 3 and 6b (the reference's analysis/attenuation.py:
// attenuation_method3, attenuation_method6b; Hills et al. 2020 after Schroeder et al. 2016).  One centre -- a trace of
// method 3, a depth of method 6b -- walks nested windows; at each window W every candidate rate N = ns[j] gets
//   pa = pc + 2 z N,   C[j] = | sum (z - mean z)(pa - mean pa) / ( sqrt(sum (z - mean z)^2) sqrt(sum (pa - mean pa)^2) ) |
// and the reference's decision follows: Cm = min C; if Cm < Cw and C[ns == 0] > Cw, Nh = max ns[C < Cw] - min ns[C < Cw]
// (halved in the depth form); stop when Nh <= Nh_target or the next window leaves the record; report the rate at the
// minimum of the last window visited and the width after the last increment.
//
// The windows (att_route.h has the launch):
//   ATT_INDEX  [tr - win/2, tr + win/2) of the NaN-free pick, integers, while win/2 <= tr and win/2 <= n - tr; win += win_step
//   ATT_DEPTH  the contiguous range of the depth-sorted pairs with |z - d| < win/2 in float64 (found by bisection on the two
//              monotone halves of that predicate), while d - win/2 >= z[0] and d + win/2 <= z[n - 1]; win += win_step by
//              repeated float64 addition
//
// The arithmetic is the reference's passes, not the five window sums: at the minimum of C the variance of pa is what is left
// of sum pc^2 after a cancellation of two to three digits, and C at its neighbours -- where the decision against Cw falls --
// would carry that loss.  Per window: the means from sums around the window's middle sample (their error enters the centred
// sums in second order), then for every rate one pass over (dz, dp) = (z - mean z, pc - mean pc), staged through LDS in
// tiles, with dpa = fma(2N, dz, dp), s1 = fma(dz, dpa, s1), s3 = fma(dpa, dpa, s3).  A thread owns one rate and one of
// `parts` interleaved parts of the window; the parts are added in their order, the lanes of a wave by a butterfly, the waves
// in their order: the order of every sum is a function of the window alone, no atomics, and two calls give the same bits.
#include "common.h"
#include "att_route.h"

struct AttArgs {
    const double *z, *pc;                 // [n]
    const double *ns;                     // [nn]
    const double *centres;                // [ncent], depth form
    double *ctab;                         // [ncent][nn]: C of the window in hand
    long long *idx;                       // [ncent]
    double *win;                          // [ncent]
    int *code;                            // [ncent]
    double *probe_c;                      // [probe_cap][nn]
    long long *probe_rows;                // [1]
    long long n, nn, j0, first, probe, probe_cap;
    long long iwin_init, iwin_step;
    double win_init, win_step, cw, nh_target;
    int parts, chunk;
};

struct AttAdd { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct AttMin {
    __device__ double operator()(double a, double b) const { return fmin(a, b); }
    __device__ long long operator()(long long a, long long b) const { return a < b ? a : b; }
};
struct AttMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// v combined over the workgroup, the result in every thread: a butterfly over each wave, then the waves in their order
template <class T, class Op> __device__ __forceinline__ T att_block_all(T v, Op op, T *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off));
    __syncthreads();                    // (the partials of the reduction before have been read)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = lds[0];
    for (int w = 1; w < ATT_WAVES; ++w) r = op(r, lds[w]);
    return r;
}

template <int DEPTH> __global__ __launch_bounds__(ATT_THREADS) void att_search_kernel(const AttArgs A)
{
    __shared__ double2 tile[ATT_TILE];
    __shared__ double p1[ATT_THREADS], p3[ATT_THREADS];
    __shared__ double red[ATT_WAVES];
    __shared__ long long redl[ATT_WAVES];
    const int tid = threadIdx.x;
    const long long c = blockIdx.x, n = A.n, nn = A.nn;
    double *crow = A.ctab + c * nn;
    const bool probe = c == A.probe;
    const int q = tid / A.chunk, jl = tid % A.chunk;      // this thread's part of a window and its rate within a chunk
    const long long tr = A.first + c;
    const double d = DEPTH ? A.centres[c] : 0.0;
    const double zmin = A.z[0], zmax = A.z[n - 1];
    const double inf = __builtin_inf();
    long long iw = A.iwin_init, rows = 0, best = -1;
    double w = A.win_init, nh = A.nh_target + 1.0;
    int code = ATT_NOT_ENTERED;
    for (;;) {
        long long lo, cnt;
        if (DEPTH) {
            const double h = w / 2;
            if (!(nh > A.nh_target && d - h >= zmin && d + h <= zmax)) break;
            // z - d rises with z: the first pair above -h, the first at or above h
            long long a = 0, b = n;
            while (a < b) {
                const long long mid = a + ((b - a) >> 1);
                if (A.z[mid] - d > -h) b = mid;
                else a = mid + 1;
            }
            lo = a;
            b = n;
            while (a < b) {
                const long long mid = a + ((b - a) >> 1);
                if (A.z[mid] - d >= h) b = mid;
                else a = mid + 1;
            }
            cnt = a - lo;
        } else {
            const long long h = iw / 2;
            if (!(nh > A.nh_target && h <= tr && h <= n - tr)) break;
            lo = tr - h;
            cnt = 2 * h;
        }
        if (cnt == 0) {                  // an empty depth window: means of nothing, every C NaN
            code = ATT_NONFINITE;
            break;
        }
        // the means, from sums around the middle sample
        const double z0 = A.z[lo + cnt / 2], p0 = A.pc[lo + cnt / 2];
        double sz = 0.0, sp = 0.0;
        for (long long i = tid; i < cnt; i += ATT_THREADS) {
            sz += A.z[lo + i] - z0;
            sp += A.pc[lo + i] - p0;
        }
        sz = att_block_all(sz, AttAdd(), red);
        sp = att_block_all(sp, AttAdd(), red);
        const double zm = z0 + sz / (double)cnt, pm = p0 + sp / (double)cnt;
        double szz = 0.0;
        for (long long jb = 0; jb < nn; jb += A.chunk) {
            const long long j = jb + jl;
            const bool live = q < A.parts && j < nn;
            const double cn = live ? 2.0 * A.ns[j] : 0.0;
            double s1 = 0.0, s3 = 0.0;
            for (long long base = 0; base < cnt; base += ATT_TILE) {
                const int m = (int)(cnt - base < (long long)ATT_TILE ? cnt - base : (long long)ATT_TILE);
                __syncthreads();        // (the tile before has been read)
                for (int i = tid; i < m; i += ATT_THREADS) {
                    const double dz = A.z[lo + base + i] - zm, dp = A.pc[lo + base + i] - pm;
                    tile[i] = make_double2(dz, dp);
                    if (jb == 0) szz = fma(dz, dz, szz);
                }
                __syncthreads();
                if (live) {
                    for (int i = q; i < m; i += A.parts) {
                        const double2 e = tile[i];
                        const double dpa = fma(cn, e.x, e.y);
                        s1 = fma(e.x, dpa, s1);
                        s3 = fma(dpa, dpa, s3);
                    }
                }
            }
            if (jb == 0) szz = att_block_all(szz, AttAdd(), red);       // (every thread now holds the total)
            p1[tid] = s1;
            p3[tid] = s3;
            __syncthreads();
            if (tid < A.chunk && jb + tid < nn) {
                double t1 = p1[tid], t3 = p3[tid];
                for (int k = 1; k < A.parts; ++k) {
                    t1 += p1[k * A.chunk + tid];
                    t3 += p3[k * A.chunk + tid];
                }
                const double C = fabs(t1 / (sqrt(szz) * sqrt(t3)));
                crow[jb + tid] = C;
                if (probe && rows < A.probe_cap) A.probe_c[rows * nn + jb + tid] = C;
            }
        }
        __syncthreads();                // the row is written
        ++rows;
        // the decision
        double cm = inf, nlo = inf, nhi = -inf;
        long long bad = 0;
        for (long long j = tid; j < nn; j += ATT_THREADS) {
            const double C = crow[j];
            if (!(C <= 1.7976931348623157e308)) bad = 1;     // NaN or Inf: NumPy's comparisons decide, on the host
            cm = fmin(cm, C);
            if (C < A.cw) {
                nlo = fmin(nlo, A.ns[j]);
                nhi = fmax(nhi, A.ns[j]);
            }
        }
        bad = att_block_all(bad, AttAdd(), redl);
        if (bad) {
            code = ATT_NONFINITE;
            break;
        }
        cm = att_block_all(cm, AttMin(), red);
        nlo = att_block_all(nlo, AttMin(), red);
        nhi = att_block_all(nhi, AttMax(), red);
        long long ties = 0, jm = 0x7fffffffffffffffLL;
        for (long long j = tid; j < nn; j += ATT_THREADS) {
            if (crow[j] == cm) {
                ++ties;
                jm = j < jm ? j : jm;
            }
        }
        ties = att_block_all(ties, AttAdd(), redl);
        best = att_block_all(jm, AttMin(), redl);
        code = ties == 1 ? ATT_VALUE : ATT_TIE;
        if (cm < A.cw && crow[A.j0] > A.cw) nh = DEPTH ? (nhi - nlo) / 2. : nhi - nlo;
        if (DEPTH) w += A.win_step;
        else iw += A.iwin_step;
        __syncthreads();                // (the row has been read before the next window writes it)
    }
    if (tid == 0) {
        A.idx[c] = best;
        A.win[c] = DEPTH ? w : (double)iw;
        A.code[c] = code;
        if (probe) A.probe_rows[0] = rows;
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct AttBufs {
    DevBuf in, out;
    void release()
    {
        in.release();
        out.release();
    }
};
static StepScratch<AttBufs> g_att;

void impdar_attsearch_forget(impdar_ctx *ctx) { g_att.forget(ctx); }

extern "C" int impdar_att_search_plan(int flavour, long long n, long long nn, long long ncent, double win_init, double win_step,
                                      long long probe, long long probe_cap, long long *scratch_bytes)
{
    const AttRoute R = att_route(flavour, n, nn, ncent, win_init, win_step, probe, probe_cap);
    IMPDAR_ARG_CHECK(R.ok, "impdar_att_search: %s (n %lld, rates %lld, centres %lld)", R.why, n, nn, ncent);
    if (scratch_bytes) *scratch_bytes = R.scratch_bytes;
    return IMPDAR_OK;
}

extern "C" int impdar_att_search(impdar_ctx *ctx, int flavour, const double *z, const double *pc, long long n, const double *ns,
                                 long long nn, long long j0, const double *centres, long long first, long long ncent, double win_init,
                                 double win_step, double cw, double nh_target, long long *idx, double *win, int *code,
                                 long long probe, double *probe_c, long long probe_cap, long long *probe_rows)
{
    IMPDAR_ARG_CHECK(ctx && z && pc && ns && idx && win && code, "impdar_att_search: null argument");
    const AttRoute R = att_route(flavour, n, nn, ncent, win_init, win_step, probe, probe_cap);
    IMPDAR_ARG_CHECK(R.ok, "impdar_att_search: %s (n %lld, rates %lld, centres %lld)", R.why, n, nn, ncent);
    IMPDAR_ARG_CHECK(att_call_ok(R, j0, first), "impdar_att_search: rate index %lld of %lld, first trace %lld", j0, nn, first);
    IMPDAR_ARG_CHECK(flavour == ATT_INDEX || centres, "impdar_att_search: the depth form needs its centres");
    IMPDAR_ARG_CHECK(probe < 0 || (probe_c && probe_rows), "impdar_att_search: a probe needs its table and its row count");
    if (flavour == ATT_DEPTH) {
        const long long bad = att_depths_bad(z, n);
        IMPDAR_ARG_CHECK(!bad, "impdar_att_search: z[%lld] is NaN or below the depth before it", bad - 1);
        const char *endless = att_depth_walk_bad(z[0], z[n - 1], win_step);
        IMPDAR_ARG_CHECK(!endless, "impdar_att_search: %s (z from %g to %g, win_step %g)", endless, z[0], z[n - 1], win_step);
    }

    const auto held = g_att.lock();
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    g_att.bind(ctx);
    const size_t zb = (size_t)n * sizeof(double), nb = (size_t)nn * sizeof(double), cb = (size_t)ncent * sizeof(double);
    const double none = 0.0;
    const void *dev[4];
    int rc = impdar_upload_tables(ctx, g_att.in, {{z, zb}, {pc, zb}, {ns, nb}, {centres ? (const void *)centres : &none, centres ? cb : sizeof(double)}}, dev);
    if (rc) return rc;
    // idx, win, code, the probe's row count and table come back; the C rows of the windows in hand stay
    const size_t pb = (size_t)R.probe_cap * nb;
    const size_t off_win = impdar_round16(cb), off_code = off_win + impdar_round16(cb);
    const size_t off_rows = off_code + impdar_round16((size_t)ncent * sizeof(int)), off_pc = off_rows + 16;
    const size_t back = off_pc + impdar_round16(pb), out_bytes = back + impdar_round16((size_t)ncent * nb);
    IMPDAR_HIP_CHECK(g_att.out.ensure(out_bytes));
    char *o = g_att.out.as<char>();
    AttArgs A;
    A.z = (const double *)dev[0];
    A.pc = (const double *)dev[1];
    A.ns = (const double *)dev[2];
    A.centres = (const double *)dev[3];
    A.idx = reinterpret_cast<long long *>(o);
    A.win = reinterpret_cast<double *>(o + off_win);
    A.code = reinterpret_cast<int *>(o + off_code);
    A.probe_rows = reinterpret_cast<long long *>(o + off_rows);
    A.probe_c = reinterpret_cast<double *>(o + off_pc);
    A.ctab = reinterpret_cast<double *>(o + back);
    A.n = n;
    A.nn = nn;
    A.j0 = j0;
    A.first = flavour == ATT_INDEX ? first : 0;
    A.probe = probe < 0 ? -1 : probe;
    A.probe_cap = R.probe_cap;
    A.iwin_init = flavour == ATT_INDEX ? (long long)win_init : 0;
    A.iwin_step = flavour == ATT_INDEX ? (long long)win_step : 0;
    A.win_init = win_init;
    A.win_step = win_step;
    A.cw = cw;
    A.nh_target = nh_target;
    A.parts = R.parts;
    A.chunk = R.chunk;
    impdar_ctx_note(ctx, "impdar_att_search", "att_search_kernel");
    rc = impdar_ctx_ktic(ctx);          // the search kernel alone: impdar_ctx_last_kernel_ms
    if (rc) return rc;
    if (flavour == ATT_DEPTH) hipLaunchKernelGGL(att_search_kernel<1>, dim3((unsigned)R.workgroups), dim3(R.threads), 0, ctx->stream, A);
    else hipLaunchKernelGGL(att_search_kernel<0>, dim3((unsigned)R.workgroups), dim3(R.threads), 0, ctx->stream, A);
    IMPDAR_HIP_CHECK(hipGetLastError());
    rc = impdar_ctx_ktoc(ctx);
    if (rc) return rc;
    const size_t take = probe < 0 ? off_rows : back;
    std::vector<char> host(take);
    IMPDAR_HIP_CHECK(hipMemcpyAsync(host.data(), o, take, hipMemcpyDeviceToHost, ctx->stream));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    memcpy(idx, host.data(), cb);
    memcpy(win, host.data() + off_win, cb);
    memcpy(code, host.data() + off_code, (size_t)ncent * sizeof(int));
    if (probe >= 0) {
        long long rows;
        memcpy(&rows, host.data() + off_rows, sizeof(rows));
        *probe_rows = rows;
        const size_t got = (size_t)(rows < R.probe_cap ? rows : R.probe_cap) * nb;
        memcpy(probe_c, host.data() + off_pc, got);
    }
    return IMPDAR_OK;
}
