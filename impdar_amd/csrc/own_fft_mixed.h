// Batched row transforms of any length M = 2^a 3^b 5^c 7^d, 16 <= M <= 8192, in LDS: own_fft.h's contract (the five modes, one
// workgroup per row, the OwnTwiddles table, taper weights on the R2C load, the caller's scale) at the lengths field records
// have -- 10000 traces are R2C / C2R rows of 5000 complex numbers.  own_fft.h includes this file at its end; its own_fft_launch
// sends the lengths that are no power of two here; the power-of-two kernel is untouched.
//
// The passes, their order and every index are own_fft_mixed_plan.h's (host-only, tested by itself); this file adds the
// butterflies.  Radix 4 is own_fft.h's butterfly (W^2j, W^3j by multiplication); radix 3, 5 and 7 pair point k with point
// r - k (sums take the cosines, differences the sines) and read each output's twiddle from the table.
#pragma once
#include "own_fft.h"            // OCp, own_pad, the radix-4 butterfly, OwnTwiddles
#include "own_fft_mixed_plan.h"

// cos and sin of 2 pi k / R for the odd radices, k = 1 .. (R - 1) / 2
__host__ __device__ constexpr double own_root_cos(int R, int k)
{
    return R == 3 ? -0.5
                  : R == 5 ? (k == 1 ? 0.30901699437494742410 : -0.80901699437494742410)
                           : (k == 1 ? 0.62348980185873353053 : (k == 2 ? -0.22252093395631440429 : -0.90096886790241912624));
}
__host__ __device__ constexpr double own_root_sin(int R, int k)
{
    return R == 3 ? 0.86602540378443864676
                  : R == 5 ? (k == 1 ? 0.95105651629515357212 : 0.58778525229247312917)
                           : (k == 1 ? 0.78183148246802980871 : (k == 2 ? 0.97492791218182360702 : 0.43388373911755812048));
}

// the length-R transform of a[0 .. R) in place, R odd:  X_m = a_0 + sum_k cos(2 pi m k / R) (a_k + a_{R-k}) -+ i sin(2 pi m k / R) (a_k - a_{R-k})
template <typename T, int R, bool INV> __device__ __forceinline__ void own_bfly_odd(OCp<T> (&a)[R])
{
    constexpr int H = (R - 1) / 2;
    OCp<T> s[H], d[H];
#pragma unroll
    for (int k = 1; k <= H; ++k) {
        s[k - 1] = own_add(a[k], a[R - k]);
        d[k - 1] = own_sub(a[k], a[R - k]);
    }
    const OCp<T> a0 = a[0];
#pragma unroll
    for (int k = 0; k < H; ++k) a[0] = own_add(a[0], s[k]);
#pragma unroll
    for (int m = 1; m <= H; ++m) {
        T cr = a0.x, ci = a0.y, sr = 0, si = 0;
#pragma unroll
        for (int k = 1; k <= H; ++k) {
            const int mk = (m * k) % R, kk = mk > H ? R - mk : mk;
            const T c = (T)own_root_cos(R, kk), sn = (T)(mk > H ? -own_root_sin(R, kk) : own_root_sin(R, kk));
            cr += c * s[k - 1].x;
            ci += c * s[k - 1].y;
            sr += sn * d[k - 1].x;
            si += sn * d[k - 1].y;
        }
        // forward: (cr, ci) - i (sr, si) for X_m, + i (sr, si) for X_{R-m}; the inverse the other way round
        const OCp<T> lo = OCp<T>{cr + si, ci - sr}, hi = OCp<T>{cr - si, ci + sr};
        a[m] = INV ? hi : lo;
        a[R - m] = INV ? lo : hi;
    }
}

// pass p of the plan, radix R, on the row at s[own_pad(i)]; every thread of the workgroup calls it (barrier inside)
template <typename T, int R, bool INV>
__device__ __forceinline__ void own_mixed_pass(OCp<T> *s, const OwnMixedPlan &pl, int p, int tid, int nth, const OCp<T> *__restrict__ tw, int TWS)
{
    const int q = pl.q[p], nb = own_mixed_count(pl, p);
    for (int b = tid; b < nb; b += nth) {
        const int g = own_mixed_group(pl, p, b), j = own_mixed_offset(pl, p, b, g), base = own_mixed_base(pl, p, b, g);
        OCp<T> a[R];
#pragma unroll
        for (int c = 0; c < R; ++c) a[c] = s[own_pad(base + c * q)];
        if constexpr (R == 4) {
            own_bfly4<T, INV>(a[0], a[1], a[2], a[3], tw[own_mixed_twiddle(pl, p, j, 1, TWS)]);
        } else {
            if constexpr (R == 2) {
                const OCp<T> t = own_sub(a[0], a[1]);
                a[0] = own_add(a[0], a[1]);
                a[1] = t;
            } else {
                own_bfly_odd<T, R, INV>(a);
            }
#pragma unroll
            for (int c = 1; c < R; ++c) {
                const OCp<T> w = tw[own_mixed_twiddle(pl, p, j, c, TWS)];
                a[c] = own_mul(a[c], INV ? own_conj(w) : w);
            }
        }
#pragma unroll
        for (int c = 0; c < R; ++c) s[own_pad(base + c * q)] = a[c];
    }
    __syncthreads();
}

// own_fft_rows' contract (own_fft.h) with M = pl.M any length the plan takes: in / out / tw / wcol / wrow / wfirst as there
template <typename T, int MODE>
__global__ __launch_bounds__(1024) void own_fft_rows_mixed(const void *__restrict__ in_, void *__restrict__ out_, const OwnMixedPlan pl, size_t in_dist,
                                                          size_t out_dist, T scale, const OCp<T> *__restrict__ tw, const double *__restrict__ wcol,
                                                          const double *__restrict__ wrow, int wfirst)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char own_lds[];
    OCp<T> *s = reinterpret_cast<OCp<T> *>(own_lds);
    const int tid = threadIdx.x, nth = blockDim.x, M = pl.M;
    const size_t row = blockIdx.x;
    constexpr bool INV = MODE == OWN_C2C_INV || MODE == OWN_C2R || MODE == OWN_C2C_INV_RE;
    constexpr int TWS = (MODE == OWN_R2C || MODE == OWN_C2R) ? 2 : 1;           // stride of the length-M twiddles in the table
    // ---- load (as own_fft_rows)
    if (MODE == OWN_C2R) {
        const OCp<T> *X = reinterpret_cast<const OCp<T> *>(in_) + row * in_dist;
        for (int k = tid; k < M; k += nth) {
            const OCp<T> a = X[k], b = own_conj(X[M - k]);
            const OCp<T> e = own_add(a, b), d = own_sub(a, b);
            const OCp<T> o = own_mul(own_conj(tw[k]), d);
            s[own_pad(k)] = OCp<T>{e.x - o.y, e.y + o.x};      // e + i o
        }
    } else {
        const OCp<T> *X = MODE == OWN_R2C ? reinterpret_cast<const OCp<T> *>(reinterpret_cast<const T *>(in_) + row * in_dist)
                                          : reinterpret_cast<const OCp<T> *>(in_) + row * in_dist;
        if (MODE == OWN_R2C && wcol) {
            const double wr = wrow[row];
            for (int i = tid; i < M; i += nth) {
                const OCp<T> v = X[i];
                s[own_pad(i)] = wfirst ? OCp<T>{(T)(((double)v.x * wcol[2 * i]) * wr), (T)(((double)v.y * wcol[2 * i + 1]) * wr)}
                                       : OCp<T>{(T)((double)v.x * (wcol[2 * i] * wr)), (T)((double)v.y * (wcol[2 * i + 1] * wr))};
            }
        } else {
            for (int i = tid; i < M; i += nth) s[own_pad(i)] = X[i];
        }
    }
    __syncthreads();
    for (int p = 0; p < pl.np; ++p) {
        switch (pl.radix[p]) {
        case 4: own_mixed_pass<T, 4, INV>(s, pl, p, tid, nth, tw, TWS); break;
        case 2: own_mixed_pass<T, 2, INV>(s, pl, p, tid, nth, tw, TWS); break;
        case 3: own_mixed_pass<T, 3, INV>(s, pl, p, tid, nth, tw, TWS); break;
        case 5: own_mixed_pass<T, 5, INV>(s, pl, p, tid, nth, tw, TWS); break;
        default: own_mixed_pass<T, 7, INV>(s, pl, p, tid, nth, tw, TWS); break;
        }
    }
    // ---- store (the digit reversal is undone here)
    if (MODE == OWN_R2C) {
        OCp<T> *Y = reinterpret_cast<OCp<T> *>(out_) + row * out_dist;
        // X[k] = (Z[k] + conj Z[M-k]) / 2 - i w_k (Z[k] - conj Z[M-k]) / 2,  k = 0 .. M  (Z[M] = Z[0]; indices modulo M)
        for (int k = tid; k <= M; k += nth) {
            const int kz = k == M ? 0 : k, km = k == 0 ? 0 : M - k;
            const OCp<T> zk = s[own_pad(own_mixed_pos(pl, kz))], zm = own_conj(s[own_pad(own_mixed_pos(pl, km))]);
            const OCp<T> e = own_add(zk, zm), d = own_sub(zk, zm);
            const OCp<T> o = own_mul(tw[kz], d);                       // w_M = -1, below
            const T sg = k == M ? (T)-1 : (T)1;
            Y[k] = OCp<T>{(T)0.5 * (e.x + sg * o.y) * scale, (T)0.5 * (e.y - sg * o.x) * scale};
        }
    } else if (MODE == OWN_C2R) {
        OCp<T> *Y = reinterpret_cast<OCp<T> *>(reinterpret_cast<T *>(out_) + row * out_dist);
        for (int n = tid; n < M; n += nth) {
            const OCp<T> z = s[own_pad(own_mixed_pos(pl, n))];
            Y[n] = OCp<T>{z.x * scale, z.y * scale};
        }
    } else if (MODE == OWN_C2C_INV_RE) {
        T *Y = reinterpret_cast<T *>(out_) + row * out_dist;
        for (int k = tid; k < M; k += nth) Y[k] = s[own_pad(own_mixed_pos(pl, k))].x * scale;
    } else {
        OCp<T> *Y = reinterpret_cast<OCp<T> *>(out_) + row * out_dist;
        for (int k = tid; k < M; k += nth) {
            const OCp<T> z = s[own_pad(own_mixed_pos(pl, k))];
            Y[k] = OCp<T>{z.x * scale, z.y * scale};
        }
    }
}

// n, dists, scale, tw and the weights as own_fft_launch's; the complex length (n, or n / 2 of the real modes) must pass
// own_fft_mixed_len_ok
template <typename T>
static int own_fft_mixed_launch(int mode, int n, size_t batch, const void *in, void *out, size_t in_dist, size_t out_dist, double scale,
                                const OwnTwiddles &tw, hipStream_t st, const double *wcol, const double *wrow, int wfirst)
{
    const bool real = mode == OWN_R2C || mode == OWN_C2R;
    OwnMixedPlan pl;
    if ((real && n % 2) || !own_mixed_plan_make(real ? n / 2 : n, pl) || tw.nt != n || tw.dbl != (sizeof(T) == 8)) {
        impdar_set_error("own_fft_mixed_launch: unsupported length %d (mode %d)", n, mode);
        return IMPDAR_ERR_UNSUPPORTED;
    }
    const int M = pl.M;
    const size_t lds = (size_t)(own_pad(M) + 1) * sizeof(OCp<T>);
    // (as the power-of-two kernel: a butterfly waits for its twiddles from global memory, so long rows want many threads)
    const int threads = M >= 4096 ? 1024 : (M >= 2048 ? 512 : (M >= 1024 ? 256 : 64));
    const OCp<T> *t = tw.buf.as<OCp<T>>();
#define OWN_MIXED_LAUNCH(MODE)                                                                                                    \
    do {                                                                                                                          \
        auto k = own_fft_rows_mixed<T, MODE>;                                                                                     \
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));             \
        hipLaunchKernelGGL(k, dim3((unsigned)batch), dim3(threads), lds, st, in, out, pl, in_dist, out_dist, (T)scale, t, wcol, wrow, wfirst); \
    } while (0)
    switch (mode) {
    case OWN_C2C_FWD: OWN_MIXED_LAUNCH(OWN_C2C_FWD); break;
    case OWN_C2C_INV: OWN_MIXED_LAUNCH(OWN_C2C_INV); break;
    case OWN_R2C: OWN_MIXED_LAUNCH(OWN_R2C); break;
    case OWN_C2C_INV_RE: OWN_MIXED_LAUNCH(OWN_C2C_INV_RE); break;
    default: OWN_MIXED_LAUNCH(OWN_C2R); break;
    }
#undef OWN_MIXED_LAUNCH
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}
