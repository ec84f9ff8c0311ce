// The recurrence of scipy.signal.filtfilt(b, a, x), shared by the vertical band pass (preproc.hip, along time) and
// the horizontal frequency filters (hpass.hip, along the traces): the coefficient block, the odd extension and
// the delay line of one signal spread over a group of lanes.  The memory side -- what a wavefront loads, where a
// step takes its sample from and where its output goes -- belongs to the kernels, because it is shaped by which
// axis is contiguous.  Every file that includes this is compiled with -ffp-contract=off.
#pragma once
#include "common.h"

// b, a normalised by a[0] and the steady-state initial conditions zi (lfilter_zi), zero past ncoef; a kernel argument
template <int MAXC> struct FiltCoefs {
    double b[MAXC];
    double a[MAXC];
    double zi[MAXC];
};

template <int MAXC>
static inline FiltCoefs<MAXC> filt_coefs(const double *b, const double *a, const double *zi, int ncoef)
{
    FiltCoefs<MAXC> c;
    memset(&c, 0, sizeof(c));
    for (int n = 0; n < ncoef; ++n) {   // SciPy normalises by a[0] once, up front
        c.b[n] = b[n] / a[0];
        c.a[n] = a[n] / a[0];
    }
    for (int n = 0; n < ncoef - 1; ++n) c.zi[n] = zi[n];
    return c;
}

// sample i of the odd extension (scipy.signal._arraytools.odd_ext) by `pad` samples of the n samples x[0],
// x[stride], ...: computed in the data's own arithmetic (2*x[0] - x[pad-i] is a float32 expression for float32
// data); i past the end is clamped (those outputs are never stored)
template <typename T>
__device__ __forceinline__ T filt_odd_ext(const T *__restrict__ x, int i, int n, int pad, size_t stride)
{
    const int L = n + 2 * pad;
    i = i < L ? i : L - 1;
    if (i < pad) return (T)((T)2 * x[0] - x[(size_t)(pad - i) * stride]);
    i -= pad;
    if (i < n) return x[(size_t)i * stride];
    i -= n;
    return (T)((T)2 * x[(size_t)(n - 1) * stride] - x[(size_t)(n - 2 - i) * stride]);
}

template <int CTRL> __device__ __forceinline__ double dpp_f64(double v)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// value of lane L (0..3) of the quad
template <int L> __device__ __forceinline__ float quad_pick(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), L * 0x55, 0xf, 0xf, true));
}
template <int L> __device__ __forceinline__ double quad_pick(double v) { return dpp_f64<L * 0x55>(v); }

// value of lane 0 of the signal's group of G lanes
template <int G> __device__ __forceinline__ double group_bcast0(double v)
{
    if constexpr (G == 4) {
        return dpp_f64<0x00>(v);   // quad_perm [0,0,0,0]
    } else {
        static_assert(G == 8, "4 or 8 lanes per signal");
        // quad broadcast, then banks 1 and 3 of each 16-lane row take it from four lanes down (row_shr:4)
        const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x00, 0xf, 0xf, true);
        const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x00, 0xf, 0xf, true);
        const int lo2 = __builtin_amdgcn_update_dpp(lo, lo, 0x114, 0xf, 0xa, false);
        const int hi2 = __builtin_amdgcn_update_dpp(hi, hi, 0x114, 0xf, 0xa, false);
        return __hiloint2double(hi2, lo2);
    }
}

// value of the next lane of the group (the last lane's result is discarded by the caller)
template <int G> __device__ __forceinline__ double group_next(double v)
{
    if constexpr (G == 4) return dpp_f64<0xF9>(v);   // quad_perm [1,2,3,3]
    else return dpp_f64<0x101>(v);                    // row_shl:1
}

// The recurrence of one signal is spread over the G lanes of a group: lane q keeps the K delays z[qK .. qK+K-1]
// (G * K >= ncoef - 1, padded with zero coefficients) and their coefficients in registers.  Every delay is
// updated by exactly SciPy's expression (_lfilter.c.in),
//   y = z[0] + b[0]*x;  z[n] = z[n+1] + x*b[n+1] - y*a[n+1];  z[last] = x*b[last] - y*a[last],
// from the old value of its neighbour, fetched across lanes with DPP moves before anything is updated.
template <int G, int K> struct FiltLane {
    double z[K], B[K], A[K];
    double b0;
    bool last;   // the last lane of the group: nothing follows its last delay
    template <int MAXC> __device__ __forceinline__ void init(const FiltCoefs<MAXC> &c, int q, int nc, double x0)
    {
        b0 = c.b[0];
        last = q == G - 1;
        // uniform indices only: a lane-indexed read of the kernel argument becomes a vector memory load, and the
        // wait bookkeeping of the compiler then drains every prefetch at the top of each chunk
#pragma unroll
        for (int k = 0; k < K; ++k) {
            B[k] = A[k] = z[k] = 0.0;
#pragma unroll
            for (int l = 0; l < G; ++l) {
                const int n = l * K + k;   // delay index; its coefficients are b[n+1], a[n+1]
                if (n + 1 < MAXC && q == l && n + 1 < nc) {
                    B[k] = c.b[n + 1];
                    A[k] = c.a[n + 1];
                    z[k] = c.zi[n] * x0;
                }
            }
        }
    }
    __device__ __forceinline__ double step(double xn)
    {
        const double y = group_bcast0<G>(z[0]) + b0 * xn;
        double zn = group_next<G>(z[0]);
        if (last) zn = 0.0;
#pragma unroll
        for (int k = 0; k < K - 1; ++k) z[k] = z[k + 1] + xn * B[k] - y * A[k];
        z[K - 1] = zn + xn * B[K - 1] - y * A[K - 1];
        return y;
    }
};
