// The frame of the steps that rewrite a resident (snum, tnum) radargram in place, element by element, with values
// that depend on the row (a gain, a taper) or on the trace (a start row): rangegain and agc of gain.hip, the apply
// pass of winavg_hfilt in hfilt.hip.  They do nothing a copy does not do: one read and one write of the array.
#pragma once
#include "vecwidth.h"

#define RW_ROWS 4            // consecutive rows per thread and trip: that many 16-byte loads in flight
#define RW_MAX_BLOCKS 2048   // resident workgroups (8 per CU); the rows beyond are reached by a grid stride

// A thread owns V consecutive traces (one 16-byte access for float32 x 4 and float64 x 2) and walks the rows
// RW_ROWS at a time.  `f(i, j, y)` rewrites the V values y of row i, traces j .. j + V - 1.  V is chosen by the host
// so that tnum % V == 0: every row then starts on a multiple of the access width and no trace is left over; V = 1
// serves every other trace count.
template <typename T, int V, class F>
__global__ __launch_bounds__(256) void rowwise_kernel(T *__restrict__ x, int snum, int tnum, F f)
{
    typedef RwVec<T, V> Vec;
    const int j = (blockIdx.x * 256 + threadIdx.x) * V;
    if (j >= tnum) return;
    for (int i0 = blockIdx.y * RW_ROWS; i0 < snum; i0 += gridDim.y * RW_ROWS) {
        Vec y[RW_ROWS];
#pragma unroll
        for (int u = 0; u < RW_ROWS; ++u) {
            const int i = i0 + u < snum ? i0 + u : snum - 1;
            y[u] = *reinterpret_cast<const Vec *>(x + (size_t)i * tnum + j);
        }
#pragma unroll
        for (int u = 0; u < RW_ROWS; ++u) {
            if (i0 + u < snum) {
                f(i0 + u, j, y[u].v);
                *reinterpret_cast<Vec *>(x + (size_t)(i0 + u) * tnum + j) = y[u];
            }
        }
    }
}

template <typename T, int V, class F>
static void rowwise_launch_v(impdar_ctx *ctx, T *d_data, int snum, int tnum, const F &f)
{
    const int gx = ((tnum + V - 1) / V + 255) / 256;
    const int groups = (snum + RW_ROWS - 1) / RW_ROWS;
    const int cap = RW_MAX_BLOCKS / gx > 1 ? RW_MAX_BLOCKS / gx : 1;
    const dim3 grid(gx, groups < cap ? groups : cap);
    hipLaunchKernelGGL((rowwise_kernel<T, V, F>), grid, dim3(256), 0, ctx->stream, d_data, snum, tnum, f);
}

// `make(RwType<T>())` gives the functor for the dtype; the access width is rw_dispatch's
template <class Make> static void rowwise_launch(impdar_ctx *ctx, void *d_data, int dtype, int snum, int tnum, const Make &make)
{
    rw_dispatch(dtype, {d_data}, tnum, [&](auto t, auto v) {
        typedef typename decltype(t)::type T;
        rowwise_launch_v<T, decltype(v)::value>(ctx, (T *)d_data, snum, tnum, make(t));
    });
}
