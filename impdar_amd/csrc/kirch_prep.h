// Kirchhoff image prep: the time gradient (numpy.gradient semantics, mig_python.py:93) fused with the (snum, tnum) ->
// trace-major transpose, or into groups of 8 (4) traces that are sample-major inside (the ring kernels' image), and the
// host function that launches it.  Included by kirchhoff.hip alone.
#pragma once
#include "kirch_plan.h"

struct PrepParams {
    const void *data;       // (snum, ld) row-major, column block [0,nloc)
    int ld;
    int snum, nloc, jlo;    // image rows written: jlo .. jlo+nloc-1
    void *GT;               // (tnum_pad, snum)
    void *DT;               // same or null
    int grad_uniform;       // see impdar_hip.h
    int precomputed;        // data already holds the gradient (mig_kirch_loop)
    double grad_h;
    const double *ga, *gb, *gc;
    int clean;              // 1: map non-finite values to 0 (fp32 ring kernels); 2: NaN only (fp64 ring kernel)
    int i8;                 // image layout: 0 trace-major [row][k]; 1 groups of 8 rows (4 for float64: 32 bytes per
                            // sample either way), sample-major inside a group: element (row, k) at
                            // ((row / G) * snum + k) * G + (row % G)
};

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void kirch_prep_kernel(PrepParams P)
{
    // tiles in the image's element type: 2 x 18 KB for float32.  Row stride 65 for the trace-major
    // store (lanes walk a tile column), 72 for the grouped store (a half wave reads 4 rows x 8 columns)
    __shared__ TO tg[64 * 72];
    __shared__ TO td[64 * 72];
    const int ld = P.i8 ? 72 : 65;
    const TI *f = reinterpret_cast<const TI *>(P.data);
    const int k0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = P.snum;
    for (int r = ty; r < 64; r += 4) {
        const int k = k0 + r, j = j0 + tx;
        double g = 0.0, d = 0.0;
        if (k < n && j < P.nloc) {
            const size_t c = (size_t)j;
            d = (double)f[(size_t)k * P.ld + c];
            if (P.precomputed) {
                g = d;
            } else if (k == 0) {
                const double h = P.grad_uniform ? P.grad_h : P.ga[0];
                g = ((double)f[(size_t)1 * P.ld + c] - d) / h;
            } else if (k == n - 1) {
                const double h = P.grad_uniform ? P.grad_h : P.ga[n - 1];
                g = (d - (double)f[(size_t)(k - 1) * P.ld + c]) / h;
            } else {
                const double fm = (double)f[(size_t)(k - 1) * P.ld + c];
                const double fp = (double)f[(size_t)(k + 1) * P.ld + c];
                if (P.grad_uniform) {
                    g = (fp - fm) / (2.0 * P.grad_h);
                } else {
                    g = (P.ga[k] * fm + P.gb[k] * d) + P.gc[k] * fp;
                }
            }
            if (sizeof(TI) == 4 && !P.precomputed) g = (double)(float)g;  // numpy keeps f32 gradients in f32
            if (P.clean == 1) {
                if (!(fabs(g) <= 1.79e308)) g = 0.0;
                if (!(fabs(d) <= 1.79e308)) d = 0.0;
            }
        }
        tg[r * ld + tx] = (TO)g;
        td[r * ld + tx] = (TO)d;
    }
    __syncthreads();
    TO *GT = reinterpret_cast<TO *>(P.GT);
    TO *DT = reinterpret_cast<TO *>(P.DT);
    if (P.i8) {
        // a wave stores 8 samples x 8 rows = 256 contiguous bytes per instruction
        const int kk = tx >> 3, jj = tx & 7;
        for (int g8 = 2 * ty; g8 < 2 * ty + 2; ++g8)
            for (int kb = 0; kb < 8; ++kb) {
                const int r = kb * 8 + kk, c = g8 * 8 + jj;
                const int j = j0 + c, k = k0 + r;
                if (j < P.nloc && k < n) {
                    const int row = P.jlo + j;
                    const size_t o = ((size_t)(row >> 3) * n + k) * 8 + (row & 7);
                    GT[o] = tg[r * ld + c];
                    if (DT) DT[o] = td[r * ld + c];
                }
            }
        return;
    }
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, k = k0 + tx;
        if (j < P.nloc && k < n) {
            const size_t o = (size_t)(P.jlo + j) * n + k;
            GT[o] = tg[tx * ld + r];
            if (DT) DT[o] = td[tx * ld + r];
        }
    }
}

// LDS-free variant for the grouped layout, float32 (the quad kernel's image).
// The diffraction sum of the previous radargram keeps all of a CU's LDS, so a producer kernel that
// needs LDS cannot start before that kernel drains (and then takes LDS from the next one); this one
// runs on the CUs' spare wave slots underneath it: 8.58 -> 8.30 ms per step at config 3, and the
// difference between a working and a counter-productive overlap for the short kernels of an 8-rank run.
// One thread per (sample k, trace j): reads are coalesced along j, writes are 32-byte runs per group.
template <typename T, int GRP>
__global__ __launch_bounds__(256) void kirch_prep_direct_kernel(PrepParams P)
{
    const T *f = reinterpret_cast<const T *>(P.data);
    const int j = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    const int n = P.snum;
    if (j >= P.nloc) return;
    const size_t c = (size_t)j;
    double d = (double)f[(size_t)k * P.ld + c], g;
    if (P.precomputed) {
        g = d;
    } else if (k == 0) {
        const double h = P.grad_uniform ? P.grad_h : P.ga[0];
        g = ((double)f[(size_t)1 * P.ld + c] - d) / h;
    } else if (k == n - 1) {
        const double h = P.grad_uniform ? P.grad_h : P.ga[n - 1];
        g = (d - (double)f[(size_t)(k - 1) * P.ld + c]) / h;
    } else {
        const double fm = (double)f[(size_t)(k - 1) * P.ld + c];
        const double fp = (double)f[(size_t)(k + 1) * P.ld + c];
        if (P.grad_uniform)
            g = (fp - fm) / (2.0 * P.grad_h);
        else
            g = (P.ga[k] * fm + P.gb[k] * d) + P.gc[k] * fp;
    }
    if (sizeof(T) == 4 && !P.precomputed) g = (double)(float)g;                  // numpy keeps f32 gradients in f32
    if (P.clean == 1) {                                        // fp32 ring kernels: every non-finite value
        if (!(fabs(g) <= 1.79e308)) g = 0.0;
        if (!(fabs(d) <= 1.79e308)) d = 0.0;
    } else if (P.clean == 2) {                                 // fp64 ring kernel: NaN terms are what nansum skips
        if (g != g) g = 0.0;                                   // (mig_python.py:53); infinities stay and propagate
        if (d != d) d = 0.0;
    }
    const int row = P.jlo + j;
    const size_t o = ((size_t)(row / GRP) * n + k) * GRP + (row % GRP);
    reinterpret_cast<T *>(P.GT)[o] = (T)g;
    if (P.DT) reinterpret_cast<T *>(P.DT)[o] = (T)d;
}

// gradient + transpose of column block [jlo, jlo + nloc) into buffer set b
static int prep_image(impdar_kirch_plan *p, const void *d_data, int ld, int jlo, int nloc, int precomputed, int b, hipStream_t st)
{
    PrepParams P;
    P.data = d_data;
    P.ld = ld;
    P.snum = p->snum;
    P.nloc = nloc;
    P.jlo = jlo;
    P.GT = img_row0(p, p->GT[b]);
    P.DT = p->nearfield ? img_row0(p, p->DT[b]) : nullptr;
    P.grad_uniform = p->grad_uniform;
    P.precomputed = precomputed;
    P.grad_h = p->grad_h;
    P.ga = p->d_ga.as<double>();
    P.gb = p->d_gb.as<double>();
    P.gc = p->d_gc.as<double>();
    P.clean = (p->mode == IMPDAR_KIRCH_FAST) ? 1 : (p->dquad ? 2 : 0);
    P.i8 = (p->quad || p->dquad) ? 1 : 0;
    dim3 grid((nloc + 63) / 64, (p->snum + 63) / 64);
    if (p->dtype == IMPDAR_F32 && P.i8)
        hipLaunchKernelGGL((kirch_prep_direct_kernel<float, 8>), dim3((nloc + 255) / 256, p->snum), dim3(256), 0, st, P);
    else if (p->dquad)
        hipLaunchKernelGGL((kirch_prep_direct_kernel<double, 4>), dim3((nloc + 255) / 256, p->snum), dim3(256), 0, st, P);
    else if (p->dtype == IMPDAR_F32)
        hipLaunchKernelGGL((kirch_prep_kernel<float, float>), grid, dim3(256), 0, st, P);
    else
        hipLaunchKernelGGL((kirch_prep_kernel<double, double>), grid, dim3(256), 0, st, P);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}
