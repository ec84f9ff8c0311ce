// What every frequency-sum kernel of the phase shift shares (ps_direct.h, ps_mfma.h, ps_smooth.h, ps_nufft.h, ps_series.h,
// ps_runs.h): the sincos, the anchor interval, PsParams, the slot loads of the two walks and the wave-level reduce-scatter.
#pragma once
#include "ps_layout.h"      // Cp

template <typename T> __device__ inline void sincos_t(T x, T *s, T *c);
// |x| <= pi here (x = w dt sqrt(coss), |w dt| <= pi): Cody-Waite reduction by
// pi/2 and the classic degree-7/8 minimax polynomials; ~1e-7 absolute error,
// about 20 VALU instructions, no slow path.
template <> __device__ inline void sincos_t<float>(float x, float *s, float *c)
{
    const float q = rintf(x * 0.636619772f);
    float r = fmaf(q, -1.5707963705062866f, x);
    r = fmaf(q, 4.37113900018624283e-8f, r);
    const float r2 = r * r;
    const float sp = fmaf(r * r2, fmaf(r2, fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), r);
    const float cp = fmaf(r2 * r2, fmaf(r2, fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f),
                                        4.166664568298827e-2f), fmaf(r2, -0.5f, 1.0f));
    const int qi = (int)q;
    const float ss = (qi & 1) ? cp : sp;
    const float cc = (qi & 1) ? sp : cp;
    *s = (qi & 2) ? -ss : ss;
    *c = ((qi + 1) & 2) ? -cc : cc;
}
template <> __device__ inline void sincos_t<double>(double x, double *s, double *c) { sincos(x, s, c); }

// float32 recurrences are re-anchored to the original spectrum and the fp64 phase every PS_ANCHOR depth steps.
// Measured at config 5 (8192^2, same box): 64 -> 65.8 / 84.0 ms (const / v(z)) with a spot-wavenumber error of
// 0.8e-6 / 2.1e-6 against the fp64 oracle; 128 -> 63.0 / 80.5 ms, 1.6e-6 / 4.2e-6; 256 -> 62.0 / 78.9 ms,
// 3.1e-6 / 8.2e-6 (the drift is systematic: it doubles with the interval).  128 keeps the error at the scale of
// the fp32 FFTs around the kernel, 50x inside the stated 2e-4.
#ifndef IMPDAR_PS_ANCHOR
#define IMPDAR_PS_ANCHOR 128
#endif
constexpr int PS_ANCHOR = IMPDAR_PS_ANCHOR;

#define PS_STAMP(point)

struct PsParams {
    const void *F;          // [tnum][nt] complex
    void *TK;               // [tnum][snum] complex
    const double *kx;       // [tnum]
    const double *w;        // [nt]   (zero frequency already replaced by 1e-10/dt)
    const double *vz;       // [snum] (v(z) mode)
    const double *thr;      // [snum] (v(z) mode): (tau/tt[-1]/1e6)^2
    double vconst, dt;
    double vtol;            // float32 v(z): relative velocity change below which the phase increments are reused
    const int *sched;       // float32 v(z), ps_vz32_kernel: [snum] 1 where a new constant-velocity run starts
    const int *tsched;      // ... [ceil(ntile/32)] bit t of word t/32 set where 16-step tile t holds such a step
    const int *rowmap;      // ... [tnum] wavenumber of workgroup b (rows holding boundary frequencies first), or null
    const double *sm_step, *sm_tile;   // float32, ps_smooth32_kernel: the tables of ps_smooth_tables
    void *sm_part;          // ps_smooth kernels: [sm_nchunks][nk][snum] complex partial images (more than one chunk)
    int sm_nchunks;
    int sm_m;               // ... and the frequencies per lane of a wave (chunks of 64 sm_m)
    const double *eps;      // float64 v(z), ps_vz64_kernel: [ceil(snum/16)] sum over the tile's steps of v / v_run - 1
    int snum, tnum, nt, vz_mode;
    // Frequency slots a workgroup walks.  Full walk: nf = nt, slot i = row i of F.  Hermitian walk (herm = 1, real
    // radargram): nf = nt/2; slot 0 = the Nyquist row nt/2 (weight 1), slots 1..nt/2-1 = rows 1..nt/2-1 with weight 2
    // (each stands for itself and for its mirror image (-w, -k)); the zero-frequency row is added by ps_dc_kernel.
    // P.w is indexed by SLOT (the host uploads it in slot order).
    int nf, herm;
    int fstride;            // complex elements between the rows of F (nt; nt/2 + 1 when the time transform is real-to-complex)
    int nk;                 // wavenumbers in this launch (tnum, or a rank's slab)
    int k0;                 // first wavenumber of this launch (a rank's slab of a kx-sharded run; 0 otherwise): workgroup b
                            // works on wavenumber k0 + b and writes row b of TK
    int fhalf;              // 1: F is [tnum/2 + 1][nt] -- the wavenumbers k >= 0 with ALL frequencies (rows fstride = nt apart, the
                            // transform over the traces taken first, on the radargram's own rows): FK[tnum - k][w] = conj FK[k][-w].
                            // ps_nufft_kernel's pairs read both of their rows out of one; ps_edge_kernel, ps_dc_kernel know it;
                            // no other kernel is launched on it (ps_run)
};

// Why half of the frequencies are enough for a real radargram (mig_python.py:268-270, 282, 396-420, 438-487):
// FK = fft2(real data) is Hermitian, FK[-w,-k] = conj FK[w,k]; the phase w dt sqrt(1 - (v kx / 2w)^2) is odd in w
// and even in kx, the propagating / evanescent masks are even in both; so the negative-frequency half of
// TK[tau,k] = sum_w alive FK e^{i Phi} equals conj(TK+[tau,-k]) of the positive half TK+, whose inverse transform
// over k is the complex conjugate of ifft_k(TK+).  Only ifft_k(TK).real is kept (:282), hence
//   image = Re ifft_k( 2 TK+  +  TK[w = 0]  +  TK[w = Nyquist] ).
// The w = 0 row (replaced by 1e-10/dt, :400-402) propagates only where kx = 0, with coss = 1: ps_dc_kernel adds
// FK[0,k0] e^{i (tau+1) 1e-10} there.  The host takes this walk only when the axes are exactly antisymmetric
// (kx[-k] = -kx[k], ws[-i] = -ws[i], ws[0] = 0) and the replaced zero frequency is evanescent for every kx != 0.
template <typename T> __device__ __forceinline__ Cp<T> ps_load_slot(const Cp<T> *__restrict__ Frow, const PsParams &P, int slot)
{
    if (!P.herm) return Frow[slot];
    Cp<T> f = Frow[slot == 0 ? (P.nt >> 1) : slot];
    if (slot != 0) {
        f.x *= (T)2;
        f.y *= (T)2;
    }
    return f;
}
// the same for wavenumber k in either layout of F (P.fhalf: the Hermitian walk's slots of row k >= tnum/2 + 1 are the mirrored
// frequencies of row tnum - k, conjugated)
template <typename T> __device__ __forceinline__ Cp<T> ps_load_slot_k(const PsParams &P, int k, int slot)
{
    const Cp<T> *F = reinterpret_cast<const Cp<T> *>(P.F);
    if (!P.fhalf) return ps_load_slot<T>(F + (size_t)k * P.fstride, P, slot);
    const int idx = slot == 0 ? (P.nt >> 1) : slot;
    const bool mirror = 2 * k > P.tnum;
    Cp<T> f = mirror ? F[(size_t)(P.tnum - k) * P.fstride + (P.nt - idx)] : F[(size_t)k * P.fstride + idx];
    if (mirror) f.y = -f.y;
    if (slot != 0) {
        f.x *= (T)2;
        f.y *= (T)2;
    }
    return f;
}

// wave-level reduce-scatter of NV (power of two <= 32) values over the 64 lanes: each
// halving step sends half of the remaining values to the partner lane; once one value is
// left the remaining lane bits are folded with plain butterflies.  On return v[0] of lane
// L holds the total of value index (L >> (6 - log2 NV)) & (NV - 1).
// value of the lane MASK away (lane ^ MASK).  float32: DPP moves inside a 16-lane row (no LDS crossbar round trip:
// ds_bpermute costs a wave ~100 cycles of latency per dependent step, and all waves of the one resident
// workgroup reduce at the same moment, so nothing hides it)
template <typename T, int MASK> __device__ __forceinline__ T lane_xor(T v)
{
    constexpr bool DPP = true;
    auto dpp32 = [](unsigned u) {
        unsigned x;
        if constexpr (MASK == 1) x = __builtin_amdgcn_update_dpp(0u, u, 0xB1, 0xf, 0xf, false);        // quad_perm:[1,0,3,2]
        else if constexpr (MASK == 2) x = __builtin_amdgcn_update_dpp(0u, u, 0x4E, 0xf, 0xf, false);   // quad_perm:[2,3,0,1]
        else if constexpr (MASK == 4) {
            x = __builtin_amdgcn_update_dpp(0u, u, 0x104, 0xf, 0x5, false);    // row_shl:4 into banks 0 and 2 (lane <- lane + 4)
            x = __builtin_amdgcn_update_dpp(x, u, 0x114, 0xf, 0xa, false);     // row_shr:4 into banks 1 and 3 (lane <- lane - 4)
        } else x = __builtin_amdgcn_update_dpp(0u, u, 0x128, 0xf, 0xf, false);                         // row_ror:8
        return x;
    };
    if constexpr (DPP && sizeof(T) == 4 && MASK <= 8) {
        return __uint_as_float(dpp32(__float_as_uint(v)));
    } else if constexpr (DPP && sizeof(T) == 8 && MASK <= 8) {
        // a double moves as its two words
        return __hiloint2double((int)dpp32((unsigned)__double2hiint(v)), (int)dpp32((unsigned)__double2loint(v)));
    } else {
        return __shfl_xor(v, MASK, 64);
    }
}

template <typename T, int HALF, int MASK, int NV>
__device__ __forceinline__ void wrs_halve(T (&v)[NV], int lane)
{
    constexpr bool SWAP = true;
    if constexpr (SWAP && sizeof(T) == 4 && (MASK == 32 || MASK == 16)) {
        // gfx950 v_permlane32_swap / v_permlane16_swap: the upper half (odd rows) of the first operand trades places
        // with the lower half (even rows) of the second -- afterwards every lane holds the value it keeps and the one
        // its partner sent, in the two registers
#pragma unroll
        for (int i = 0; i < HALF; ++i) {
            const unsigned a = __float_as_uint(v[i]), b = __float_as_uint(v[i + HALF]);
            if constexpr (MASK == 32) {
                const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
                v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
            } else {
                const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
                v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
            }
        }
    } else if constexpr (SWAP && sizeof(T) == 8 && (MASK == 32 || MASK == 16)) {
        // float64: the same swap on the low and the high words
#pragma unroll
        for (int i = 0; i < HALF; ++i) {
            const unsigned alo = (unsigned)__double2loint(v[i]), ahi = (unsigned)__double2hiint(v[i]);
            const unsigned blo = (unsigned)__double2loint(v[i + HALF]), bhi = (unsigned)__double2hiint(v[i + HALF]);
            if constexpr (MASK == 32) {
                const auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
                const auto hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
                v[i] = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
            } else {
                const auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
                const auto hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
                v[i] = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
            }
        }
    } else {
        // keep HALF of the 2*HALF live values, hand the other half to the lane MASK away
        const bool up = (lane & MASK) != 0;
#pragma unroll
        for (int i = 0; i < HALF; ++i) {
            const T send = up ? v[i] : v[i + HALF];
            const T keep = up ? v[i + HALF] : v[i];
            v[i] = keep + lane_xor<T, MASK>(send);
        }
    }
}

template <typename T, int NV>
__device__ __forceinline__ void wave_reduce_scatter(T (&v)[NV], int lane)
{
    static_assert(NV == 8 || NV == 32, "instantiated for 8 and 32 values");
    // every index below is a compile-time constant (a runtime-indexed register array is
    // lowered to compare/select chains: ~2000 instructions per call when this was a loop)
    if constexpr (NV == 32) {
        wrs_halve<T, 16, 32>(v, lane);
        wrs_halve<T, 8, 16>(v, lane);
        wrs_halve<T, 4, 8>(v, lane);
        wrs_halve<T, 2, 4>(v, lane);
        wrs_halve<T, 1, 2>(v, lane);
        v[0] += lane_xor<T, 1>(v[0]);
    } else {
        wrs_halve<T, 4, 32>(v, lane);
        wrs_halve<T, 2, 16>(v, lane);
        wrs_halve<T, 1, 8>(v, lane);
        v[0] += lane_xor<T, 4>(v[0]);
        v[0] += lane_xor<T, 2>(v[0]);
        v[0] += lane_xor<T, 1>(v[0]);
    }
}

// Frequency slot of (thread, m) in the vector kernels: PAIRS of owned frequencies are 64 slots apart (a wave's pair covers
// 128 consecutive slots, the waves of a workgroup interleave at that grain).  The kernels skip a pair that is zero in all
// 64 lanes, and the evanescent frequencies are a contiguous band of slots: with the pair's two frequencies a whole
// workgroup width apart (tid + m BLOCK, rounds 1-3) a pair went out only 512 slots after its first half did.
template <int BLOCK, int M> __device__ __forceinline__ int ps_slot(int tid, int m)
{
    if constexpr (M >= 2 && M % 2 == 0) return (m >> 1) * (2 * BLOCK) + ((tid >> 6) << 7) + ((m & 1) << 6) + (tid & 63);
    else return tid + m * BLOCK;
}
