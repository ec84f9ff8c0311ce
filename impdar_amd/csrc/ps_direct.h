// The vector path of the phase shift: the three direct frequency-sum kernels, the zero-frequency row of the Hermitian
// walk, and their launch (ps_dispatch; the route's PS_VECTOR attempt, ps_run in phaseshift.hip).
//
// Kernel mapping: one workgroup per wavenumber k.  Each lane keeps the
// complex state of M = nt/BLOCK frequencies in registers and walks tau in
// tiles of TT; the per-tau sum over frequencies is a wavefront
// reduce-scatter (DPP/shuffle butterfly, 2*TT values in ~2*TT shuffles)
// followed by one LDS pass across the waves, so each workgroup emits 128-byte
// contiguous runs of TK_T[k][tau].
#pragma once
#include "ps_common.h"
#include <type_traits>

template <typename T, int BLOCK, int M, bool VZ>
__global__ __launch_bounds__(BLOCK) void ps_kernel(PsParams P)
{
    // tau per tile: the v(z) update is ~40 instructions per (tau, frequency) and is fully
    // unrolled, so its tile is kept short to bound the code size
    constexpr int PS_TT = VZ ? 4 : 16;
    constexpr int NW = BLOCK / 64;
    constexpr int SH = VZ ? 3 : 1;            // lane >> SH = value index held after the reduce-scatter
    __shared__ T red[2][NW][2 * PS_TT];
    // float32 v(z): the fp64 phase increment of every owned frequency at the current velocity lives in LDS
    // ([m][thread], each thread reads only what it wrote): 2M registers too many, and recomputing it (fp64
    // divide + square root) at every anchor cost as much as the steps in between
    __shared__ double phd_lds[(VZ && sizeof(T) == 4) ? M * BLOCK : 1];
    const int k = P.k0 + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Cp<T> *F = reinterpret_cast<const Cp<T> *>(P.F) + (size_t)k * P.fstride;
    Cp<T> *TK = reinterpret_cast<Cp<T> *>(P.TK) + (size_t)(k - P.k0) * P.snum;
    const double kxk = P.kx[k];

    // float32 data: a multiplicative recurrence in fp32 drifts systematically (the rounded rotation is the
    // same at every depth step of a constant-velocity run: 8192 steps x 6e-8 = 5e-4 .. 2e-3 at config 5),
    // so the accumulated phase is kept in fp64 and the spectrum is rotated from its ORIGINAL value:
    //   constant v: recurrence, re-anchored to FK0 * exp(i tau phi) every PS_ANCHOR depth steps
    //   v(z):       Phi += w dt sqrt(coss) in fp64 (the increment is recomputed in fp64 only when the
    //               velocity changes); F = FK0 * exp(i Phi) at every velocity change and every PS_ANCHOR-th step,
    //               a fixed fp32 rotation per step in between (as for constant v)
    // float64 data keeps the reference's recurrence (rounding 1e-16 per step).
    constexpr bool F32 = sizeof(T) == 4;
    T fr[M], fi[M];          // complex state per owned frequency (F32 v(z): the original spectrum FK0)
    T pa[M], pb[M];          // const-v: (cos phi, sin phi); v(z) fp64: (g = (kx/2w)^2, w*dt); v(z) fp32: (coss, -)
    double phd[F32 && !VZ ? M : 1]; // F32 const v: phase increment per depth step
    constexpr bool FZ = F32 && VZ;
    double Phi[FZ ? M : 1];          // F32 v(z): accumulated phase at the last anchor, kept in [-pi, pi]
    T gr[FZ ? M : 1], gi[FZ ? M : 1];   // F32 v(z): rotated state FK0 * exp(i Phi_tau)
    T pc[FZ ? M : 1], ps[FZ ? M : 1];   // F32 v(z): exp(i increment) of the current velocity
    T f0r[F32 && !VZ ? M : 1], f0i[F32 && !VZ ? M : 1];   // F32 const v: original spectrum for re-anchoring
    constexpr bool FD = VZ && !F32;
    T pw[FD ? M : 1];                 // fp64 v(z): w (pa holds 1/w)
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int iw = ps_slot<BLOCK, M>(tid, m);
        fr[m] = fi[m] = pa[m] = pb[m] = 0;
        if (FD) pw[FD ? m : 0] = 0;
        if (F32 && !VZ) phd[F32 && !VZ ? m : 0] = 0.0;
        if (FZ) {
            Phi[FZ ? m : 0] = 0.0;
            gr[FZ ? m : 0] = gi[FZ ? m : 0] = pc[FZ ? m : 0] = ps[FZ ? m : 0] = 0;
        }
        if (F32 && !VZ) f0r[F32 && !VZ ? m : 0] = f0i[F32 && !VZ ? m : 0] = 0;
        if (iw < P.nf) {
            const Cp<T> f = ps_load_slot<T>(F, P, iw);
            const double w = P.w[iw];
            if (!VZ) {
                const double vk = P.vconst * kxk / 2.0;
                const double vkx2 = vk * vk;                           // :411
                if (vkx2 < w * w) {                                    // :412 propagating only
                    const double ph = w * P.dt * sqrt(1.0 - vkx2 / (w * w));   // :415
                    double s, c;
                    sincos(ph, &s, &c);
                    pa[m] = (T)c;
                    pb[m] = (T)s;
                    fr[m] = f.x;
                    fi[m] = f.y;
                    if (F32) {
                        phd[F32 && !VZ ? m : 0] = ph;
                        f0r[F32 && !VZ ? m : 0] = f.x;
                        f0i[F32 && !VZ ? m : 0] = f.y;
                    }
                }
            } else {
                // coss = 1 - ((0.5 v) kx / w)^2 in the reference's own rounding (:460): a frequency that sits on the
                // evanescent boundary (coss = 0 up to an ulp or two; round-number geometries produce whole families)
                // is kept or dropped by the sign of that rounding.  pa = rn(1/w) and w itself turn the per-step
                // division into three operations with the correctly rounded quotient (below).
                pa[m] = (T)(1.0 / w);
                pb[m] = (T)(w * P.dt);
                pw[FD ? m : 0] = (T)w;
                fr[m] = f.x;
                fi[m] = f.y;
            }
        }
        // one frequency's fp64 set-up at a time (interleaved, the M chains spill)
        asm volatile("" : "+v"(fr[m]), "+v"(fi[m]), "+v"(pa[m]), "+v"(pb[m]));
    }
    // float32 helpers: exp(i x) for a phase kept in fp64, |x| <= pi after the wrap
    auto rot32 = [](double ph, T *s, T *c) { sincos_t<T>((T)ph, s, c); };
    // F32 v(z): fp64 phase increment w dt sqrt(coss) of owned frequency m at velocity v (0 past the end of the axis)
    auto incr = [&](int m, double v, double *cs_out) -> double {
        const int iw = ps_slot<BLOCK, M>(tid, m);
        double inc = 0.0, cs = 1.0;
        if (iw < P.nf) {
            const double w = P.w[iw];
            const double a = 0.5 * v * kxk / w;                 // :456
            cs = 1.0 - a * a;
            inc = w * P.dt * (cs > 0.0 ? sqrt(cs) : 0.0);       // :458-460
        }
        *cs_out = cs;
        return inc;
    };
    double v_prev = -1.0;    // F32 v(z): velocity of the last depth step
    unsigned edge = 0;       // F32 v(z): bit m = frequency m sits on the evanescent boundary (|coss| < 1e-8)
    double vz_next = (FZ && P.vz) ? P.vz[0] : 0.0, thr_next = (FZ && P.thr) ? P.thr[0] : 0.0;   // F32 v(z): prefetched
    int nrec = 0;            // F32 v(z): depth steps since the last anchor (uniform)
    bool rot_valid = false;  // F32 v(z): pc/ps hold exp(i phd) of the current velocity (uniform)

    const int ntile = (P.snum + PS_TT - 1) / PS_TT;
    for (int tile = 0; tile < ntile; ++tile) {
        PS_STAMP(0)
        T acc[2 * PS_TT];
#pragma unroll
        for (int i = 0; i < 2 * PS_TT; ++i) acc[i] = 0;
        const int tau0 = tile * PS_TT;
        // The chains carry no memory dependence, so instruction selection is free to interleave
        // all M x TT of them and the live temporaries spill; threading the state through an empty
        // volatile asm after every (tau, frequency) update pins the order without adding code.
        if (!VZ) {
            if (F32 && tile > 0 && (tile & (PS_ANCHOR / PS_TT - 1)) == 0) {
                // re-anchor: state after tau0 steps = FK0 * exp(i tau0 phi), phase reduced in fp64
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const double x = (double)tau0 * phd[F32 && !VZ ? m : 0];
                    const double r = x - 6.283185307179586 * rint(x * 0.15915494309189535);
                    T sn, cs;
                    rot32(r, &sn, &cs);
                    const T a = f0r[F32 && !VZ ? m : 0], b = f0i[F32 && !VZ ? m : 0];
                    fr[m] = fma(a, cs, -(b * sn));
                    fi[m] = fma(a, sn, b * cs);
                    asm volatile("" : "+v"(fr[m]), "+v"(fi[m]));
                }
            }
            // (pairs of frequencies that are zero in all 64 lanes -- the evanescent band, masked once at the start,
            // :404-412 -- are skipped: see ps_vz32_kernel; exact zeros, the order of the other terms kept)
            constexpr int QG = M >= 2 ? 2 : 1;
#pragma unroll
            for (int m0 = 0; m0 < M; m0 += QG) {
                bool nz = false;
#pragma unroll
                for (int j = 0; j < QG; ++j) nz = nz || fr[m0 + j] != (T)0 || fi[m0 + j] != (T)0;
                if (__builtin_amdgcn_ballot_w64(nz) == 0) continue;     // uniform
#pragma unroll
                for (int t = 0; t < PS_TT; ++t) {
#pragma unroll
                    for (int j = 0; j < QG; ++j) {
                        const int m = m0 + j;
                        const T nr = fma(fr[m], pa[m], -(fi[m] * pb[m]));   // FFK *= cp, :418
                        const T ni = fma(fr[m], pb[m], fi[m] * pa[m]);
                        fr[m] = nr;
                        fi[m] = ni;
                        acc[2 * t] += nr;                                   // TK[itau] += FFK, :420
                        acc[2 * t + 1] += ni;
                        asm volatile("" : "+v"(fr[m]), "+v"(fi[m]), "+v"(acc[2 * t]), "+v"(acc[2 * t + 1]));
                    }
                }
            }
        } else if (F32) {
            // not unrolled: the rare blocks (velocity change, anchor, boundary frequencies) appear once in the
            // code and the per-step sums are filed into acc[] by a uniform index (unrolled four times the body
            // exceeded the unroller's budget and acc[2t] turned into select chains: 2x slower than before)
#pragma unroll 1
            for (int t = 0; t < PS_TT; ++t) {
                const int tau = tau0 + t;
                if (tau < P.snum) {   // uniform
                    // this step's velocity and threshold were requested a step ago (a load-and-wait per step
                    // cost as much as the step)
                    const double vd = vz_next;
                    const T thr = (T)thr_next;
                    const int tn = tau + 1 < P.snum ? tau + 1 : tau;
                    vz_next = P.vz[tn];
                    thr_next = P.thr[tn];
                    const bool changed = fabs(vd - v_prev) > P.vtol * fabs(vd);   // uniform
                    if (changed) {
                        // new velocity (layered profiles get here a few times).  Velocities within 1e-10 of
                        // the last one count as the same: 2*gradient(z(t)) of a layered table is constant
                        // inside a layer up to ~4e-13 of rounding noise, and a 1e-10 velocity error moves the
                        // phase by < 3e-6 rad over 8192 steps (float32 path only).
                        unsigned new_edge = 0;
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            if (nrec > 0) {   // uniform: the steps since the last anchor turned by the OLD increment
                                const double ph = Phi[FZ ? m : 0] + (double)nrec * phd_lds[FZ ? m * BLOCK + tid : 0];
                                Phi[FZ ? m : 0] = ph - 6.283185307179586 * rint(ph * 0.15915494309189535);
                            }
                            // A frequency on the evanescent boundary (coss = 0 to rounding; with round-number
                            // geometries whole families of (kx, w) sit exactly there) is kept or dropped for
                            // good by the sign of coss, which the reference re-evaluates with every step's
                            // velocity: those (a handful per radargram) are advanced step by step below, in
                            // fp64, and take no part in the shared-increment scheme (increment 0 for them).
                            double cs;
                            const double inc = incr(m, vd, &cs);
                            const bool on_edge = fabs(cs) < 1e-8;
                            phd_lds[FZ ? m * BLOCK + tid : 0] = on_edge ? 0.0 : inc;
                            new_edge |= (on_edge ? 1u : 0u) << m;
                            pa[m] = (T)cs;
                            // evanescent at this velocity: zero from here on (:484-485).  The threshold the
                            // reference compares coss with is (tau/tt_end/1e6)^2 <= 1e-12, so away from the
                            // boundary the test is the sign of coss and is settled once per velocity; the
                            // boundary frequencies are tested step by step below.
                            if (!on_edge && cs <= 0.0) {
                                fr[m] = 0;
                                fi[m] = 0;
                            }
                            asm volatile("" : "+v"(pa[m]), "+v"(fr[m]), "+v"(fi[m]));
                        }
                        v_prev = vd;
                        edge = new_edge;
                        rot_valid = false;
                        nrec = 0;
                    }
                    nrec += 1;
                    if (changed || nrec == PS_ANCHOR) {
                        // anchor: the state from the ORIGINAL spectrum and the fp64 phase
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            double ph = Phi[FZ ? m : 0] + (double)nrec * phd_lds[FZ ? m * BLOCK + tid : 0];
                            ph -= 6.283185307179586 * rint(ph * 0.15915494309189535);
                            Phi[FZ ? m : 0] = ph;
                            T sn, cs;
                            rot32(ph, &sn, &cs);
                            gr[FZ ? m : 0] = fma(fr[m], cs, -(fi[m] * sn));     // FK0 * exp(i Phi), :464 cumulated
                            gi[FZ ? m : 0] = fma(fr[m], sn, fi[m] * cs);
                            asm volatile("" : "+v"(gr[FZ ? m : 0]), "+v"(gi[FZ ? m : 0]));
                        }
                        nrec = 0;
                    } else {
                        // same velocity as the last step: every frequency turns by its fixed increment; the
                        // fp32 recurrence runs for fewer than PS_ANCHOR steps between anchors (8e-6 rad of drift)
                        if (!rot_valid) {
#pragma unroll
                            for (int m = 0; m < M; ++m) {
                                T sn, cs;
                                rot32(phd_lds[FZ ? m * BLOCK + tid : 0], &sn, &cs);   // |increment| <= |w| dt <= pi
                                pc[FZ ? m : 0] = cs;
                                ps[FZ ? m : 0] = sn;
                                asm volatile("" : "+v"(pc[FZ ? m : 0]), "+v"(ps[FZ ? m : 0]));
                            }
                            rot_valid = true;
                        }
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            const T a = gr[FZ ? m : 0], b = gi[FZ ? m : 0];
                            gr[FZ ? m : 0] = fma(a, pc[FZ ? m : 0], -(b * ps[FZ ? m : 0]));
                            gi[FZ ? m : 0] = fma(a, ps[FZ ? m : 0], b * pc[FZ ? m : 0]);
                        }
                    }
                    if (edge) {
                        // boundary frequencies: this step's increment from this step's velocity, in fp64
#pragma unroll
                        for (int m = 0; m < M; ++m)
                            if ((edge >> m) & 1u) {
                                const double w = P.w[ps_slot<BLOCK, M>(tid, m)];
                                const double a = 0.5 * vd * kxk / w;
                                const double cs = 1.0 - a * a;
                                pa[m] = (T)cs;
                                double ph = Phi[FZ ? m : 0] + w * P.dt * (cs > 0.0 ? sqrt(cs) : 0.0);
                                ph -= 6.283185307179586 * rint(ph * 0.15915494309189535);
                                Phi[FZ ? m : 0] = ph;
                                T sn, c2;
                                rot32(ph, &sn, &c2);
                                gr[FZ ? m : 0] = fma(fr[m], c2, -(fi[m] * sn));
                                gi[FZ ? m : 0] = fma(fr[m], sn, fi[m] * c2);
                                if (pa[m] <= thr) {                         // :484-485, stays zero afterwards
                                    fr[m] = 0;
                                    fi[m] = 0;
                                    gr[FZ ? m : 0] = 0;
                                    gi[FZ ? m : 0] = 0;
                                }
                            }
                    }
                    // :487, four partial sums per component (one 16-deep dependent chain of adds stalls a
                    // lone wavefront)
                    T pr[4] = {0, 0, 0, 0}, pi[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        pr[m & 3] += gr[FZ ? m : 0];
                        pi[m & 3] += gi[FZ ? m : 0];
                    }
                    const T sr = (pr[0] + pr[1]) + (pr[2] + pr[3]), si = (pi[0] + pi[1]) + (pi[2] + pi[3]);
#pragma unroll
                    for (int u = 0; u < PS_TT; ++u)
                        if (t == u) {   // uniform
                            acc[2 * u] = sr;
                            acc[2 * u + 1] = si;
                        }
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < PS_TT; ++t) {
                const int tau = min(tau0 + t, P.snum - 1);
                const T num = ((T)0.5 * (T)P.vz[tau]) * (T)kxk;         // (0.5 vbg) kx, :460
                const T thr = (T)P.thr[tau];
                const bool live_tau = (tau0 + t) < P.snum;
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    // a = rn(num / w): q = rn(num rn(1/w)), exact remainder by fma, one correction (Markstein);
                    // a padded lane has pa = pw = 0 and gets a = 0
                    const T q = num * pa[m];
                    const T a = fma(fma(-q, pw[FD ? m : 0], num), pa[m], q);
                    const T coss = (T)1 - a * a;                        // :460
                    const T ph = pb[m] * sqrt(coss > 0 ? coss : (T)0);  // :460 (real part of the complex sqrt)
                    T s, c;
                    sincos_t<T>(ph, &s, &c);
                    T nr = fma(fr[m], c, -(fi[m] * s));                 // :464
                    T ni = fma(fr[m], s, fi[m] * c);
                    if (coss <= thr) {                                  // :484-485, stays zero afterwards
                        nr = 0;
                        ni = 0;
                    }
                    if (live_tau) {
                        fr[m] = nr;
                        fi[m] = ni;
                        acc[2 * t] += nr;                               // :487
                        acc[2 * t + 1] += ni;
                    }
                    asm volatile("" : "+v"(fr[m]), "+v"(fi[m]), "+v"(acc[2 * t]), "+v"(acc[2 * t + 1]));
                }
            }
        }
        // ---- sum over frequencies: wave butterfly, then across waves via LDS
        PS_STAMP(1)
        wave_reduce_scatter<T, 2 * PS_TT>(acc, lane);
        T (*buf)[2 * PS_TT] = red[tile & 1];
        if ((lane & ((1 << SH) - 1)) == 0) buf[wave][lane >> SH] = acc[0];
        PS_STAMP(2)
        __syncthreads();
        PS_STAMP(3)
        if (tid < 2 * PS_TT) {
            T s = 0;
#pragma unroll
            for (int q = 0; q < NW; ++q) s += buf[q][tid];
            const int tau = tau0 + (tid >> 1);
            if (tau < P.snum) {
                T *dst = reinterpret_cast<T *>(TK + tau) + (tid & 1);
                *dst = s / (T)P.snum;                                   // TK /= snum, :492
            }
        }
        PS_STAMP(4)
        // red[] is double-buffered: the next tile writes the other buffer and the
        // barrier of that tile orders it against these reads
    }
}

// loads through the scalar cache (uniform address, data read-only for the kernel), load and wait in one statement:
// a split request / wait pair is not safe in C++ -- the compiler is free to copy the destination register between
// the two statements, i.e. before the data has arrived
__device__ __forceinline__ int scalar_load_i32(const int *p)
{
    int v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}
__device__ __forceinline__ void scalar_load_2f64(const double *p, const double *q, double *a, double *b)
{
    double x, y;
    asm volatile("s_load_dwordx2 %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(x), "=&s"(y)
                 : "s"(p), "s"(q)
                 : "memory");
    *a = x;
    *b = y;
}

// ---------------------------------------------------------------------------
// float32 v(z) (Gazdag), layered profiles: the depth axis is cut into runs of constant velocity (the host
// marks the steps where the velocity moves by more than P.vtol, the same rule ps_kernel applies on the fly),
// and inside a run every frequency turns by a fixed rotation -- the constant-velocity inner loop.  A 16-step
// tile without a run boundary and inside the axis ("quiet") takes the fully unrolled rotate-accumulate body of
// the constant-velocity kernel (6 instructions per (tau, frequency)); every other tile walks its steps one by
// one with the general update (velocity change: fold the pending steps into the fp64 phase, new fp64 increment,
// evanescence settled for the run, mig_python.py:456-485; anchors).  Frequencies on the evanescent boundary
// (|coss| < 1e-8: kept or dropped by the sign of coss at every step's own velocity) take no part in the shared
// rotation: they are walked in fp64, step by step -- inline in the per-step tiles, as a correction to the
// step sums after the unrolled body in quiet tiles.  The state is anchored to FK0 * exp(i Phi) with the fp64
// phase at every run start and at least every PS_ANCHOR steps.
// Registers per owned frequency: the rotating state, the run's rotation and the fp64 phase at the last
// anchor; the original spectrum FK0 and the fp64 increment live in LDS ([m][thread], each thread reads only
// what it wrote) -- 128 KB at 8192 frequencies, one workgroup per CU.
// ---------------------------------------------------------------------------
#ifndef IMPDAR_PS_VZ32_M8_WAVES
#define IMPDAR_PS_VZ32_M8_WAVES 1      // min waves per SIMD asked of the 512 x 8 instantiation (4: two workgroups per CU at 128 VGPRs, with spills)
#endif
template <int BLOCK, int M>
__global__ __launch_bounds__(BLOCK, (BLOCK == 512 && M == 8) ? IMPDAR_PS_VZ32_M8_WAVES : 1) void ps_vz32_kernel(PsParams P)
{
    constexpr int TT = 16;
    constexpr int NW = BLOCK / 64;
    extern __shared__ __attribute__((aligned(16))) char ps_smem[];
    double *phd_lds = reinterpret_cast<double *>(ps_smem);                              // [M][BLOCK] fp64 increment of the run
    float2 *f0_lds = reinterpret_cast<float2 *>(ps_smem + (size_t)M * BLOCK * 8);       // [M][BLOCK] original spectrum
    float(*red)[NW][2 * TT] = reinterpret_cast<float(*)[NW][2 * TT]>(ps_smem + (size_t)M * BLOCK * 16);
    // boundary frequencies in quiet tiles (see below): per-step corrections to the frequency sum, double-buffered over tiles
    float *corr = reinterpret_cast<float *>(ps_smem + (size_t)M * BLOCK * 16 + 2 * NW * 2 * TT * sizeof(float));   // [2][2 * TT]
    const int k = P.rowmap ? P.rowmap[blockIdx.x] : P.k0 + (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Cp<float> *F = reinterpret_cast<const Cp<float> *>(P.F) + (size_t)k * P.fstride;
    Cp<float> *TK = reinterpret_cast<Cp<float> *>(P.TK) + (size_t)(k - P.k0) * P.snum;
    const double kxk = P.kx[k];
    if (tid < 4 * TT) corr[tid] = 0.f;

    float gr[M], gi[M];      // FK0 * exp(i Phi_tau): the rotating state
    float pc[M], ps[M];      // exp(i increment) of the current run
    double Phi[M];           // accumulated phase at the last anchor, kept in [-pi, pi]
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int iw = ps_slot<BLOCK, M>(tid, m);
        float2 f = make_float2(0.f, 0.f);
        if (iw < P.nf) {
            const Cp<float> c = ps_load_slot<float>(F, P, iw);
            f = make_float2(c.x, c.y);
        }
        f0_lds[m * BLOCK + tid] = f;
        phd_lds[m * BLOCK + tid] = 0.0;
        gr[m] = gi[m] = ps[m] = 0.f;
        pc[m] = 1.f;
        Phi[m] = 0.0;
    }
    auto rot32 = [](double ph, float *s, float *c) { sincos_t<float>((float)ph, s, c); };
    auto anchor = [&](int nrec) {
        // the state from the ORIGINAL spectrum and the fp64 phase: nrec steps at the run's increment since the last anchor
#pragma unroll
        for (int m = 0; m < M; ++m) {
            double ph = Phi[m] + (double)nrec * phd_lds[m * BLOCK + tid];
            ph -= 6.283185307179586 * rint(ph * 0.15915494309189535);
            Phi[m] = ph;
            float sn, cs;
            rot32(ph, &sn, &cs);
            const float2 f = f0_lds[m * BLOCK + tid];
            gr[m] = fmaf(f.x, cs, -(f.y * sn));          // FK0 * exp(i Phi), :464 cumulated
            gi[m] = fmaf(f.x, sn, f.y * cs);
            asm volatile("" : "+v"(gr[m]), "+v"(gi[m]));
        }
    };
    unsigned edge = 0;       // bit m = frequency m sits on the evanescent boundary of the current run (|coss| < 1e-8)
    bool wg_edge = false;    // ... some thread of the workgroup has one (uniform)
    int nrec = 0;            // depth steps since the last anchor (uniform)

    const int ntile = (P.snum + TT - 1) / TT;
    // One 16-step tile, instantiated twice: quiet tiles and per-step tiles each get their own loop below.  With both
    // paths in one loop body (the per-step path is ~40 KB of code between the unrolled body and the tile's tail)
    // every part of a quiet tile ran 8-40 % slower -- same instructions, stamps in profiles/r02_ps_stamps.txt:
    // 9140 cycles per tile against 7870 with the per-step code out of the loop (12 % of the kernel at config 5).
    auto do_tile = [&](const int tile, auto quiet_tag) __attribute__((always_inline)) {
        constexpr bool quiet = decltype(quiet_tag)::value;
        float acc[2 * TT];
#pragma unroll
        for (int i = 0; i < 2 * TT; ++i) acc[i] = 0.f;
        const int tau0 = tile * TT;
        PS_STAMP(0)
        if constexpr (quiet) {
            if (nrec + TT > PS_ANCHOR) {
                anchor(nrec);
                nrec = 0;
            }
            // Pairs of frequencies whose state is zero in all 64 lanes of the wave are skipped (round 4): once evanescent,
            // zero for good (:484-485), and the frequencies below v kx / 2 are a contiguous band -- 42 % of the (kx, w)
            // plane at config 5, whole waves' worth of slots.  A skipped term is an exact zero and the order of the
            // others is kept (for every step: frequencies in rising order): the sums are bit for bit what they were.
            constexpr int QG = M >= 2 ? 2 : 1;
#pragma unroll
            for (int m0 = 0; m0 < M; m0 += QG) {
                bool nz = false;
#pragma unroll
                for (int j = 0; j < QG; ++j) nz = nz || gr[m0 + j] != 0.f || gi[m0 + j] != 0.f;
                if (__builtin_amdgcn_ballot_w64(nz) == 0) continue;             // uniform
#pragma unroll
                for (int t = 0; t < TT; ++t) {
#pragma unroll
                    for (int j = 0; j < QG; ++j) {
                        const int m = m0 + j;
                        const float nr = fmaf(gr[m], pc[m], -(gi[m] * ps[m]));     // FK *= exp(i w dt sqrt(coss)), :464
                        const float ni = fmaf(gr[m], ps[m], gi[m] * pc[m]);
                        gr[m] = nr;
                        gi[m] = ni;
                        acc[2 * t] += nr;                                           // TK[itau] += FK, :487
                        acc[2 * t + 1] += ni;
                        asm volatile("" : "+v"(gr[m]), "+v"(gi[m]), "+v"(acc[2 * t]), "+v"(acc[2 * t + 1]));
                    }
                }
            }
            nrec += TT;
        } else {
#pragma unroll 1
            for (int t = 0; t < TT; ++t) {
                const int tau = tau0 + t;
                if (tau >= P.snum) break;      // uniform
                const double vd = P.vz[tau];
                const float thr = (float)P.thr[tau];
                const bool changed = P.sched[tau] != 0;      // uniform
                if (changed) {
                    unsigned new_edge = 0;
                    // opaque copy of the thread index: otherwise the M 64-bit addresses of P.w[...] below are hoisted
                    // out of the tile loop and held in 2M registers for the whole kernel (spills in the tile tail)
                    int tid_here = tid;
                    asm volatile("" : "+v"(tid_here));
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const int iw = ps_slot<BLOCK, M>(tid_here, m);
                        {
                            // (a frequency that is out -- original spectrum zeroed -- in all 64 lanes has nothing to turn:
                            // the divide, square root and sincos of a run's start are skipped for it, round 4)
                            const float2 f0c = f0_lds[m * BLOCK + tid];
                            if (__builtin_amdgcn_ballot_w64(f0c.x != 0.f || f0c.y != 0.f) == 0) {      // uniform
                                pc[m] = 1.f;
                                ps[m] = 0.f;
                                phd_lds[m * BLOCK + tid] = 0.0;
                                continue;
                            }
                        }
                        if (nrec > 0) {   // the steps since the last anchor turned by the OLD increment
                            const double ph = Phi[m] + (double)nrec * phd_lds[m * BLOCK + tid];
                            Phi[m] = ph - 6.283185307179586 * rint(ph * 0.15915494309189535);
                        }
                        double inc = 0.0, cs = 1.0;
                        if (iw < P.nf) {
                            const double w = P.w[iw];
                            const double a = 0.5 * vd * kxk / w;                 // :456
                            cs = 1.0 - a * a;
                            inc = w * P.dt * (cs > 0.0 ? sqrt(cs) : 0.0);       // :458-460
                        }
                        // a frequency on the evanescent boundary (coss = 0 to rounding) is kept or dropped by the
                        // sign of coss at every step's own velocity: advanced step by step below, in fp64
                        const bool on_edge = fabs(cs) < 1e-8;
                        const double use = on_edge ? 0.0 : inc;
                        phd_lds[m * BLOCK + tid] = use;
                        new_edge |= (on_edge ? 1u : 0u) << m;
                        // evanescent at this velocity: zero from here on (:484-485; away from the boundary the
                        // reference's threshold (tau/tt_end/1e6)^2 <= 1e-12 is the sign of coss)
                        if (!on_edge && cs <= 0.0) f0_lds[m * BLOCK + tid] = make_float2(0.f, 0.f);
                        float sn, c2;
                        rot32(use, &sn, &c2);                                   // |increment| <= |w| dt <= pi
                        pc[m] = c2;
                        ps[m] = sn;
                        asm volatile("" : "+v"(pc[m]), "+v"(ps[m]));
                    }
                    edge = new_edge;
                    wg_edge = __syncthreads_or(new_edge != 0) != 0;
                    nrec = 0;
                }
                nrec += 1;
                if (changed || nrec == PS_ANCHOR) {
                    anchor(nrec);
                    nrec = 0;
                } else {
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const float a = gr[m], b = gi[m];
                        gr[m] = fmaf(a, pc[m], -(b * ps[m]));
                        gi[m] = fmaf(a, ps[m], b * pc[m]);
                    }
                }
                if (edge) {
                    // boundary frequencies: this step's increment from this step's velocity, in fp64
                    int tid_here = tid;
                    asm volatile("" : "+v"(tid_here));
#pragma unroll
                    for (int m = 0; m < M; ++m)
                        if ((edge >> m) & 1u) {
                            const double w = P.w[ps_slot<BLOCK, M>(tid_here, m)];
                            const double a = 0.5 * vd * kxk / w;
                            const double cs = 1.0 - a * a;
                            double ph = Phi[m] + w * P.dt * (cs > 0.0 ? sqrt(cs) : 0.0);
                            ph -= 6.283185307179586 * rint(ph * 0.15915494309189535);
                            Phi[m] = ph;
                            float sn, c2;
                            rot32(ph, &sn, &c2);
                            float2 f = f0_lds[m * BLOCK + tid];
                            if ((float)cs <= thr) {                             // :484-485, stays zero afterwards
                                f = make_float2(0.f, 0.f);
                                f0_lds[m * BLOCK + tid] = f;
                            }
                            gr[m] = fmaf(f.x, c2, -(f.y * sn));
                            gi[m] = fmaf(f.x, sn, f.y * c2);
                        }
                }
                float pr[4] = {0, 0, 0, 0}, pi[4] = {0, 0, 0, 0};               // :487
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    pr[m & 3] += gr[m];
                    pi[m & 3] += gi[m];
                }
                const float sr = (pr[0] + pr[1]) + (pr[2] + pr[3]), si = (pi[0] + pi[1]) + (pi[2] + pi[3]);
#pragma unroll
                for (int u = 0; u < TT; ++u)
                    if (t == u) {   // uniform
                        acc[2 * u] = sr;
                        acc[2 * u + 1] = si;
                    }
            }
        }
        // ---- sum over frequencies: wave butterfly, then across waves via LDS
        PS_STAMP(1)
        wave_reduce_scatter<float, 2 * TT>(acc, lane);
        float(*buf)[2 * TT] = red[tile & 1];
        if ((lane & 1) == 0) buf[wave][lane >> 1] = acc[0];
        PS_STAMP(2)
        if (quiet && wg_edge && edge) {
            // Boundary frequencies of this thread (a handful per radargram; whole families of (kx, w) with
            // round-number geometries: dx 1 m, dt 10 ns, v 1.68e8 puts one on every 25th wavenumber).  Their
            // shared increment is zero, so the unrolled body carried their state through the tile unchanged and
            // added it to every step's sum; here each is walked through the tile's 16 steps in fp64 at every
            // step's own velocity (kept or dropped by the sign of coss, mig_python.py:456-485, as in the
            // per-step path below) and the difference to the state the body added goes to the step's
            // correction, which the tile's tail adds to the frequency sum.  Placed here, after the reduce-scatter,
            // because the 32 per-step sums are then out of the registers (before it: 35 spilled).  (Sending such workgroups through
            // the per-step path for the whole run cost them 12x: 28 ms of tail at config 5.)
            int tid_here = tid;
            asm volatile("" : "+v"(tid_here));
            // the steps' velocities and thresholds come through the scalar cache (uniform addresses; as vector loads
            // each would stall the walk for a microsecond)
            const double *svz = P.vz + tau0, *sthr = P.thr + tau0;
            float *cr = corr + (tile & 1) * 2 * TT;
            // one copy of the walk, the owned frequency picked by compare-and-select (an unrolled copy per m kept
            // 16 sets of fp64 temporaries alive: 28 spilled registers)
            for (unsigned e = edge; e; e &= e - 1) {
                const int m = __builtin_ctz(e);
                double ph = 0.0;
                float hr = 0.f, hi = 0.f;
#pragma unroll
                for (int q = 0; q < M; ++q)
                    if (q == m) {
                        ph = Phi[q];
                        hr = gr[q];
                        hi = gi[q];
                    }
                const double w = P.w[ps_slot<BLOCK, M>(tid_here, m)];
                float2 f = f0_lds[m * BLOCK + tid];
                float sr = hr, si = hi;
#pragma unroll 1
                for (int t = 0; t < TT; ++t) {
                    double vd, thr_d;
                    scalar_load_2f64(svz + t, sthr + t, &vd, &thr_d);
                    const float thr = (float)thr_d;
                    const double a = 0.5 * vd * kxk / w;
                    const double cs = 1.0 - a * a;
                    ph += w * P.dt * (cs > 0.0 ? sqrt(cs) : 0.0);
                    ph -= 6.283185307179586 * rint(ph * 0.15915494309189535);
                    float sn, c2;
                    rot32(ph, &sn, &c2);
                    if ((float)cs <= thr) f = make_float2(0.f, 0.f);      // :484-485, stays zero afterwards
                    sr = fmaf(f.x, c2, -(f.y * sn));
                    si = fmaf(f.x, sn, f.y * c2);
                    atomicAdd(&cr[2 * t], sr - hr);
                    atomicAdd(&cr[2 * t + 1], si - hi);
                }
                f0_lds[m * BLOCK + tid] = f;
#pragma unroll
                for (int q = 0; q < M; ++q)
                    if (q == m) {
                        Phi[q] = ph;
                        gr[q] = sr;
                        gi[q] = si;
                    }
            }
        }
        __syncthreads();
        PS_STAMP(3)
        if (tid < 2 * TT) {
            float sum = corr[(tile & 1) * 2 * TT + tid];     // boundary frequencies of a quiet tile (zero otherwise)
            corr[(tile & 1) * 2 * TT + tid] = 0.f;           // next written two tiles on, a barrier in between
#pragma unroll
            for (int q = 0; q < NW; ++q) sum += buf[q][tid];
            const int tau = tau0 + (tid >> 1);
            if (tau < P.snum) {
                float *dst = reinterpret_cast<float *>(TK + tau) + (tid & 1);
                *dst = sum / (float)P.snum;                                     // TK /= snum, :492
            }
        }
        PS_STAMP(4)
        // red[] is double-buffered: the next tile writes the other buffer and the barrier of that tile
        // orders it against these reads
    };
    // the tiles' schedule flags come through the scalar cache, 32 tiles per word (as plain loads they are vector
    // loads -- the compiler cannot prove the table read-only -- whose s_waitcnt vmcnt(0) also waits for the write
    // acknowledgement of the sums wave 0 stored a few instructions earlier)
    unsigned dirty_bits = 0;
    auto is_quiet = [&](const int tile) __attribute__((always_inline)) {
        if ((tile & 31) == 0) dirty_bits = (unsigned)scalar_load_i32(P.tsched + (tile >> 5));
        return ((dirty_bits >> (tile & 31)) & 1u) == 0 && tile * TT + TT <= P.snum;      // uniform
    };
    int tile = 0;
    while (tile < ntile) {
        for (; tile < ntile && !is_quiet(tile); ++tile) do_tile(tile, std::false_type());
        for (; tile < ntile && is_quiet(tile); ++tile) do_tile(tile, std::true_type());
    }
}

// ---------------------------------------------------------------------------
// float64 v(z), layered profiles: the float64 counterpart of ps_vz32_kernel (what a float64 .mat file gets).  The
// per-step kernel (ps_kernel<double, ..., true>) evaluates a square root and a sincos for every (tau, frequency):
// 232 ms at 4096^2 where the constant-velocity float64 kernel takes 19 ms.  Here, inside a run of constant velocity
// every frequency turns by the run's rotation (float64: no anchors needed, the recurrence loses ~1e-16 per step
// like the reference's own product), 6 float64 instructions per (tau, frequency) in fully unrolled 16-step tiles.
//  * Velocity noise inside a run (2*gradient(z(t)) of a layered table is constant only to ~4e-13) is not
//    dropped: the host sums eps = v/v_run - 1 over every tile, and at the end of the tile each frequency is turned
//    by exp(i coef eps_sum) (first order: the angle stays below 5e-7), coef = d(increment)/d(ln v) = -w dt a^2 / sqrt(coss) kept in LDS
//    ([m][thread]); the per-step tiles apply it step by step.
//  * Frequencies near the evanescent boundary (|coss| < 1e-6) take no part in the shared rotation: they are walked
//    step by step at every step's own velocity with the reference's rounding of coss (kept or dropped by its sign,
//    mig_python.py:456-485) -- inline in the per-step tiles, as a correction to the step sums in quiet tiles
//    (float64 LDS atomics), exactly as in ps_vz32_kernel.
// ---------------------------------------------------------------------------
template <int BLOCK, int M>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2))) void ps_vz64_kernel(PsParams P)
{
    constexpr int TT = 16;
    constexpr int NW = BLOCK / 64;
    extern __shared__ __attribute__((aligned(16))) char ps_smem[];
    double *coef = reinterpret_cast<double *>(ps_smem);                                  // [M][BLOCK]
    double(*red)[NW][2 * TT] = reinterpret_cast<double(*)[NW][2 * TT]>(ps_smem + (size_t)M * BLOCK * 8);
    double *corr = reinterpret_cast<double *>(ps_smem + (size_t)M * BLOCK * 8 + 2 * NW * 2 * TT * sizeof(double));   // [2][2 * TT]
    const int k = P.rowmap ? P.rowmap[blockIdx.x] : P.k0 + (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Cp<double> *F = reinterpret_cast<const Cp<double> *>(P.F) + (size_t)k * P.fstride;
    Cp<double> *TK = reinterpret_cast<Cp<double> *>(P.TK) + (size_t)(k - P.k0) * P.snum;
    const double kxk = P.kx[k];
    if (tid < 4 * TT) corr[tid] = 0.0;

    double gr[M], gi[M];     // the field of every owned frequency
    double pc[M], ps[M];     // exp(i increment) of the current run (identity for boundary and dead frequencies)
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int iw = ps_slot<BLOCK, M>(tid, m);
        gr[m] = gi[m] = ps[m] = 0.0;
        pc[m] = 1.0;
        if (iw < P.nf) {
            const Cp<double> c = ps_load_slot<double>(F, P, iw);
            gr[m] = c.x;
            gi[m] = c.y;
        }
        coef[m * BLOCK + tid] = 0.0;
    }
    unsigned edge = 0;       // bit m = frequency m sits near the evanescent boundary of the current run
    bool wg_edge = false;    // ... some thread of the workgroup has one (uniform)
    double v_run = 1.0;      // the current run's velocity (uniform)

    const int ntile = (P.snum + TT - 1) / TT;
    // one boundary frequency, one depth step, the reference's way: FK *= exp(i w dt sqrt(coss)), zero for good once
    // coss <= threshold
    auto edge_step = [&](double w, double vd, double thr, double &sr, double &si) {
        const double a = 0.5 * vd * kxk / w;                                    // :456
        const double cs = 1.0 - a * a;
        const double inc = w * P.dt * (cs > 0.0 ? sqrt(cs) : 0.0);              // :458-460
        double sn, c2;
        sincos(inc, &sn, &c2);
        const double nr = sr * c2 - si * sn, ni = sr * sn + si * c2;           // :464
        sr = nr;
        si = ni;
        if (cs <= thr) {                                                        // :484-485
            sr = 0.0;
            si = 0.0;
        }
    };
    auto do_tile = [&](const int tile, auto quiet_tag) __attribute__((always_inline)) {
        constexpr bool quiet = decltype(quiet_tag)::value;
        double acc[2 * TT];
#pragma unroll
        for (int i = 0; i < 2 * TT; ++i) acc[i] = 0.0;
        const int tau0 = tile * TT;
        if constexpr (quiet) {
            // (pairs of frequencies that are zero in all 64 lanes are skipped: see ps_vz32_kernel)
            constexpr int QG = M >= 2 ? 2 : 1;
#pragma unroll
            for (int m0 = 0; m0 < M; m0 += QG) {
                bool nz = false;
#pragma unroll
                for (int j = 0; j < QG; ++j) nz = nz || gr[m0 + j] != 0.0 || gi[m0 + j] != 0.0;
                if (__builtin_amdgcn_ballot_w64(nz) == 0) continue;             // uniform
#pragma unroll
                for (int t = 0; t < TT; ++t) {
#pragma unroll
                    for (int j = 0; j < QG; ++j) {
                        const int m = m0 + j;
                        const double nr = fma(gr[m], pc[m], -(gi[m] * ps[m]));      // FK *= exp(i w dt sqrt(coss)), :464
                        const double ni = fma(gr[m], ps[m], gi[m] * pc[m]);
                        gr[m] = nr;
                        gi[m] = ni;
                        acc[2 * t] += nr;                                           // TK[itau] += FK, :487
                        acc[2 * t + 1] += ni;
                        asm volatile("" : "+v"(gr[m]), "+v"(gi[m]), "+v"(acc[2 * t]), "+v"(acc[2 * t + 1]));
                    }
                }
            }
        } else {
#pragma unroll 1
            for (int t = 0; t < TT; ++t) {
                const int tau = tau0 + t;
                if (tau >= P.snum) break;      // uniform
                const double vd = P.vz[tau];
                const double thr = P.thr[tau];
                const bool changed = P.sched[tau] != 0;      // uniform
                int tid_here = tid;
                asm volatile("" : "+v"(tid_here));
                if (changed) {
                    unsigned new_edge = 0;
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const int iw = ps_slot<BLOCK, M>(tid_here, m);
                        double c2 = 1.0, sn = 0.0, cf = 0.0;
                        // (a frequency whose state is zero in all 64 lanes is out for good: nothing to compute for it)
                        const bool wave_out = __builtin_amdgcn_ballot_w64(gr[m] != 0.0 || gi[m] != 0.0) == 0;      // uniform
                        if (iw < P.nf && !wave_out) {
                            const double w = P.w[iw];
                            const double a = 0.5 * vd * kxk / w;                 // :456
                            const double cs = 1.0 - a * a;
                            const bool on_edge = fabs(cs) < 1e-6;
                            new_edge |= (on_edge ? 1u : 0u) << m;
                            if (!on_edge) {
                                if (cs <= 0.0) {
                                    // evanescent at this velocity: zero from here on (:484-485; away from the
                                    // boundary the threshold (tau/tt_end/1e6)^2 <= 1e-12 is the sign of coss)
                                    gr[m] = 0.0;
                                    gi[m] = 0.0;
                                } else {
                                    const double root = sqrt(cs);
                                    sincos(w * P.dt * root, &sn, &c2);          // :458-464
                                    cf = -(w * P.dt) * (a * a) / root;
                                }
                            }
                        }
                        pc[m] = c2;
                        ps[m] = sn;
                        coef[m * BLOCK + tid] = cf;
                        asm volatile("" : "+v"(pc[m]), "+v"(ps[m]), "+v"(gr[m]), "+v"(gi[m]));
                    }
                    edge = new_edge;
                    wg_edge = __syncthreads_or(new_edge != 0) != 0;
                    v_run = vd;
                }
                const double eps = vd / v_run - 1.0;         // this step's velocity against the run's (uniform)
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    double a = gr[m], b = gi[m];
                    const double nr = fma(a, pc[m], -(b * ps[m]));
                    const double ni = fma(a, ps[m], b * pc[m]);
                    a = nr;
                    b = ni;
                    if (eps != 0.0) {                        // uniform
                        const double d = coef[m * BLOCK + tid] * eps;
                        a = fma(-ni, d, nr);
                        b = fma(nr, d, ni);
                    }
                    gr[m] = a;
                    gi[m] = b;
                }
                if (edge) {
                    // boundary frequencies: this step's increment from this step's velocity (their pc/ps are the identity)
#pragma unroll
                    for (int m = 0; m < M; ++m)
                        if ((edge >> m) & 1u) edge_step(P.w[ps_slot<BLOCK, M>(tid_here, m)], vd, thr, gr[m], gi[m]);
                }
                double pr[4] = {0, 0, 0, 0}, pi[4] = {0, 0, 0, 0};              // :487
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    pr[m & 3] += gr[m];
                    pi[m & 3] += gi[m];
                }
                const double sr = (pr[0] + pr[1]) + (pr[2] + pr[3]), si = (pi[0] + pi[1]) + (pi[2] + pi[3]);
#pragma unroll
                for (int u = 0; u < TT; ++u)
                    if (t == u) {   // uniform
                        acc[2 * u] = sr;
                        acc[2 * u + 1] = si;
                    }
            }
        }
        // ---- sum over frequencies: wave butterfly, then across waves via LDS
        wave_reduce_scatter<double, 2 * TT>(acc, lane);
        double(*buf)[2 * TT] = red[tile & 1];
        if ((lane & 1) == 0) buf[wave][lane >> 1] = acc[0];
        if constexpr (quiet) {
            // velocity noise of the tile: F *= exp(i coef eps_sum) = 1 + i d up to d^2 / 2, and d = coef eps_sum stays
            // below 5e-7 even for a frequency next to the boundary band (coef <= 3e3 |w dt|) under a drift that uses
            // the whole run tolerance (eps_sum <= 16 x 1e-11): the dropped term is < 2e-13
            double es, unused;
            scalar_load_2f64(P.eps + tile, P.eps + tile, &es, &unused);
            if (es != 0.0) {     // uniform
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const double d = coef[m * BLOCK + tid] * es;
                    const double a = gr[m], b = gi[m];
                    gr[m] = fma(-b, d, a);
                    gi[m] = fma(a, d, b);
                }
            }
            if (wg_edge && edge) {
                // boundary frequencies of this thread: the unrolled body carried their state through the tile
                // unchanged (identity rotation) and added it to every step's sum; walk the 16 steps and file the
                // difference (see ps_vz32_kernel)
                int tid_here = tid;
                asm volatile("" : "+v"(tid_here));
                const double *svz = P.vz + tau0, *sthr = P.thr + tau0;
                double *cr = corr + (tile & 1) * 2 * TT;
                for (unsigned e = edge; e; e &= e - 1) {
                    const int m = __builtin_ctz(e);
                    double hr = 0.0, hi = 0.0;
#pragma unroll
                    for (int q = 0; q < M; ++q)
                        if (q == m) {
                            hr = gr[q];
                            hi = gi[q];
                        }
                    const double w = P.w[ps_slot<BLOCK, M>(tid_here, m)];
                    double sr = hr, si = hi;
#pragma unroll 1
                    for (int t = 0; t < TT; ++t) {
                        double vd, thr;
                        scalar_load_2f64(svz + t, sthr + t, &vd, &thr);
                        edge_step(w, vd, thr, sr, si);
                        atomicAdd(&cr[2 * t], sr - hr);
                        atomicAdd(&cr[2 * t + 1], si - hi);
                    }
#pragma unroll
                    for (int q = 0; q < M; ++q)
                        if (q == m) {
                            gr[q] = sr;
                            gi[q] = si;
                        }
                }
            }
        }
        __syncthreads();
        if (tid < 2 * TT) {
            double sum = corr[(tile & 1) * 2 * TT + tid];    // boundary frequencies of a quiet tile (zero otherwise)
            corr[(tile & 1) * 2 * TT + tid] = 0.0;           // next written two tiles on, a barrier in between
#pragma unroll
            for (int q = 0; q < NW; ++q) sum += buf[q][tid];
            const int tau = tau0 + (tid >> 1);
            if (tau < P.snum) {
                double *dst = reinterpret_cast<double *>(TK + tau) + (tid & 1);
                *dst = sum / (double)P.snum;                                    // TK /= snum, :492
            }
        }
    };
    unsigned dirty_bits = 0;
    auto is_quiet = [&](const int tile) __attribute__((always_inline)) {
        if ((tile & 31) == 0) dirty_bits = (unsigned)scalar_load_i32(P.tsched + (tile >> 5));
        return ((dirty_bits >> (tile & 31)) & 1u) == 0 && tile * TT + TT <= P.snum;      // uniform
    };
    int tile = 0;
    while (tile < ntile) {
        for (; tile < ntile && !is_quiet(tile); ++tile) do_tile(tile, std::false_type());
        for (; tile < ntile && is_quiet(tile); ++tile) do_tile(tile, std::true_type());
    }
}

// Hermitian walk: the zero-frequency row.  The reference replaces w = 0 by 1e-10/dt (:400-402); that frequency
// propagates only where kx = 0, and there coss = 1 at every velocity, so both branches turn it by w0 dt per depth
// step: TK[tau, k0] += FK[0, k0] e^{i (tau + 1) w0 dt} / snum (:415-420, :456-487, :492).  One thread per depth step,
// after the frequency kernel has stored its sums.
template <typename T>
__global__ __launch_bounds__(256) void ps_dc_kernel(const Cp<T> *__restrict__ F, Cp<T> *__restrict__ TK, int k0, int tk_row,
                                                    int fstride, int snum, double w0dt)
{
    const int tau = blockIdx.x * 256 + threadIdx.x;
    if (tau >= snum) return;
    const Cp<T> f = F[(size_t)k0 * fstride];
    double sn, cs;
    sincos((double)(tau + 1) * w0dt, &sn, &cs);
    const double re = (double)f.x * cs - (double)f.y * sn, im = (double)f.x * sn + (double)f.y * cs;
    Cp<T> *dst = TK + (size_t)tk_row * snum + tau;
    dst->x += (T)(re / (double)snum);
    dst->y += (T)(im / (double)snum);
}

static thread_local const char *t_ps_kernel = "";       // the frequency-sum kernel of the call in progress (metrics)

template <typename T, int BLOCK, int M>
static void ps_launch(const PsParams &P, hipStream_t st)
{
    constexpr size_t vz32_lds = (size_t)M * BLOCK * 16 + 2 * (BLOCK / 64) * 32 * sizeof(float) + 2 * 32 * sizeof(float);
    if constexpr (sizeof(T) == 4 && vz32_lds <= 160 * 1024) {
        if (P.vz_mode && P.sched) {
            auto k = ps_vz32_kernel<BLOCK, M>;
            (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)vz32_lds);
            hipLaunchKernelGGL(k, dim3(P.nk), dim3(BLOCK), vz32_lds, st, P);
            t_ps_kernel = "ps_vz32_kernel";
            return;
        }
    }
    constexpr size_t vz64_lds = (size_t)M * BLOCK * 8 + 2 * (BLOCK / 64) * 32 * sizeof(double) + 2 * 32 * sizeof(double);
    if constexpr (sizeof(T) == 8 && vz64_lds <= 160 * 1024 && M <= 16) {
        if (P.vz_mode && P.sched && P.eps) {
            auto k = ps_vz64_kernel<BLOCK, M>;
            (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)vz64_lds);
            hipLaunchKernelGGL(k, dim3(P.nk), dim3(BLOCK), vz64_lds, st, P);
            t_ps_kernel = "ps_vz64_kernel";
            return;
        }
    }
    t_ps_kernel = P.vz_mode ? "ps_kernel (per step)" : "ps_kernel (constant velocity)";
    if (P.vz_mode)
        hipLaunchKernelGGL((ps_kernel<T, BLOCK, M, true>), dim3(P.nk), dim3(BLOCK), 0, st, P);
    else
        hipLaunchKernelGGL((ps_kernel<T, BLOCK, M, false>), dim3(P.nk), dim3(BLOCK), 0, st, P);
}

template <typename T>
static int ps_dispatch(const PsParams &P, hipStream_t st)
{
    const int nt = P.nf;                // frequency slots per wavenumber (half of the padded samples in a Hermitian walk)
    // Workgroup shape.  "deep": 16 frequencies per lane and as few waves as that takes (the reduce-scatter and the
    // tile barrier are a fixed cost per wave and tile, the rotate-accumulate body scales with the frequencies per
    // lane; smaller workgroups also put two or more on a CU, so one's barrier wait overlaps another's body).
    // "wide": 512 threads as soon as there are 512 frequencies (round 1-2 shape).
    // Measured at 8192^2 with the half walk (4096 frequencies per wavenumber; profiles/r03_ps_shapes.txt): float32 constant
    // v 35.0 (wide) / 41.6 (deep) ms, v(z) 43.4 / 44.9; float64 constant v 63.6 / 56.8, v(z) 72.6 / 70.7.
    const bool deep = sizeof(T) == 8;
    if (nt <= 64) ps_launch<T, 64, 1>(P, st);
    else if (nt <= 128) ps_launch<T, 128, 1>(P, st);
    else if (nt <= 256) ps_launch<T, 256, 1>(P, st);
    else if (nt <= 512) ps_launch<T, 512, 1>(P, st);
    else if (nt <= 1024) { if (deep) ps_launch<T, 64, 16>(P, st); else ps_launch<T, 512, 2>(P, st); }
    else if (nt <= 2048) { if (deep) ps_launch<T, 128, 16>(P, st); else ps_launch<T, 512, 4>(P, st); }
    else if (nt <= 4096) { if (deep) ps_launch<T, 256, 16>(P, st); else ps_launch<T, 512, 8>(P, st); }
    else if (nt <= 8192) ps_launch<T, 512, 16>(P, st);     // (1024 x 8 for the float32 v(z) runs kernel: 33 spilled VGPRs, 12 % slower)
    else if (nt <= 16384) ps_launch<T, 512, 32>(P, st);
    else {
        impdar_set_error("phase-shift kernel supports up to 16384 frequencies per wavenumber (got %d)", nt);
        return IMPDAR_ERR_UNSUPPORTED;
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}
