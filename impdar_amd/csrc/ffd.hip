// ===========================================================================
// 2-D v(x,z): Fourier finite-difference branch of phaseShift
// (mig_python.py:428-432, 448-487; fourierFiniteDiff :496-525; Sp_Matr :528-540)
//
// The reference keeps ONE FFX_last for the whole (tau, omega) nest (:478): the update of
// frequency iw uses the field of frequency iw-1 (and of the last frequency of the previous tau
// at iw = 0), so the nest is a single serial chain of snum*nt steps, each with a length-tnum
// inverse and forward FFT over the traces.  That order is reproduced literally: per step
//   [post of the previous step + retardation phase of this row]  ->  rocFFT inverse (row, in place)
//   ->  [thin-lens phase + finite-difference update, one workgroup]  ->  rocFFT forward (into the row).
// float64 throughout, operation order of the reference (the file is compiled with
// -ffp-contract=off).  Arrays are (row = frequency, column = trace), traces contiguous.
// ===========================================================================
#include "ps_layout.h"      // Cp; fft.h: FftPlan, DevBuf, impdar_taper_w
#include <algorithm>

typedef Cp<double> Cd;

__device__ inline Cd cmul(Cd a, Cd b) { return Cd{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// (snum,tnum) real -> tapered (:253-258), zero padded to nt rows, complex
__global__ __launch_bounds__(256) void ffd_load(const double *__restrict__ in, Cd *__restrict__ X, int snum, int tnum,
                                                int nt, double htaper, double vtaper)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nt * tnum) return;
    const int k = (int)(i / tnum), j = (int)(i % tnum);
    double v = 0.0;
    if (k < snum) v = in[i] * (impdar_taper_w(j, tnum, htaper) * impdar_taper_w(k, snum, vtaper));
    X[i] = Cd{v, 0.0};
}

struct FfdStep {
    Cd *FK;              // (nt, tnum)
    Cd *TK;              // (snum, tnum)
    const double *kx;    // (tnum)
    const double *vmig;  // (snum, tnum)
    const double *vbg;   // (snum) min over traces
    const double *thr;   // (snum) (tau / tt[-1] / 1e6)^2, :484
    int tnum;
    // "post" half: row post_iw of step (post_itau): zero evanescent columns, accumulate into TK
    int post_itau, post_iw;
    double post_w;
    // "pre" half: retardation phase of row pre_iw at depth step pre_itau
    int pre_itau, pre_iw;
    double pre_w;
    double dt;
};

__device__ inline double ffd_coss(double vbg, double kx, double w)
{
    const double a = 0.5 * vbg * kx / w;          // :456
    return 1.0 - a * a;
}

__global__ __launch_bounds__(256) void ffd_post_pre(FfdStep P)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P.tnum) return;
    if (P.post_iw >= 0) {
        Cd *row = P.FK + (size_t)P.post_iw * P.tnum;
        const double coss = ffd_coss(P.vbg[P.post_itau], P.kx[k], P.post_w);
        Cd v = row[k];
        if (coss <= P.thr[P.post_itau]) {          // :484-485 (sticky: written back)
            v = Cd{0.0, 0.0};
            row[k] = v;
        }
        Cd *t = P.TK + (size_t)P.post_itau * P.tnum + k;   // :487
        t->x += v.x;
        t->y += v.y;
    }
    if (P.pre_iw >= 0) {
        Cd *row = P.FK + (size_t)P.pre_iw * P.tnum;
        const double coss = ffd_coss(P.vbg[P.pre_itau], P.kx[k], P.pre_w);
        // phase = (-w dt sqrt(coss)).real with a complex sqrt: 0 for coss < 0 (:458-460)
        const double root = coss >= 0.0 ? sqrt(coss) : 0.0;
        const double phase = -P.pre_w * P.dt * root;
        double sn, cs;
        sincos(phase, &sn, &cs);
        row[k] = cmul(row[k], Cd{cs, -sn});        // conj(cos + i sin), :461-464
    }
}

struct FfdMid {
    const Cd *row;       // ifft of FK[iw] (tnum)
    const Cd *last;      // FFX_last (tnum)
    Cd *next;            // FFX of this step (tnum): becomes FFX_last and the forward FFT's input
    const double *vmig;  // row itau of (snum, tnum)
    double vbg, w, dt, dx;
    int tnum, first;     // first: itau == 0 (no finite-difference term, :475)
};

// one workgroup: the last stencil row is a sum over all traces
__global__ __launch_bounds__(256) void ffd_mid(FfdMid P)
{
    extern __shared__ Cd sm[];          // thin-lensed field (tnum) + 2 x 256 partial sums
    Cd *fx = sm;
    Cd *part = sm + P.tnum;
    const int tid = threadIdx.x, n = P.tnum;
    Cd sf = {0.0, 0.0}, sl = {0.0, 0.0};
    for (int x = tid; x < n; x += 256) {
        const double v = P.vmig[x];
        const double ufg = 1. / v - 1. / P.vbg;                            // :453
        const double phase2 = 2. * ufg * P.w * P.dt + 1. * P.vbg * P.w * P.dt;   // :471
        double sn, cs;
        sincos(phase2, &sn, &cs);
        const Cd f = cmul(P.row[x], Cd{cs, sn});                           // :472-473
        fx[x] = f;
        sf.x += f.x;
        sf.y += f.y;
        if (!P.first) {
            sl.x += P.last[x].x;
            sl.y += P.last[x].y;
        }
    }
    part[tid] = sf;
    part[256 + tid] = sl;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            part[tid].x += part[tid + s].x;
            part[tid].y += part[tid + s].y;
            part[256 + tid].x += part[256 + tid + s].x;
            part[256 + tid].y += part[256 + tid + s].y;
        }
        __syncthreads();
    }
    const Cd sumf = part[0], suml = part[256];
    for (int x = tid; x < n; x += 256) {
        Cd out = fx[x];
        if (!P.first) {
            // stencil = Sp_Matr(N,-2,1,1) as built: zero main diagonal (:533 overwrites it), row 0 = e0,
            // last row all ones (:536-539)
            Cd a, b;
            if (x == 0) {
                a = fx[0];
                b = P.last[0];
            } else if (x == n - 1) {
                a = sumf;
                b = suml;
            } else {
                a = Cd{fx[x - 1].x + fx[x + 1].x, fx[x - 1].y + fx[x + 1].y};
                b = Cd{P.last[x - 1].x + P.last[x + 1].x, P.last[x - 1].y + P.last[x + 1].y};
            }
            const double vs = P.vmig[x] - P.vbg;                           // :452
            const double num = P.dt * 0.5 * (vs * vs);                     // dt*alpha*vs**2, alpha = 0.5
            const double den = 4. * P.w * (P.dx * P.dx);                   // imaginary part of 1j*4.*w*dx**2
            // real / (0 + i den) the way NumPy divides complex numbers (Smith: scale by 1/den), :517
            const double scl = 1.0 / den;
            const Cd c1 = {0.0, (0.0 - num) * scl};
            const double c2 = (-0.25 * (vs * vs)) / (4. * (P.w * P.w) * (P.dx * P.dx));   // :518
            const Cd t1 = cmul(c1, a);
            const Cd d = {a.x - b.x, a.y - b.y};
            const Cd l = P.last[x];
            out = Cd{(l.x + t1.x) + c2 * d.x, (l.y + t1.y) + c2 * d.y};   // :521
        }
        P.next[x] = out;
    }
}

// ---------------------------------------------------------------------------
// The whole (tau, omega) chain in ONE workgroup (power-of-two trace counts up to 512).  The chain is serial by the
// reference's construction (one FFX_last for the whole nest), each step touches one row of tnum complex numbers,
// and issued as four launches per step it costs ~26 us a step, all of it launch / enqueue overhead.  Here the
// row lives in LDS for the whole step: retardation phase on load, inverse FFT over the traces (radix-4 Stockham,
// float64, twiddles from a table built on the host), thin-lens phase and finite-difference update against the
// FFX_last kept in LDS, forward FFT, evanescent zeroing, row written back; the sums into TK[itau] stay in
// registers over the frequencies of a depth step.  Same element formulas, in the same operation order, as
// ffd_post_pre / ffd_mid above; the transforms are its own instead of rocFFT's (rounding-level differences).
// LDS: four rows (two transform buffers, FFX_last, the thin-lensed field) + the twiddles = 4.5 tnum x 16 B.
// ---------------------------------------------------------------------------
struct FfdChain {
    Cd *FK;              // (nt, tnum) spectrum, updated in place
    Cd *TK;              // (snum, tnum)
    const double *kx;    // (tnum)
    const double *vmig;  // (snum, tnum)
    const double *vbg;   // (snum)
    const double *thr;   // (snum)
    const double *w;     // (nt), zero frequency already replaced
    const Cd *tw;        // (tnum / 2) exp(-2 pi i k / tnum)
    int tnum, snum, nt;
    double dt, dx;
};

// Stockham autosort transform of n (a power of two) points between two LDS buffers: radix-4 passes, one radix-2
// pass at the end when log2 n is odd (every pass is one barrier; with a handful of waves the barriers are most of
// a pass).  W[m] = exp(-2 pi i m / n), m < n / 2.  Returns the buffer that holds the result.
template <bool INV>
__device__ __forceinline__ Cd *ffd_fft_lds(Cd *in, Cd *out, const Cd *W, int n, int tid, int nthr)
{
    const int half = n >> 1, quarter = n >> 2;
    auto twiddle = [&](int m) {             // exp(-+ 2 pi i m / n) for m < n
        Cd t = W[m < half ? m : m - half];
        if (m >= half) t = Cd{-t.x, -t.y};
        if (INV) t.y = -t.y;
        return t;
    };
    int Ns = 1;
    for (; Ns * 4 <= n; Ns <<= 2) {
        const int wstep = quarter / Ns;
        for (int j = tid; j < quarter; j += nthr) {
            const int k = j & (Ns - 1);
            const int m1 = k * wstep;
            const Cd v0 = in[j];
            const Cd v1 = cmul(in[j + quarter], twiddle(m1));
            const Cd v2 = cmul(in[j + 2 * quarter], twiddle(2 * m1));
            const Cd v3 = cmul(in[j + 3 * quarter], twiddle(3 * m1));
            const Cd t0 = {v0.x + v2.x, v0.y + v2.y}, t1 = {v0.x - v2.x, v0.y - v2.y};
            const Cd t2 = {v1.x + v3.x, v1.y + v3.y};
            const Cd d = {v1.x - v3.x, v1.y - v3.y};
            const Cd t3 = INV ? Cd{-d.y, d.x} : Cd{d.y, -d.x};      // (v1 - v3) times +i / -i
            const int j0 = ((j - k) << 2) + k;
            out[j0] = Cd{t0.x + t2.x, t0.y + t2.y};
            out[j0 + Ns] = Cd{t1.x + t3.x, t1.y + t3.y};
            out[j0 + 2 * Ns] = Cd{t0.x - t2.x, t0.y - t2.y};
            out[j0 + 3 * Ns] = Cd{t1.x - t3.x, t1.y - t3.y};
        }
        __syncthreads();
        Cd *sw = in;
        in = out;
        out = sw;
    }
    if (Ns < n) {                           // Ns == n / 2
        for (int j = tid; j < half; j += nthr) {
            const int k = j & (Ns - 1);
            const Cd a = in[j], b = cmul(in[j + half], twiddle(k));      // angle -2 pi k / (2 Ns) = -2 pi k / n
            const int j0 = ((j - k) << 1) + k;
            out[j0] = Cd{a.x + b.x, a.y + b.y};
            out[j0 + Ns] = Cd{a.x - b.x, a.y - b.y};
        }
        __syncthreads();
        Cd *sw = in;
        in = out;
        out = sw;
    }
    return in;
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void ffd_chain_kernel(FfdChain P)
{
    extern __shared__ Cd sm[];
    const int n = P.tnum, tid = threadIdx.x;
    Cd *A = sm, *B = sm + n, *L = sm + 2 * n, *F = sm + 3 * n, *W = sm + 4 * n;
    Cd *part = W + (n >> 1);                 // 2 x (BLOCK / 64) partial sums
    constexpr int NW = BLOCK / 64;
    constexpr int EPT = 2;                   // BLOCK >= tnum / 2
    const double inv_n = 1.0 / n;
    for (int x = tid; x < n; x += BLOCK) L[x] = Cd{0.0, 0.0};
    for (int k = tid; k < (n >> 1); k += BLOCK) W[k] = P.tw[k];
    __syncthreads();
    for (int itau = 0; itau < P.snum; ++itau) {
        const double vbg = P.vbg[itau], thr = P.thr[itau];
        const double *vm = P.vmig + (size_t)itau * n;
        // what a depth step's frequencies share, per owned trace / wavenumber (the same expressions, evaluated once)
        Cd tk[EPT];
        double kxe[EPT], ufg[EPT], vs2[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int x = tid + e * BLOCK;
            tk[e] = Cd{0.0, 0.0};
            kxe[e] = x < n ? P.kx[x] : 0.0;
            const double v = x < n ? vm[x] : vbg;
            ufg[e] = 1. / v - 1. / vbg;                                            // :453
            const double vs = v - vbg;                                             // :452
            vs2[e] = vs * vs;
        }
        for (int iw = 0; iw < P.nt; ++iw) {
            const double w = P.w[iw];
            Cd *row = P.FK + (size_t)iw * n;
            // retardation phase (:456-464); coss is needed again after the forward transform (:484)
            double coss[EPT];
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int k = tid + e * BLOCK;
                coss[e] = ffd_coss(vbg, kxe[e], w);
                if (k < n) {
                    const double root = coss[e] >= 0.0 ? sqrt(coss[e]) : 0.0;
                    const double phase = -w * P.dt * root;
                    double sn, cs;
                    sincos(phase, &sn, &cs);
                    A[k] = cmul(row[k], Cd{cs, -sn});
                }
            }
            __syncthreads();
            Cd *R = ffd_fft_lds<true>(A, B, W, n, tid, BLOCK);          // :467, unscaled
            Cd *S = R == A ? B : A;
            // thin-lens term (:470-473) and the sums the last stencil row needs
            Cd sf = {0.0, 0.0}, sl = {0.0, 0.0};
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int x = tid + e * BLOCK;
                if (x < n) {
                    const double phase2 = 2. * ufg[e] * w * P.dt + 1. * vbg * w * P.dt;   // :471
                    double sn, cs;
                    sincos(phase2, &sn, &cs);
                    const Cd r = {R[x].x * inv_n, R[x].y * inv_n};
                    const Cd f = cmul(r, Cd{cs, sn});
                    F[x] = f;
                    sf.x += f.x;
                    sf.y += f.y;
                    if (itau > 0) {
                        sl.x += L[x].x;
                        sl.y += L[x].y;
                    }
                }
            }
#pragma unroll
            for (int msk = 32; msk > 0; msk >>= 1) {
                sf.x += __shfl_xor(sf.x, msk, 64);
                sf.y += __shfl_xor(sf.y, msk, 64);
                sl.x += __shfl_xor(sl.x, msk, 64);
                sl.y += __shfl_xor(sl.y, msk, 64);
            }
            if ((tid & 63) == 0) {
                part[tid >> 6] = sf;
                part[NW + (tid >> 6)] = sl;
            }
            __syncthreads();
            Cd sumf = {0.0, 0.0}, suml = {0.0, 0.0};
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                sumf.x += part[q].x;
                sumf.y += part[q].y;
                suml.x += part[NW + q].x;
                suml.y += part[NW + q].y;
            }
            // finite-difference update (:496-525) -> S
            const double den = 4. * w * (P.dx * P.dx);                   // imaginary part of 1j*4.*w*dx**2
            const double scl = 1.0 / den;                                // real / (0 + i den), NumPy's way (:517)
            const double den2 = 4. * (w * w) * (P.dx * P.dx);
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int x = tid + e * BLOCK;
                if (x < n) {
                    Cd out = F[x];
                    if (itau > 0) {
                        Cd a, b;
                        if (x == 0) {
                            a = F[0];
                            b = L[0];
                        } else if (x == n - 1) {
                            a = sumf;
                            b = suml;
                        } else {
                            a = Cd{F[x - 1].x + F[x + 1].x, F[x - 1].y + F[x + 1].y};
                            b = Cd{L[x - 1].x + L[x + 1].x, L[x - 1].y + L[x + 1].y};
                        }
                        const double num = P.dt * 0.5 * vs2[e];                    // dt*alpha*vs**2, alpha = 0.5
                        const Cd c1 = {0.0, (0.0 - num) * scl};
                        const double c2 = (-0.25 * vs2[e]) / den2;                 // :518
                        const Cd t1 = cmul(c1, a);
                        const Cd d = {a.x - b.x, a.y - b.y};
                        const Cd l = L[x];
                        out = Cd{(l.x + t1.x) + c2 * d.x, (l.y + t1.y) + c2 * d.y};   // :521
                    }
                    S[x] = out;
                }
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int x = tid + e * BLOCK;
                if (x < n) L[x] = S[x];                                            // FFX_last = FFX, :478
            }
            Cd *Q = ffd_fft_lds<false>(S, R, W, n, tid, BLOCK);                   // :481
            // zero outside the domain, accumulate, keep the row (:484-487)
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int k = tid + e * BLOCK;
                if (k < n) {
                    Cd v = Q[k];
                    if (coss[e] <= thr) v = Cd{0.0, 0.0};
                    row[k] = v;
                    tk[e].x += v.x;
                    tk[e].y += v.y;
                }
            }
            // the next load writes A[k] for the same k this thread just read from Q: no barrier needed before it,
            // and its own barrier comes before anyone reads a neighbour's element
        }
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int k = tid + e * BLOCK;
            if (k < n) P.TK[(size_t)itau * n + k] = tk[e];
        }
    }
}

// TK (snum,tnum) complex -> out (snum,tnum) real: ifft over the traces done by rocFFT, /snum here (:491)
__global__ __launch_bounds__(256) void ffd_real_out(const Cd *__restrict__ Z, double *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = Z[i].x;
}

__global__ __launch_bounds__(256) void ffd_scale(Cd *__restrict__ Z, size_t n, double div)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        Z[i].x /= div;
        Z[i].y /= div;
    }
}

// the end of both forms: TK (snum,tnum) / snum (:491), ifft over the traces (:282), real part, download
static int ffd_finish(impdar_ctx *ctx, DevBuf &TK, FftPlan &tk_inv, DevBuf &dout, double *out, size_t nreal, int snum, const char *kernel)
{
    hipStream_t st = ctx->stream;
    int rc;
    const unsigned gtk = (unsigned)((nreal + 255) / 256);
    hipLaunchKernelGGL(ffd_scale, dim3(gtk), dim3(256), 0, st, TK.as<Cd>(), nreal, (double)snum);
    if ((rc = tk_inv.exec(TK.p, nullptr))) return rc;
    hipLaunchKernelGGL(ffd_real_out, dim3(gtk), dim3(256), 0, st, TK.as<Cd>(), dout.as<double>(), nreal);
    IMPDAR_HIP_CHECK(hipGetLastError());
    IMPDAR_HIP_CHECK(hipMemcpyAsync(out, dout.p, nreal * 8, hipMemcpyDeviceToHost, st));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(st));
    impdar_ctx_note(ctx, "impdar_phaseshift_ffd", kernel);
    return IMPDAR_OK;
}

extern "C" int impdar_phaseshift_ffd(impdar_ctx *ctx, const double *data, int snum, int tnum, int nt, const double *kx,
                                     const double *ws, double dt, const double *tt_us, const double *vmig2d,
                                     double dx_mean, double htaper, double vtaper, double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && out && kx && ws && tt_us && vmig2d, "null argument");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 2 && nt >= snum, "bad sizes snum %d tnum %d nt %d", snum, tnum, nt);
    IMPDAR_ARG_CHECK((size_t)tnum * 16 + 2 * 256 * 16 <= 150 * 1024, "the finite-difference step keeps a trace row in LDS: "
                     "tnum %d is above its 9000-trace limit", tnum);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nreal = (size_t)snum * tnum;
    DevBuf din, dout, X, TK, L, N, d_kx, d_vm, d_vbg, d_thr;
    IMPDAR_HIP_CHECK(din.ensure(nreal * 8));
    IMPDAR_HIP_CHECK(dout.ensure(nreal * 8));
    IMPDAR_HIP_CHECK(X.ensure((size_t)nt * tnum * 16));
    IMPDAR_HIP_CHECK(TK.ensure(nreal * 16));
    IMPDAR_HIP_CHECK(L.ensure((size_t)tnum * 16));
    IMPDAR_HIP_CHECK(N.ensure((size_t)tnum * 16));
    IMPDAR_HIP_CHECK(d_kx.ensure((size_t)tnum * 8));
    IMPDAR_HIP_CHECK(d_vm.ensure(nreal * 8));
    IMPDAR_HIP_CHECK(d_vbg.ensure((size_t)snum * 8));
    IMPDAR_HIP_CHECK(d_thr.ensure((size_t)snum * 8));
    std::vector<double> w(ws, ws + nt), thr(snum), vbg(snum);
    for (int i = 0; i < nt; ++i)
        if (w[i] == 0.0) w[i] = 1.0e-10 / dt;                            // :445-447
    for (int i = 0; i < snum; ++i) {
        const double tau = tt_us[i] / 1.0e6;
        const double r = tau / tt_us[snum - 1] / 1e6;                    // :484
        thr[i] = r * r;
        double m = vmig2d[(size_t)i * tnum];
        for (int j = 1; j < tnum; ++j) m = std::min(m, vmig2d[(size_t)i * tnum + j]);   // :450
        vbg[i] = m;
    }
    IMPDAR_HIP_CHECK(hipMemcpyAsync(din.p, data, nreal * 8, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(d_kx.p, kx, (size_t)tnum * 8, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(d_vm.p, vmig2d, nreal * 8, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(d_vbg.p, vbg.data(), (size_t)snum * 8, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(d_thr.p, thr.data(), (size_t)snum * 8, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemsetAsync(TK.p, 0, nreal * 16, st));
    IMPDAR_HIP_CHECK(hipMemsetAsync(L.p, 0, (size_t)tnum * 16, st));

    const rocfft_array_type ci = rocfft_array_type_complex_interleaved;
    FftPlan f_x, f_t, row_inv, row_fwd, tk_inv;
    int rc;
    // fft2(data, (nt, tnum)) (:270): over the traces (contiguous), then over time (stride tnum)
    if ((rc = f_x.create(rocfft_transform_type_complex_forward, true, true, tnum, nt, ci, ci, 1, tnum, 1, tnum, 1.0, st))) return rc;
    if ((rc = f_t.create(rocfft_transform_type_complex_forward, true, true, nt, tnum, ci, ci, tnum, 1, tnum, 1, 1.0, st))) return rc;
    if ((rc = row_inv.create(rocfft_transform_type_complex_inverse, true, true, tnum, 1, ci, ci, 1, tnum, 1, tnum, 1.0 / tnum, st))) return rc;
    if ((rc = row_fwd.create(rocfft_transform_type_complex_forward, true, false, tnum, 1, ci, ci, 1, tnum, 1, tnum, 1.0, st))) return rc;
    if ((rc = tk_inv.create(rocfft_transform_type_complex_inverse, true, true, tnum, snum, ci, ci, 1, tnum, 1, tnum, 1.0 / tnum, st))) return rc;

    const unsigned gall = (unsigned)(((size_t)nt * tnum + 255) / 256);
    hipLaunchKernelGGL(ffd_load, dim3(gall), dim3(256), 0, st, din.as<double>(), X.as<Cd>(), snum, tnum, nt, htaper, vtaper);
    if ((rc = f_x.exec(X.p, nullptr))) return rc;
    if ((rc = f_t.exec(X.p, nullptr))) return rc;

    // power-of-two trace counts up to 512: the whole chain in one persistent workgroup (IMPDAR_FFD_CHAIN=0 keeps the
    // launch-per-step form below, which also serves every other trace count).  Measured us per step, one workgroup /
    // launch per step (the latter varies by box): 64 traces 4.5 / 11-17, 128 traces 5.4 / 12-15, 512 traces 8.2 / 12.4-17.5,
    // 1024 traces 19 / 18.5-20, 2048 traces 37 / 28 -- one CU does all of a step's float64 sincos and butterflies and
    // the barriers of a wider workgroup cost more (one trace per thread: 28 us at 1024; four per thread: 11.8 us at 512),
    // so the wide rows stay with the spread-out form.
    const bool pow2 = tnum >= 2 && tnum <= 512 && (tnum & (tnum - 1)) == 0;
    const char *ce = getenv("IMPDAR_FFD_CHAIN");
    if (pow2 && !(ce && ce[0] == '0')) {
        DevBuf d_w, d_tw;
        IMPDAR_HIP_CHECK(d_w.ensure((size_t)nt * 8));
        IMPDAR_HIP_CHECK(d_tw.ensure((size_t)(tnum / 2) * 16));
        std::vector<Cd> twid(tnum / 2);
        for (int k = 0; k < tnum / 2; ++k) {
            const long double ang = -2.0L * 3.141592653589793238462643383279502884L * (long double)k / (long double)tnum;
            twid[k] = Cd{(double)cosl(ang), (double)sinl(ang)};
        }
        IMPDAR_HIP_CHECK(hipMemcpyAsync(d_w.p, w.data(), (size_t)nt * 8, hipMemcpyHostToDevice, st));
        IMPDAR_HIP_CHECK(hipMemcpyAsync(d_tw.p, twid.data(), twid.size() * 16, hipMemcpyHostToDevice, st));
        FfdChain C;
        C.FK = X.as<Cd>();
        C.TK = TK.as<Cd>();
        C.kx = d_kx.as<double>();
        C.vmig = d_vm.as<double>();
        C.vbg = d_vbg.as<double>();
        C.thr = d_thr.as<double>();
        C.w = d_w.as<double>();
        C.tw = d_tw.as<Cd>();
        C.tnum = tnum, C.snum = snum, C.nt = nt;
        C.dt = dt, C.dx = dx_mean;
        const int block = std::max(64, tnum / 2);
        const size_t lds = ((size_t)tnum * 4 + tnum / 2 + 2 * (block / 64)) * 16;
        auto launch = [&](auto kern) {
            (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, dim3(1), dim3(block), lds, st, C);
        };
        switch (block) {
        case 64: launch(ffd_chain_kernel<64>); break;
        case 128: launch(ffd_chain_kernel<128>); break;
        case 256: launch(ffd_chain_kernel<256>); break;
        case 512: launch(ffd_chain_kernel<512>); break;
        default: launch(ffd_chain_kernel<1024>); break;
        }
        IMPDAR_HIP_CHECK(hipGetLastError());
        return ffd_finish(ctx, TK, tk_inv, dout, out, nreal, snum, "ffd_chain_kernel");      // (the staging vectors above live until its sync)
    }

    FfdStep S;
    S.FK = X.as<Cd>();
    S.TK = TK.as<Cd>();
    S.kx = d_kx.as<double>();
    S.vmig = d_vm.as<double>();
    S.vbg = d_vbg.as<double>();
    S.thr = d_thr.as<double>();
    S.tnum = tnum;
    S.dt = dt;
    S.post_iw = -1;
    S.post_itau = 0;
    S.post_w = 1.0;
    const unsigned grow = (unsigned)((tnum + 255) / 256);
    const size_t mid_lds = ((size_t)tnum + 512) * 16;
    IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)ffd_mid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mid_lds));
    Cd *last = L.as<Cd>(), *next = N.as<Cd>();
    for (int itau = 0; itau < snum; ++itau)
        for (int iw = 0; iw < nt; ++iw) {
            S.pre_itau = itau;
            S.pre_iw = iw;
            S.pre_w = w[iw];
            hipLaunchKernelGGL(ffd_post_pre, dim3(grow), dim3(256), 0, st, S);
            Cd *row = X.as<Cd>() + (size_t)iw * tnum;
            if ((rc = row_inv.exec(row, nullptr))) return rc;                       // :467
            FfdMid M;
            M.row = row;
            M.last = last;
            M.next = next;
            M.vmig = d_vm.as<double>() + (size_t)itau * tnum;
            M.vbg = vbg[itau];
            M.w = w[iw];
            M.dt = dt;
            M.dx = dx_mean;
            M.tnum = tnum;
            M.first = itau == 0;
            hipLaunchKernelGGL(ffd_mid, dim3(1), dim3(256), mid_lds, st, M);
            if ((rc = row_fwd.exec(next, row))) return rc;                          // :481
            std::swap(last, next);                                                   // FFX_last = FFX, :478
            S.post_itau = itau;
            S.post_iw = iw;
            S.post_w = w[iw];
        }
    S.pre_iw = -1;
    hipLaunchKernelGGL(ffd_post_pre, dim3(grow), dim3(256), 0, st, S);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return ffd_finish(ctx, TK, tk_inv, dout, out, nreal, snum, "ffd_post_pre + rocFFT + ffd_mid per (step, frequency)");
}
