// The plan of the library's own mixed-radix row transforms (own_fft_mixed.h): which lengths they take, the passes of a length
// and every piece of index arithmetic of the kernel -- plain C++, for the host-only tests too (the kernel calls these same
// helpers; tests/test_fft_mixed_plan.py runs them on a host array against numpy.fft).
//
// Decimation in frequency, in place.  A pass of radix r over spans of L = r q points: butterfly b = g q + j (group g, offset
// j < q) takes the points base + c q (base = g L + j, c < r), forms their length-r transform, multiplies output c by
// e^{-2 pi i j c / L} -- entry j c (M / L) of the table e^{-2 pi i k / M}: j c < L, so the index stays below M -- and stores it
// at base + c q; the next pass works on spans of q.  Output index k ends up at the position whose digits, most significant
// first, are the digits of k, least significant first, in the radices in pass order.
#pragma once
#include <initializer_list>

#if defined(__HIPCC__)
#define OWN_MIXED_HD __host__ __device__ inline
#else
#define OWN_MIXED_HD inline
#endif

enum { OWN_MIXED_MAX_PASSES = 8 };       // 3^8 = 6561 <= 8192 < 2 * 3^8: no length has more factors (a pair of 2s is one radix 4)

// complex length M the mixed-radix kernel takes: 16 ... 8192 (the LDS of a float64 row of 8192), no prime factor above 7
static inline bool own_fft_mixed_len_ok(long long m)
{
    if (m < 16 || m > 8192) return false;
    for (int p : {2, 3, 5, 7})
        while (m % p == 0) m /= p;
    return m == 1;
}

struct OwnMixedPlan {
    int M = 0, np = 0;
    int radix[OWN_MIXED_MAX_PASSES];     // pass p: butterflies of radix[p] points, q[p] apart, in spans of radix[p] * q[p]
    int q[OWN_MIXED_MAX_PASSES];
    int tstep[OWN_MIXED_MAX_PASSES];     // M / span: the step of the pass in the table e^{-2 pi i k / M}
};

// The passes of M: radix 4 while two factors 2 are left, one radix 2, then 3s, 5s and 7s -- the odd radices last: in the passes
// of small q a lane's points lie r complex numbers from its neighbour's, and an odd r spreads them over the LDS banks where
// 4 puts every eighth lane on one.  false (np = 0) for a length own_fft_mixed_len_ok refuses.
static inline bool own_mixed_plan_make(int M, OwnMixedPlan &pl)
{
    pl.M = M;
    pl.np = 0;
    if (!own_fft_mixed_len_ok(M)) return false;
    int rest = M, span = M;
    for (int r : {4, 2, 3, 5, 7})
        while (rest % r == 0) {
            pl.radix[pl.np] = r;
            pl.q[pl.np] = span / r;
            pl.tstep[pl.np] = M / span;
            span /= r;
            rest /= r;
            ++pl.np;
        }
    return true;
}

// butterflies of pass p: M / radix[p], b = g q + j
OWN_MIXED_HD int own_mixed_count(const OwnMixedPlan &pl, int p) { return pl.M / pl.radix[p]; }
OWN_MIXED_HD int own_mixed_group(const OwnMixedPlan &pl, int p, int b) { return b / pl.q[p]; }
// first point of butterfly b (group g): g L + j; its points are base + c q[p]
OWN_MIXED_HD int own_mixed_base(const OwnMixedPlan &pl, int p, int b, int g) { return g * (pl.radix[p] - 1) * pl.q[p] + b; }
OWN_MIXED_HD int own_mixed_offset(const OwnMixedPlan &pl, int p, int b, int g) { return b - g * pl.q[p]; }
// table index of the twiddle of output c of a butterfly at offset j: j c (M / L), times the stride tws of the length-M
// twiddles in the table (2 in the table of a real transform of 2 M points)
OWN_MIXED_HD int own_mixed_twiddle(const OwnMixedPlan &pl, int p, int j, int c, int tws) { return j * c * pl.tstep[p] * tws; }

// k / r and k % r for the radices of a plan (constant divisors: a multiplication each)
OWN_MIXED_HD int own_mixed_divmod(int k, int r, int &rem)
{
    int d;
    switch (r) {
    case 2: d = k >> 1; rem = k & 1; break;
    case 4: d = k >> 2; rem = k & 3; break;
    case 3: d = k / 3; rem = k - 3 * d; break;
    case 5: d = k / 5; rem = k - 5 * d; break;
    default: d = k / 7; rem = k - 7 * d; break;
    }
    return d;
}

// position of output index k after the in-place passes (the mixed-radix digit reversal)
OWN_MIXED_HD int own_mixed_pos(const OwnMixedPlan &pl, int k)
{
    int pos = 0;
    for (int p = 0; p < pl.np; ++p) {
        int digit;
        k = own_mixed_divmod(k, pl.radix[p], digit);
        pos += digit * pl.q[p];
    }
    return pos;
}

#ifndef __HIPCC__
#include <complex>
#include <vector>
// The passes on a host array of M complex numbers, with the helpers above: s is left in the kernel's order (index k at
// own_mixed_pos(k)).  tab: e^{-2 pi i k / M}, k < M; inv: the conjugate transform (no 1 / M).
template <typename R>
static void own_mixed_passes_host(const OwnMixedPlan &pl, std::complex<R> *s, const std::complex<R> *tab, bool inv)
{
    typedef std::complex<R> Cp;
    auto W = [&](int idx) { return inv ? std::conj(tab[idx]) : tab[idx]; };
    for (int p = 0; p < pl.np; ++p) {
        const int r = pl.radix[p], q = pl.q[p];
        for (int b = 0; b < own_mixed_count(pl, p); ++b) {
            const int g = own_mixed_group(pl, p, b), j = own_mixed_offset(pl, p, b, g), base = own_mixed_base(pl, p, b, g);
            Cp x[7], y[7];
            for (int c = 0; c < r; ++c) x[c] = s[base + c * q];
            for (int c = 0; c < r; ++c) {
                Cp acc = 0;
                for (int a = 0; a < r; ++a) acc += x[a] * W((a * c) % r * (pl.M / r));
                y[c] = acc * W(own_mixed_twiddle(pl, p, j, c, 1));
            }
            for (int c = 0; c < r; ++c) s[base + c * q] = y[c];
        }
    }
}
#endif

#ifdef OWN_FFT_MIXED_PROBE
// what tests/test_fft_mixed_plan.py calls
#include <cmath>
extern "C" int impdar_own_mixed_len_ok(long long m) { return own_fft_mixed_len_ok(m) ? 1 : 0; }
// the radices of M in pass order into radix[OWN_MIXED_MAX_PASSES]: how many, 0 for a length that is refused
extern "C" int impdar_own_mixed_radices(int M, int *radix)
{
    OwnMixedPlan pl;
    if (!own_mixed_plan_make(M, pl)) return 0;
    for (int p = 0; p < pl.np; ++p) radix[p] = pl.radix[p];
    return pl.np;
}
extern "C" int impdar_own_mixed_positions(int M, int *pos)
{
    OwnMixedPlan pl;
    if (!own_mixed_plan_make(M, pl)) return 1;
    for (int k = 0; k < M; ++k) pos[k] = own_mixed_pos(pl, k);
    return 0;
}
// in, out: M complex numbers as (re, im) pairs of float64; the unnormalised transform, forward or (inv) conjugate
extern "C" int impdar_own_mixed_transform(int M, int inv, const double *in, double *out)
{
    OwnMixedPlan pl;
    if (!own_mixed_plan_make(M, pl)) return 1;
    typedef std::complex<double> Cp;
    std::vector<Cp> s((size_t)M), tab((size_t)M);
    for (int k = 0; k < M; ++k) {
        const long double a = -2.0L * 3.141592653589793238462643383279502884L * (long double)k / (long double)M;
        tab[(size_t)k] = Cp((double)cosl(a), (double)sinl(a));
        s[(size_t)k] = Cp(in[2 * k], in[2 * k + 1]);
    }
    own_mixed_passes_host(pl, s.data(), tab.data(), inv != 0);
    for (int k = 0; k < M; ++k) {
        const Cp z = s[(size_t)own_mixed_pos(pl, k)];
        out[2 * k] = z.real();
        out[2 * k + 1] = z.imag();
    }
    return 0;
}
#endif
