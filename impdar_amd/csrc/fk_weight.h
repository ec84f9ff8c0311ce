// The weight of the f-k fan (dip) filter at one element (w, kx) of the radargram's 2-D spectrum -- the one statement of this
// arithmetic: every fan kernel of fk_kernels.h calls it, and g++ compiles it by itself into the CPU suite's probe
// (tests/test_fk_cpu.py).  Float64 throughout, for float32 data too: a float32 slowness would move the taper by 1e-7 / taper.
//
//   slowness   p = 0 where |kx| == 0 (a flat event, and DC); else +inf where |w| == 0; else |kx| / |w|
//   edge       E(p; pc, tau), a low pass in slowness with lo = pc (1 - tau), hi = pc (1 + tau):
//              p <= lo: 1 (tested first: the hard edge tau = 0 keeps p == pc); p >= hi: 0; else (1 + cos(pi (p - lo) / (hi - lo))) / 2
//   fan        W = A B, A = E(p; 1 / va_lo, tau) (1 without va_lo), B = 1 - E(p; 1 / va_hi, tau) (1 without va_hi):
//              apparent velocities va_lo <= |w| / |kx| <= va_hi pass
//   dip        'down_right' (arrival time grows with distance, g(t - p x), on kx = -p w in NumPy's sign convention) keeps
//              w kx < 0, 'down_left' w kx > 0; elements with w kx == 0 and those on a Nyquist row or column belong to both
//              sides (which keeps the weight Hermitian and the result real); off the side W = 0
//   mode       'pass': W, 'reject': 1 - W
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define FK_HD __host__ __device__ inline
#else
#define FK_HD inline
#endif

enum { FK_PASS = 0, FK_REJECT = 1 };
enum { FK_DIP_BOTH = 0, FK_DIP_DOWN_RIGHT = 1, FK_DIP_DOWN_LEFT = 2 };

// One edge: lo and hi as above.
struct FkEdge {
    int on;
    double lo, hi;
};
struct FkFan {
    FkEdge a, b;        // a: from va_lo, b: from va_hi
    int mode, dip;
};

FK_HD FkEdge fk_edge_make(double va, double taper)
{
    FkEdge e;
    e.on = !(va != va);             // NaN: no edge
    const double pc = 1.0 / va;
    e.lo = pc * (1.0 - taper);
    e.hi = pc * (1.0 + taper);
    return e;
}
FK_HD FkFan fk_fan_make(double va_lo, double va_hi, double taper, int mode, int dip)
{
    FkFan f;
    f.a = fk_edge_make(va_lo, taper);
    f.b = fk_edge_make(va_hi, taper);
    f.mode = mode;
    f.dip = dip;
    return f;
}

// E at |kx| = ak, |w| = aw.  The division and the cosine are for the taper alone: an element whose ratio is beyond rounding's
// reach of lo or hi (the products below are within 2 ulp of lo aw and hi aw, the guard is 4) is decided by two products.
FK_HD double fk_edge(const FkEdge e, double ak, double aw)
{
    const double below = 1.0 - 0x1p-50, above = 1.0 + 0x1p-50;
    if (ak < e.lo * aw * below) return 1.0;
    if (ak > e.hi * aw * above) return 0.0;
    const double p = ak == 0.0 ? 0.0 : (aw == 0.0 ? INFINITY : ak / aw);
    if (p <= e.lo) return 1.0;
    if (p >= e.hi) return 0.0;
    return 0.5 * (1.0 + cos(3.14159265358979323846 * ((p - e.lo) / (e.hi - e.lo))));
}

// The weight at (w, kx); nyq: the element lies on a Nyquist row (snum even, index snum / 2) or column (tnum even, tnum / 2).
FK_HD double fk_weight(const FkFan f, double w, double kx, bool nyq)
{
    const double aw = fabs(w), ak = fabs(kx);
    double W = 1.0;
    if (f.a.on) W = fk_edge(f.a, ak, aw);
    if (f.b.on) W = W * (1.0 - fk_edge(f.b, ak, aw));
    if (f.dip != FK_DIP_BOTH && !nyq) {
        // the sign of w kx without the product (which may underflow)
        const int s = (w > 0.0 ? 1 : (w < 0.0 ? -1 : 0)) * (kx > 0.0 ? 1 : (kx < 0.0 ? -1 : 0));
        if ((f.dip == FK_DIP_DOWN_RIGHT && s > 0) || (f.dip == FK_DIP_DOWN_LEFT && s < 0)) W = 0.0;
    }
    return f.mode == FK_REJECT ? 1.0 - W : W;
}
