// The exact-arithmetic Kirchhoff kernels -- the reference's float64 index math pair by pair (kirch_exact_kernel), the same
// picks and weights tabulated on uniform grids (kirch_tablex_kernel / kirch_exact_tab_kernel), the scan for picks that
// rounding noise decides and their correction (kirch_tiescan_kernel / kirch_tiefix_kernel) -- and the host code that
// launches them.  Included by kirchhoff.hip alone.
#pragma once
#include "kirch_plan.h"
#include <algorithm>
#include <vector>

// ===========================================================================
// exact kernel: reference operation order, fp64 index math, any geometry
// ===========================================================================
struct ExactParams {
    const void *GT, *DT;
    void *out;
    int ldo;
    int snum, tnum, xlo, xhi;
    const double *dist, *zs, *zs2, *tt;
    double vel, tmax, r2lim, inv_dt, tt0;
    int dist_sorted;     // dist is non-decreasing: the traces inside the aperture are one index range
};

template <typename T, bool NEAR>
__global__ __launch_bounds__(256) void kirch_exact_kernel(ExactParams P)
{
    const int ti = blockIdx.x * 256 + threadIdx.x;
    const int xi = P.xlo + blockIdx.y;
    if (ti >= P.snum || xi >= P.xhi) return;
    const T *GT = reinterpret_cast<const T *>(P.GT);
    const T *DT = reinterpret_cast<const T *>(P.DT);
    const double dxi = P.dist[xi];
    const double z = P.zs[ti], z2 = P.zs2[ti];
    const int n = P.snum;
    double far = 0.0, near = 0.0;
    int jlo = 0, jhi = P.tnum;
    if (P.dist_sorted) {
        // traces with (dist - dist[xi])^2 + z^2 <= r2lim form one index range: bisect its ends (a guard
        // trace on both sides; the per-pair test below still decides)
        const double rad2 = P.r2lim - z2;
        if (rad2 < 0.0) {
            jhi = 0;
        } else {
            const double rad = sqrt(rad2) * (1.0 + 1e-12);
            int a = 0, b = xi;                       // first j with dist[j] >= dxi - rad
            while (a < b) {
                const int m = (a + b) >> 1;
                if (P.dist[m] < dxi - rad) a = m + 1; else b = m;
            }
            jlo = max(a - 1, 0);
            a = xi;
            b = P.tnum;                              // first j with dist[j] > dxi + rad
            while (a < b) {
                const int m = (a + b) >> 1;
                if (P.dist[m] <= dxi + rad) a = m + 1; else b = m;
            }
            jhi = min(a + 1, P.tnum);
        }
    }
    for (int j = jlo; j < jhi; ++j) {
        const double dx = P.dist[j] - dxi;
        const double q = dx * dx + z2;                 // :44 (compiled with -ffp-contract=off)
        if (q > P.r2lim) continue;                     // far outside the aperture
        const double rs = sqrt(q);
        const double cost = z / rs;                    // :47
        const double t = 2.0 * rs / P.vel;             // :49
        if (t > P.tmax) continue;                      // :52 -> term is 0 (or NaN, skipped)
        // nearest sample, ties to the lower index (:49 argmin)
        int k0 = (int)floor((t - P.tt0) * P.inv_dt);
        k0 = min(max(k0, 0), n - 1);
        while (k0 < n - 1 && P.tt[k0 + 1] <= t) ++k0;
        while (k0 > 0 && P.tt[k0] > t) --k0;
        const int k1 = min(k0 + 1, n - 1);
        const int k = (fabs(P.tt[k1] - t) < fabs(P.tt[k0] - t)) ? k1 : k0;
        const size_t o = (size_t)j * n + k;
        const double term = (double)GT[o] * cost / P.vel;   // :53
        if (term == term) far += term;                       // nansum
        if (NEAR) {
            const double term2 = (double)DT[o] * cost / (rs * rs);   // :58
            if (term2 == term2) near += term2;
        }
    }
    const double c = 1.0 / (2.0 * 3.141592653589793);
    T *out = reinterpret_cast<T *>(P.out);
    out[(size_t)ti * P.ldo + (xi - P.xlo)] = (T)(c * (far + near));   // :60
}

// ---------------------------------------------------------------------------
// exact path on uniform grids: the pick and the obliquity factor of a pair depend on (sample, |trace
// offset|) only, so they are tabulated once per geometry -- in fp64, in the reference's operation order
// (mig_python.py:44-58) -- and the diffraction sum becomes one gather + one fp64 FMA per pair.  Same
// picks as kirch_exact_kernel; the weight cos/vel is rounded once more than the reference's
// (g*cos)/vel (1 ulp, far inside the 1e-12 bar).
// ---------------------------------------------------------------------------
struct TableXParams {
    int *XK;                 // [ntab][snum] picked sample (0 where the pair is dropped)
    double *XW, *XW2;        // cos/vel and cos/rs^2 (0 where dropped: t > t_max or the 0/0 apex)
    const double *zs, *zs2, *tt;
    double dx, vel, tmax, inv_dt, tt0;
    int snum, ntab, near;
};

__global__ __launch_bounds__(256) void kirch_tablex_kernel(TableXParams P)
{
    const int ti = blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (ti >= P.snum) return;
    const size_t o = (size_t)n * P.snum + ti;
    int kk = 0;
    double w = 0.0, w2 = 0.0;
    const double dx = (double)n * P.dx;
    const double q = dx * dx + P.zs2[ti];
    const double rs = sqrt(q);
    const double cost = P.zs[ti] / rs;
    const double t = 2.0 * rs / P.vel;
    if (!(t > P.tmax) && cost == cost) {
        const int ns = P.snum;
        int k0 = (int)floor((t - P.tt0) * P.inv_dt);
        k0 = min(max(k0, 0), ns - 1);
        while (k0 < ns - 1 && P.tt[k0 + 1] <= t) ++k0;
        while (k0 > 0 && P.tt[k0] > t) --k0;
        const int k1 = min(k0 + 1, ns - 1);
        kk = (fabs(P.tt[k1] - t) < fabs(P.tt[k0] - t)) ? k1 : k0;
        w = cost / P.vel;
        w2 = cost / (rs * rs);
    }
    P.XK[o] = kk;
    P.XW[o] = w;
    if (P.near) P.XW2[o] = w2;
}

// Every table above assumes that the pick of a pair depends on (sample, |trace offset|) only.  That fails exactly
// where the reference's own answer is decided by rounding noise: a travel time that falls (to float64 rounding) on
// the midpoint between two samples, or on t_max itself.  The reference evaluates t from dist[j] - dist[xi], whose
// last bits differ from pair to pair with the same offset, so such ties break either way inside ONE offset
// (geometries with a rational moveout 2dx/(v dt), e.g. 2.5 samples per trace, are full of them: 4a^2 + 25n^2 is
// an odd square for whole families of (a, n)).  This scan flags a geometry that has any such entry inside an
// aperture; the plan then keeps the per-pair kernel, which repeats the reference's arithmetic pair by pair.
// Margin: the relative rounding noise of t, ~1e-15, plus the noise of dist[j] - dist[xi] against n * dx, times
// |t|/dt, in samples.  `xnoise` is that position noise in units of dx, MEASURED on the profile by the host: twice the
// largest deviation of dist[] from the fitted grid (the plan accepts up to 1e-9 dx as "uniform") plus the rounding of
// the largest |dist| (a profile that starts 50 km along a line has ulp(dist)/dx ~ 7e-12, far above what a profile
// starting at 0 has), never less than 4.5e-16 * tnum.
__global__ __launch_bounds__(256) void kirch_tiescan_kernel(TableXParams P, double xnoise, int *count, int2 *list, int cap)
{
    const int ti = blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (ti >= P.snum) return;
    const double dx = (double)n * P.dx;
    const double q = dx * dx + P.zs2[ti];
    const double rs = sqrt(q);
    const double cost = P.zs[ti] / rs;
    const double t = 2.0 * rs / P.vel;
    if (!(cost == cost)) return;                       // 0/0 apex: dropped whatever the noise
    const double u = (t - P.tt0) * P.inv_dt, um = (P.tmax - P.tt0) * P.inv_dt;
    // ten times the noise estimate: a wider net only makes the list (a handful of entries) longer
    const double eps = 10.0 * (fabs(t * P.inv_dt) + 1.0) * (1.0e-15 + xnoise / (double)max(n, 1));
    if (u > um + eps) return;                          // clearly outside the aperture
    bool amb = fabs(u - um) <= eps && n > 0;           // the t > t_max test itself (n = 0: t = tt exactly)
    if (u >= 0.0 && u <= um + eps && n > 0) {
        const double fr = u - floor(u);
        amb = amb || fabs(fr - 0.5) <= eps;
    }
    if (amb) {
        const int at = atomicAdd(count, 1);
        if (at < cap) list[at] = make_int2(ti, n);
    }
}

// ---------------------------------------------------------------------------
// ... and the table-driven kernels keep running on such geometries: the flagged (sample, offset) entries (one in
// 1.1e7 for dx 1 m, dt 10 ns, v 1.68e8 m/s -- the velocity RadarData.migrate defaults to -- a few thousand for a
// moveout of exactly 2.5) are re-done pair by pair in the reference's arithmetic after the diffraction sum, and
// where a pair's own answer (pick, or the t > t_max drop) differs from the table's, the output gets the
// difference.  One thread per (sample with flagged offsets, output trace), its offsets and the two sides in a
// fixed order: deterministic, no atomics.  Per-pair parity on every geometry at the cost of a few microseconds.
// ---------------------------------------------------------------------------
struct TieFixParams {
    const void *GT, *DT;     // images (layout: grp = 0 trace-major [row][k]; else groups of `grp` rows, sample-major inside)
    void *out;
    int ldo, snum, tnum, xlo, xhi, grp, near;
    const double *dist, *zs, *zs2, *tt;
    double dx, vel, tmax, inv_dt, tt0;
    const int *g_ti, *g_off, *g_n;   // groups: sample, [first, last) into g_n (offsets, ascending)
    const int *hmax;                 // per 256-sample chunk: offsets beyond are not walked
    int nmax;                        // offsets >= nmax are dropped by the tables whatever t is
};

template <typename T>
__global__ __launch_bounds__(256) void kirch_tiefix_kernel(TieFixParams P)
{
    const int g = blockIdx.y;
    const int xi = P.xlo + blockIdx.x * 256 + threadIdx.x;
    if (xi >= P.xhi) return;
    const int ti = P.g_ti[g];
    const T *GT = reinterpret_cast<const T *>(P.GT);
    const T *DT = reinterpret_cast<const T *>(P.DT);
    const int ns = P.snum;
    auto at = [&](const T *img, int j, int k) -> double {
        const size_t o = P.grp ? ((size_t)(j / P.grp) * ns + k) * P.grp + (j % P.grp) : (size_t)j * ns + k;
        return (double)img[o];
    };
    auto pick = [&](double t) {
        int k0 = (int)floor((t - P.tt0) * P.inv_dt);
        k0 = min(max(k0, 0), ns - 1);
        while (k0 < ns - 1 && P.tt[k0 + 1] <= t) ++k0;
        while (k0 > 0 && P.tt[k0] > t) --k0;
        const int k1 = min(k0 + 1, ns - 1);
        return (fabs(P.tt[k1] - t) < fabs(P.tt[k0] - t)) ? k1 : k0;      // :49, ties to the lower index
    };
    const double z = P.zs[ti], z2 = P.zs2[ti];
    const double c2pi = 1.0 / (2.0 * 3.141592653589793);
    const int hm = P.hmax[ti >> 8];
    double far = 0.0, nearsum = 0.0;
    for (int e = P.g_off[g]; e < P.g_off[g + 1]; ++e) {
        const int n = P.g_n[e];
        // what the table holds for (ti, n): the pick at dx = n * spacing (kirch_tableq / tabled / tablex kernels)
        const double dxn = (double)n * P.dx;
        const double rsn = sqrt(dxn * dxn + z2);
        const double costn = z / rsn;
        const double tn = 2.0 * rsn / P.vel;
        const bool drop_tab = n >= P.nmax || n > hm || tn > P.tmax || !(costn == costn);
        const int k_tab = drop_tab ? 0 : pick(tn);
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            const int j = xi + sgn * n;
            if (j < 0 || j >= P.tnum) continue;
            const double dxj = P.dist[j] - P.dist[xi];
            const double q = dxj * dxj + z2;                   // :44
            const double rs = sqrt(q);
            const double cost = z / rs;                        // :47
            const double t = 2.0 * rs / P.vel;                 // :49
            const bool drop = t > P.tmax || !(cost == cost);   // :52, nansum
            const int k = drop ? 0 : pick(t);
            if (drop == drop_tab && (drop || k == k_tab)) continue;
            // the weight the diffraction sum gave this offset (a function of (ti, n) in every table-driven kernel)
            const double wf = costn / P.vel, wn = costn / (rsn * rsn);
            const double gt = drop ? 0.0 : at(GT, j, k), gb = drop_tab ? 0.0 : at(GT, j, k_tab);
            far += (gt - gb) * wf;
            if (P.near) {
                const double dt_ = drop ? 0.0 : at(DT, j, k), db = drop_tab ? 0.0 : at(DT, j, k_tab);
                nearsum += (dt_ - db) * wn;
            }
        }
    }
    const double delta = c2pi * (far + nearsum);
    if (delta != 0.0) {
        T *o = reinterpret_cast<T *>(P.out) + (size_t)ti * P.ldo + (xi - P.xlo);
        *o = (T)((double)*o + delta);
    }
}

struct ExactTabParams {
    const void *GT, *DT;
    void *out;
    int ldo, snum, tnum, xlo, xhi;
    const int *XK;
    const double *XW, *XW2;
    const int *hmax;         // per 256-sample chunk: largest aperture half width of its samples
    int ntab;
};

template <typename T, bool NEAR, int XE>
__global__ __launch_bounds__(256) void kirch_exact_tab_kernel(ExactTabParams P)
{
    const int ti_raw = blockIdx.x * 256 + threadIdx.x;
    const int ti = min(ti_raw, P.snum - 1);
    const int x0 = P.xlo + blockIdx.y * XE;
    const T *GT = reinterpret_cast<const T *>(P.GT);
    const T *DT = reinterpret_cast<const T *>(P.DT);
    const int hm = min(P.hmax[blockIdx.x], P.ntab - 1);
    const int nlo = max(-hm, -(x0 + XE - 1)), nhi = min(hm, P.tnum - 1 - x0);
    double far[XE], near[XE];
#pragma unroll
    for (int e = 0; e < XE; ++e) far[e] = near[e] = 0.0;
    const size_t sn = (size_t)P.snum;
    for (int n = nlo; n <= nhi; ++n) {
        const size_t o = (size_t)abs(n) * sn + ti;
        const int k = P.XK[o];
        const double w = P.XW[o];
        const double w2 = NEAR ? P.XW2[o] : 0.0;
#pragma unroll
        for (int e = 0; e < XE; ++e) {
            const int j = x0 + e + n;
            if (j >= 0 && j < P.tnum) {
                const size_t g = (size_t)j * sn + k;
                const double term = (double)GT[g] * w;            // :53
                if (term == term) far[e] += term;                 // nansum
                if (NEAR) {
                    const double term2 = (double)DT[g] * w2;      // :58
                    if (term2 == term2) near[e] += term2;
                }
            }
        }
    }
    if (ti_raw < P.snum) {
        const double c = 1.0 / (2.0 * 3.141592653589793);
        T *out = reinterpret_cast<T *>(P.out);
#pragma unroll
        for (int e = 0; e < XE; ++e)
            if (x0 + e < P.xhi) out[(size_t)ti_raw * P.ldo + (x0 + e - P.xlo)] = (T)(c * (far[e] + near[e]));   // :60
    }
}

// ===========================================================================
// host side
// ===========================================================================
// the images and the output block of the global-memory kernels' structs (the axes: kirch_fill_axes, kirch_plan.h)
template <typename P>
static void kirch_fill_io(P &T, const impdar_kirch_plan *p, void *d_out, int xlo, int xhi)
{
    T.GT = img_row0(p, p->GT[p->buf]);
    T.DT = p->nearfield ? img_row0(p, p->DT[p->buf]) : nullptr;
    T.out = d_out;
    T.ldo = xhi - xlo;
    T.snum = p->snum;
    T.tnum = p->tnum;
    T.xlo = xlo;
    T.xhi = xhi;
}

// the picks that rounding noise decides (kirch_tiescan_kernel), and what their number does to the route
static int kirch_tie_scan(impdar_kirch_plan *p)
{
    constexpr int TIE_CAP = 1 << 20;
    static_assert(sizeof(KirchTie) == sizeof(int2), "the tie list is downloaded as it lies");
    hipStream_t st = p->ctx->stream;
    int hg = 0, rc;
    for (int k = 0; k < p->snum; ++k) hg = std::max(hg, p->h_half[k] + 1);
    hg = std::min(hg, p->tnum) + 1;
    DevBuf d_flag, d_list;
    if (d_flag.ensure(64) != hipSuccess || d_list.ensure((size_t)TIE_CAP * sizeof(int2)) != hipSuccess) {
        impdar_set_error("hipMalloc failed");
        return IMPDAR_ERR_HIP;
    }
    (void)hipMemsetAsync(d_flag.p, 0, 64, st);
    TableXParams T;
    T.XK = nullptr;
    T.XW = T.XW2 = nullptr;
    kirch_fill_axes(T, p);
    T.dx = p->dx;
    T.ntab = hg;
    T.near = 0;
    hipLaunchKernelGGL(kirch_tiescan_kernel, dim3((p->snum + 255) / 256, hg), dim3(256), 0, st, T, p->xnoise, d_flag.as<int>(),
                       d_list.as<int2>(), TIE_CAP);
    int count = 0;
    if (hipMemcpyAsync(&count, d_flag.p, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        impdar_set_error("tie scan failed: %s", hipGetErrorString(hipGetLastError()));
        return IMPDAR_ERR_HIP;
    }
    kirch_route_after_ties(*p, count, TIE_CAP);
    if (!p->want_tie_groups) return IMPDAR_OK;
    std::vector<KirchTie> list(count);
    if (hipMemcpy(list.data(), d_list.p, (size_t)count * sizeof(int2), hipMemcpyDeviceToHost) != hipSuccess) {
        impdar_set_error("tie list download failed");
        return IMPDAR_ERR_HIP;
    }
    const KirchTieGroups G = kirch_group_ties(list);
    p->ntie_groups = (int)G.g_ti.size();
    if ((rc = upload(p->d_tie_ti, G.g_ti.data(), G.g_ti.size() * 4)) || (rc = upload(p->d_tie_off, G.g_off.data(), G.g_off.size() * 4)) ||
        (rc = upload(p->d_tie_n, G.g_n.data(), G.g_n.size() * 4)))
        return rc;
    return IMPDAR_OK;
}

// the float64 pick / weight tables of kirch_exact_tab_kernel, built at the first migrate
static int build_exact_tables(impdar_kirch_plan *p, hipStream_t st)
{
    const int nch = (p->snum + 255) / 256;
    int hg = 0;
    std::vector<int> hm(nch, 0);
    for (int k = 0; k < p->snum; ++k) {
        hm[k / 256] = std::max(hm[k / 256], p->h_half[k] + 1);
        hg = std::max(hg, p->h_half[k] + 1);
    }
    hg = std::min(hg, p->tnum) + 1;
    const size_t ent = (size_t)hg * p->snum;
    if (p->d_XK.ensure(ent * 4) != hipSuccess || p->d_XW.ensure(ent * 8) != hipSuccess ||
        (p->nearfield && p->d_XW2.ensure(ent * 8) != hipSuccess) || p->d_xhmax.ensure((size_t)nch * 4) != hipSuccess) {
        impdar_set_error("hipMalloc of the %zu-entry exact pick/weight table failed", ent);
        return IMPDAR_ERR_HIP;
    }
    IMPDAR_HIP_CHECK(hipMemcpyAsync(p->d_xhmax.p, hm.data(), (size_t)nch * 4, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(st));          // hm is a stack vector
    TableXParams T;
    T.XK = p->d_XK.as<int>();
    T.XW = p->d_XW.as<double>();
    T.XW2 = p->d_XW2.as<double>();
    kirch_fill_axes(T, p);
    T.dx = p->dx;
    T.ntab = hg;
    T.near = p->nearfield;
    hipLaunchKernelGGL(kirch_tablex_kernel, dim3(nch, hg), dim3(256), 0, st, T);
    IMPDAR_HIP_CHECK(hipGetLastError());
    p->xntab = hg;
    p->xtab_ready = true;
    return IMPDAR_OK;
}

// exact arithmetic on uniform grids: tabulated fp64 picks / weights, one gather + FMA per pair
static int migrate_exact_tab(impdar_kirch_plan *p, void *d_out, int xlo, int xhi, hipStream_t st)
{
    int rc;
    if (!p->xtab_ready && (rc = build_exact_tables(p, st))) return rc;
    ExactTabParams P;
    kirch_fill_io(P, p, d_out, xlo, xhi);
    P.XK = p->d_XK.as<int>();
    P.XW = p->d_XW.as<double>();
    P.XW2 = p->d_XW2.as<double>();
    P.hmax = p->d_xhmax.as<int>();
    P.ntab = p->xntab;
#ifndef KX_XE
#define KX_XE 16
#endif
    constexpr int XE = KX_XE;
    dim3 grid((p->snum + 255) / 256, (xhi - xlo + XE - 1) / XE);
    if (p->dtype == IMPDAR_F32) {
        if (p->nearfield)
            hipLaunchKernelGGL((kirch_exact_tab_kernel<float, true, XE>), grid, dim3(256), 0, st, P);
        else
            hipLaunchKernelGGL((kirch_exact_tab_kernel<float, false, XE>), grid, dim3(256), 0, st, P);
    } else {
        if (p->nearfield)
            hipLaunchKernelGGL((kirch_exact_tab_kernel<double, true, XE>), grid, dim3(256), 0, st, P);
        else
            hipLaunchKernelGGL((kirch_exact_tab_kernel<double, false, XE>), grid, dim3(256), 0, st, P);
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

// the reference's arithmetic pair by pair: any geometry
static int migrate_exact_pair(impdar_kirch_plan *p, void *d_out, int xlo, int xhi, hipStream_t st)
{
    ExactParams P;
    kirch_fill_io(P, p, d_out, xlo, xhi);
    kirch_fill_axes(P, p);
    P.dist = p->d_dist.as<double>();
    const double rlim = p->vel * p->tmax / 2.0;
    P.r2lim = rlim * rlim * (1.0 + 1e-9);
    P.dist_sorted = p->dist_sorted ? 1 : 0;
    dim3 grid((p->snum + 255) / 256, xhi - xlo);
    if (p->dtype == IMPDAR_F32) {
        if (p->nearfield)
            hipLaunchKernelGGL((kirch_exact_kernel<float, true>), grid, dim3(256), 0, st, P);
        else
            hipLaunchKernelGGL((kirch_exact_kernel<float, false>), grid, dim3(256), 0, st, P);
    } else {
        if (p->nearfield)
            hipLaunchKernelGGL((kirch_exact_kernel<double, true>), grid, dim3(256), 0, st, P);
        else
            hipLaunchKernelGGL((kirch_exact_kernel<double, false>), grid, dim3(256), 0, st, P);
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

// the (sample, offset) entries whose pick rounding noise decides, pair by pair (kirch_tiefix_kernel)
static int migrate_tiefix(impdar_kirch_plan *p, int kern, void *d_out, int xlo, int xhi, hipStream_t st)
{
    TieFixParams F;
    kirch_fill_io(F, p, d_out, xlo, xhi);
    kirch_fill_axes(F, p);
    F.grp = kern == IMPDAR_KERNEL_QUAD ? 8 : (kern == IMPDAR_KERNEL_DQUAD ? 4 : 0);
    F.near = p->nearfield;
    F.dist = p->d_dist.as<double>();
    F.dx = p->dx;
    F.g_ti = p->d_tie_ti.as<int>();
    F.g_off = p->d_tie_off.as<int>();
    F.g_n = p->d_tie_n.as<int>();
    const bool xtab = kern == IMPDAR_KERNEL_EXACT_TAB;
    F.hmax = xtab ? p->d_xhmax.as<int>() : p->d_hmax.as<int>();
    F.nmax = xtab ? p->xntab : p->ntab - 1;
    const dim3 grid((xhi - xlo + 255) / 256, p->ntie_groups);
    if (p->dtype == IMPDAR_F32)
        hipLaunchKernelGGL(kirch_tiefix_kernel<float>, grid, dim3(256), 0, st, F);
    else
        hipLaunchKernelGGL(kirch_tiefix_kernel<double>, grid, dim3(256), 0, st, F);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}
