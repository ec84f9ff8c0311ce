// Phase-shift (Gazdag) migration on gfx950 and the taper-only "T-K" stub.
//
// Behaviour restated from src/impdar/lib/migrationlib/mig_python.py:
//   :211-287  migrationPhaseShift: taper (in place, d*(H*V)), zero-pad time to
//             nt = 2^ceil(log2 snum), FK = fft2(data,(nt,tnum)), phaseShift,
//             image = ifft_k(TK).real
//   :396-420  constant velocity:  TK[tau,k] = sum_w 1[(v kx/2)^2 < w^2] FK[w,k] e^{i (tau+1) phi},
//             phi = w dt sqrt(1-(v kx/2w)^2)   (recurrence FFK *= e^{i phi} per tau)
//   :438-487  1-D v(z): per tau  FK[w,k] *= e^{i w dt Re sqrt(coss)},
//             coss = 1-(v_tau kx/2w)^2;  FK[w,k] = 0 for good once coss <= thr_tau;
//             TK[tau,k] = sum_w FK[w,k]
//   :490-492  TK /= snum
//   :290-355  migrationTimeWavenumber = taper only
//
// What is here: the cached plan's one instance (g_ps_plan), the path runners, the stages of ps_run, and the C entry points
// -- impdar_phaseshift, its device-resident form, the three calls of the wavenumber-sharded run, impdar_taper.
// The kernels and what they share live in headers, each including what it uses:
//   ps_layout.h   Cp<T>, taper / pad / transpose / real-part kernels and their launchers
//   ps_common.h   sincos_t, PS_ANCHOR, PsParams, the slot loads, the wave-level reduce-scatter
//   ps_direct.h   the vector path: ps_kernel, ps_vz32_kernel, ps_vz64_kernel, ps_dc_kernel, ps_dispatch
//   ps_mfma.h, ps_smooth.h, ps_nufft.h, ps_series.h, ps_runs.h   the other paths' kernels
//   ps_plan.h     struct PsPlan
//   ps_route.h, ps_path_plan.h, ps_series_plan.h   what is decided on the host (plain C++, no device code)
// The Fourier finite-difference migration of a 2-D velocity field (impdar_phaseshift_ffd) is ffd.hip.
#include "fft.h"
#include "own_fft.h"
#include "ps_layout.h"
#include "ps_common.h"
#include "ps_direct.h"
#include "ps_mfma.h"
#include "ps_smooth.h"      // v(z) that changes at every step: carried square roots and rotations
#include "ps_nufft.h"
#include "ps_series.h"      // a velocity that changes inside a piece: a few transforms with shared nodes + direct sums at the boundary
#include "ps_runs.h"        // many runs of constant velocity: float32 MFMA, phases generated in the kernel
#include "ps_plan.h"
#include "ps_route.h"
#include <algorithm>
#include <mutex>

static std::mutex g_ps_mu;
static PsPlan *g_ps_plan = nullptr;

// called by impdar_ctx_destroy: a cached plan must not outlive the stream it was created on
void impdar_ps_forget(const impdar_ctx *ctx)
{
    std::lock_guard<std::mutex> lk(g_ps_mu);
    if (g_ps_plan && (g_ps_plan->owner == ctx || g_ps_plan->slab_owner == ctx)) {      // (the sharded calls' plan and buffers too)
        delete g_ps_plan;
        g_ps_plan = nullptr;
    }
}

// impdar_release_caches: out of device memory somewhere -- drop the cached plan unless a phase-shift call is using it
static thread_local bool t_ps_busy = false;
void impdar_ps_trim()
{
    if (t_ps_busy) return;
    std::unique_lock<std::mutex> lk(g_ps_mu, std::try_to_lock);
    if (lk.owns_lock() && g_ps_plan) {
        delete g_ps_plan;
        g_ps_plan = nullptr;
    }
}

// ---- the path runners: ps_runs_run, ps_nufft_run, ps_series_run, ps_mfma_run (and ps_smooth_run further down), one signature.
// What a path plans on the host and every host-side reason to decline is ps_path_plan.h's (ps_series_plan.h for the series path);
// a runner tests what depends on the device, allocates, uploads and launches.  *done = true: the frequency sums were produced
// here; false with IMPDAR_OK: the call is not for this path, the next attempt of the route takes it.
struct PsCall {
    const double *kx, *vmig;    // the caller's host arrays: [tnum]; [snum] per-step velocities (vlen != 0)
    int vlen;
    bool tk_out;                // the sums go to a caller who asked for the rows TK themselves (a rank of a kx-sharded run): rows k and
                                // tnum - k may not be written as their Hermitian combination and its conjugate
    PsKnobs K;
};

// did a matrix-core path find more boundary frequencies than it lists on this (kx, runs) geometry before?  (ADVICE r4:
// such inputs paid set-up + sums + a blocking read-back on EVERY call, discarded, before the vector kernels ran)
static bool ps_known_overflow(const PsPlan &pl, const double *kx, int tnum, const std::vector<PsMfmaRun> &runs)
{
    if (pl.ovf_kx.size() != (size_t)tnum || pl.ovf_runs.size() != runs.size() || runs.empty()) return false;
    if (memcmp(pl.ovf_kx.data(), kx, (size_t)tnum * 8) != 0) return false;
    for (size_t i = 0; i < runs.size(); ++i)
        if (runs[i].v != pl.ovf_runs[i].v || runs[i].start != pl.ovf_runs[i].start || runs[i].len != pl.ovf_runs[i].len) return false;
    return true;
}
static void ps_note_overflow(PsPlan &pl, const double *kx, int tnum, const std::vector<PsMfmaRun> &runs)
{
    pl.ovf_kx.assign(kx, kx + tnum);
    pl.ovf_runs = runs;
}

// the whole wavenumber axis with kx[tnum - k] = -kx[k] (the Nyquist row of an even axis is its own partner): rows k and tnum - k
// turn by the same angles and share a workgroup; a slab of a kx-sharded run has no mirror rows
static bool ps_mirror_rows(const PsParams &P, const PsRoute &R) { return R.kx_antisym && P.k0 == 0 && P.nk == P.tnum && P.tnum >= 2; }

// every buffer of a path at its size, or none of the path: not getting them is not an error, the other paths take the call
static bool ps_ensure_all(std::initializer_list<std::pair<DevBuf *, size_t>> needs)
{
    for (const auto &n : needs)
        if (n.first->ensure(n.second) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
    return true;
}

// rw = 1 / w by slot on the device (rw: the runner's staging, alive until its stream drain; pl.d_rw: ensured by the runner)
static int ps_rw_upload(PsPlan &pl, const PsRoute &R, int nf, std::vector<double> &rw, hipStream_t st)
{
    rw.resize((size_t)nf);
    for (int i = 0; i < nf; ++i) rw[i] = 1.0 / R.w[i];
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_rw.p, rw.data(), rw.size() * 8, hipMemcpyHostToDevice, st));
    return IMPDAR_OK;
}

// MFMA instructions the kernel issued, counted by the kernel (the stream is drained)
static int ps_mcount_read(PsPlan &pl)
{
    unsigned long long n = 0;
    IMPDAR_HIP_CHECK(hipMemcpy(&n, pl.d_mcount.p, 8, hipMemcpyDeviceToHost));
    pl.mfma_instructions = (double)n;
    return IMPDAR_OK;
}

// Boundary frequencies: a path's kernel takes the frequencies on the evanescent boundary of some run out of its sums and lists the
// first PM_EMAX per wavenumber; ps_edge_kernel walks the listed ones the reference's way.  The counter keeps counting: more
// than PM_EMAX means contributions are missing from TK -- the result is discarded and another path produces it.
// Before the path's kernel: room for the lists (*room false: none), E filled (ps_edge_kernel reads P and the lists only), counts cleared
static int ps_edge_prepare(PsPlan &pl, const PsParams &P, bool clear, hipStream_t st, PsMfmaParams &E, bool *room)
{
    *room = ps_ensure_all({{&pl.d_edge, (size_t)P.tnum * (1 + PM_EMAX) * sizeof(int)}});
    if (!*room) return IMPDAR_OK;
    E.mfma_count = nullptr;
    E.P = P;
    E.nruns = 0;
    E.pairs = 0;
    E.edge_cnt = pl.d_edge.as<int>();
    E.edge_list = E.edge_cnt + P.tnum;
    if (clear) IMPDAR_HIP_CHECK(hipMemsetAsync(E.edge_cnt, 0, (size_t)P.tnum * sizeof(int), st));
    return IMPDAR_OK;
}
// After it: ps_edge_kernel (walk; else the drain only), the stream drained (the runner's host tables must outlive their copies), the
// counts of [k0, k0 + nk) read back.  *worst > PM_EMAX: lists overflowed, the geometry is remembered and not tried again
template <typename T>
static int ps_edge_finish(PsPlan &pl, const PsRoute &R, const PsCall &c, const PsMfmaParams &E, bool walk, const char *who, hipStream_t st, int *worst)
{
    const PsParams &P = E.P;
    *worst = 0;
    if (walk) hipLaunchKernelGGL(ps_edge_kernel_t<T>, dim3(P.nk), dim3(256), 0, st, E);
    IMPDAR_HIP_CHECK(hipGetLastError());
    if (who) impdar_trace("%s: buffers ready, tables copied, kernels enqueued", who);
    IMPDAR_HIP_CHECK(hipStreamSynchronize(st));
    if (who) impdar_trace("%s: stream drained", who);
    if (!walk) return IMPDAR_OK;
    std::vector<int> cnt((size_t)P.nk);
    IMPDAR_HIP_CHECK(hipMemcpy(cnt.data(), E.edge_cnt + P.k0, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int n : cnt) *worst = std::max(*worst, n);
    if (*worst > PM_EMAX) ps_note_overflow(pl, c.kx, P.tnum, R.runs);
    return IMPDAR_OK;
}

// ---- many-runs matrix-core path (ps_runs.h): stages (pr_plan), launch
static int ps_runs_run(PsPlan &pl, PsParams &P, const PsRoute &R, const PsCall &c, const PsAttempt &, hipStream_t st, bool *done, const char **kernel)
{
    *done = false;
    *kernel = "ps_runs_kernel";
    const int snum = P.snum, tnum = P.tnum;
    if (!pr_gate((int)R.runs.size(), P.nf, snum) || !ps_thr_off_band(R.thr.data(), snum) || ps_known_overflow(pl, c.kx, tnum, R.runs)) return IMPDAR_OK;
    PrPlan plan;
    if (!pr_plan(plan, R.runs, P.nf, snum)) return IMPDAR_OK;
    const std::vector<PrRun> &pr = plan.pr;
    const std::vector<PrStage> &stages = plan.stages;
    impdar_trace("ps_runs: %zu pieces in %zu stages", pr.size(), stages.size());
    const int nparts = plan.nparts;
    const size_t part_bytes = nparts > 1 ? (size_t)nparts * P.nk * snum * sizeof(Cp<float>) : 0;
    PsMfmaParams E;
    bool room;
    int rc;
    if (!ps_ensure_all({{&pl.d_pr_runs, pr.size() * sizeof(PrRun)}, {&pl.d_pr_stages, stages.size() * sizeof(PrStage)}, {&pl.d_rw, (size_t)P.nf * 8},
                        {&pl.d_part, part_bytes}, {&pl.d_mcount, 8}}))
        return IMPDAR_OK;
    if ((rc = ps_edge_prepare(pl, P, true, st, E, &room)) || !room) return rc;
    std::vector<double> rw;
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_pr_runs.p, pr.data(), pr.size() * sizeof(PrRun), hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_pr_stages.p, stages.data(), stages.size() * sizeof(PrStage), hipMemcpyHostToDevice, st));
    if ((rc = ps_rw_upload(pl, R, P.nf, rw, st))) return rc;
    PrParams Q;
    Q.P = P;
    Q.runs = pl.d_pr_runs.as<PrRun>();
    Q.stages = pl.d_pr_stages.as<PrStage>();
    Q.rw = pl.d_rw.as<double>();
    Q.nstages = (int)stages.size();
    Q.nruns = (int)pr.size();
    Q.nparts = nparts;
    Q.part = pl.d_part.p;
    Q.edge_cnt = E.edge_cnt;
    Q.edge_list = E.edge_list;
    Q.mfma_count = pl.d_mcount.as<unsigned long long>();
    IMPDAR_HIP_CHECK(hipMemsetAsync(Q.mfma_count, 0, 8, st));
    const bool pairs = ps_mirror_rows(P, R);     // rows k and tnum - k in one workgroup (ps_runs.h)
    const bool tr = impdar_trace_on();           // tracing: drain the stream between the launches, a line each
    auto drained = [&](const char *what) {
        if (!tr) return;
        (void)hipStreamSynchronize(st);
        impdar_trace("ps_runs: %s", what);
    };
    drained("stream idle before the frequency sums");
    if (pairs) {
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)ps_runs_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pr_lds_bytes(2)));
        hipLaunchKernelGGL(ps_runs_kernel<2>, dim3((unsigned)(tnum / 2 + 1) * nparts), dim3(256), pr_lds_bytes(2), st, Q);
    } else {
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)ps_runs_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pr_lds_bytes(1)));
        hipLaunchKernelGGL(ps_runs_kernel<1>, dim3((unsigned)P.nk * nparts), dim3(256), pr_lds_bytes(1), st, Q);
    }
    drained("ps_runs_kernel done");
    if (nparts > 1) {
        const size_t n = (size_t)P.nk * snum;
        hipLaunchKernelGGL((ps_smooth_sum_kernel<float>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<const Cp<float> *>(pl.d_part.p), reinterpret_cast<Cp<float> *>(P.TK), nparts, n, snum);
    }
    drained("partial images summed");
    // every part of a wavenumber counts its own boundary frequencies into the same list: the first PM_EMAX are walked
    int worst;
    if ((rc = ps_edge_finish<float>(pl, R, c, E, true, "ps_runs", st, &worst)) || worst > PM_EMAX) return rc;
    if ((rc = ps_mcount_read(pl))) return rc;
    impdar_trace("ps_runs: counters read back: %.0f MFMA instructions, worst edge count %d, %d parts, pairs %d", pl.mfma_instructions, worst, nparts, (int)pairs);
    *done = true;
    return IMPDAR_OK;
}

// 1 / psihat(n), n = 0 .. Lp/2, of every padded length in `need` (pn_corr_of_length, ps_path_plan.h).  Made once per length and
// plan; *grew: the device copy is stale.  (Shared by the transform paths ps_nufft.h and ps_series.h: same window, same tables.)
template <typename T>
static std::vector<T> &pn_corr_tables(PsPlan &pl, const bool (&need)[13], int (&off_out)[13], bool *grew)
{
    std::vector<T> &corr = sizeof(T) == 4 ? reinterpret_cast<std::vector<T> &>(pl.h_pn_corr) : reinterpret_cast<std::vector<T> &>(pl.h_pn_corr64);
    int *corr_off = pl.pn_corr_off[sizeof(T) == 8 ? 1 : 0];
    for (int l = 0; l < 13; ++l) {
        if (!need[l] || corr_off[l] >= 0) continue;
        corr_off[l] = (int)corr.size();
        *grew = true;
        for (double x : pn_corr_of_length(PnCfg<T>::W, l)) corr.push_back((T)x);
    }
    for (int l = 0; l < 13; ++l) off_out[l] = corr_off[l] < 0 ? 0 : corr_off[l];
    return corr;
}

// the grid tables of a transform path on the device and in its parameters Q: the twiddles of the grid lengths 2^(l + 1) in `need`,
// the correction tables of the window.  *room false: no room for the tables
template <typename T, typename Params>
static int ps_grid_tables(PsPlan &pl, const bool (&need)[13], Params &Q, hipStream_t st, bool *room)
{
    bool grew = false;
    std::vector<T> &corr = pn_corr_tables<T>(pl, need, Q.corr_off, &grew);
    *room = ps_ensure_all({{&pl.d_pn_corr, corr.size() * sizeof(T) + 16}});
    if (!*room) return IMPDAR_OK;
    for (int l = 5; l <= 13; ++l)
        if (need[l - 1]) {
            int rc = pl.pn_tw[l].ensure<T>(1 << l, st);
            if (rc) return rc;
        }
    for (int l = 0; l < 14; ++l) Q.tw[l] = pl.pn_tw[l].buf.p;
    if (grew || pl.pn_corr_dev != (int)sizeof(T)) {
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_pn_corr.p, corr.data(), corr.size() * sizeof(T), hipMemcpyHostToDevice, st));
        pl.pn_corr_dev = (int)sizeof(T);
    }
    Q.corr = pl.d_pn_corr.p;
    return IMPDAR_OK;
}

// ---- transform path (ps_nufft.h): pieces (pn_plan), correction tables, launch
template <typename T>
static int ps_nufft_run(PsPlan &pl, PsParams &P, const PsRoute &R, const PsCall &c, const PsAttempt &, hipStream_t st, bool *done, const char **kernel)
{
    constexpr bool dbl = sizeof(T) == 8;
    *done = false;
    *kernel = "ps_nufft_kernel";
    const bool vz = c.vlen != 0;
    const int snum = P.snum, tnum = P.tnum, nf = P.nf;
    double dw;
    if (!pn_gate((int)R.runs.size(), nf, snum, P.herm != 0) || (vz && ps_known_overflow(pl, c.kx, tnum, R.runs)) ||
        (vz && !ps_thr_off_band(R.thr.data(), snum)) || !ps_axis_uniform(R.w.data(), nf, 1e-9, &dw))
        return IMPDAR_OK;
    // a pair of rows per workgroup, as ps_runs_kernel's -- where the sums go on into the inverse transform: the rows are written as
    // their Hermitian combination and its conjugate (ps_nufft_kernel<T, true>)
    const bool pairs = !c.tk_out && tnum % 2 == 0 && ps_mirror_rows(P, R);
    if (P.fhalf && !pairs) return IMPDAR_OK;           // (the half layout is read by the pairs only; ps_run repeats the transforms)
    // float64 data, v(z): the per-step velocities too -- the runs' rounding noise enters as a first-order term (ps_nufft.h)
    const bool first_order = dbl && vz;
    PnPlan plan;
    if (!pn_plan(plan, R.runs, vz, dbl, pairs, nf, snum, P.herm != 0, first_order ? c.vmig : nullptr)) return IMPDAR_OK;
    const std::vector<PnPiece> &pc = plan.pieces;
    PnParams Q;
    PsMfmaParams E;
    std::vector<double> rw;
    bool room;
    int rc;
    if (!ps_ensure_all({{&pl.d_pn_e1, plan.e1.size() * 8}, {&pl.d_pn_pieces, pc.size() * sizeof(PnPiece)}, {&pl.d_rw, (size_t)nf * 8}})) return IMPDAR_OK;
    if ((rc = ps_grid_tables<T>(pl, plan.need, Q, st, &room)) || !room) return rc;
    if ((rc = ps_edge_prepare(pl, P, vz, st, E, &room)) || !room) return rc;
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_pn_pieces.p, pc.data(), pc.size() * sizeof(PnPiece), hipMemcpyHostToDevice, st));
    if ((rc = ps_rw_upload(pl, R, nf, rw, st))) return rc;
    Q.e1 = nullptr;
    if (first_order) {
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_pn_e1.p, plan.e1.data(), plan.e1.size() * 8, hipMemcpyHostToDevice, st));
        Q.e1 = pl.d_pn_e1.as<double>();
    }
    Q.P = P;
    Q.pieces = pl.d_pn_pieces.as<PnPiece>();
    Q.npieces = (int)pc.size();
    Q.rw = pl.d_rw.as<double>();
    Q.edge_cnt = E.edge_cnt;
    Q.edge_list = E.edge_list;
    Q.vz = vz ? 1 : 0;
    Q.gmax = plan.gmax;
    if (pairs) {
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)ps_nufft_kernel<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)pn_lds_bytes<T>(2 * pn_lmax<T>(true), sizeof(T) == 8, true)));
        hipLaunchKernelGGL((ps_nufft_kernel<T, true>), dim3((unsigned)(tnum / 2 + 1)), dim3(PnCfg<T>::NTH), pn_lds_bytes<T>(Q.gmax, first_order, true), st, Q);
    } else {
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)ps_nufft_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pn_lds_bytes<T>(2 * PnCfg<T>::LMAX, sizeof(T) == 8)));
        hipLaunchKernelGGL(ps_nufft_kernel<T>, dim3((unsigned)P.nk), dim3(PnCfg<T>::NTH), pn_lds_bytes<T>(Q.gmax, first_order), st, Q);
    }
    int worst;
    if ((rc = ps_edge_finish<T>(pl, R, c, E, vz, nullptr, st, &worst)) || worst > PM_EMAX) return rc;
    *done = true;
    return IMPDAR_OK;
}

// ---- series path (ps_series.h): any v(z) profile -- pieces from the planner (ps_series_plan.h, cached per profile), tables, launch
template <typename T>
static int ps_series_run(PsPlan &pl, PsParams &P, const PsRoute &R, const PsCall &c, const PsAttempt &a, hipStream_t st, bool *done, const char **kernel)
{
    // a.alt > 0: what the kernel that would take the call otherwise is expected to need (per 8192 wavenumbers); the call is
    // taken only where the estimate from the planner.s model is SR_MARGIN (0.9) of that or less.  0: taken regardless (IMPDAR_PS_MFMA=7)
    *done = false;
    *kernel = "ps_series_kernel";
    const double *vmig = c.vmig, alt_ms_8192 = a.alt;
    const int snum = P.snum, tnum = P.tnum, nf = P.nf;
    constexpr bool dbl = sizeof(T) == 8;
    if (!P.herm || nf < 64 || nf > SR_NFMAX || snum < 32 || !R.vfinite || !ps_thr_off_band(R.thr.data(), snum)) return IMPDAR_OK;
    // (the kernel's coefficients take w = (i + 1) dw: the axis must be that to rounding -- 2 pi fftfreq is)
    double dw;
    if (!ps_axis_uniform(R.w.data(), nf, 2e-15, &dw)) return IMPDAR_OK;
    double kxh_max = 0.0;
    for (int k = 0; k < tnum; ++k) kxh_max = std::max(kxh_max, 0.5 * std::fabs(c.kx[k]));
    if (!(kxh_max > 0.0) || !std::isfinite(kxh_max)) return IMPDAR_OK;
    SrHostPlan &hp = pl.sr_plan;
    const bool same = hp.v.size() == (size_t)snum && memcmp(hp.v.data(), vmig, (size_t)snum * 8) == 0 && hp.dt == P.dt && hp.dw == dw &&
                      hp.nf == nf && hp.kxh_max == kxh_max && hp.dbl == dbl && !hp.pieces.empty();
    if (!same) {
        pl.sr_dev = false;
        impdar_trace("ps_series: planning the pieces of a %d-step profile", snum);
        if (!sr_make_plan(hp, vmig, snum, P.dt, dw, nf, kxh_max, dbl)) {
            hp.pieces.clear();
            return IMPDAR_OK;
        }
        impdar_trace("ps_series: %zu pieces", hp.pieces.size());
    }
    if (hp.pieces.empty() || hp.pieces.size() > 4096) return IMPDAR_OK;
    // a pair of rows per workgroup (ps_series_kernel<T, true>), as ps_nufft_run's.
    // float32 only: on float64 data the pair's records take the frequencies through LDS in four rounds of two gather passes each and the
    // kernel spills twice as much -- 8192^2: rising gradient 368 -> 365 ms, falling 274 -> 312, firn column 66 -> 72 (float32: 110 -> 77.5,
    // 52 -> 41, 14.7 -> 11.5; profiles/r06_series.txt section 7)
    const bool pairs = !dbl && !c.tk_out && tnum % 2 == 0 && !P.fhalf && ps_mirror_rows(P, R);
    if (alt_ms_8192 != 0.0) {
        // (alt < 0: per alive pair -- the per-step kernels)
        const double alt = alt_ms_8192 > 0.0 ? alt_ms_8192 : -alt_ms_8192 * hp.alive_pairs;
        const double rest = hp.model_cost - hp.model_gather;
        const double est = dbl ? SR_MS_GATHER_F64 * hp.model_gather + SR_MS_REST_F64 * rest
                               : SR_MS_GATHER_F32 * hp.model_gather + (pairs ? SR_MS_REST_PAIR_F32 : SR_MS_REST_F32) * rest;
        impdar_trace("ps_series: estimate %.1f ms per 8192 wavenumbers against %.1f", est, alt);
        if (est > SR_MARGIN * alt) return IMPDAR_OK;
    }
    bool need[13] = {};
    for (const SrPiece &pc : hp.pieces) need[pc.loglp] = true;
    SrParams Q;
    std::vector<double> rw;
    std::vector<T> ev(hp.ev.begin(), hp.ev.end());
    bool room;
    int rc;
    if (!ps_ensure_all({{&pl.d_sr_pieces, hp.pieces.size() * sizeof(SrPiece)}, {&pl.d_sr_ev, ev.size() * sizeof(T) + 16}, {&pl.d_rw, (size_t)nf * 8}})) return IMPDAR_OK;
    if ((rc = ps_grid_tables<T>(pl, need, Q, st, &room)) || !room) return rc;
    if ((rc = pl.pn_tw[9].ensure<T>(SR_TWLDS, st))) return rc;       // (the kernel keeps this one in LDS)
    Q.tw[9] = pl.pn_tw[9].buf.p;
    if (!pl.sr_dev) {
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_sr_pieces.p, hp.pieces.data(), hp.pieces.size() * sizeof(SrPiece), hipMemcpyHostToDevice, st));
        if (!ev.empty()) IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_sr_ev.p, ev.data(), ev.size() * sizeof(T), hipMemcpyHostToDevice, st));
    }
    if ((rc = ps_rw_upload(pl, R, nf, rw, st))) return rc;
    Q.P = P;
    Q.pieces = pl.d_sr_pieces.as<SrPiece>();
    Q.npieces = (int)hp.pieces.size();
    Q.ev = pl.d_sr_ev.p;
    Q.rw = pl.d_rw.as<double>();
    Q.kxh_max = kxh_max;
    {
        // the grids' LDS doubles as the scratch of the direct sums: the chunk sums of every wave and lane + one group's [L] partial sums
        int lmax = 0;
        for (const SrPiece &pc : hp.pieces) lmax = std::max(lmax, pc.len);
        const int direct_scratch = (SrCfg<T>::NTH / 64) * 64 * 12 + lmax * (int)sizeof(OCp<T>);
        Q.grid_bytes = (std::max(hp.grid_bytes, direct_scratch) + 15) & ~15;
    }
    if constexpr (!dbl) {
        if (pairs) {
            IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)ps_series_kernel<float, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)sr_lds_bytes<float>(SR_GRID_BYTES + 16, true)));
            hipLaunchKernelGGL((ps_series_kernel<float, true>), dim3((unsigned)(tnum / 2 + 1)), dim3(SrCfg<float>::NTH), sr_lds_bytes<float>(Q.grid_bytes, true), st, Q);
        }
    }
    if (!pairs) {
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)ps_series_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sr_lds_bytes<T>(SR_GRID_BYTES + 16)));
        hipLaunchKernelGGL(ps_series_kernel<T>, dim3((unsigned)P.nk), dim3(SrCfg<T>::NTH), sr_lds_bytes<T>(Q.grid_bytes), st, Q);
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    IMPDAR_HIP_CHECK(hipStreamSynchronize(st));            // (the host tables must outlive their copies)
    pl.sr_dev = true;
    *done = true;
    return IMPDAR_OK;
}

// ---- matrix-core path (ps_mfma.h): row-block table (pm_plan), launch
static int ps_mfma_run(PsPlan &pl, PsParams &P, const PsRoute &R, const PsCall &c, const PsAttempt &, hipStream_t st, bool *done, const char **kernel)
{
    *done = false;
    *kernel = "ps_mfma_kernel";
    const bool vz = c.vlen != 0;
    const int snum = P.snum, tnum = P.tnum;
    const std::vector<PsMfmaRun> &runs = R.runs;
    if ((vz && ps_known_overflow(pl, c.kx, tnum, runs)) || !pm_gate((int)runs.size(), P.nf, snum) || (vz && !ps_thr_off_band(R.thr.data(), snum))) return IMPDAR_OK;
    PmPlan plan;
    if (!pm_plan(plan, runs, vz, P.nf, snum)) return IMPDAR_OK;
    PsMfmaParams Q;
    Q.nruns = (int)runs.size();
    for (int r = 0; r < Q.nruns; ++r) Q.runs[r] = runs[r];
    for (int r = Q.nruns; r < PM_MAX_RUNS; ++r) Q.runs[r] = PsMfmaRun{0.0, 0, 0};
    Q.ngroups = plan.ngroups;
    Q.nlong = plan.nlong;
    std::copy(plan.long_of, plan.long_of + PM_MAX_RUNS, Q.long_of);
    // The path's own buffers (runtab: 16 bytes per wavenumber, frequency and long run -- 8.6 GB for 16 runs at
    // 8192 x 4096).  Not getting them is not an error: the vector kernels need none of it and take the call.
    const size_t rt_bytes = (size_t)P.nk * P.nf * Q.nlong * sizeof(double2);
    size_t free_b = 0, total_b = 0;
    if (rt_bytes > pl.d_runtab.bytes && hipMemGetInfo(&free_b, &total_b) == hipSuccess && rt_bytes > free_b / 2) {
        (void)hipGetLastError();
        return IMPDAR_OK;                  // would take more than half of what is free: leave it to the vector kernels
    }
    PsMfmaParams E;
    bool room;
    int rc;
    static_assert(sizeof(PmBlock) == sizeof(int2), "the row-block table is the kernel's int2 array");
    if (!ps_ensure_all({{&pl.d_blocks, plan.table.size() * sizeof(PmBlock)}, {&pl.d_runtab, rt_bytes}, {&pl.d_mcount, 8}})) return IMPDAR_OK;
    if ((rc = ps_edge_prepare(pl, P, vz, st, E, &room)) || !room) return rc;
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_blocks.p, plan.table.data(), plan.table.size() * sizeof(PmBlock), hipMemcpyHostToDevice, st));
    Q.P = P;
    Q.blocks = pl.d_blocks.as<int2>();
    Q.edge_cnt = E.edge_cnt;
    Q.edge_list = E.edge_list;
    Q.mfma_count = pl.d_mcount.as<unsigned long long>();
    IMPDAR_HIP_CHECK(hipMemsetAsync(Q.mfma_count, 0, 8, st));
    Q.vz = vz ? 1 : 0;
    Q.runtab = pl.d_runtab.as<double2>();
    // rows k and tnum - k turn by the same angles -- one set-up walk and one table row for both
    const bool sym = ps_mirror_rows(P, R);
    Q.pairs = sym ? 1 : 0;
    {
        // set-up pass: per-run phases of every (wavenumber, frequency), boundary frequencies, the steps of the short runs
        const size_t lds = 2 * 8 * 2 * PM_SHORT * sizeof(float);
        const dim3 grid(sym ? tnum / 2 + 1 : P.nk);
        if (P.nf <= 2048) hipLaunchKernelGGL(ps_setup_kernel<4>, grid, dim3(512), lds, st, Q);
        else if (P.nf <= 4096) hipLaunchKernelGGL(ps_setup_kernel<8>, grid, dim3(512), lds, st, Q);
        else hipLaunchKernelGGL(ps_setup_kernel<12>, grid, dim3(512), lds, st, Q);
    }
    IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)ps_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PM_LDS_BYTES));
    hipLaunchKernelGGL(ps_mfma_kernel, dim3((unsigned)P.nk * Q.ngroups), dim3(PM_WAVES * 64), PM_LDS_BYTES, st, Q);
    // (an overflow, or IMPDAR_PS_TEST_EDGE_OVERFLOW behaving as one: *done stays false, the vector kernels, which walk every
    // boundary frequency themselves, produce the result)
    int worst;
    if ((rc = ps_edge_finish<float>(pl, R, c, E, vz, nullptr, st, &worst)) || worst > PM_EMAX || (vz && c.K.edge_overflow)) return rc;
    if ((rc = ps_mcount_read(pl))) return rc;
    *done = true;
    return IMPDAR_OK;
}

// ---- ps_run, stage by stage.  What is decided on the host -- the walk, the runs, the layout, the order of attempts -- is
// ps_route.h's; the stages below allocate, upload and launch.

// the cached plan belongs to one context, size, dtype and transform form: anything else starts it over
static int ps_plan_bind(impdar_ctx *ctx, PsPlan &pl, bool dbl, int snum, int tnum, int nt, bool rows_form)
{
    const size_t csize = dbl ? 16 : 8;
    if (pl.owner == ctx && pl.dtype == (dbl ? IMPDAR_F64 : IMPDAR_F32) && pl.snum == snum && pl.tnum == tnum && pl.nt == nt &&
        pl.rows_form == rows_form)
        return IMPDAR_OK;
    pl.own_calls = 0;
    pl.dtype = -1;
    pl.rm_state = -1;
    if (pl.owner != ctx) {               // another device / stream: drop everything bound to the old one
        pl.release_device();
        pl.owner = ctx;
    }
    pl.r_ready = pl.c_ready = false;     // the forward transforms are made on first use (ps_make_plans): which pair depends on the walk
    pl.rows_form = rows_form;
    pl.b_ready = false;                  // the inverse transform over the traces: made beside the forward pair
    IMPDAR_HIP_CHECK(pl.X.ensure((size_t)tnum * nt * csize));
    IMPDAR_HIP_CHECK(pl.d_kx.ensure((size_t)tnum * 8));
    IMPDAR_HIP_CHECK(pl.d_w.ensure((size_t)nt * 8));
    IMPDAR_HIP_CHECK(pl.d_vz.ensure((size_t)snum * 8));
    IMPDAR_HIP_CHECK(pl.d_thr.ensure((size_t)snum * 8));
    pl.dtype = dbl ? IMPDAR_F64 : IMPDAR_F32;
    pl.snum = snum;
    pl.tnum = tnum;
    pl.nt = nt;
    return IMPDAR_OK;
}

// what the transforms run on: the twiddles of the library's own row kernels, or the rocFFT plans this call still lacks
template <typename T>
static int ps_make_plans(impdar_ctx *ctx, PsPlan &pl, const PsRoute &R, int snum, int tnum, int nt)
{
    hipStream_t st = ctx->stream;
    const bool dbl = sizeof(T) == 8, herm = R.herm;
    const int fstride = R.fstride;
    int rc;
    if (R.use_own) {
        IMPDAR_HIP_CHECK(pl.Xr.ensure((size_t)tnum * nt * sizeof(T)));
        pl.own_calls += 1;
        impdar_trace("phaseshift: transforms on the library's own row kernels");
        if ((rc = pl.tw_time.ensure<T>(nt, st)) || (rc = pl.tw_trace.ensure<T>(tnum, st))) return rc;
        return IMPDAR_OK;
    }
    // n-point complex transforms in place, `batch` of them: on contiguous rows, or strided through the array as it lies
    auto c2c = [&](FftPlan &p, rocfft_transform_type type, int n, int batch, bool rows, double scale) {
        const rocfft_array_type ci = rocfft_array_type_complex_interleaved;
        return rows ? p.create(type, dbl, true, n, batch, ci, ci, 1, n, 1, n, scale, st) : p.create(type, dbl, true, n, batch, ci, ci, batch, 1, batch, 1, scale, st);
    };
    // created side by side (run-time compilation: impdar_parallel_plans)
    std::vector<std::function<int()>> makers;
    if (!pl.b_ready) makers.push_back([&] { return c2c(pl.b_trace, rocfft_transform_type_complex_inverse, tnum, snum, pl.rows_form, 1.0 / tnum); });
    if (herm && !pl.r_ready) {
        IMPDAR_HIP_CHECK(pl.Xr.ensure((size_t)tnum * nt * sizeof(T)));
        makers.push_back([&] {
            return pl.r_time.create(rocfft_transform_type_real_forward, dbl, false, nt, tnum, rocfft_array_type_real,
                                    rocfft_array_type_hermitian_interleaved, 1, nt, 1, fstride, 1.0, st);
        });
        makers.push_back([&] { return c2c(pl.r_trace, rocfft_transform_type_complex_forward, tnum, fstride, pl.rows_form, 1.0); });
    }
    if (!herm && !pl.c_ready) {
        makers.push_back([&] { return c2c(pl.f_time, rocfft_transform_type_complex_forward, nt, tnum, true, 1.0); });
        makers.push_back([&] { return c2c(pl.f_trace, rocfft_transform_type_complex_forward, tnum, nt, false, 1.0); });
    }
    if (!makers.empty()) {
        impdar_trace("phaseshift: %zu rocFFT plans to make", makers.size());
        if ((rc = impdar_parallel_plans(ctx->device, makers))) return rc;
        impdar_trace("phaseshift: plans ready");
        pl.b_ready = true;
        if (herm) pl.r_ready = true;
        else pl.c_ready = true;
    }
    return IMPDAR_OK;
}

// the axes, the profile and the runs schedule of the call on the device (R owns the host copies: alive until ps_run's last sync)
static int ps_upload(PsPlan &pl, PsParams &P, const PsRoute &R, bool dbl, const double *kx, const double *vmig, hipStream_t st)
{
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_kx.p, kx, (size_t)P.tnum * 8, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_w.p, R.w.data(), (size_t)R.nf * 8, hipMemcpyHostToDevice, st));
    if (P.vz_mode) {
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_vz.p, vmig, (size_t)P.snum * 8, hipMemcpyHostToDevice, st));
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_thr.p, R.thr.data(), (size_t)P.snum * 8, hipMemcpyHostToDevice, st));
    }
    if (R.use_sched) {
        IMPDAR_HIP_CHECK(pl.d_sched.ensure(R.sched.size() * sizeof(int)));
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_sched.p, R.sched.data(), R.sched.size() * sizeof(int), hipMemcpyHostToDevice, st));
        P.sched = pl.d_sched.as<int>();
        P.tsched = P.sched + P.snum;
        if (dbl) {
            IMPDAR_HIP_CHECK(pl.d_eps.ensure(R.epsum.size() * sizeof(double)));
            IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_eps.p, R.epsum.data(), R.epsum.size() * sizeof(double), hipMemcpyHostToDevice, st));
            P.eps = pl.d_eps.as<double>();
        }
    }
    return IMPDAR_OK;
}

// the taper weights of the half layout (tap: the caller's, alive until its last sync); no room for them: the full layout
static int ps_taper_upload(PsPlan &pl, std::vector<double> &tap, int snum, int tnum, double htaper, double vtaper, hipStream_t st, bool *half_front)
{
    tap.resize((size_t)tnum + snum);
    for (int j = 0; j < tnum; ++j) tap[j] = impdar_taper_w(j, tnum, htaper);
    for (int i = 0; i < snum; ++i) tap[(size_t)tnum + i] = impdar_taper_w(i, snum, vtaper);
    if (pl.d_taper.ensure(((size_t)tnum + snum) * 8) != hipSuccess) {
        (void)hipGetLastError();
        *half_front = false;
        return IMPDAR_OK;
    }
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_taper.p, tap.data(), (size_t)tnum * 8, hipMemcpyHostToDevice, st));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_taper.as<double>() + tnum, tap.data() + tnum, (size_t)snum * 8, hipMemcpyHostToDevice, st));
    return IMPDAR_OK;
}

// the transforms of the [k][w > 0] layout every kernel reads (Hermitian walk on the library's own or rocFFT's plans)
template <typename T>
static int ps_front_full(PsPlan &pl, const PsParams &P, const PsRoute &R, const void *d_data, double htaper, double vtaper, hipStream_t st)
{
    const int snum = P.snum, tnum = P.tnum, nt = P.nt, fstride = R.fstride;
    int rc;
    hipLaunchKernelGGL((ps_taper_pad_transpose_real<T>), dim3((tnum + 63) / 64, (nt + 63) / 64), dim3(256), 0, st, (const T *)d_data,
                       pl.Xr.as<T>(), snum, tnum, nt, htaper, vtaper);
    if (R.use_own) {
        if ((rc = own_fft_launch<T>(OWN_R2C, nt, (size_t)tnum, pl.Xr.p, pl.X.p, (size_t)nt, (size_t)fstride, 1.0, pl.tw_time, st))) return rc;
    } else if ((rc = pl.r_time.exec(pl.Xr.p, pl.X.p))) {
        return rc;
    }
    if (pl.rows_form) {
        // over the traces on contiguous rows: X [x][fstride] -> [fstride][x] (pl.TK is free until the frequency sums
        // write it, and large enough: snum > nt / 2), transform, and back -> X [k][fstride]
        ps_launch_transpose<T>(pl.X.p, pl.TK.p, tnum, fstride, st);
        if (R.use_own) {
            if ((rc = own_fft_launch<T>(OWN_C2C_FWD, tnum, (size_t)fstride, pl.TK.p, pl.TK.p, (size_t)tnum, (size_t)tnum, 1.0, pl.tw_trace, st))) return rc;
        } else if ((rc = pl.r_trace.exec(pl.TK.p, nullptr))) {
            return rc;
        }
        ps_launch_transpose<T>(pl.TK.p, pl.X.p, fstride, tnum, st);
        IMPDAR_HIP_CHECK(hipGetLastError());
    } else if ((rc = pl.r_trace.exec(pl.X.p, nullptr))) {
        return rc;
    }
    return IMPDAR_OK;
}

// the forward transforms in one of three layouts: k >= 0 with all frequencies (half_front: the trace transform first), the
// Hermitian walk's [k][w > 0], or the reference's complex walk
template <typename T>
static int ps_front(PsPlan &pl, PsParams &P, const PsRoute &R, bool half_front, const void *d_data, double htaper, double vtaper, hipStream_t st)
{
    const int snum = P.snum, tnum = P.tnum, nt = P.nt;
    int rc;
    if (R.herm && half_front) {
        const int hs = tnum / 2 + 1;
        const double *th = pl.d_taper.as<double>(), *tv = th + tnum;
        // (pl.TK: free until the frequency sums write it, and at least tnum x snum complex)
        if ((rc = own_fft_launch<T>(OWN_R2C, tnum, (size_t)snum, d_data, pl.TK.p, (size_t)tnum, (size_t)hs, 1.0, pl.tw_trace, st, th, tv))) return rc;
        constexpr int TS = sizeof(T) == 4 ? 64 : 32;
        hipLaunchKernelGGL((ps_transpose_pad<T, TS>), dim3((hs + TS - 1) / TS, (nt + TS - 1) / TS), dim3(256), 0, st, pl.TK.as<Cp<T>>(),
                           pl.X.as<Cp<T>>(), snum, hs, nt);
        if ((rc = own_fft_launch<T>(OWN_C2C_FWD, nt, (size_t)hs, pl.X.p, pl.X.p, (size_t)nt, (size_t)nt, 1.0, pl.tw_time, st))) return rc;
        IMPDAR_HIP_CHECK(hipGetLastError());
        P.fhalf = 1;
        P.fstride = nt;
        impdar_trace("phaseshift: the transform over the traces first: wavenumbers k >= 0 with all frequencies, for pairs in ps_nufft_kernel");
        return IMPDAR_OK;
    }
    if (R.herm) return ps_front_full<T>(pl, P, R, d_data, htaper, vtaper, st);
    hipLaunchKernelGGL((ps_taper_pad_transpose<T>), dim3((tnum + 63) / 64, (nt + 63) / 64), dim3(256), 0, st, (const T *)d_data,
                       pl.X.as<Cp<T>>(), snum, tnum, nt, htaper, vtaper);
    if ((rc = pl.f_time.exec(pl.X.p, nullptr))) return rc;
    return pl.f_trace.exec(pl.X.p, nullptr);
}

// the launch order of the runs kernels of the vector path (ps_row_order, ps_route.h).  It depends on the axes and the profile
// only: a repeated geometry re-uses the last one.  rowmap: the caller's, alive until its last sync.
static int ps_order_rows(PsPlan &pl, PsParams &P, const PsRoute &R, std::vector<int> &rowmap, const double *kx, const double *ws,
                         const double *vmig, bool dbl, hipStream_t st)
{
    const int snum = P.snum, tnum = P.tnum, nt = P.nt;
    if (P.nk != tnum) return IMPDAR_OK;                          // (a slab of a sharded run keeps the natural order)
    if (pl.rm_state >= 0 && pl.rm_kx.size() == (size_t)tnum && pl.rm_ws.size() == (size_t)nt && pl.rm_v.size() == (size_t)snum &&
        memcmp(pl.rm_kx.data(), kx, (size_t)tnum * 8) == 0 && memcmp(pl.rm_ws.data(), ws, (size_t)nt * 8) == 0 &&
        memcmp(pl.rm_v.data(), vmig, (size_t)snum * 8) == 0) {
        if (pl.rm_state == 1) P.rowmap = pl.d_rowmap.as<int>();
        return IMPDAR_OK;
    }
    pl.rm_state = -1;
    pl.rm_kx.assign(kx, kx + tnum);
    pl.rm_ws.assign(ws, ws + nt);
    pl.rm_v.assign(vmig, vmig + snum);
    rowmap = ps_row_order(kx, tnum, ws, nt, R.runs, P.dt, dbl);
    pl.rm_state = 0;
    if (!rowmap.empty()) {
        IMPDAR_HIP_CHECK(pl.d_rowmap.ensure((size_t)tnum * sizeof(int)));
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_rowmap.p, rowmap.data(), (size_t)tnum * sizeof(int), hipMemcpyHostToDevice, st));
        P.rowmap = pl.d_rowmap.as<int>();
        pl.rm_state = 1;
    }
    return IMPDAR_OK;
}

// no runs of constant velocity to live on (the velocity changes in most 16-step tiles): ps_smooth_kernel.  Declines (*done
// false) on a profile that is not finite, a vertical taper inside the record, or no room for the partial images.
template <typename T>
static int ps_smooth_run(PsPlan &pl, PsParams &P, const PsRoute &R, const PsCall &c, const PsAttempt &, hipStream_t st, bool *done, const char **kernel)
{
    const int snum = P.snum;
    const double *vmig = c.vmig;
    *done = false;
    if (!R.vfinite || !ps_thr_off_band(R.thr.data(), snum)) return IMPDAR_OK;
    // float32, the whole wavenumber axis with kx[tnum - k] = -kx[k]: rows k and tnum - k in one wave (ps_smooth.h)
    const bool sm_pairs = ps_mirror_rows(P, R);
    P.sm_m = ps_smooth_m(sizeof(T) == 8, sm_pairs);
    P.sm_nchunks = ps_smooth_chunks(R.nf, P.sm_m);
    const size_t part_bytes = P.sm_nchunks > 1 ? (size_t)P.sm_nchunks * P.nk * snum * sizeof(Cp<T>) : 0;
    std::vector<double> &sm_step = pl.h_sm_step, &sm_tile = pl.h_sm_tile;     // (alive until the next call: async copies)
    if (sizeof(T) == 4) ps_smooth_tables(vmig, R.thr.data(), snum, sm_step, sm_tile);
    if (pl.d_sm.ensure((sm_step.size() + sm_tile.size()) * 8 + 64) != hipSuccess || (part_bytes && pl.d_part.ensure(part_bytes) != hipSuccess)) {
        (void)hipGetLastError();
        P.sm_nchunks = 1;
        return IMPDAR_OK;
    }
    if (sizeof(T) == 4) {
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_sm.p, sm_step.data(), sm_step.size() * 8, hipMemcpyHostToDevice, st));
        IMPDAR_HIP_CHECK(hipMemcpyAsync(pl.d_sm.as<double>() + sm_step.size(), sm_tile.data(), sm_tile.size() * 8, hipMemcpyHostToDevice, st));
        P.sm_step = pl.d_sm.as<double>();
        P.sm_tile = pl.d_sm.as<double>() + sm_step.size();
    }
    P.sm_part = pl.d_part.p;
    ps_smooth_launch<T>(P, st, sm_pairs);
    IMPDAR_HIP_CHECK(hipGetLastError());
    *kernel = sizeof(T) == 4 ? "ps_smooth32_kernel" : "ps_smooth_kernel";
    *done = true;
    return IMPDAR_OK;
}

// the metrics line of the call (kernel: the frequency-sum kernel that took it)
static void ps_metrics(impdar_ctx *ctx, const PsPlan &pl, const PsParams &P, const PsRoute &R, const char *kernel, bool matrix_counted, bool tk_out)
{
    ctx->m_entry = tk_out ? "impdar_phaseshift_tk_dev" : "impdar_phaseshift";
    ctx->m_kernel = kernel;
    ctx->m_kernel_ms = -1.f;                 // (bracketed by ktic / ktoc)
    char *x = ctx->m_extra;
    const size_t cap = sizeof ctx->m_extra;      // (320: the part both forms share is under 110)
    const int n = snprintf(x, cap, "\"hermitian_walk\": %s, \"frequencies\": %d, \"transforms\": \"%s\", \"long_runs\": %d, ", R.herm ? "true" : "false", R.nf,
                           R.use_own ? "own" : "rocfft", R.long_runs_metric);
    if (matrix_counted)      // (MFMA instructions the kernel issued, counted by the kernel: rounds and blocks it skips are not in it)
        snprintf(x + n, cap - n, "\"mfma_instructions\": %.0f, \"flop_per_mfma\": %d", pl.mfma_instructions, strcmp(kernel, "ps_runs_kernel") == 0 ? 16384 : 32768);
    else
        snprintf(x + n, cap - n, "\"spectrum\": \"%s\"", P.fhalf ? "k >= 0, all frequencies" : "all k, frequencies walked");
}

// the zero-frequency rows, then the inverse transform over k and the real part (:282); a rank of a kx-sharded run stops at its sums
template <typename T>
static int ps_back(impdar_ctx *ctx, PsPlan &pl, const PsParams &P, const PsRoute &R, bool tk_out, void *d_out)
{
    hipStream_t st = ctx->stream;
    const int snum = P.snum, tnum = P.tnum;
    int rc;
    if (R.herm)
        for (int kz : R.k_zero)
            if (kz >= P.k0 && kz < P.k0 + P.nk)
                hipLaunchKernelGGL((ps_dc_kernel<T>), dim3((snum + 255) / 256), dim3(256), 0, st, pl.X.as<Cp<T>>(),
                                   reinterpret_cast<Cp<T> *>(P.TK), kz, kz - P.k0, P.fstride, snum, R.w0 * P.dt);
    if ((rc = impdar_ctx_ktoc(ctx))) return rc;
    if (tk_out) {
        IMPDAR_HIP_CHECK(hipGetLastError());
        return impdar_ctx_toc(ctx);
    }
    if (pl.rows_form) {
        // inverse over k on contiguous rows: TK [k][tau] -> [tau][k] (pl.X: the spectrum is not needed any more, and
        // nt >= snum), transform, real part (:282) -- already (snum, tnum)
        if (R.use_own && tnum >= 32) {
            // (the real part is all that is kept: the Hermitian half of the sums goes through a real inverse transform of half
            // the length -- ps_transpose_herm; until round 6 a full transpose and a complex transform that stored real parts:
            // 175 + 314 us at 8192^2 float32)
            const int hs = tnum / 2 + 1;
            ps_launch_transpose_herm<T>(pl.TK.p, pl.X.p, tnum, snum, hs, st);
            if ((rc = own_fft_launch<T>(OWN_C2R, tnum, (size_t)snum, pl.X.p, d_out, (size_t)hs, (size_t)tnum, 1.0 / tnum, pl.tw_trace, st))) return rc;
        } else if (R.use_own) {
            ps_launch_transpose<T>(pl.TK.p, pl.X.p, tnum, snum, st);
            if ((rc = own_fft_launch<T>(OWN_C2C_INV_RE, tnum, (size_t)snum, pl.X.p, d_out, (size_t)tnum, (size_t)tnum, 1.0 / tnum, pl.tw_trace, st))) return rc;
        } else {
            ps_launch_transpose<T>(pl.TK.p, pl.X.p, tnum, snum, st);
            if ((rc = pl.b_trace.exec(pl.X.p, nullptr))) return rc;
            const size_t n = (size_t)snum * tnum;
            hipLaunchKernelGGL((ps_real_part<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pl.X.as<Cp<T>>(), (T *)d_out, n);
        }
    } else {
        if ((rc = pl.b_trace.exec(pl.TK.p, nullptr))) return rc;
        hipLaunchKernelGGL((ps_real_transpose<T>), dim3((tnum + 63) / 64, (snum + 63) / 64), dim3(256), 0, st, pl.TK.as<Cp<T>>(), (T *)d_out, snum, tnum);
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    if ((rc = impdar_ctx_toc(ctx))) return rc;
    impdar_trace("phaseshift: all kernels enqueued");
    return IMPDAR_OK;
}

template <typename T>
static int ps_run(impdar_ctx *ctx, PsPlan &pl, const void *d_data, int snum, int tnum, int nt, const double *kx,
                  const double *ws, double dt, const double *tt_us, double vconst, const double *vmig, int vlen,
                  double htaper, double vtaper, void *d_out, int k0 = 0, int nk = -1, void *tk_out = nullptr)
{
    // tk_out != null: a rank of a kx-sharded run -- the transforms (replicated on every rank) and the frequency sums of
    // wavenumbers [k0, k0 + nk) only, written to tk_out [nk][snum]; no inverse transform (impdar_phaseshift_finish_dev)
    if (nk < 0) nk = tnum;
    hipStream_t st = ctx->stream;
    const bool dbl = sizeof(T) == 8;
    const PsKnobs K = ps_knobs_read();
    int rc;
    if ((rc = ps_plan_bind(ctx, pl, dbl, snum, tnum, nt, K.rows_form))) return rc;
    const PsRoute R = ps_route(dbl, snum, tnum, nt, kx, ws, dt, tt_us, vconst, vmig, vlen, k0, nk, tk_out != nullptr, K);
    {
        // TK: the frequency sums [tnum][snum] of an unsharded call, and the scratch of the transposed forward transform
        // (nt / 2 + 1 rows of tnum -- more than snum rows when the caller pads the time axis beyond the next power of
        // two).  A rank of a kx-sharded run writes its sums to the caller's slab: it only needs the scratch.
        const size_t scratch_rows = (R.herm && pl.rows_form) ? (size_t)(nt / 2 + 1) : 0;
        const size_t rows = tk_out ? scratch_rows : std::max<size_t>((size_t)snum, scratch_rows);
        if (rows) IMPDAR_HIP_CHECK(pl.TK.ensure((size_t)tnum * rows * 2 * sizeof(T)));
    }
    if ((rc = ps_make_plans<T>(ctx, pl, R, snum, tnum, nt))) return rc;
    PsParams P = {};                         // (no schedule, row order or smooth tables, fhalf 0: set where they are made)
    P.F = pl.X.p;
    P.TK = tk_out ? tk_out : pl.TK.p;
    P.kx = pl.d_kx.as<double>();
    P.w = pl.d_w.as<double>();
    P.vz = pl.d_vz.as<double>();
    P.thr = pl.d_thr.as<double>();
    P.vconst = vconst;
    P.dt = dt;
    P.vtol = dbl ? 1e-11 : 1e-10;
    P.snum = snum;
    P.tnum = tnum;
    P.nt = nt;
    P.nf = R.nf;
    P.fstride = R.fstride;
    P.k0 = k0;
    P.nk = nk;
    P.herm = R.herm ? 1 : 0;
    P.vz_mode = vlen ? 1 : 0;
    P.sm_nchunks = 1;
    P.sm_m = 8;
    if ((rc = ps_upload(pl, P, R, dbl, kx, vmig, st))) return rc;
    bool half_front = R.half_front;
    std::vector<double> tap;                 // (host staging of this call: alive until the last sync)
    std::vector<int> rowmap;
    if (half_front && (rc = ps_taper_upload(pl, tap, snum, tnum, htaper, vtaper, st, &half_front))) return rc;
    if ((rc = impdar_ctx_tic(ctx))) return rc;
    if ((rc = ps_front<T>(pl, P, R, half_front, d_data, htaper, vtaper, st))) return rc;
    if ((rc = impdar_ctx_ktic(ctx))) return rc;
    impdar_trace("phaseshift: forward transforms enqueued");
    bool done = false;
    const char *kernel = "";
    pl.mfma_instructions = -1.0;
    using PsRunner = int (*)(PsPlan &, PsParams &, const PsRoute &, const PsCall &, const PsAttempt &, hipStream_t, bool *, const char **);
    static const PsRunner runners[] = {ps_series_run<T>, ps_nufft_run<T>, ps_runs_run, ps_mfma_run, ps_smooth_run<T>};      // by PsAttemptKind
    static_assert(PS_SERIES == 0 && PS_NUFFT == 1 && PS_RUNS == 2 && PS_MFMA == 3 && PS_SMOOTH == 4, "the runners in the order of their kinds");
    const PsCall call{kx, vmig, vlen, tk_out != nullptr, K};
    for (const PsAttempt &a : R.attempts) {
        // Only ps_nufft_kernel reads the half layout: a call it handed on gets the other one (SERIES never meets fhalf: its conditions exclude half_front's)
        if (P.fhalf && a.kind != PS_NUFFT) {
            impdar_trace("phaseshift: the transform path handed the call on: transforms repeated in the [k][w > 0] layout");
            P.fhalf = 0;
            P.fstride = R.fstride;
            if ((rc = ps_front_full<T>(pl, P, R, d_data, htaper, vtaper, st))) return rc;
        }
        if (a.kind == PS_VECTOR) {      // with a schedule, the launch order of its runs kernels is made now
            if (R.use_sched && (rc = ps_order_rows(pl, P, R, rowmap, kx, ws, vmig, dbl, st))) return rc;
            if ((rc = ps_dispatch<T>(P, st))) return rc;
            kernel = t_ps_kernel;
            done = true;
        } else {
            rc = runners[a.kind](pl, P, R, call, a, st, &done, &kernel);
        }
        if (rc) return rc;
        if (done) {
            ps_metrics(ctx, pl, P, R, kernel, a.kind <= PS_MFMA && pl.mfma_instructions >= 0.0, tk_out != nullptr);
            break;
        }
    }
    if ((rc = ps_back<T>(ctx, pl, P, R, tk_out != nullptr, d_out))) return rc;
    // host staging vectors (R.w, R.thr, the schedule, tap, rowmap) must outlive the async copies
    IMPDAR_HIP_CHECK(hipStreamSynchronize(st));
    return IMPDAR_OK;
}

// What the three entry points that run ps_run share: the argument checks in their one order, the device, the lock on the
// cached plan, the float / double choice.  `slab`: the call is a rank of a kx-sharded run -- `out` takes the frequency sums of
// wavenumbers [k0, k0 + nk) and there is no inverse transform.  `before(&in, &out)` runs on the device set and ahead of the
// lock; it may replace the two arrays (impdar_phaseshift: its host arrays by device copies).
template <typename Before>
static int ps_enter(impdar_ctx *ctx, const void *in, void *out, int dtype, int snum, int tnum, int nt, const double *kx,
                    const double *ws, double dt, const double *tt_us, double vconst, const double *vmig, int vmig_len,
                    double htaper, double vtaper, bool slab, int k0, int nk, Before before)
{
    IMPDAR_ARG_CHECK(ctx && in && out && kx && ws && tt_us, "null argument");
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1 && nt >= snum, "bad sizes snum %d tnum %d nt %d", snum, tnum, nt);
    if (slab) IMPDAR_ARG_CHECK(k0 >= 0 && nk >= 0 && k0 + nk <= tnum, "wavenumber slab [%d, %d) outside [0, %d)", k0, k0 + nk, tnum);
    IMPDAR_ARG_CHECK(vmig_len == 0 || (vmig_len == snum && vmig),
                     "Interpolated velocity profile is not the length of the number of samples in a trace.");
    if (slab && nk == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    int rc = before(&in, &out);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_ps_mu);
    ImpdarBusy busy(t_ps_busy);
    if (!g_ps_plan) g_ps_plan = new PsPlan();
    auto run = dtype == IMPDAR_F32 ? ps_run<float> : ps_run<double>;
    return run(ctx, *g_ps_plan, in, snum, tnum, nt, kx, ws, dt, tt_us, vconst, vmig, vmig_len, htaper, vtaper, slab ? nullptr : out,
               slab ? k0 : 0, slab ? nk : -1, slab ? out : nullptr);
}
static int ps_nothing_before(const void **, void **) { return IMPDAR_OK; }

extern "C" int impdar_phaseshift(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum, int nt,
                                 const double *kx, const double *ws, double dt, const double *tt_us, double vconst,
                                 const double *vmig, int vmig_len, double htaper, double vtaper, void *out)
{
    CallArrays a{ctx};
    const size_t bytes = (size_t)snum * tnum * impdar_dtype_size(dtype);
    int rc = ps_enter(ctx, data, out, dtype, snum, tnum, nt, kx, ws, dt, tt_us, vconst, vmig, vmig_len, htaper, vtaper, false, 0, -1,
                      [&](const void **d_in, void **d_out) -> int {
        impdar_trace("impdar_phaseshift: enter (%d x %d, nt %d)", snum, tnum, nt);
        impdar_ctx_pinned_prefetch(ctx, std::min(bytes, IMPDAR_STAGE_RING_BYTES));      // the download's staging ring, pinned while the call works
        const int rc = a.alloc(bytes, bytes);
        if (rc) return rc;
        IMPDAR_HIP_CHECK(hipMemcpyAsync(a.din, data, bytes, hipMemcpyHostToDevice, ctx->stream));
        impdar_trace("impdar_phaseshift: upload enqueued");
        *d_in = a.din;
        *d_out = a.dout;
        return IMPDAR_OK;
    });
    if (rc) return rc;
    impdar_trace("impdar_phaseshift: device work complete");
    rc = impdar_download(ctx, out, a.dout, bytes, ctx->stream);
    impdar_trace("impdar_phaseshift: downloaded");
    return rc;
}

// resident form: d_data and d_out are device arrays of `dtype` (snum, tnum); runs on the context's compute stream
extern "C" int impdar_phaseshift_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int nt,
                                     const double *kx, const double *ws, double dt, const double *tt_us, double vconst,
                                     const double *vmig, int vmig_len, double htaper, double vtaper, void *d_out)
{
    const int rc = ps_enter(ctx, d_data, d_out, dtype, snum, tnum, nt, kx, ws, dt, tt_us, vconst, vmig, vmig_len, htaper, vtaper,
                            false, 0, -1, ps_nothing_before);
    return rc ? rc : impdar_ctx_mark_produced(ctx);
}

// ---------------------------------------------------------------------------
// Sharding over the wavenumbers (optional row): every wavenumber is independent in phaseShift
// (mig_python.py:396-487), so rank r computes TK for its slab of k -- the cheap forward transforms are replicated on
// every rank from the whole radargram --, the slabs are redistributed into depth-row slabs by one all-to-all, and
// every rank finishes its rows with the inverse transform over k (:282).  Three calls per rank:
//   impdar_phaseshift_tk_dev      d_tk [nk][snum] complex: frequency sums of wavenumbers [k0, k0 + nk)
//   impdar_ps_alltoall_dev        d_tk -> d_t2 [tnum][tw] complex: ALL wavenumbers, this rank's depth rows [tau0, tau0 + tw)
//   impdar_phaseshift_finish_dev  d_t2 -> d_out (tw, tnum) real: ifft over k, real part
// ---------------------------------------------------------------------------
extern "C" int impdar_phaseshift_tk_dev(impdar_ctx *ctx, const void *d_data, int dtype, int snum, int tnum, int nt,
                                        const double *kx, const double *ws, double dt, const double *tt_us, double vconst,
                                        const double *vmig, int vmig_len, double htaper, double vtaper, int k0, int nk,
                                        void *d_tk)
{
    const int rc = ps_enter(ctx, d_data, d_tk, dtype, snum, tnum, nt, kx, ws, dt, tt_us, vconst, vmig, vmig_len, htaper, vtaper,
                            true, k0, nk, ps_nothing_before);
    if (rc || nk == 0) return rc;       // (an empty slab: nothing was enqueued)
    return impdar_ctx_mark_produced(ctx);
}

// rows [0, nk) x columns [tau0, tau0 + tw) of a [nk][snum] complex array -> contiguous [nk][tw]
template <typename T>
__global__ __launch_bounds__(256) void ps_pack_kernel(const Cp<T> *__restrict__ src, Cp<T> *__restrict__ dst, int nk, int snum,
                                                      int tau0, int tw)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nk * tw) return;
    const size_t r = i / tw, j = i % tw;
    dst[i] = src[r * snum + tau0 + j];
}

// defined in comm.hip
int impdar_exchange_buffers(impdar_ctx *ctx, const void *sendbuf, void *recvbuf, int npeer, const int *peer, const size_t *soff,
                            const size_t *slen, const size_t *roff, const size_t *rlen, hipStream_t stream);

// `tau_edges` / `k_edges`: nranks + 1 edges of the depth-row and wavenumber slabs (the same on every rank).  Rank r
// sends block (its k slab) x (depth slab of s) to every rank s and receives (k slab of s) x (its depth slab), which
// lands at row k_edges[s] of d_t2 [tnum][tw]: the k-major layout the inverse transform wants, no unpacking.
extern "C" int impdar_ps_alltoall_dev(impdar_ctx *ctx, const void *d_tk, int dtype, int snum, int tnum, int nranks, int rank,
                                      const int *tau_edges, const int *k_edges, void *d_t2)
{
    IMPDAR_ARG_CHECK(ctx && d_tk && d_t2 && tau_edges && k_edges, "null argument");
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    IMPDAR_ARG_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank %d of %d", rank, nranks);
    IMPDAR_ARG_CHECK(tau_edges[0] == 0 && tau_edges[nranks] == snum && k_edges[0] == 0 && k_edges[nranks] == tnum,
                     "slab edges must run from 0 to snum / tnum");
    for (int s = 0; s < nranks; ++s)
        IMPDAR_ARG_CHECK(tau_edges[s + 1] >= tau_edges[s] && k_edges[s + 1] >= k_edges[s], "slab edges must not decrease");
    IMPDAR_ARG_CHECK(nranks == 1 || (ctx->comm && ctx->nranks == nranks), "communicator of %d ranks needed", nranks);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t esz = 2 * impdar_dtype_size(dtype);
    const int nk = k_edges[rank + 1] - k_edges[rank], tw = tau_edges[rank + 1] - tau_edges[rank];
    std::lock_guard<std::mutex> lk(g_ps_mu);
    ImpdarBusy busy(t_ps_busy);
    if (!g_ps_plan) g_ps_plan = new PsPlan();
    PsPlan &pl = *g_ps_plan;
    IMPDAR_HIP_CHECK(pl.d_sendbuf.ensure(std::max<size_t>((size_t)nk * snum * esz, 16)));
    std::vector<int> peer(nranks);
    std::vector<size_t> soff(nranks), slen(nranks), roff(nranks), rlen(nranks);
    size_t at = 0;
    for (int s = 0; s < nranks; ++s) {
        const int tws = tau_edges[s + 1] - tau_edges[s], nks = k_edges[s + 1] - k_edges[s];
        peer[s] = s;
        soff[s] = at;
        slen[s] = (size_t)nk * tws * esz;
        roff[s] = (size_t)k_edges[s] * tw * esz;
        rlen[s] = (size_t)nks * tw * esz;
        if (nk > 0 && tws > 0) {
            const unsigned grid = (unsigned)(((size_t)nk * tws + 255) / 256);
            if (dtype == IMPDAR_F32)
                hipLaunchKernelGGL((ps_pack_kernel<float>), dim3(grid), dim3(256), 0, st, (const Cp<float> *)d_tk,
                                   reinterpret_cast<Cp<float> *>(pl.d_sendbuf.as<char>() + at), nk, snum, tau_edges[s], tws);
            else
                hipLaunchKernelGGL((ps_pack_kernel<double>), dim3(grid), dim3(256), 0, st, (const Cp<double> *)d_tk,
                                   reinterpret_cast<Cp<double> *>(pl.d_sendbuf.as<char>() + at), nk, snum, tau_edges[s], tws);
        }
        at += slen[s];
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    int rc;
    if (ctx->comm) {
        if ((rc = impdar_exchange_buffers(ctx, pl.d_sendbuf.p, d_t2, nranks, peer.data(), soff.data(), slen.data(), roff.data(),
                                          rlen.data(), st)))
            return rc;
    } else {
        // one rank, no communicator: the only block goes to itself
        IMPDAR_HIP_CHECK(hipMemcpyAsync(reinterpret_cast<char *>(d_t2) + roff[0], pl.d_sendbuf.as<char>() + soff[0], slen[0],
                                        hipMemcpyDeviceToDevice, st));
    }
    IMPDAR_HIP_CHECK(hipStreamSynchronize(st));
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_phaseshift_finish_dev(impdar_ctx *ctx, void *d_t2, int dtype, int tw, int tnum, void *d_out)
{
    IMPDAR_ARG_CHECK(ctx && d_t2 && d_out, "null argument");
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    IMPDAR_ARG_CHECK(tw >= 0 && tnum >= 1, "bad sizes tw %d tnum %d", tw, tnum);
    if (tw == 0) return IMPDAR_OK;
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(g_ps_mu);
    ImpdarBusy busy(t_ps_busy);
    if (!g_ps_plan) g_ps_plan = new PsPlan();
    PsPlan &pl = *g_ps_plan;
    const bool dbl = dtype == IMPDAR_F64;
    hipStream_t st = ctx->stream;
    int rc;
    if (pl.slab_key[0] != dtype || pl.slab_key[1] != tw || pl.slab_key[2] != tnum || pl.slab_owner != ctx) {
        const rocfft_array_type ci = rocfft_array_type_complex_interleaved;
        if ((rc = pl.b_slab.create(rocfft_transform_type_complex_inverse, dbl, true, tnum, tw, ci, ci, 1, tnum, 1, tnum, 1.0 / tnum, st)))
            return rc;
        pl.slab_key[0] = dtype, pl.slab_key[1] = tw, pl.slab_key[2] = tnum;
        pl.slab_owner = ctx;
    }
    // ifft over k (:282) on contiguous rows: [k][tau] -> [tau][k], transform, real part
    const size_t n = (size_t)tw * tnum;
    IMPDAR_HIP_CHECK(pl.d_slab.ensure(n * 2 * impdar_dtype_size(dtype)));
    if (dbl) ps_launch_transpose<double>(d_t2, pl.d_slab.p, tnum, tw, st);
    else ps_launch_transpose<float>(d_t2, pl.d_slab.p, tnum, tw, st);
    if ((rc = pl.b_slab.exec(pl.d_slab.p, nullptr))) return rc;
    if (dbl)
        hipLaunchKernelGGL((ps_real_part<double>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pl.d_slab.as<Cp<double>>(),
                           (double *)d_out, n);
    else
        hipLaunchKernelGGL((ps_real_part<float>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pl.d_slab.as<Cp<float>>(),
                           (float *)d_out, n);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return impdar_ctx_mark_produced(ctx);
}

extern "C" int impdar_taper(impdar_ctx *ctx, void *data_inout, int dtype, int snum, int tnum, double htaper,
                            double vtaper)
{
    IMPDAR_ARG_CHECK(ctx && data_inout, "null argument");
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    IMPDAR_ARG_CHECK(snum >= 1 && tnum >= 1, "bad sizes snum %d tnum %d", snum, tnum);
    IMPDAR_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)snum * tnum, bytes = n * impdar_dtype_size(dtype);
    DevBuf d;
    IMPDAR_HIP_CHECK(d.ensure(bytes));
    IMPDAR_HIP_CHECK(hipMemcpyAsync(d.p, data_inout, bytes, hipMemcpyHostToDevice, ctx->stream));
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (dtype == IMPDAR_F32)
        hipLaunchKernelGGL((ps_taper_inplace<float>), dim3(grid), dim3(256), 0, ctx->stream, d.as<float>(), snum, tnum,
                           htaper, vtaper);
    else
        hipLaunchKernelGGL((ps_taper_inplace<double>), dim3(grid), dim3(256), 0, ctx->stream, d.as<double>(), snum, tnum,
                           htaper, vtaper);
    IMPDAR_HIP_CHECK(hipGetLastError());
    IMPDAR_HIP_CHECK(hipMemcpyAsync(data_inout, d.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    IMPDAR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    impdar_ctx_note(ctx, "impdar_taper", "ps_taper_inplace");
    return IMPDAR_OK;
}
