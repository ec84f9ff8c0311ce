// What the path runners of the phase shift (ps_nufft_run, ps_runs_run, ps_mfma_run, ps_series_run: phaseshift.hip) plan on the host
// before they launch: the runs of constant velocity cut into the pieces, stages and row blocks their kernels walk, every rule by
// which a path declines a call for a host-side reason, and the checks on the axes they share.  Plain C++, no device code -- compiled
// into the library by phaseshift.hip (through ps_route.h) and, by itself with g++, into the CPU suite's checker
// (tests/test_ps_path_plan.py).  The structs that go to the device as they are (PnPiece, PrRun, PrStage, PmBlock, PsMfmaRun) and the
// constants both sides read live here; ps_nufft.h, ps_runs.h and ps_mfma.h hold the kernels.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

struct PsMfmaRun {
    double v;               // velocity of the run (v(z)); unused for constant velocity
    int start, len;         // first depth step, number of steps
};

// ---- checks several paths share ------------------------------------------------------------------------------------------------
// the evanescence test must be the sign of coss off the boundary band: (tau / tau_max)^2 below 1e-10 at every step
static inline bool ps_thr_off_band(const double *thr, int snum)
{
    for (int i = 0; i < snum; ++i)
        if (!(thr[i] < 1e-10)) return false;
    return true;
}

// the transform paths' gather inverts the dispersion relation on a uniform frequency axis: slot i + 1 at (i + 1) dw, the Nyquist
// row (slot 0) at nf dw, each within tol (relative).  *dw: the spacing
static inline bool ps_axis_uniform(const double *w, int nf, double tol, double *dw_out)
{
    const double dw = w[1];
    *dw_out = dw;
    if (!(dw > 0.0)) return false;
    for (int i = 1; i < nf; ++i)
        if (std::fabs(w[i] - (double)i * dw) > tol * (double)i * dw) return false;
    return !(std::fabs(std::fabs(w[0]) - (double)nf * dw) > tol * (double)nf * dw);
}

// ---- transform path (ps_nufft.h) -----------------------------------------------------------------------------------------------
constexpr int PN_NFMAX = 4096;              // frequencies per wavenumber ps_nufft_kernel takes (one workgroup holds them all)
constexpr int PN_SHORT = 8;                 // runs of up to this many steps are summed directly by ps_nufft_kernel
constexpr int PN_LMAX_F32 = 4096, PN_LMAX_F64 = 1024;     // steps per piece at most (PnCfg<T>::LMAX; G = 2 LMAX grid points)
// (a pair of float64 rows takes the frequencies a quarter at a time and has room for pieces twice as long: ps_nufft.h)
constexpr int pn_lmax_steps(bool dbl, bool pair) { return dbl ? (pair ? 2 * PN_LMAX_F64 : PN_LMAX_F64) : PN_LMAX_F32; }

struct PnPiece {
    double v;               // velocity (kind 0)
    int start, len;         // first depth step, steps
    int kind;               // 0: transform, 1: direct sums (len <= PN_SHORT steps, each at its own velocity: the single steps of a
                            // smeared layer boundary, and short runs, taken in ONE pass over the frequencies)
    int loglp;              // kind 0: log2 of the padded length Lp >= len (G = 2 Lp)
    double vs[PN_SHORT];    // kind 1: the steps' velocities
};
static_assert(sizeof(PnPiece) == 24 + 8 * PN_SHORT, "the kernel reads the pieces as the host lays them out");

struct PnPlan {
    std::vector<PnPiece> pieces;
    bool need[13] = {};         // need[l]: a piece of padded length 2^l
    int nshort_steps = 0;       // steps summed directly
    int gmax = 2 << 4;          // grid points of the longest piece, 2 Lp (the LDS layout)
    std::vector<double> e1;     // float64 v(z) tables: [snum] E(n) / cbar^2 = sum_{t <= n} (v_t^2 / mean - 1) inside the piece
};

static inline bool pn_gate(int nruns, int nf, int snum, bool herm) { return herm && nf >= 64 && nf <= PN_NFMAX && snum >= 64 && nruns > 0; }

// runs -> pieces of at most pn_lmax_steps, the short runs of a smeared boundary merged up to PN_SHORT steps.  vmig (float64 data,
// v(z)): the per-step velocities -- the runs' rounding noise enters as a first-order term (ps_nufft.h).  false: declined
static inline bool pn_plan(PnPlan &pn, const std::vector<PsMfmaRun> &runs, bool vz, bool dbl, bool pairs, int nf, int snum, bool herm,
                           const double *vmig)
{
    if (!pn_gate((int)runs.size(), nf, snum, herm)) return false;
    const int lmax_steps = pn_lmax_steps(dbl, pairs);
    std::vector<PnPiece> &pc = pn.pieces;
    for (const PsMfmaRun &r : runs) {
        if (vz && r.len <= PN_SHORT) {
            // consecutive short runs (the single steps of one smeared boundary) share a piece: one pass over the frequencies
            pn.nshort_steps += r.len;
            if (!pc.empty() && pc.back().kind == 1 && pc.back().start + pc.back().len == r.start && pc.back().len + r.len <= PN_SHORT) {
                for (int q = 0; q < r.len; ++q) pc.back().vs[pc.back().len + q] = r.v;
                pc.back().len += r.len;
            } else {
                PnPiece p1{r.v, r.start, r.len, 1, 0, {}};
                for (int q = 0; q < PN_SHORT; ++q) p1.vs[q] = r.v;
                pc.push_back(p1);
            }
            continue;
        }
        const int npiece = (r.len + lmax_steps - 1) / lmax_steps;
        for (int i = 0, at = 0; i < npiece; ++i) {
            const int len = (r.len - at) / (npiece - i);
            int l = 4;
            while ((1 << l) < len) ++l;
            PnPiece p0{r.v, r.start + at, len, 0, l, {}};
            pc.push_back(p0);
            pn.need[l] = true;
            pn.gmax = std::max(pn.gmax, 2 << l);
            at += len;
        }
    }
    // a direct step costs as much as a tenth of a piece: tables of many layers stay with ps_runs_kernel
    if (pn.nshort_steps > 128 || pc.size() > 256) return false;
    if (dbl && vz && vmig != nullptr) {
        // per piece: the reference velocity sqrt(mean v^2) and E(n) / cbar^2 = sum_{t <= n} (v_t^2 / mean - 1)
        pn.e1.assign((size_t)snum, 0.0);
        for (PnPiece &p0 : pc) {
            if (p0.kind != 0) continue;
            long double acc = 0.0L;
            for (int t = 0; t < p0.len; ++t) acc += (long double)vmig[p0.start + t] * vmig[p0.start + t];
            const double vb2 = (double)(acc / p0.len);
            p0.v = std::sqrt(vb2);
            long double run = 0.0L;
            for (int t = 0; t < p0.len; ++t) {
                run += ((long double)vmig[p0.start + t] * vmig[p0.start + t] - (long double)vb2) / (long double)vb2;
                pn.e1[(size_t)p0.start + t] = (double)run;
            }
        }
    }
    return true;
}

// 1 / psihat(n), n = 0 .. Lp/2, of the padded length Lp = 2^l: psihat(n) = int psi(x) cos(2 pi n x / G) dx over |x| < W/2, G = 2 Lp
// (Simpson, float64; the integrand ends at e^{-beta} = 1e-8 of its maximum).  Shared by ps_nufft.h and ps_series.h: same window
static inline std::vector<double> pn_corr_of_length(int W, int l)
{
    const int Lp = 1 << l, G = 2 * Lp, NS = 512;
    const double beta = 2.30 * W, h = (double)W / NS;
    std::vector<double> psi((size_t)NS + 1);
    for (int q = 0; q <= NS; ++q) {
        const double x = -0.5 * W + q * h, z = 1.0 - (2.0 * x / W) * (2.0 * x / W);
        psi[q] = std::exp(beta * (std::sqrt(z > 0.0 ? z : 0.0) - 1.0)) * ((q == 0 || q == NS) ? 1.0 : ((q & 1) ? 4.0 : 2.0));
    }
    // (sum_q psi_q cos(n theta_q), theta_q = 2 pi x_q / G, for all n at once: per node a rotation by theta_q from n to n + 1,
    // re-seeded with the library's cos / sin every 64 -- a cos() per (n, q) was ~20 ms of a process's first call at 8192^2)
    std::vector<double> acc((size_t)Lp / 2 + 1, 0.0);
    for (int q = 0; q <= NS; ++q) {
        const double th = 6.283185307179586 * (-0.5 * W + q * h) / G, ct = std::cos(th), st_ = std::sin(th), pq = psi[q];
        double c = 1.0, sn = 0.0;
        for (int n = 0; n <= Lp / 2; ++n) {
            if ((n & 63) == 0) {
                c = std::cos(th * n);
                sn = std::sin(th * n);
            }
            acc[(size_t)n] += pq * c;
            const double c2 = c * ct - sn * st_;
            sn = sn * ct + c * st_;
            c = c2;
        }
    }
    for (double &a : acc) a = 1.0 / (a * h / 3.0);
    return acc;
}

// ---- many-runs matrix-core path (ps_runs.h) ------------------------------------------------------------------------------------
constexpr int PR_TT = 8;            // depth steps per tile
constexpr int PR_ROWS = 16;         // tiles per block
constexpr int PR_NM = 4;            // frequencies per thread (super-chunks of 256 slots per part)
constexpr int PR_PART = PR_NM * 256;
constexpr int PR_LONGS = 4;         // long runs per stage = waves
constexpr int PR_NBLK = 4;          // blocks per long run: up to 512 steps
constexpr int PR_LONG_MAX = PR_NBLK * PR_ROWS * PR_TT;
constexpr int PR_SHORT_LEN = 2;     // runs of up to this many steps: every step a row of its own
constexpr int PR_SROWS = 12;        // single-step rows per stage
constexpr int PR_STAGE_RUNS = 16;   // runs per stage

struct PrRun {
    double v;               // velocity
    int start, len;         // first depth step, steps
    int kind;               // 0: long (tiles of 8 steps), 1: single steps
    int slot;               // long: the wave that multiplies it; short: its first row among the stage's single-step rows
};
static_assert(sizeof(PrRun) == 24, "the kernel copies a stage's runs to LDS as 6 words each");
struct PrStage {
    int run0, nruns;        // the stage's runs, in depth order
    int nshort, short_wave; // single-step rows and the wave that multiplies them
    int long_run[PR_LONGS]; // run of wave p (-1: none)
    int long_nblk[PR_LONGS];
    int short_tau[PR_SROWS];
};

struct PrPlan {
    std::vector<PrRun> pr;
    std::vector<PrStage> stages;
    int nparts = 0;         // parts of the spectrum (PR_PART slots each), a partial image per part
};

static inline bool pr_gate(int nruns, int nf, int snum) { return !(nf % 32 != 0 || nf < 256 || snum < 64 || nruns == 0); }

// runs -> pieces: long (<= 512 steps, tiles of 8) and single steps, packed into stages.  false: declined
static inline bool pr_plan(PrPlan &plan, const std::vector<PsMfmaRun> &runs, int nf, int snum)
{
    if (!pr_gate((int)runs.size(), nf, snum)) return false;
    std::vector<PrRun> &pr = plan.pr;
    int nshort_total = 0, nblk_total = 0;
    for (const PsMfmaRun &r : runs) {
        if (r.len <= PR_SHORT_LEN) {
            pr.push_back(PrRun{r.v, r.start, r.len, 1, 0});
            nshort_total += r.len;
            continue;
        }
        const int npiece = (r.len + PR_LONG_MAX - 1) / PR_LONG_MAX;
        for (int i = 0, at = 0; i < npiece; ++i) {
            // pieces of (nearly) equal length, whole tiles except the last
            int len = ((r.len - at) / (npiece - i) + PR_TT - 1) / PR_TT * PR_TT;
            len = std::min(len, r.len - at);
            pr.push_back(PrRun{r.v, r.start + at, len, 0, 0});
            nblk_total += ((len + PR_TT - 1) / PR_TT + PR_ROWS - 1) / PR_ROWS;
            at += len;
        }
    }
    // a record that is mostly single steps (a velocity that changes at nearly every step) is ps_smooth's
    if (nshort_total > snum / 4 || nblk_total == 0) return false;
    PrStage cur;
    auto open = [&](int run0) {
        cur = PrStage{};
        cur.run0 = run0;
        for (int i = 0; i < PR_LONGS; ++i) cur.long_run[i] = -1;
    };
    auto close = [&]() {
        if (cur.nruns == 0) return;
        // the single steps go to the wave with the fewest blocks
        int best = 0;
        for (int i = 1; i < PR_LONGS; ++i)
            if (cur.long_nblk[i] < cur.long_nblk[best]) best = i;
        cur.short_wave = best;
        plan.stages.push_back(cur);
    };
    open(0);
    int nlong = 0;
    for (int i = 0; i < (int)pr.size(); ++i) {
        const bool is_long = pr[i].kind == 0;
        // (single steps lead the long run that follows them: the set-up chains their states into its anchor -- a stage
        // that has its four long runs is closed before the next group)
        const bool fits = cur.nruns < PR_STAGE_RUNS && (is_long ? nlong < PR_LONGS : (nlong < PR_LONGS && cur.nshort + pr[i].len <= PR_SROWS));
        if (!fits) {
            close();
            open(i);
            nlong = 0;
        }
        if (is_long) {
            pr[i].slot = nlong;
            cur.long_run[nlong] = i;
            cur.long_nblk[nlong] = ((pr[i].len + PR_TT - 1) / PR_TT + PR_ROWS - 1) / PR_ROWS;
            ++nlong;
        } else {
            pr[i].slot = cur.nshort;
            for (int s_ = 0; s_ < pr[i].len; ++s_) cur.short_tau[cur.nshort++] = pr[i].start + s_;
        }
        ++cur.nruns;
    }
    close();
    plan.nparts = (nf + PR_PART - 1) / PR_PART;
    return true;
}

// ---- matrix-core path (ps_mfma.h) ----------------------------------------------------------------------------------------------
constexpr int PM_SHORT = 8;                 // runs of up to this many steps (the few steps a layer boundary is smeared over) get no row blocks: ps_trans_kernel
constexpr int PM_TT = 64;                   // depth steps per tile
constexpr int PM_NRB = 5;                   // row blocks per group (state tiles per frequency half, accumulators per wave)
constexpr int PM_EMAX = 16;                 // boundary frequencies listed per wavenumber
constexpr int PM_MAX_RUNS = 96;
constexpr int PM_SLOTS = 32;                // the frequency slots of a call are a multiple of this (PM_CH * PM_NQ of ps_mfma.h)

struct PmBlock {
    int run, tile0;         // run and first tile inside it of a row block (32 tiles); run = -1: none.  An int2 on the device
};
static_assert(sizeof(PmBlock) == 8, "uploaded as the kernel's int2");

struct PmPlan {
    std::vector<PmBlock> table;     // [ngroups][PM_NRB]
    int ngroups = 0;
    int nlong = 0;                  // runs that get row blocks
    int long_of[PM_MAX_RUNS];       // run -> index among the long runs (-1: short)
};

static inline bool pm_gate(int nruns, int nf, int snum)
{
    return !(nf % PM_SLOTS != 0 || nf < 256 || nf > 4096 + 2048 || snum < 256 || nruns == 0 || nruns > PM_MAX_RUNS);
}

// runs -> row blocks of 32 tiles of 64 steps in groups of up to PM_NRB.  false: declined
static inline bool pm_plan(PmPlan &pm, const std::vector<PsMfmaRun> &runs, bool vz, int nf, int snum)
{
    if (!pm_gate((int)runs.size(), nf, snum)) return false;
    // row blocks: 32 tiles of 64 steps of one run; runs of a few steps (a layer boundary smeared over 3-4 steps by
    // 2 * gradient(z(t))) get none: ps_trans_kernel sums their steps directly
    std::vector<PmBlock> blocks;
    int nshort_steps = 0;
    for (size_t r = 0; r < runs.size(); ++r) {
        if (vz && runs[r].len <= PM_SHORT) {
            nshort_steps += runs[r].len;
            continue;
        }
        const int ntile = (runs[r].len + PM_TT - 1) / PM_TT;
        for (int a0 = 0; a0 < ntile; a0 += 32) blocks.push_back(PmBlock{(int)r, a0});
    }
    const int nb = (int)blocks.size();
    // limits of the matrix-core path: long runs, row padding (blocks x 2048 steps against the record), steps in short
    // runs.  A row block costs ~2.4 ms at 8192^2 and the vector runs kernels ~40-50 ms for the whole record: 16 runs /
    // 3 x padding is where the two meet (a 21-row table of equal layers: 44.5 -> 38.1 ms; profiles/r03_ps_layers.txt)
    constexpr int max_long = 16, max_short = 200;
    constexpr double max_pad = 3.0;
    if (nb == 0 || nshort_steps > max_short || (int)runs.size() - (vz ? (int)std::count_if(runs.begin(), runs.end(), [](const PsMfmaRun &r) { return r.len <= PM_SHORT; }) : 0) > max_long) return false;
    if ((double)nb * 32 * PM_TT > (double)snum * max_pad + 32 * PM_TT) return false;      // many medium runs: rows mostly padding
    // groups of up to PM_NRB row blocks (the state tiles a workgroup keeps in LDS), consecutive blocks together
    pm.ngroups = (nb + PM_NRB - 1) / PM_NRB;
    const int per_group = (nb + pm.ngroups - 1) / pm.ngroups;
    pm.table.assign((size_t)pm.ngroups * PM_NRB, PmBlock{-1, 0});
    for (int g = 0, at = 0; g < pm.ngroups; ++g) {
        const int n = std::min(per_group, nb - at);
        for (int i = 0; i < n; ++i, ++at) pm.table[(size_t)g * PM_NRB + i] = blocks[at];
    }
    pm.nlong = 0;
    for (int r = 0; r < PM_MAX_RUNS; ++r) pm.long_of[r] = -1;
    for (int r = 0; r < (int)runs.size(); ++r)
        if (!(vz && runs[r].len <= PM_SHORT)) pm.long_of[r] = pm.nlong++;
    return true;
}

#ifdef PS_PATH_PLAN_PROBE
// the plans as flat arrays (tests/test_ps_path_plan.py compiles this header by itself).  The runs are ps_route_runs' of a per-step
// profile vmig [snum], or of the constant vconst (vmig null); every entry point sets ints[0] = 0 and nothing else where the plan
// is declined, and returns -1 where the caller's arrays (cap entries) are too small.
#include "ps_route.h"       // ps_route_runs (this header is included first: ps_route.h finds it done)
#include <cstring>

static inline std::vector<PsMfmaRun> ps_probe_runs(int dbl, int snum, double vconst, const double *vmig)
{
    PsRoute R;
    ps_route_runs(R, dbl != 0, snum, vconst, vmig, vmig ? snum : 0);
    return R.runs;
}

// ints[6]: taken, pieces, nshort_steps, gmax, need as bits, length of e1; per piece (start, len, kind, loglp), v, vs[PN_SHORT]
extern "C" int impdar_pn_plan_probe(int dbl, int snum, int nf, int pairs, int vz, int herm, double vconst, const double *vmig, int cap, int *ints,
                                    int *piece_ints, double *piece_v, double *piece_vs, double *e1 /* [snum] */)
{
    PnPlan pn;
    ints[0] = pn_plan(pn, ps_probe_runs(dbl, snum, vconst, vmig), vz != 0, dbl != 0, pairs != 0, nf, snum, herm != 0, dbl && vz ? vmig : nullptr);
    if (!ints[0]) return 0;
    if ((int)pn.pieces.size() > cap) return -1;
    int mask = 0;
    for (int l = 0; l < 13; ++l) mask |= pn.need[l] ? 1 << l : 0;
    const int I[5] = {(int)pn.pieces.size(), pn.nshort_steps, pn.gmax, mask, (int)pn.e1.size()};
    std::copy(I, I + 5, ints + 1);
    for (size_t i = 0; i < pn.pieces.size(); ++i) {
        const PnPiece &p = pn.pieces[i];
        const int J[4] = {p.start, p.len, p.kind, p.loglp};
        std::copy(J, J + 4, piece_ints + 4 * i);
        piece_v[i] = p.v;
        std::copy(p.vs, p.vs + PN_SHORT, piece_vs + PN_SHORT * i);
    }
    std::copy(pn.e1.begin(), pn.e1.end(), e1);
    return 0;
}

// ints[4]: taken, runs, stages, nparts; per run (start, len, kind, slot), v; per stage its 24 ints as PrStage lays them out
extern "C" int impdar_pr_plan_probe(int dbl, int snum, int nf, double vconst, const double *vmig, int cap, int *ints, int *run_ints, double *run_v,
                                    int *stage_ints)
{
    PrPlan plan;
    ints[0] = pr_plan(plan, ps_probe_runs(dbl, snum, vconst, vmig), nf, snum);
    if (!ints[0]) return 0;
    if ((int)plan.pr.size() > cap) return -1;
    ints[1] = (int)plan.pr.size();
    ints[2] = (int)plan.stages.size();
    ints[3] = plan.nparts;
    for (size_t i = 0; i < plan.pr.size(); ++i) {
        const PrRun &r = plan.pr[i];
        const int J[4] = {r.start, r.len, r.kind, r.slot};
        std::copy(J, J + 4, run_ints + 4 * i);
        run_v[i] = r.v;
    }
    static_assert(sizeof(PrStage) == 24 * sizeof(int), "24 ints per stage");
    for (size_t i = 0; i < plan.stages.size(); ++i) memcpy(stage_ints + 24 * i, &plan.stages[i], sizeof(PrStage));
    return 0;
}

// ints[3]: taken, ngroups, nlong; table [ngroups][PM_NRB] x (run, first tile); long_of [PM_MAX_RUNS]
extern "C" int impdar_pm_plan_probe(int dbl, int snum, int nf, int vz, double vconst, const double *vmig, int cap, int *ints, int *table, int *long_of)
{
    PmPlan pm;
    ints[0] = pm_plan(pm, ps_probe_runs(dbl, snum, vconst, vmig), vz != 0, nf, snum);
    if (!ints[0]) return 0;
    if ((int)pm.table.size() > cap) return -1;
    ints[1] = pm.ngroups;
    ints[2] = pm.nlong;
    memcpy(table, pm.table.data(), pm.table.size() * sizeof(PmBlock));
    std::copy(pm.long_of, pm.long_of + PM_MAX_RUNS, long_of);
    return 0;
}

// out [2^l / 2 + 1]; returns the entries written
extern "C" int impdar_pn_corr_probe(int W, int l, double *out)
{
    const std::vector<double> c = pn_corr_of_length(W, l);
    std::copy(c.begin(), c.end(), out);
    return (int)c.size();
}
#endif
