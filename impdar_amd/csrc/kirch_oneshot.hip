// The Kirchhoff entry points that keep a plan between calls: impdar_kirchhoff, the one-shot call on host buffers, and
// mig_kirch_loop, the reference's native hook.  Host code only; plan creation, prep and migrate are kirchhoff.hip's and are
// reached through kirch_plan.h.
#include "kirch_plan.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <mutex>
#include <vector>

// ---------------------------------------------------------------------------
// one-shot host-buffer entry point
// ---------------------------------------------------------------------------
// The one-shot entry point keeps its last plan and device buffers (as the Stolt and phase-shift entry points do):
// a second radargram of the same geometry skips the plan, the pick table, the allocations and their release
// (19.9 -> 18.1 ms host-to-host at config 3).
// IMPDAR_KIRCH_ONESHOT_CACHE=0 releases everything at the end of each call, as before.
namespace {
struct KirchOneShot {
    const impdar_ctx *owner = nullptr;
    impdar_kirch_plan *plan = nullptr;
    DevBuf din, dout;
    hipEvent_t ev_blk[8] = {};       // output block i of a split one-shot call summed (see impdar_kirchhoff)
    int dtype = -1, snum = 0, tnum = 0, nearfield = 0, grad_uniform = 0, mode = 0;
    double vel = 0, grad_h = 0;
    std::vector<double> dist, tt, ga, gb, gc;
    KirchKnobs knobs;        // the IMPDAR_KIRCH_* settings the plan was built under
    void drop()
    {
        if (plan) impdar_kirch_plan_destroy(plan);
        plan = nullptr;
        din.release();
        dout.release();
        for (hipEvent_t &e : ev_blk) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        owner = nullptr;
    }
};
std::mutex g_k1_mu;
KirchOneShot *g_k1 = nullptr;
thread_local bool t_k1_busy = false, t_hook_busy = false;     // this thread is inside impdar_kirchhoff / mig_kirch_loop

bool same_vec(const std::vector<double> &have, const double *p, size_t n)
{
    if (!p) return have.empty();
    return have.size() == n && memcmp(have.data(), p, n * sizeof(double)) == 0;
}
}   // namespace

// called by impdar_ctx_destroy: the cached plan must not outlive the context it was created on
void impdar_kirch_forget(const impdar_ctx *ctx)
{
    std::lock_guard<std::mutex> lk(g_k1_mu);
    if (g_k1 && g_k1->owner == ctx) {
        g_k1->drop();
        delete g_k1;
        g_k1 = nullptr;
    }
}

extern "C" int impdar_kirchhoff(impdar_ctx *ctx, const void *data, int dtype, int snum, int tnum,
                                const double *dist_m, const double *tt_sec, double vel, int nearfield,
                                int grad_uniform, double grad_h, const double *ga, const double *gb,
                                const double *gc, int mode, double *out)
{
    IMPDAR_ARG_CHECK(ctx && data && out, "null context/data/output");
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto t0 = now();
    std::lock_guard<std::mutex> lk(g_k1_mu);
    ImpdarBusy busy(t_k1_busy);
    if (!g_k1) g_k1 = new KirchOneShot();
    KirchOneShot &c = *g_k1;
    const char *ce = getenv("IMPDAR_KIRCH_ONESHOT_CACHE");
    const bool keep = !(ce && ce[0] == '0');
    const KirchKnobs knobs = KirchKnobs::from_env();
    const bool hit = c.plan && c.owner == ctx && c.dtype == dtype && c.snum == snum && c.tnum == tnum && c.vel == vel &&
                     c.nearfield == nearfield && c.grad_uniform == grad_uniform && c.grad_h == grad_h && c.mode == mode &&
                     dist_m && tt_sec && same_vec(c.dist, dist_m, (size_t)tnum) && same_vec(c.tt, tt_sec, (size_t)snum) &&
                     same_vec(c.ga, ga, (size_t)snum) && same_vec(c.gb, gb, (size_t)snum) &&
                     same_vec(c.gc, gc, (size_t)snum) && c.knobs == knobs;
    int rc;
    if (!hit) {
        c.drop();
        if ((rc = kirch_plan_create_impl(ctx, dtype, snum, tnum, dist_m, tt_sec, vel, nearfield, grad_uniform, grad_h,
                                         ga, gb, gc, mode, 1, knobs, nullptr, &c.plan))) {
            c.plan = nullptr;
            return rc;
        }
        c.owner = ctx;
        c.dtype = dtype, c.snum = snum, c.tnum = tnum, c.nearfield = nearfield, c.grad_uniform = grad_uniform, c.mode = mode;
        c.vel = vel, c.grad_h = grad_h;
        c.dist.assign(dist_m, dist_m + tnum);
        c.tt.assign(tt_sec, tt_sec + snum);
        auto take = [&](std::vector<double> &v, const double *p) {
            if (p) v.assign(p, p + snum);
            else v.clear();
        };
        take(c.ga, ga);
        take(c.gb, gb);
        take(c.gc, gc);
        c.knobs = knobs;
    }
    impdar_kirch_plan *p = c.plan;
    const size_t esz = impdar_dtype_size(dtype);
    const size_t bytes = (size_t)snum * tnum * esz;
    auto done = [&](int code) {
        if (code != IMPDAR_OK) {
            // the uploads of the pipelined form read the caller's array asynchronously: nothing may still be in flight
            // when an error hands the array back
            (void)hipStreamSynchronize(ctx->aux);
            (void)hipStreamSynchronize(ctx->stream);
        }
        if (code != IMPDAR_OK || !keep) c.drop();
        return code;
    };
    if (c.din.ensure(bytes) != hipSuccess || c.dout.ensure(bytes) != hipSuccess) {
        impdar_set_error("hipMalloc of %zu bytes failed", bytes);
        return done(IMPDAR_ERR_HIP);
    }
    const auto t0b = now();
    // Large radargrams on the ring kernels go through in pieces, so that PCIe and the kernels work at the same time.
    // OUTPUT traces in blocks, one launch each (output blocks equal the whole image bit for bit: every output
    // accumulates its pairs in the same order): a block crosses PCIe and is widened on the host while the next is
    // summed.  INPUT traces in column chunks: a block's launch starts when the traces it reads are on the device and the
    // rest of the upload runs under it; later chunks are prepared into the same image (kirch_prep_impl's `more`).  Every
    // launch must drain (~0.3 ms each) -- the copies they hide are worth more.  Where the cuts lie: kirch_oneshot_cuts,
    // kirch_route.h.
    // IMPDAR_KIRCH_ONESHOT_SPLIT=0: one upload, one launch, one download; =2: one upload, two launches.
    const char *se = getenv("IMPDAR_KIRCH_ONESHOT_SPLIT");
    const int kern = impdar_kirch_plan_kernel(p);
    const bool split = !(se && atoi(se) == 0) && tnum >= 4096 && bytes >= ((size_t)64 << 20) &&
                       (kern == IMPDAR_KERNEL_QUAD || kern == IMPDAR_KERNEL_DQUAD);
    // the download's staging buffer, pinned by a thread of its own while this call uploads and sums (started behind the
    // plan: beside it the two contend for the runtime -- plan 18 -> 40 ms): the 64 MB ring of download.hip, for the
    // pipelined blocks and the one-piece download alike
    impdar_ctx_pinned_prefetch(ctx, std::min(bytes, IMPDAR_STAGE_RING_BYTES));
    int nlaunch = 1;
    if (split) {
        const int halo = p->ntab + 16;                 // aperture half width (+ the kernels' staging look-ahead)
        const bool two = se && atoi(se) == 2;          // the round-3 first form, kept for A/B
        const KirchOneShotCuts cuts = kirch_oneshot_cuts(tnum, halo, two);
        const std::vector<int> &cut = cuts.cut;
        const int nblk = (int)cut.size() - 1;
        nlaunch = nblk;
        for (int i = 0; i < nblk; ++i)
            if (!c.ev_blk[i] && hipEventCreateWithFlags(&c.ev_blk[i], hipEventDisableTiming) != hipSuccess) {
                c.ev_blk[i] = nullptr;
                impdar_set_error("hipEventCreate failed");
                return done(IMPDAR_ERR_HIP);
            }
        char *dout = reinterpret_cast<char *>(c.dout.p);
        int have = 0;                                  // input traces [0, have) are on the device and prepared
        for (int i = 0; i < nblk; ++i) {
            const int need = cuts.need[i];
            if (need > have) {
                // column block [have, need) of the (snum, tnum) host array; on the producer stream, in front of its prep
                if (hipMemcpy2DAsync(reinterpret_cast<char *>(c.din.p) + (size_t)have * esz, (size_t)tnum * esz,
                                     reinterpret_cast<const char *>(data) + (size_t)have * esz, (size_t)tnum * esz,
                                     (size_t)(need - have) * esz, (size_t)snum, hipMemcpyHostToDevice, ctx->aux) != hipSuccess) {
                    impdar_set_error("H2D copy failed");
                    return done(IMPDAR_ERR_HIP);
                }
                if ((rc = kirch_prep_impl(p, reinterpret_cast<const char *>(c.din.p) + (size_t)have * esz, tnum, have,
                                          need - have, 0, have > 0)))
                    return done(rc);
                have = need;
            }
            if ((rc = impdar_kirch_migrate(p, dout + (size_t)snum * cut[i] * esz, cut[i], cut[i + 1]))) return done(rc);
            if (hipEventRecord(c.ev_blk[i], ctx->stream) != hipSuccess) return done(IMPDAR_ERR_HIP);
        }
        // the blocks leave on the producer stream (idle after the last prep) as their launches finish: all copies
        // enqueued at once, the host widens what has arrived
        {
            std::vector<size_t> col0(nblk), width(nblk);
            std::vector<const void *> src(nblk);
            for (int i = 0; i < nblk; ++i) {
                col0[i] = (size_t)cut[i];
                width[i] = (size_t)(cut[i + 1] - cut[i]);
                src[i] = dout + (size_t)snum * cut[i] * esz;
            }
            if ((rc = impdar_download_blocks_f64(ctx, out, (size_t)tnum, (size_t)snum, dtype, nblk, col0.data(), width.data(),
                                                 src.data(), c.ev_blk, ctx->aux)))
                return done(rc);
        }
    } else {
        if (hipMemcpyAsync(c.din.p, data, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {      // prep runs on the aux stream
            impdar_set_error("H2D copy failed");
            return done(IMPDAR_ERR_HIP);
        }
        if ((rc = impdar_kirch_prep(p, c.din.p, tnum, 0, tnum))) return done(rc);
        if ((rc = impdar_kirch_migrate(p, c.dout.p, 0, tnum))) return done(rc);
        // device -> pinned staging (in pieces) -> the caller's float64 array on several host threads
        // (mig_python.py:118 returns float64); waits for the diffraction sum on the compute stream
        if ((rc = impdar_dev_download_f64(ctx, out, c.dout.p, dtype, (size_t)snum * tnum))) return done(rc);
    }
    // what this call did, for impdar_ctx_last_metrics (the downloads above have synchronised the streams)
    float kms = -1.f;
    {
        float a = 0.f, b = 0.f, c2 = 0.f;
        if (impdar_kirch_last_ms(p, &a, &b, &c2) == IMPDAR_OK) kms = c2;       // first launch's start to last launch's end
        (void)hipGetLastError();
    }
    static const char *kernel_names[] = {"kirch_exact_kernel", "kirch_exact_tab_kernel", "kirch_dquad_kernel", "kirch_quad_kernel",
                                         "kirch_tab_kernel", "kirch_gen_kernel"};
    ctx->m_entry = "impdar_kirchhoff";
    ctx->m_kernel = (kern >= 0 && kern < 6) ? kernel_names[kern] : "";
    ctx->m_kernel_ms = kms;
    ctx->timed = false;
    const auto t2 = now();
    // xnoise: the position noise of the profile against its fitted grid, in trace spacings (impdar_kirch_plan_xnoise); the
    // float64 ring / tabulated kernels weight a pair by its trace OFFSET, so their stated bar against the reference is
    // max(1e-12, 0.1 xnoise) of the image maximum -- parity_bar says which one this call ran under (the per-pair kernel,
    // IMPDAR_KIRCH_EXACT_IMPL=pair, holds 1e-12 on any profile)
    const bool offset_weighted = kern == IMPDAR_KERNEL_DQUAD || kern == IMPDAR_KERNEL_EXACT_TAB;
    snprintf(ctx->m_extra, sizeof ctx->m_extra,
             "\"plan\": \"%s\", \"launches\": %d, \"plan_ms\": %.3f, \"call_ms\": %.3f, \"xnoise\": %.3g, \"window\": \"%s\", \"parity_bar\": %.3g",
             hit ? "cached" : "new", nlaunch, ms(t0, t0b), ms(t0, t2), p->xnoise,
             kern != IMPDAR_KERNEL_QUAD ? "" : (p->window == KIRCH_WINDOW_QUAD ? "quad" : "slide"),
             dtype == IMPDAR_F32 && p->mode == IMPDAR_KIRCH_FAST ? 1e-4 : (offset_weighted ? std::max(1e-12, 0.1 * p->xnoise) : 1e-12));
    rc = done(IMPDAR_OK);
    return rc;
}

// ---------------------------------------------------------------------------
// reference-compatible native hook (mig_cython.h:11)
// ---------------------------------------------------------------------------
// void return, no error channel (_mig_cython.pyx:19-20): whatever goes wrong, migdata is filled with NaN -- the
// wrapper returns it as the migrated image, and an untouched (all-zero) array would read as a result.
//
// The caller hands over its own depth tables and time limit (mig_python.py:98-102 computes them).  When they are what
// the reference's driver computes -- zs = vel tt / 2 and zs2 = zs^2 bit for bit, max_travel_time = max(tt) up to the
// single-precision rounding _mig_cython.pyx:30-32 applies to it -- on a uniform profile, the float64 LDS-ring kernel
// runs (kirch_dquad_kernel, the library's own float64 default; its plan is created with the caller's time limit); any
// other tables go through the per-pair kernel, which reads them as given.  The plan and the device buffers are kept
// between calls of one geometry, as the one-shot entry point keeps its own.
namespace {
struct KirchHook {
    impdar_ctx *ctx = nullptr;
    impdar_kirch_plan *plan = nullptr;
    DevBuf din, dout;
    int snum = 0, tnum = 0;
    double vel = 0, tmax = 0;
    bool standard = false;
    std::vector<double> dist, tt, zs, zs2;
    KirchKnobs knobs;
    void drop()
    {
        if (plan) impdar_kirch_plan_destroy(plan);
        plan = nullptr;
        din.release();
        dout.release();
    }
};
std::mutex g_hook_mu;
KirchHook g_hook;
}   // namespace

// impdar_release_caches: out of device memory somewhere -- drop the one-shot and the hook caches unless their entry
// point is the one running
void impdar_kirch_trim()
{
    if (!t_k1_busy) {
        std::unique_lock<std::mutex> lk(g_k1_mu, std::try_to_lock);
        if (lk.owns_lock() && g_k1) g_k1->drop();
    }
    if (!t_hook_busy) {
        std::unique_lock<std::mutex> lk(g_hook_mu, std::try_to_lock);
        if (lk.owns_lock()) g_hook.drop();
    }
}

extern "C" void mig_kirch_loop(double *migdata, int tnum, int snum, double *dist, double *zs, double *zs2,
                               double *tt_sec, double vel, double *gradD, double max_travel_time, int nearfield)
{
    auto fail = [&](const char *why) {
        fprintf(stderr, "impdar mig_kirch_loop: %s -- migdata filled with NaN\n", why);
        if (migdata && snum > 0 && tnum > 0) {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            for (size_t i = 0, n = (size_t)snum * tnum; i < n; ++i) migdata[i] = nan;
        }
    };
    if (!migdata || !dist || !zs || !zs2 || !tt_sec || !gradD || snum < 1 || tnum < 1) return fail("null pointer or empty array");
    if (nearfield)
        return fail("the reference prototype carries no data pointer, so the near-field term cannot be formed "
                    "(use impdar_kirchhoff)");
    std::lock_guard<std::mutex> lk(g_hook_mu);
    ImpdarBusy busy(t_hook_busy);
    KirchHook &c = g_hook;
    if (!c.ctx && impdar_ctx_create(0, &c.ctx) != IMPDAR_OK) {
        c.ctx = nullptr;
        return fail(impdar_last_error());
    }
    impdar_ctx *ctx = c.ctx;
    double ttmax = tt_sec[0];
    bool standard = true;
    for (int k = 0; k < snum; ++k) {
        ttmax = std::max(ttmax, tt_sec[k]);
        standard = standard && zs[k] == vel * tt_sec[k] / 2.0 && zs2[k] == zs[k] * zs[k];     // mig_python.py:101-102
    }
    standard = standard && std::fabs(max_travel_time - ttmax) <= 1e-6 * std::fabs(ttmax);
    const KirchKnobs knobs = KirchKnobs::from_env();
    const bool hit = c.plan && c.snum == snum && c.tnum == tnum && c.vel == vel && c.tmax == max_travel_time &&
                     c.standard == standard && same_vec(c.dist, dist, (size_t)tnum) && same_vec(c.tt, tt_sec, (size_t)snum) &&
                     same_vec(c.zs, zs, (size_t)snum) && same_vec(c.zs2, zs2, (size_t)snum) && c.knobs == knobs;
    if (!hit) {
        c.drop();
        // (the caller's own tables: per-pair kernel -- the table-driven ones derive picks and apertures from the plan's tables)
        const KirchCallerTables own{max_travel_time, zs, zs2, standard};
        if (kirch_plan_create_impl(ctx, IMPDAR_F64, snum, tnum, dist, tt_sec, vel, 0, 1, 1.0, nullptr, nullptr, nullptr,
                                   IMPDAR_KIRCH_EXACT, 1, knobs, &own, &c.plan)) {
            c.plan = nullptr;
            return fail(impdar_last_error());
        }
        c.snum = snum, c.tnum = tnum, c.vel = vel, c.tmax = max_travel_time, c.standard = standard;
        c.dist.assign(dist, dist + tnum);
        c.tt.assign(tt_sec, tt_sec + snum);
        c.zs.assign(zs, zs + snum);
        c.zs2.assign(zs2, zs2 + snum);
        c.knobs = knobs;
    }
    impdar_kirch_plan *p = c.plan;
    const size_t bytes = (size_t)snum * tnum * 8;
    const bool ok = c.din.ensure(bytes) == hipSuccess && c.dout.ensure(bytes) == hipSuccess &&
                    hipMemcpyAsync(c.din.p, gradD, bytes, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
                    hipStreamSynchronize(ctx->stream) == hipSuccess &&          // prep runs on the producer stream
                    impdar_kirch_prep_precomputed(p, c.din.p, tnum, 0, tnum) == IMPDAR_OK &&
                    impdar_kirch_migrate(p, c.dout.p, 0, tnum) == IMPDAR_OK &&
                    impdar_download(ctx, migdata, c.dout.p, bytes, ctx->stream) == IMPDAR_OK;
    if (!ok) {
        (void)hipGetLastError();
        c.drop();
        return fail(impdar_last_error());
    }
    const char *ce = getenv("IMPDAR_KIRCH_ONESHOT_CACHE");
    if (ce && ce[0] == '0') c.drop();
}
