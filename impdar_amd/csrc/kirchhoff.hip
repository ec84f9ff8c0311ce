// Kirchhoff diffraction-summation migration for gfx950 (MI355X).
//
// Behaviour restated from the reference (paths relative to the ImpDAR tree):
//   src/impdar/lib/migrationlib/mig_python.py:35-60   migrationKirchhoffLoop
//   src/impdar/lib/migrationlib/mig_python.py:63-123  migrationKirchhoff
//   src/impdar/lib/migrationlib/mig_cython.h:11       mig_kirch_loop (native hook)
//
// File map (every kernel lives in exactly one unit):
//   kirchhoff.hip      this file, host only: plan creation in its stages, prep, the migrate dispatch, all-gather and halo
//                      exchange, the timing history, pair counting.
//   kirch_prep.h       kirch_prep_kernel / kirch_prep_direct_kernel: gradient + transpose into the image.    (included here)
//   kirch_exact.h      kirch_exact_kernel, kirch_tablex_kernel / kirch_exact_tab_kernel, kirch_tiescan_kernel /
//                      kirch_tiefix_kernel: the reference's float64 arithmetic, and their launches.           (included here)
//   kirch_ring.h       what the two ring units share: parameter structs, device fragments, launch_ring.
//   kirch_ring32.hip   kirch_quad_kernel (the MI355X hot path), kirch_tab_kernel and their pick tables: float32.
//   kirch_ring64.hip   kirch_dquad_kernel and its pick table: float64.
//   kirch_gen.hip      kirch_gen_kernel: float32 on a non-uniform trace spacing.
//   kirch_oneshot.hip  impdar_kirchhoff (cached one-shot entry on host buffers) and mig_kirch_loop (the reference's hook).
//   kirch_plan.h       the plan object and the functions by which the units reach each other.
//   kirch_route.h      everything the plan decides on the host, plain C++ tested without a device.
#include "common.h"
#include "kirch_plan.h"
#include "kirch_prep.h"
#include "kirch_exact.h"
#include <algorithm>
#include <memory>
#include <vector>

// ===========================================================================
// host side
// ===========================================================================
// What is decided on the host -- the analysis of the axes, the choice of kernel, the host tables -- is kirch_route.h: pure
// code, tested without a device.  Here: the stages that allocate and upload for it, and the launches.

static int kirch_alloc_images(impdar_kirch_plan *p)
{
    const size_t img = (size_t)(p->tnum_pad + 2 * KF_PAD_ROWS) * p->snum * impdar_dtype_size(p->dtype);   // zero rows on both sides
    for (int b = 0; b < 2; ++b) {
        if (p->GT[b].ensure(img) != hipSuccess || (p->nearfield && p->DT[b].ensure(img) != hipSuccess)) {
            impdar_set_error("hipMalloc of %zu-byte image failed", img);
            return IMPDAR_ERR_HIP;
        }
        (void)hipMemsetAsync(p->GT[b].p, 0, img, p->ctx->stream);
        if (p->nearfield) (void)hipMemsetAsync(p->DT[b].p, 0, img, p->ctx->stream);
    }
    (void)hipStreamSynchronize(p->ctx->stream);
    return IMPDAR_OK;
}

// the gradient coefficients, dist, tt and the depth tables zs = v t / 2, zs^2 (mig_python.py:101-102) or the caller's own
static int kirch_upload_axes(impdar_kirch_plan *p, const double *dist_m, const double *tt_sec, const double *ga, const double *gb,
                             const double *gc, const double *zs_own, const double *zs2_own)
{
    const int snum = p->snum, tnum = p->tnum;
    int rc;
    if (!p->grad_uniform) {
        if ((rc = upload(p->d_ga, ga, snum * 8)) || (rc = upload(p->d_gb, gb, snum * 8)) || (rc = upload(p->d_gc, gc, snum * 8)))
            return rc;
    }
    std::vector<double> zs(snum), zs2(snum);
    for (int k = 0; k < snum; ++k) {
        zs[k] = p->vel * tt_sec[k] / 2.0;
        zs2[k] = zs[k] * zs[k];
    }
    std::vector<double> dpad(dist_m, dist_m + tnum);
    dpad.resize((size_t)tnum + 64, dist_m[tnum - 1]);      // kirch_gen_kernel reads up to 31 entries past a tile's end
    if ((rc = upload(p->d_dist, dpad.data(), dpad.size() * 8)) || (rc = upload(p->d_tt, tt_sec, (size_t)snum * 8)) ||
        (rc = upload(p->d_zs, zs_own ? zs_own : zs.data(), (size_t)snum * 8)) ||
        (rc = upload(p->d_zs2, zs2_own ? zs2_own : zs2.data(), (size_t)snum * 8)))
        return rc;
    if (p->uniform) p->h_half = kirch_half_widths(*p, tt_sec, snum);
    return IMPDAR_OK;
}

static int kirch_upload_gen_tables(impdar_kirch_plan *p, const double *dist_m, const double *tt_sec)
{
    KirchGenTables T = kirch_gen_tables(*p, tt_sec, p->snum, p->vel, p->genW);
    p->nchunks = (int)T.alo2.size();
    p->h_zs2min.swap(T.zs2min);
    p->h_dist.assign(dist_m, dist_m + p->tnum);
    int rc;
    if ((rc = upload(p->d_ga32, T.a.data(), p->snum * 4)) || (rc = upload(p->d_ga2_32, T.a2.data(), p->snum * 4)) ||
        (rc = upload(p->d_alo2, T.alo2.data(), p->nchunks * 4)))
        return rc;
    return IMPDAR_OK;
}

// the per-sample factors, the pick table's allocation and the staging windows of quad / dquad / tab
static int kirch_upload_ring_tables(impdar_kirch_plan *p, const double *tt_sec)
{
    const int snum = p->snum;
    const bool ring = p->quad || p->dquad;
    int rc;
    if (p->dquad) {
        const KirchFactors<double> F = kirch_factors<double>(*p, tt_sec, snum, p->vel);
        if ((rc = upload(p->d_c1d, F.c1.data(), snum * 8)) || (rc = upload(p->d_c2d, F.c2.data(), snum * 8)) ||
            (rc = upload(p->d_find, F.fin.data(), snum * 8)))
            return rc;
    } else {
        const KirchFactors<float> F = kirch_factors<float>(*p, tt_sec, snum, p->vel);
        if ((rc = upload(p->d_c1, F.c1.data(), snum * 4)) || (rc = upload(p->d_c2, F.c2.data(), snum * 4)) ||
            (rc = upload(p->d_fin, F.fin.data(), snum * 4)))
            return rc;
    }
    KirchRingTables T = kirch_ring_tables(*p, *p, tt_sec, snum, p->tnum, p->h_half);
    p->nchunks = T.nchunks;
    p->nb = T.nb;
    p->ntab = T.ntab;
    p->mrow0 = T.mrow0;
    p->nrows = T.nrows;
    if (T.tkbytes >= ((size_t)1 << 31)) {      // the kernels address it as one raw buffer
        impdar_set_error("fast Kirchhoff pick table of %zu bytes exceeds 2 GiB; use the exact mode", T.tkbytes);
        return IMPDAR_ERR_UNSUPPORTED;
    }
    const size_t ent = (size_t)p->ntab * snum;
    bool ok = true;
    for (int b = 0; b < 2; ++b) {
        ok = ok && p->d_TK[b].ensure(T.tkbytes) == hipSuccess;
        if (!ring) ok = ok && p->d_TW[b].ensure(ent * 4) == hipSuccess;
        if (!ring && p->nearfield) ok = ok && p->d_TW2[b].ensure(ent * 4) == hipSuccess;
    }
    if (!ok) {
        impdar_set_error("hipMalloc of the %zu-byte pick table failed", T.tkbytes);
        return IMPDAR_ERR_HIP;
    }
    if (ring && (rc = upload(p->d_WIN, T.win.data(), T.win.size() * 4))) return rc;
    if ((rc = upload(p->d_hmax, T.hmax.data(), T.nchunks * 4)) || (rc = upload(p->d_klo, T.klo.data(), T.klo.size() * 4)) ||
        (rc = upload(p->d_khi, T.khi.data(), T.khi.size() * 4)))
        return rc;
    p->h_hmax.swap(T.hmax);
    return IMPDAR_OK;
}

static int kirch_create_events(impdar_kirch_plan *p)
{
    bool ok = true;
    for (int s = 0; s < impdar_kirch_plan::NSLOT; ++s)
        for (int i = 0; i < 6; ++i) ok = ok && hipEventCreate(&p->evs[s][i]) == hipSuccess;
    for (hipEvent_t *e : {&p->ev_ready[0], &p->ev_ready[1], &p->ev_free[0], &p->ev_free[1]})
        ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!ok) impdar_set_error("hipEventCreate failed");
    return ok ? IMPDAR_OK : IMPDAR_ERR_HIP;
}

// (KirchCallerTables: kirch_plan.h)
int kirch_plan_create_impl(impdar_ctx *ctx, int dtype, int snum, int tnum, const double *dist_m, const double *tt_sec, double vel,
                           int nearfield, int grad_uniform, double grad_h, const double *ga, const double *gb, const double *gc,
                           int mode, int nranks, const KirchKnobs &knobs, const KirchCallerTables *caller, impdar_kirch_plan **out)
{
    IMPDAR_ARG_CHECK(ctx && out, "null context/plan pointer");
    IMPDAR_ARG_CHECK(dtype == IMPDAR_F32 || dtype == IMPDAR_F64, "dtype must be 0 (f32) or 1 (f64)");
    IMPDAR_ARG_CHECK(snum >= 2 && tnum >= 1, "need snum >= 2 and tnum >= 1 (got %d, %d)", snum, tnum);
    IMPDAR_ARG_CHECK(dist_m && tt_sec, "dist/travel_time must not be null");
    IMPDAR_ARG_CHECK(vel > 0, "vel must be positive");
    IMPDAR_ARG_CHECK(nranks >= 1, "nranks must be >= 1");
    IMPDAR_ARG_CHECK(grad_uniform || (ga && gb && gc), "non-uniform gradient needs ga/gb/gc");

    // (the geometry analysis and the kernel choice are pure host code and run before the first HIP call, so their
    // argument errors do not need a device: tests/test_sanitizer.py drives them under ASan/UBSan)
    const KirchGeometry G = kirch_geometry(snum, tnum, dist_m, tt_sec, vel, caller ? &caller->tmax : nullptr);
    IMPDAR_ARG_CHECK(G.increasing, "travel_time must be strictly increasing");
    const KirchRoute R = kirch_route(G, dtype, snum, tnum, nranks, nearfield, mode, knobs, caller && !caller->standard);
    if (R.status != IMPDAR_OK) {
        impdar_set_error("the float32 Kirchhoff kernels need float32 data on a uniform travel_time axis and either a "
                         "uniform dist with moveout 2dx/(v dt) <= %.1f samples per trace (got %.2f) or a sorted dist "
                         "whose 32-trace windows span <= 760 samples of moveout",
                         R.err_limit, R.err_sa);
        return R.status;
    }
    std::unique_ptr<impdar_kirch_plan> p(new impdar_kirch_plan());
    static_cast<KirchGeometry &>(*p) = G;
    static_cast<KirchRoute &>(*p) = R;
    p->knobs = knobs;
    p->ctx = ctx;
    p->dtype = dtype;
    p->snum = snum;
    p->tnum = tnum;
    p->nranks = nranks;
    p->nearfield = nearfield ? 1 : 0;
    p->grad_uniform = grad_uniform;
    p->grad_h = grad_h;
    p->vel = vel;

    if (hipSetDevice(ctx->device) != hipSuccess) {
        impdar_set_error("hipSetDevice(%d) failed: %s", ctx->device, hipGetErrorString(hipGetLastError()));
        return IMPDAR_ERR_HIP;
    }
    const bool own = caller && !caller->standard;
    int rc;
    if ((rc = kirch_alloc_images(p.get())) ||
        (rc = kirch_upload_axes(p.get(), dist_m, tt_sec, ga, gb, gc, own ? caller->zs : nullptr, own ? caller->zs2 : nullptr)) ||
        (p->want_tie_scan && (rc = kirch_tie_scan(p.get()))) ||
        (p->gen && (rc = kirch_upload_gen_tables(p.get(), dist_m, tt_sec))) ||
        (((p->mode == IMPDAR_KIRCH_FAST && !p->gen) || p->dquad) && (rc = kirch_upload_ring_tables(p.get(), tt_sec))) ||
        (rc = kirch_create_events(p.get())))
        return rc;
    *out = p.release();
    return IMPDAR_OK;
}

extern "C" int impdar_kirch_plan_create(impdar_ctx *ctx, int dtype, int snum, int tnum,
                                        const double *dist_m, const double *tt_sec, double vel,
                                        int nearfield, int grad_uniform, double grad_h,
                                        const double *ga, const double *gb, const double *gc,
                                        int mode, int nranks, impdar_kirch_plan **out)
{
    return kirch_plan_create_impl(ctx, dtype, snum, tnum, dist_m, tt_sec, vel, nearfield, grad_uniform, grad_h, ga, gb, gc, mode, nranks,
                                  KirchKnobs::from_env(), nullptr, out);
}

extern "C" void impdar_kirch_plan_destroy(impdar_kirch_plan *p)
{
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->aux);
    (void)hipStreamSynchronize(p->ctx->stream);
    delete p;
}

extern "C" int impdar_kirch_plan_mode(const impdar_kirch_plan *p) { return p ? p->mode : IMPDAR_ERR_ARG; }
extern "C" double impdar_kirch_plan_xnoise(const impdar_kirch_plan *p) { return p ? p->xnoise : -1.0; }
extern "C" int impdar_kirch_plan_tnum_pad(const impdar_kirch_plan *p) { return p ? p->tnum_pad : IMPDAR_ERR_ARG; }
extern "C" int impdar_kirch_plan_kernel(const impdar_kirch_plan *p) { return p ? p->kernel() : IMPDAR_ERR_ARG; }
extern "C" int impdar_kirch_queue_policy(int order, int gang)
{
    if (order < KirchKnobs::ORDER_DEFAULT || order > KirchKnobs::ORDER_PACKED || !(gang == 0 || gang == 1 || gang == 2 || gang == 4))
        return IMPDAR_ERR_ARG;
    KirchKnobs::queue_policy()[0] = order;
    KirchKnobs::queue_policy()[1] = gang;
    return IMPDAR_OK;
}

extern "C" int impdar_kirch_window_policy(int window)
{
    if (window < KirchKnobs::WINDOW_DEFAULT || window > KirchKnobs::WINDOW_QUAD) return IMPDAR_ERR_ARG;
    *KirchKnobs::window_policy() = window;
    return IMPDAR_OK;
}
extern "C" int impdar_kirch_plan_window(const impdar_kirch_plan *p) { return p ? p->window : IMPDAR_ERR_ARG; }

// `more`: further input traces of the radargram whose first traces an earlier prep took, AFTER a migrate that reads
// only those has been enqueued (the pipelined one-shot call): same buffer set, and no wait for that migrate -- it does
// not read the rows written here.
int kirch_prep_impl(impdar_kirch_plan *p, const void *d_data, int ld, int jlo, int nloc, int precomputed, bool more)
{
    IMPDAR_ARG_CHECK(p && d_data, "null plan/data");
    IMPDAR_ARG_CHECK(jlo >= 0 && nloc >= 0 && jlo + nloc <= p->tnum_pad && ld >= nloc,
                     "column block [%d,%d) with ld %d does not fit the plan (tnum_pad %d)", jlo, jlo + nloc, ld,
                     p->tnum_pad);
    IMPDAR_HIP_CHECK(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->aux;
    if (more) {
        p->migrated_since_prep = false;
    } else if (p->migrated_since_prep) {
        // first prep after a migrate: a new radargram -> other buffer set, next event slot
        p->migrated_since_prep = false;
        p->buf ^= 1;
        p->slot = (p->slot + 1) % impdar_kirch_plan::NSLOT;
        p->haves[p->slot][0] = p->haves[p->slot][1] = p->haves[p->slot][2] = false;
    }
    const int b = p->buf;
    // the buffer set may still be read by the migrate of the radargram before last.  (The
    // input itself must already be complete: the upload entry points are blocking, and the
    // one-shot paths below synchronise their own copy before calling prep.)
    if (p->free_recorded[b] && !more) IMPDAR_HIP_CHECK(hipStreamWaitEvent(st, p->ev_free[b], 0));
    // d_data may have been produced by a *_dev step (band pass, re-spacing, cast, another migration).  Those only
    // enqueue on the compute stream and mark the context (impdar_ctx_mark_produced): the producer stream waits
    // for the last such mark.  The mark sits in FRONT of any diffraction sum enqueued since, so the prep of
    // radargram s+1 still overlaps the migrate of radargram s; only when the input IS the previous migrate's
    // output does prep wait for that kernel.
    if (p->ctx->produced) IMPDAR_HIP_CHECK(hipStreamWaitEvent(st, p->ctx->ev_produced, 0));
    if (p->last_out && d_data == p->last_out && p->free_recorded[p->last_out_buf])
        IMPDAR_HIP_CHECK(hipStreamWaitEvent(st, p->ev_free[p->last_out_buf], 0));
    hipEvent_t *ev = p->evs[p->slot];
    if (!p->haves[p->slot][0]) IMPDAR_HIP_CHECK(hipEventRecord(ev[0], st));
    int rc;
    if (nloc > 0 && (rc = prep_image(p, d_data, ld, jlo, nloc, precomputed, b, st))) return rc;
    if (p->dquad)
        rc = kirch_table_ring64(p, b, st);
    else
        rc = (p->mode == IMPDAR_KIRCH_FAST && !p->gen) ? kirch_table_ring32(p, b, st) : IMPDAR_OK;
    if (rc) return rc;
    IMPDAR_HIP_CHECK(hipEventRecord(ev[1], st));
    IMPDAR_HIP_CHECK(hipEventRecord(p->ev_ready[b], st));
    p->haves[p->slot][0] = true;
    return IMPDAR_OK;
}

extern "C" int impdar_kirch_prep(impdar_kirch_plan *p, const void *d_data, int ld, int jlo, int nloc)
{
    return kirch_prep_impl(p, d_data, ld, jlo, nloc, 0);
}

int impdar_kirch_prep_precomputed(impdar_kirch_plan *p, const void *d_grad, int ld, int jlo, int nloc)
{
    return kirch_prep_impl(p, d_grad, ld, jlo, nloc, 1);
}

extern "C" int impdar_kirch_migrate(impdar_kirch_plan *p, void *d_out, int xlo, int xhi)
{
    IMPDAR_ARG_CHECK(p && d_out, "null plan/output");
    IMPDAR_ARG_CHECK(0 <= xlo && xlo <= xhi && xhi <= p->tnum, "bad output trace range [%d,%d) for tnum %d", xlo,
                     xhi, p->tnum);
    IMPDAR_HIP_CHECK(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    hipEvent_t *ev = p->evs[p->slot];
    const int b = p->buf;
    IMPDAR_HIP_CHECK(hipStreamWaitEvent(st, p->ev_ready[b], 0));      // image + table of this radargram
    if (!p->haves[p->slot][2]) IMPDAR_HIP_CHECK(hipEventRecord(ev[4], st));
    const int kern = p->kernel();
    if (xhi > xlo) {
        const int rc = kern == IMPDAR_KERNEL_GEN          ? kirch_launch_gen(p, d_out, xlo, xhi, st)
                       : kern == IMPDAR_KERNEL_EXACT_TAB  ? migrate_exact_tab(p, d_out, xlo, xhi, st)
                       : kern == IMPDAR_KERNEL_EXACT_PAIR ? migrate_exact_pair(p, d_out, xlo, xhi, st)
                       : p->dquad                         ? kirch_launch_ring64(p, d_out, xlo, xhi, st)
                                                          : kirch_launch_ring32(p, d_out, xlo, xhi, st);
        if (rc) return rc;
        if (p->ntie_groups > 0 && kern != IMPDAR_KERNEL_EXACT_PAIR) {
            const int frc = migrate_tiefix(p, kern, d_out, xlo, xhi, st);
            if (frc) return frc;
        }
    }
    IMPDAR_HIP_CHECK(hipEventRecord(ev[5], st));
    IMPDAR_HIP_CHECK(hipEventRecord(p->ev_free[b], st));
    p->free_recorded[b] = true;
    p->last_out = d_out;
    p->last_out_buf = b;
    p->migrated_since_prep = true;
    p->haves[p->slot][2] = true;
    return IMPDAR_OK;
}

// defined in comm.hip
int impdar_allgather_rows(impdar_ctx *ctx, void *image, size_t bytes_per_rank, hipStream_t stream);

extern "C" int impdar_kirch_allgather(impdar_kirch_plan *p)
{
    IMPDAR_ARG_CHECK(p, "null plan");
    // (IMPDAR_COMM_EMULATE=1, diagnostics: a plan built for N ranks driven over a 1-rank communicator -- one rank of an
    // N-rank run emulated on a single GPU with self send/recv, profiles/tools/exchange_overlap.py)
    IMPDAR_ARG_CHECK(p->nranks == p->ctx->nranks || getenv("IMPDAR_COMM_EMULATE"),
                     "plan was built for %d ranks but the communicator has %d", p->nranks, p->ctx->nranks);
    IMPDAR_HIP_CHECK(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->aux;                       // behind this radargram's prep
    hipEvent_t *ev = p->evs[p->slot];
    const int b = p->buf;
    IMPDAR_HIP_CHECK(hipEventRecord(ev[2], st));
    if (p->nranks > 1 || p->ctx->comm) {        // a 1-rank communicator still runs the (trivial) collective
        const size_t per = (size_t)(p->tnum_pad / p->nranks) * p->snum * impdar_dtype_size(p->dtype);
        int rc = impdar_allgather_rows(p->ctx, img_row0(p, p->GT[b]), per, st);
        if (rc) return rc;
        if (p->nearfield && (rc = impdar_allgather_rows(p->ctx, img_row0(p, p->DT[b]), per, st))) return rc;
    }
    IMPDAR_HIP_CHECK(hipEventRecord(ev[3], st));
    IMPDAR_HIP_CHECK(hipEventRecord(p->ev_ready[b], st));
    p->haves[p->slot][1] = true;
    return IMPDAR_OK;
}

// defined in comm.hip
int impdar_exchange_ranges(impdar_ctx *ctx, void *image, int nsend, const int *speer, const size_t *soff,
                           const size_t *slen, int nrecv, const int *rpeer, const size_t *roff, const size_t *rlen,
                           hipStream_t stream);

// Halo exchange: grouped ncclSend/ncclRecv of image-row ranges instead of the all-gather, for shards whose
// aperture halo is narrower than the rest of the profile.  Row ranges are whole 8-trace groups
// (contiguous in both image layouts); rows nobody sends stay whatever the buffer set held -- the kernels never
// pick from rows beyond their block's aperture.
extern "C" int impdar_kirch_exchange(impdar_kirch_plan *p, int nsend, const int *speer, const int *slo, const int *shi,
                                     int nrecv, const int *rpeer, const int *rlo, const int *rhi)
{
    IMPDAR_ARG_CHECK(p, "null plan");
    IMPDAR_ARG_CHECK(nsend >= 0 && nrecv >= 0 && nsend <= 4096 && nrecv <= 4096, "bad range counts %d / %d", nsend, nrecv);
    IMPDAR_ARG_CHECK((nsend == 0 || (speer && slo && shi)) && (nrecv == 0 || (rpeer && rlo && rhi)), "null range arrays");
    // (IMPDAR_COMM_EMULATE=1, diagnostics: a plan built for N ranks driven over a 1-rank communicator -- one rank of an
    // N-rank run emulated on a single GPU with self send/recv, profiles/tools/exchange_overlap.py)
    IMPDAR_ARG_CHECK(p->nranks == p->ctx->nranks || getenv("IMPDAR_COMM_EMULATE"),
                     "plan was built for %d ranks but the communicator has %d", p->nranks, p->ctx->nranks);
    const size_t rowb = (size_t)p->snum * impdar_dtype_size(p->dtype);
    std::vector<size_t> soff(nsend), slen(nsend), roff(nrecv), rlen(nrecv);
    auto conv = [&](int lo, int hi, size_t &off, size_t &len) {
        if (lo < 0 || hi < lo || hi > p->tnum_pad || (lo & 7) || (hi & 7)) return false;
        off = (size_t)lo * rowb;
        len = (size_t)(hi - lo) * rowb;
        return true;
    };
    for (int i = 0; i < nsend; ++i)
        IMPDAR_ARG_CHECK(conv(slo[i], shi[i], soff[i], slen[i]), "send rows [%d,%d) are not whole 8-trace groups of the image", slo[i], shi[i]);
    for (int i = 0; i < nrecv; ++i)
        IMPDAR_ARG_CHECK(conv(rlo[i], rhi[i], roff[i], rlen[i]), "receive rows [%d,%d) are not whole 8-trace groups of the image", rlo[i], rhi[i]);
    IMPDAR_HIP_CHECK(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->aux;                       // behind this radargram's prep
    hipEvent_t *ev = p->evs[p->slot];
    const int b = p->buf;
    IMPDAR_HIP_CHECK(hipEventRecord(ev[2], st));
    int rc = impdar_exchange_ranges(p->ctx, img_row0(p, p->GT[b]), nsend, speer, soff.data(), slen.data(), nrecv, rpeer,
                                    roff.data(), rlen.data(), st);
    if (rc) return rc;
    if (p->nearfield && (rc = impdar_exchange_ranges(p->ctx, img_row0(p, p->DT[b]), nsend, speer, soff.data(), slen.data(),
                                                     nrecv, rpeer, roff.data(), rlen.data(), st)))
        return rc;
    IMPDAR_HIP_CHECK(hipEventRecord(ev[3], st));
    IMPDAR_HIP_CHECK(hipEventRecord(p->ev_ready[b], st));
    p->haves[p->slot][1] = true;
    return IMPDAR_OK;
}

extern "C" int impdar_kirch_history_ms(impdar_kirch_plan *p, int back, float *prep_ms, float *gather_ms,
                                       float *migrate_ms)
{
    IMPDAR_ARG_CHECK(p, "null plan");
    IMPDAR_ARG_CHECK(back >= 0 && back < impdar_kirch_plan::NSLOT, "history depth is %d steps",
                     impdar_kirch_plan::NSLOT);
    IMPDAR_HIP_CHECK(hipSetDevice(p->ctx->device));
    const int s = ((p->slot - back) % impdar_kirch_plan::NSLOT + impdar_kirch_plan::NSLOT) % impdar_kirch_plan::NSLOT;
    float *outs[3] = {prep_ms, gather_ms, migrate_ms};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        *outs[i] = 0.f;
        if (!p->haves[s][i]) continue;
        IMPDAR_HIP_CHECK(hipEventSynchronize(p->evs[s][2 * i + 1]));
        IMPDAR_HIP_CHECK(hipEventElapsedTime(outs[i], p->evs[s][2 * i], p->evs[s][2 * i + 1]));
    }
    return IMPDAR_OK;
}

extern "C" int impdar_kirch_last_ms(impdar_kirch_plan *p, float *prep_ms, float *gather_ms, float *migrate_ms)
{
    return impdar_kirch_history_ms(p, 0, prep_ms, gather_ms, migrate_ms);
}


extern "C" long long impdar_kirch_count_pairs(const impdar_kirch_plan *p, int xlo, int xhi)
{
    if (!p || !p->uniform || xlo < 0 || xhi > p->tnum || xlo > xhi) return -1;
    long long total = 0;
    for (int k = 0; k < p->snum; ++k) {
        const long long h = p->h_half[k];
        if (h < 0) continue;
        for (int xi = xlo; xi < xhi; ++xi) {
            const long long lo = std::max<long long>(xi - h, 0), hi = std::min<long long>(xi + h, p->tnum - 1);
            total += hi - lo + 1;
        }
    }
    return total;
}

