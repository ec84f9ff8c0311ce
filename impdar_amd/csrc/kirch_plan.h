// The Kirchhoff plan object and the functions by which the Kirchhoff units reach each other: kirchhoff.hip (plan creation,
// prep, migrate dispatch, exchange), kirch_ring32.hip / kirch_ring64.hip (the LDS-ring kernels and their launches),
// kirch_gen.hip (the non-uniform-spacing kernel) and kirch_oneshot.hip (the cached one-shot entry and the reference hook).
#pragma once
#include "common.h"
#include "kirch_route.h"
#include <vector>

#define KF_PAD_ROWS 128      // zero traces kept on both sides of the image (loops are clipped to the profile)

// What the host decided when the plan was created (the axes, the kernel and its sizes: kirch_route.h) are its base classes:
// p->dt, p->uniform, p->mode, p->quad, p->xb ... are read from there and never written after creation.
struct impdar_kirch_plan : KirchGeometry, KirchRoute {
    impdar_ctx *ctx = nullptr;
    KirchKnobs knobs;           // the IMPDAR_KIRCH_* settings the plan was created under
    int dtype = IMPDAR_F32, snum = 0, tnum = 0, nranks = 1;
    int nearfield = 0;
    int grad_uniform = 0;
    double grad_h = 1.0, vel = 0;
    // exact path on uniform grids: fp64 pick / weight tables (built at the first migrate)
    DevBuf d_XK, d_XW, d_XW2, d_xhmax;
    int xntab = 0;
    bool xtab_ready = false;
    int diag_tables_built = 0;
    bool table_built[2] = {false, false};   // ring kernels: the geometry-only pick table of buffer set b exists
    // device tables
    DevBuf d_dist, d_tt, d_zs, d_zs2, d_ga, d_gb, d_gc;
    // Everything a prep produces is double-buffered: prep / table / all-gather of radargram
    // s+1 run on the context's aux stream while the diffraction sum of radargram s runs on
    // the compute stream.  `buf` flips at the first prep after a migrate.
    DevBuf GT[2], DT[2];           // images with KF_PAD_ROWS all-zero rows before row 0 and after row tnum_pad-1
    int buf = 0;
    bool migrated_since_prep = false;
    const void *last_out = nullptr;   // output of the last migrate (a prep that reads it must wait for that kernel)
    int last_out_buf = 0;
    hipEvent_t ev_ready[2] = {nullptr, nullptr};   // image + table of buffer b complete (aux stream)
    hipEvent_t ev_free[2] = {nullptr, nullptr};    // last migrate reading buffer b done (compute stream)
    bool free_recorded[2] = {false, false};
    DevBuf d_hmax, d_klo, d_khi;
    DevBuf d_TK[2], d_TW[2], d_TW2[2], d_c1, d_c2, d_fin, d_WIN;
    int nrows = 0, mrow0 = 0;   // quad kernel: step-block table rows (see FastParams)
    int nb = 0, ntab = 0;
    std::vector<int> h_hmax;    // host copy of the per-chunk aperture half widths (tile cost model)
    DevBuf d_queue;             // quad kernel, persistent workgroups: per-XCD item counters
    int slots = 0;              // ... and how many of them are resident at once (occupancy query, cached)
    DevBuf d_partial;           // the partial images of the pieces of a walk (walk_parts_log2)
    DevBuf d_side_l, d_side_r;  // quad-aligned window: the tiles' sums of the columns they share with a neighbour (FastParams::side_l)
    DevBuf d_tilemap;           // ring kernels: (chunk, slot, XCD) -> output tile, balanced over the XCDs
    std::vector<short> h_tilemap;
    int tm_key[5] = {-1, -1, -1, -1, -1};   // (xlo, xhi, tile width, G, tiles_per_xcd) the cached map was built for
    DevBuf d_items;             // ... persistent workgroups: the XCDs' item lists (FastParams::items)
    std::vector<int> h_items;
    int gm_key[5] = {-1, -1, -1, -1, -1};   // (xlo, xhi, tile width, gang size, order) the cached lists were built for
    // float32 data on a non-uniform (sorted) dist[]: kirch_gen_kernel (kirch_gen.h)
    DevBuf d_ga32, d_ga2_32, d_alo2, d_jr;
    std::vector<double> h_dist, h_zs2min;   // host copies for the per-(chunk, tile) input trace ranges
    std::vector<int2> h_jr;
    int jr_key[2] = {-1, -1};   // (xlo, xhi) the cached ranges were built for
    int ntie_groups = 0;        // samples with flagged offsets (kirch_tiefix_kernel after every table-driven diffraction sum)
    DevBuf d_tie_ti, d_tie_off, d_tie_n;
    DevBuf d_c1d, d_c2d, d_find;
    // host copies for pair counting
    std::vector<int> h_half;       // exact aperture half-width per sample (uniform grids)
    int nchunks = 0;
    // ring of HIP-event sets so a timed loop can read per-step kernel
    // durations afterwards without synchronising inside the loop
    static constexpr int NSLOT = 64;
    hipEvent_t evs[NSLOT][6] = {};
    bool haves[NSLOT][3] = {};
    int slot = 0;

    ~impdar_kirch_plan()
    {
        for (hipEvent_t e : {ev_ready[0], ev_ready[1], ev_free[0], ev_free[1]})
            if (e) (void)hipEventDestroy(e);
        for (int s = 0; s < NSLOT; ++s)
            for (int i = 0; i < 6; ++i)
                if (evs[s][i]) (void)hipEventDestroy(evs[s][i]);
    }
};

static inline char *img_row0(const impdar_kirch_plan *p, const DevBuf &b)  // b = GT[buf] / DT[buf]
{
    return reinterpret_cast<char *>(b.p) + (size_t)KF_PAD_ROWS * p->snum * impdar_dtype_size(p->dtype);
}

static int upload(DevBuf &b, const void *src, size_t bytes)
{
    IMPDAR_HIP_CHECK(b.ensure(bytes ? bytes : 8));
    if (bytes) IMPDAR_HIP_CHECK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return IMPDAR_OK;
}

// the axes every table / per-pair parameter struct carries
template <typename P>
static void kirch_fill_axes(P &T, const impdar_kirch_plan *p)
{
    T.zs = p->d_zs.as<double>();
    T.zs2 = p->d_zs2.as<double>();
    T.tt = p->d_tt.as<double>();
    T.vel = p->vel;
    T.tmax = p->tmax;
    T.inv_dt = 1.0 / p->dt;
    T.tt0 = p->tt0;
    T.snum = p->snum;
}

// ---- what the units call of each other ----
// (what this split made a cross-unit call stays out of the library's dynamic symbol table)
#define KIRCH_LOCAL __attribute__((visibility("hidden")))
// kirch_gen.hip: kirch_gen_kernel + kirch_gen_shell_kernel on output traces [xlo, xhi) of the prepared image
int kirch_launch_gen(impdar_kirch_plan *p, void *d_out, int xlo, int xhi, hipStream_t st);
// kirch_ring32.hip (kirch_quad_kernel, kirch_tab_kernel) and kirch_ring64.hip (kirch_dquad_kernel): the diffraction sum of the
// plan's ring kernel on output traces [xlo, xhi), and the pick / weight table of buffer set b on the producer stream
KIRCH_LOCAL int kirch_launch_ring32(impdar_kirch_plan *p, void *d_out, int xlo, int xhi, hipStream_t st);
KIRCH_LOCAL int kirch_table_ring32(impdar_kirch_plan *p, int b, hipStream_t st);
KIRCH_LOCAL int kirch_launch_ring64(impdar_kirch_plan *p, void *d_out, int xlo, int xhi, hipStream_t st);
KIRCH_LOCAL int kirch_table_ring64(impdar_kirch_plan *p, int b, hipStream_t st);

// kirchhoff.hip, for the cached entry points of kirch_oneshot.hip.
// What mig_kirch_loop hands over with its call: the time limit t > t_max drops a pair at (mig_python.py:52) is the caller's
// argument there, not max(tt); `standard`: the depth tables are what the plan computes itself, bit for bit.
struct KirchCallerTables {
    double tmax;
    const double *zs, *zs2;
    bool standard;
};
KIRCH_LOCAL int kirch_plan_create_impl(impdar_ctx *ctx, int dtype, int snum, int tnum, const double *dist_m, const double *tt_sec,
                                       double vel, int nearfield, int grad_uniform, double grad_h, const double *ga, const double *gb,
                                       const double *gc, int mode, int nranks, const KirchKnobs &knobs, const KirchCallerTables *caller,
                                       impdar_kirch_plan **out);
// (`more`: further input traces of a radargram whose first traces an earlier prep took; see the definition)
KIRCH_LOCAL int kirch_prep_impl(impdar_kirch_plan *p, const void *d_data, int ld, int jlo, int nloc, int precomputed, bool more = false);
int impdar_kirch_prep_precomputed(impdar_kirch_plan *p, const void *d_grad, int ld, int jlo, int nloc);
