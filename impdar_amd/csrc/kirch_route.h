// What the Kirchhoff plan (impdar_kirch_plan_create, kirchhoff.hip) decides on the host: the analysis of the two axes, the
// choice between the six kernels with their tile widths, ring sizes and table shifts, and the host tables the stages of the
// plan upload; and where the one-shot entry point (kirch_oneshot.hip) cuts a large radargram.  Plain C++, no device code --
// compiled into the library through kirch_plan.h by every Kirchhoff unit and, by itself with g++, into the CPU suite's
// checker (tests/test_kirch_route.py).  The IMPDAR_KIRCH_* plan knobs are read once, by KirchKnobs::from_env() when
// a plan is created; the plan keeps them with its route, and prep / migrate go by what is stored.
#pragma once
#include "../../include/impdar_hip.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define KIRCH_HD __host__ __device__
#else
#define KIRCH_HD
#endif

#define KF_THREADS 256
#define KF_W 512            // LDS floats per ring slot (circular window)

// ---- ring geometry of kirch_quad_kernel / kirch_dquad_kernel (the LDS image is described at kirch_quad_kernel) ----
#define KQ_GS 1056          // bytes between the trace groups inside a piece (32 rows x 32 B + spare row)
// ring slots for an XB-trace output tile (XB + 15 traces are live, in whole 8-trace groups) and bytes per
// 32-row piece: the groups + pad to a multiple of 256 B (rows of neighbouring pieces then keep distinct
// banks inside one ds_read_b128 lane group)
KIRCH_HD constexpr int kq_ring_slots(int xb) { return ((xb + 15 + 7) / 8) * 8; }
KIRCH_HD constexpr int kq_piece_bytes(int xb) { return ((kq_ring_slots(xb) / 8 * KQ_GS + 255) / 256) * 256; }
// ... and with LK extra ring groups (deeper staging lookahead, see kirch_quad_kernel)
KIRCH_HD constexpr int kq_piece_bytes_lk(int xb, int lk) { return (((kq_ring_slots(xb) / 8 + lk) * KQ_GS + 255) / 256) * 256; }
static_assert(kq_piece_bytes_lk(40, 0) == 7424 && kq_piece_bytes_lk(40, 1) == 8448 && kq_piece_bytes_lk(24, 0) == 5376, "");
static_assert(kq_ring_slots(24) == 40 && kq_piece_bytes(24) == 5376 && kq_ring_slots(32) == 48 && kq_piece_bytes(32) == 6400 &&
              kq_ring_slots(40) == 56 && kq_piece_bytes(40) == 7424, "");
KIRCH_HD constexpr int kd_ring_slots(int xb) { return ((xb + 7 + 3) / 4) * 4; }     // XB + 2 S - 1 live traces, whole groups
KIRCH_HD constexpr int kd_piece_bytes(int xb) { return ((kd_ring_slots(xb) / 4 * KQ_GS + 255) / 256) * 256; }
static_assert(kd_ring_slots(20) == 28 && kd_piece_bytes(20) == 7424 && kd_ring_slots(16) == 24 && kd_piece_bytes(16) == 6400, "");
#ifndef KQ_DEFAULT_NH
#define KQ_DEFAULT_NH 1     // output tiles per workgroup of the quad kernel (IMPDAR_KIRCH_NH overrides)
#endif
#ifndef KD_DEFAULT_NH
#define KD_DEFAULT_NH 1     // the same for the float64 ring kernel (IMPDAR_KIRCH_NHD), with tiles of KD_DEFAULT_XB2 traces
#endif
#ifndef KD_DEFAULT_XB2
#define KD_DEFAULT_XB2 16
#endif
#ifndef KQ_DEFAULT_LK
#define KQ_DEFAULT_LK 0     // extra ring groups / blocks of staging lookahead with NH >= 2 (IMPDAR_KIRCH_LK overrides)
#endif
// The queue lists of the persistent ring kernels (kirch_gangmap): their order, and the adjacent tiles per gang where a
// launch has tiles enough for KQ_GANG_MIN_GROUPS gangs per chunk on every XCD (kirch_queue_order, kirch_gang_size).  Same-box
// A/B at config 3 (157 workgroup tiles; profiles/kirch_gangs.txt): packed order with gangs of 4 is 2.7-3.1 % faster than the chunk
// order without gangs; the order alone gives 1.5 %, gangs of 4 alone 1.1 %, gangs of 2 half of that; the float64 ring (250
// tiles) gains 2.4 %.  Launches too short for gangs keep the chunk order: on the block of a rank of a 4-rank plan (63 tiles,
// walks in 2 pieces) the packed order measured 3.4 % SLOWER, of an 8-rank plan (32 tiles, 4 pieces) the same.
enum { KIRCH_ORDER_AUTO = -1, KIRCH_ORDER_CHUNK = 0, KIRCH_ORDER_PACKED = 1 };
#ifndef KQ_DEFAULT_ORDER
#define KQ_DEFAULT_ORDER KIRCH_ORDER_AUTO       // packed where the launch has tiles for gangs, else chunk; impdar_kirch_queue_policy overrides
#endif
#ifndef KQ_DEFAULT_GANG
#define KQ_DEFAULT_GANG 4                       // of the packed order; impdar_kirch_queue_policy overrides
#endif
#ifndef KQ_GANG_MIN_GROUPS
#define KQ_GANG_MIN_GROUPS 4
#endif
// The output window of a tile of kirch_quad_kernel (far field).  SLIDE: outputs [x0, x0 + XB) at every step; a lane's XB
// ring slots start on a quad boundary one step in four, and it reads XB/4 + 1 quads at the other three.  QUAD: at offset n
// the outputs [x0 - (n & 3), x0 - (n & 3) + XB), read from the ALIGNED XB slots -- XB/4 quads at every step, XB + 3
// accumulators, and the three columns left of every tile start are the sum of two tiles' partial sums (kirch_quadwin_cover
// below, kirch_fixup_kernel).  Tiles then start at multiples of the workgroup tile from trace 0, whatever the output block,
// so that a block of a launch still equals the same columns of the whole image bit for bit.
enum { KIRCH_WINDOW_SLIDE = 0, KIRCH_WINDOW_QUAD = 1 };
#define KQ_WIN_EXTRA 3      // steps a staged trace stays in use longer, and a walk runs longer, under KIRCH_WINDOW_QUAD
#ifndef KQ_DEFAULT_WINDOW
#define KQ_DEFAULT_WINDOW KIRCH_WINDOW_QUAD     // where it is routed (kirch_route); impdar_kirch_window_policy overrides
#endif
// One step of the quad-aligned window, as kirch_quad_kernel's load_step / fma_step and the host-side cover
// (kirch_quadwin_cover) both take it.  pm: the step's index mod the ring slots (a multiple of 8); a walk starts at an offset
// nlo = 1 (mod 8) and relative trace q sits in ring slot q + 1, so pm + 1 = n (mod 8).
KIRCH_HD constexpr int kq_win_phase(int pm) { return (pm + 1) & 3; }                            // n & 3
KIRCH_HD constexpr int kq_win_first_quad(int pm, int nq) { return ((pm + 1) >> 2) % nq; }       // the run is XB/4 quads long
// component c of the t-th quad of the run feeds accumulator a of XB + 3; accumulator a is output x0 - 3 + a
KIRCH_HD constexpr int kq_win_acc(int pm, int t, int c) { return 4 * t + c + 3 - kq_win_phase(pm); }

// The trace offsets nlo .. nhi an item of a ring kernel walks (kirch_ring_walk, kirch_ring.h, documents them); returns true
// for an empty piece.  wx: KQ_WIN_EXTRA under KIRCH_WINDOW_QUAD -- outputs x0w - 3 .. x0w - 1 see their last offsets.
KIRCH_HD static inline bool kirch_walk_range(int hmax, int x0w, int tnum, int S, int NB, int XB, int NH, int parts_log2, int part, int wx,
                                             int &nlo, int &nhi)
{
    auto mx = [](int a, int b) { return a > b ? a : b; };
    auto mn = [](int a, int b) { return a < b ? a : b; };
    int nlo_ = mx(-hmax, -(x0w + XB - 1));
    nlo_ -= (nlo_ - 1) & (S - 1);
    int nhi_ = mn(hmax + (NH - 1) * XB, tnum - 1 - x0w + wx);
    bool empty_part = false;
    if (parts_log2) {
        // piece boundaries (all = 1 mod S): ..., 1 - U k | 1 - U k .. 0 | 1 .. U k | 1 + U k, ...   (2 pieces: n <= 0 | n >= 1)
        const int uk = (NB * S) * mx(1, (hmax + NB * S) / (2 * NB * S));
        const int inner = parts_log2 == 2 ? uk : (1 << 28);
        const int side = parts_log2 == 2 ? (part >> 1) : part;          // 0: n <= 0, 1: n >= 1
        const bool far = parts_log2 == 2 && ((part & 1) ^ side) == 0;    // pieces 0 and 3 are the outer ones
        const int lo = side == 0 ? (far ? -(1 << 28) : 1 - inner) : (far ? 1 + inner : 1);
        const int hi = side == 0 ? (far ? -inner : 0) : (far ? (1 << 28) : inner);
        nlo_ = mx(nlo_, lo);
        nhi_ = mn(nhi_, hi);
        empty_part = nhi_ < nlo_;
    }
    nlo = nlo_;
    nhi = nhi_;
    return empty_part;
}
// Row stride of the step-block pick table in 16-byte entries.  Not snum: with snum a power of two a chunk's
// slice of consecutive rows (256 entries out of every snum) lands on 1/16 of the L2's sets (and of whatever else
// indexes by address bits); the odd number of 256-byte lines of padding walks the slice over all of them.
#ifndef KQ_TKB_PAD
#define KQ_TKB_PAD 272       // entries (4352 bytes)
#endif
KIRCH_HD static inline size_t kq_tkb_stride(int snum) { return (size_t)snum + KQ_TKB_PAD; }

// Ring rows (samples per slot, whole 32-row pieces) of a workgroup with nh tiles of xb traces and step blocks of S traces
// at a moveout of sa samples per trace.  (A moveout no ring can hold -- NaN included -- gives a size that fits nothing.)
// (`extra`: further traces of moveout a staged trace stays in use for -- the quad-aligned window, KIRCH_WINDOW_QUAD)
static inline int kirch_ring_rows(double sa, int xb, int nh, int S, int extra = 0)
{
    const double m = std::ceil(sa * (xb * nh + S - 2 + extra));
    if (!(std::fabs(m) < 1e9)) return 1 << 30;
    return ((KF_THREADS + (int)m + 8 + 31) / 32) * 32;
}

// ---- the knobs of a plan -------------------------------------------------------------------------------------
// "set" is kept apart from the value where the route tests presence.  (IMPDAR_KIRCH_RESERVE, _ONESHOT_CACHE, _ONESHOT_SPLIT
// and IMPDAR_COMM_EMULATE are no plan knobs: they are read per launch / per call where they act.)
struct KirchKnobs {
    enum { IMPL_DEFAULT = 0, IMPL_TAB = 1, IMPL_GEN = 2 };
    enum { EXACT_DEFAULT = 0, EXACT_TAB = 1, EXACT_PAIR = 2 };      // (any value that is not "pair" acts as "tab")
    bool xb_set = false, nh_set = false, lk_set = false, parts_set = false, nhd_set = false, xbd_set = false;
    int xb = 0, nh = 0, lk = 0, parts = 0, nhd = 0, xbd = 0;      // XB 24|32|40, NH 1|2|3, LK 0|1, PARTS 1|2|4, NHD 1|2, XBD 16|20
    int impl = IMPL_DEFAULT;            // IMPDAR_KIRCH_IMPL = tab | gen
    int exact_impl = EXACT_DEFAULT;     // IMPDAR_KIRCH_EXACT_IMPL = tab | pair: keeps the float64 ring out
    bool tiefix_off = false;            // IMPDAR_KIRCH_TIEFIX = 0 (diagnostic)
    // The two queue knobs are no environment variables of the library (it reads 20, and that is its limit): the caller hands
    // them over with impdar_kirch_queue_policy, process-wide, and a plan takes what stands when it is created.  The Python
    // host side does that from IMPDAR_KIRCH_ORDER / IMPDAR_KIRCH_G (impdar_amd._hip.apply_queue_policy).
    enum { ORDER_DEFAULT = 0, ORDER_CHUNK = 1, ORDER_PACKED = 2 };
    bool g_set = false;
    int g = 0;                          // 1 | 2 | 4: adjacent tiles per gang of the queue lists (kirch_gangmap)
    int order = ORDER_DEFAULT;          // chunk | packed: the order of the queue lists
    // (order, gang) as impdar_kirch_queue_policy left them: ORDER_*, and 0 = the library's choice.  One instance per library.
    __attribute__((visibility("hidden"))) static int *queue_policy()
    {
        static int v[2] = {ORDER_DEFAULT, 0};
        return v;
    }

    // The window kind of the quad kernel comes the same way (impdar_kirch_window_policy; IMPDAR_KIRCH_WINDOW on the Python side).
    enum { WINDOW_DEFAULT = 0, WINDOW_SLIDE = 1, WINDOW_QUAD = 2 };
    int window = WINDOW_DEFAULT;
    __attribute__((visibility("hidden"))) static int *window_policy()
    {
        static int v = WINDOW_DEFAULT;
        return &v;
    }

    static KirchKnobs from_env()
    {
        KirchKnobs K;
        auto num = [](const char *e, bool &set, int &v) {
            set = e != nullptr;
            v = e ? atoi(e) : 0;
        };
        num(getenv("IMPDAR_KIRCH_XB"), K.xb_set, K.xb);
        num(getenv("IMPDAR_KIRCH_NH"), K.nh_set, K.nh);
        num(getenv("IMPDAR_KIRCH_LK"), K.lk_set, K.lk);
        num(getenv("IMPDAR_KIRCH_PARTS"), K.parts_set, K.parts);
        num(getenv("IMPDAR_KIRCH_NHD"), K.nhd_set, K.nhd);
        num(getenv("IMPDAR_KIRCH_XBD"), K.xbd_set, K.xbd);
        const char *ie = getenv("IMPDAR_KIRCH_IMPL"), *ee = getenv("IMPDAR_KIRCH_EXACT_IMPL"), *te = getenv("IMPDAR_KIRCH_TIEFIX");
        K.impl = !ie ? IMPL_DEFAULT : (!strcmp(ie, "tab") ? IMPL_TAB : (!strcmp(ie, "gen") ? IMPL_GEN : IMPL_DEFAULT));
        K.exact_impl = !ee ? EXACT_DEFAULT : (!strcmp(ee, "pair") ? EXACT_PAIR : EXACT_TAB);
        K.tiefix_off = te && !strcmp(te, "0");
        K.order = queue_policy()[0];
        K.g = queue_policy()[1];
        K.g_set = K.g != 0;
        K.window = *window_policy();
        return K;
    }
    bool operator==(const KirchKnobs &o) const
    {
        return xb_set == o.xb_set && nh_set == o.nh_set && lk_set == o.lk_set && parts_set == o.parts_set && nhd_set == o.nhd_set &&
               xbd_set == o.xbd_set && xb == o.xb && nh == o.nh && lk == o.lk && parts == o.parts && nhd == o.nhd && xbd == o.xbd &&
               impl == o.impl && exact_impl == o.exact_impl && tiefix_off == o.tiefix_off && g_set == o.g_set && g == o.g && order == o.order &&
               window == o.window;
    }
};

// ---- the two axes ----------------------------------------------------------------------------------------------
struct KirchGeometry {
    double tmax = 0;            // the time limit t > t_max drops a pair at (mig_python.py:52): max(tt), or the caller's own
    bool tmax_given = false;
    bool increasing = true;     // tt strictly increasing (anything else is an argument error)
    double dt = 1, dx = 1, tt0 = 0;
    bool uni_t = false, uni_t11 = false, uni_x = false;    // tt on its fitted grid to 1e-9 dt / to 1e-11 dt; dist to 1e-9 dx
    bool uniform = false;       // uni_t && uni_x
    bool dist_sorted = false;
    double xnoise = 0;          // position noise of a pair's dist[j] - dist[xi] against n dx, in units of dx
    double sa = 0, alpha = 1;   // samples of moveout per trace at far offset, 2 dx / (v dt); its square
    double hest = 0;            // aperture half width in traces (upper bound)
    double gen_need = 0;        // kirch_gen_kernel: 264 + the largest extent of 32 consecutive traces, in samples
};

static inline KirchGeometry kirch_geometry(int snum, int tnum, const double *dist_m, const double *tt_sec, double vel, const double *tmax_override)
{
    KirchGeometry G;
    G.tmax = tt_sec[0];
    for (int k = 1; k < snum; ++k) {
        G.tmax = std::max(G.tmax, tt_sec[k]);
        if (!(tt_sec[k] > tt_sec[k - 1])) G.increasing = false;
    }
    G.tmax_given = tmax_override != nullptr;
    if (tmax_override) G.tmax = *tmax_override;
    const double dt = (tt_sec[snum - 1] - tt_sec[0]) / (snum - 1);
    G.uni_t = dt > 0;
    for (int k = 0; k < snum && G.uni_t; ++k)
        if (std::fabs(tt_sec[k] - (tt_sec[0] + k * dt)) > 1e-9 * dt) G.uni_t = false;
    G.uni_t11 = G.uni_t;        // the float64 re-decision of a pick (kirch_gen_kernel) takes tt[k] = tt[0] + k dt: to 1e-11 dt
    for (int k = 0; k < snum && G.uni_t11; ++k)
        if (std::fabs(tt_sec[k] - (tt_sec[0] + k * dt)) > 1e-11 * dt) G.uni_t11 = false;
    double dx = 1.0;
    G.uni_x = true;
    if (tnum >= 2) {
        dx = (dist_m[tnum - 1] - dist_m[0]) / (tnum - 1);
        G.uni_x = dx > 0;
        for (int j = 0; j < tnum && G.uni_x; ++j)
            if (std::fabs(dist_m[j] - (dist_m[0] + j * dx)) > 1e-9 * dx) G.uni_x = false;
    }
    G.dist_sorted = true;
    for (int j = 1; j < tnum; ++j)
        if (!(dist_m[j] >= dist_m[j - 1])) G.dist_sorted = false;
    // measured on the profile: twice the largest deviation from the fitted grid plus the rounding of the largest |dist|
    // (never less than 4.5e-16 tnum)
    double dev = 0.0, amax = 0.0, ext = 0.0;
    for (int j = 0; j < tnum; ++j) {
        dev = std::max(dev, std::fabs(dist_m[j] - (dist_m[0] + j * dx)));
        amax = std::max(amax, std::fabs(dist_m[j]));
        ext = std::max(ext, dist_m[std::min(j + 31, tnum - 1)] - dist_m[j]);
    }
    G.xnoise = std::max(4.5e-16 * (double)tnum, (2.0 * dev + 4.5e-16 * amax) / (dx > 0 ? dx : 1.0));
    G.dt = dt;
    G.dx = dx;
    G.tt0 = tt_sec[0];
    G.uniform = G.uni_t && G.uni_x;
    G.sa = 2.0 * dx / (vel * dt);
    G.alpha = G.sa * G.sa;
    // below 65536 (the kernels square trace offsets in 32 bits); the span of image groups one workgroup walks must stay
    // inside its 2 GiB raw buffer (kirch_route)
    G.hest = std::min(std::fabs(G.tmax / dt) / G.sa + 2.0, (double)tnum + 128.0);
    G.gen_need = 264.0 + std::ceil(ext * 2.0 / (vel * dt));
    return G;
}

// ---- the choice of kernel --------------------------------------------------------------------------------------
struct KirchRoute {
    int status = IMPDAR_OK;         // IMPDAR_ERR_UNSUPPORTED: FAST asked for where no float32 kernel applies ...
    double err_limit = 0, err_sa = 0;   // ... with the two numbers of its message
    int requested_mode = IMPDAR_KIRCH_AUTO, mode = IMPDAR_KIRCH_EXACT;
    int tnum_pad = 0;               // equal input shards of whole 8-row groups (the grouped image layout keeps a shard contiguous)
    bool gen = false;               // float32 data on a non-uniform (sorted) dist[]: kirch_gen_kernel
    int genW = 0;                   // ... samples per LDS slot
    bool quad = false;              // sample-major LDS ring (kirch_quad_kernel); FAST without it: kirch_tab_kernel
    bool dquad = false;             // the same ring in float64 (kirch_dquad_kernel): exact mode, float64 data, uniform grids
    int xb = 24;                    // output traces per tile (ring kernels; 16: tab ring; 32: gen)
    int nh = 1;                     // ring kernels: output tiles per workgroup sharing one ring (256 nh threads)
    int lk = 0;                     // ... and extra ring groups = blocks of additional staging lookahead (nh >= 2 only)
    int quadW = 0;                  // samples per ring slot
    int quadSH = 0;                 // table entries are LDS byte offsets >> quadSH
    int walk_parts_log2 = 0;        // every tile's aperture walk as 1, 2 or 4 queue items (plans of 4+ / 8+ ranks)
    bool want_tie_scan = false;     // the table-driven kernels need the list of picks that rounding noise decides
    bool tiefix_off = false;
    bool exact_tab = false;         // exact mode off the ring: tabulated picks (uniform grids, not "pair") unless xtab_off
    bool xtab_off = false;
    bool tie_ambiguous = false;     // more rounding-noise ties than the list holds: per-pair kernel only
    bool want_tie_groups = false;   // (kirch_route_after_ties) the downloaded list is to be grouped and kept
    int order = KIRCH_ORDER_AUTO;   // ring kernels, queue lists: KIRCH_ORDER_CHUNK | _PACKED (kirch_gangmap); _AUTO: by the launch (kirch_queue_order)
    int gang = 0;                   // ... adjacent tiles per gang, 1 | 2 | 4; 0: by the tile count of the launch (kirch_gang_size)
    int window = KIRCH_WINDOW_SLIDE;    // quad kernel, far field: KIRCH_WINDOW_QUAD where the ring holds its 3 further traces of moveout

    int kernel() const             // what impdar_kirch_plan_kernel reports
    {
        if (gen) return IMPDAR_KERNEL_GEN;
        if (mode == IMPDAR_KIRCH_FAST) return quad ? IMPDAR_KERNEL_QUAD : IMPDAR_KERNEL_TAB;
        if (dquad) return IMPDAR_KERNEL_DQUAD;
        return (exact_tab && !xtab_off) ? IMPDAR_KERNEL_EXACT_TAB : IMPDAR_KERNEL_EXACT_PAIR;
    }
};

// caller_tables: the depth tables and the time limit are the caller's own and not what the plan would compute
// (mig_kirch_loop): only the per-pair kernel reads them as given.
static inline KirchRoute kirch_route(const KirchGeometry &G, int dtype, int snum, int tnum, int nranks, int nearfield, int requested_mode,
                                     const KirchKnobs &K, bool caller_tables)
{
    KirchRoute R;
    R.requested_mode = requested_mode;
    R.tnum_pad = ((tnum + 8 * nranks - 1) / (8 * nranks)) * 8 * nranks;
    R.tiefix_off = K.tiefix_off;
    const double sa = G.sa;
    const bool whole = (long long)tnum >= 8000LL * nranks;      // a rank's block of under ~8000 traces gives two-tile workgroups too few items per slot
    auto ring32 = [&](int xb, int nh, int lk) { return (size_t)(kirch_ring_rows(sa, xb, nh, 8) / 32) * kq_piece_bytes_lk(xb, lk); };
    // The fast kernels need the moveout small enough for their LDS windows: quad (sample-major ring, 8-step blocks) or,
    // for steeper moveout, tab (trace-major ring of 16 traces, 512-sample slots).
    // quad kernel's output-trace tile: 24 traces (40-slot ring, three workgroups per CU) or 40 traces (56-slot ring, two
    // workgroups per CU).  The wider tile stages and picks 40 % less per pair and is 2.5-5 % faster on a whole radargram
    // (same-box A/B at config 3; 32 traces: 1.3 %); with the balanced tile map and the work queues it is ahead on the
    // short launches of a many-rank run too (1.31 vs 1.41 ms for an 8-rank block of config 3).
    int xbq = 24;
    if (K.xb_set && (K.xb == 24 || K.xb == 32 || K.xb == 40))
        xbq = K.xb;
    else if (ring32(40, 1, 0) <= 80 * 1024)
        xbq = 40;
    // Whole radargrams by default: TWO tiles of 32 traces per workgroup on one ring (NH = 2) when that ring fits half a
    // CU's LDS: two workgroups of 8 waves per CU instead of two of 4.  Same-box A/B at config 3: 2 % faster than one
    // 40-trace tile per workgroup, and the fabric traffic roughly halves.  (Blocks of a many-rank run keep 40 x 1:
    // profiles/r02_rank_steps_tiles.txt, 4.28 / 2.32 / 1.31 ms at 2 / 4 / 8 ranks against 4.33 / 2.39 / 1.65.)
    bool pair32 = false;
    if (!K.xb_set && !K.nh_set && !nearfield && xbq == 40 && whole && ring32(32, 2, 0) <= 80 * 1024 && ring32(32, 2, 0) > 65535) {
        pair32 = true;
        xbq = 32;
    }
    // tiles per workgroup on one ring: the staging window grows by the moveout over the (nh - 1) xb traces the later
    // tiles lag behind; one workgroup per CU then (up to the whole 160 KB)
    int nhq = 1;
    {
        const int want = K.nh_set ? K.nh : (pair32 ? 2 : KQ_DEFAULT_NH);
        if ((want == 2 || want == 3) && (xbq == 40 || (xbq == 32 && want == 2)) && !nearfield && (K.nh_set || pair32) &&
            ring32(xbq, want, 0) <= 160 * 1024 && ring32(xbq, want, 0) > 65535)
            nhq = want;
    }
    const int wq = kirch_ring_rows(sa, xbq, nhq, 8);
    // every wave must own at least one DMA piece per block (the in-order wait counts on it)
    const int lkq = ((K.lk_set ? K.lk : KQ_DEFAULT_LK) == 1 && nhq >= 2 && wq / 32 >= 4 * nhq && ring32(xbq, nhq, 1) <= 160 * 1024) ? 1 : 0;
    // (two workgroups per CU: 80 KB of LDS each; table entries are 16-bit byte offsets up to 12 pieces, 16-byte units beyond)
    const bool quad_ok = ring32(xbq, nhq, lkq) <= (size_t)(nhq > 1 ? 160 : 80) * 1024;
    const bool tab_ok = (KF_THREADS + sa * (16 - 1) + 8.0) <= (double)KF_W;
    const bool aperture_ok = snum < 65536 && std::fabs(G.tmax / G.dt) / sa < 65000.0;
    const bool fast_ok = dtype == IMPDAR_F32 && G.uniform && (quad_ok || tab_ok) && aperture_ok &&
                         (2.0 * G.hest + 400.0) / 8.0 * (double)snum * 32.0 < 2147483648.0;
    // float32 data on a profile whose spacing is NOT uniform (mig_python.py:44 takes any dist[]): kirch_gen_kernel
    // computes every pair's pick from the positions.  It needs a uniform time axis, a sorted dist[] (the staging windows
    // and the input range of a tile come from bisections) and, per 32 consecutive output traces, a moveout that fits
    // its LDS slots: W >= 264 + (extent of the 32 traces in samples).  IMPDAR_KIRCH_IMPL=gen takes it on uniform
    // profiles too (A/B against the ring kernels).
    int gen_w = 0;
    const bool gen_ok = dtype == IMPDAR_F32 && G.uni_t11 && G.dist_sorted && tnum >= 2 && snum >= 4 && snum < (1 << 22) && !G.tmax_given &&
                        (double)tnum * snum * 4.0 < 2147483648.0 && G.gen_need <= 1024.0;
    if (gen_ok) gen_w = std::max(((int)G.gen_need + 255) / 256 * 256, 512);
    int mode = requested_mode;
    const bool gen = gen_ok && mode != IMPDAR_KIRCH_EXACT && (K.impl == KirchKnobs::IMPL_GEN || !fast_ok);
    if (mode == IMPDAR_KIRCH_AUTO) mode = (fast_ok || gen) ? IMPDAR_KIRCH_FAST : IMPDAR_KIRCH_EXACT;
    if (mode == IMPDAR_KIRCH_FAST && !fast_ok && !gen) {
        R.status = IMPDAR_ERR_UNSUPPORTED;
        R.err_limit = (KF_W - KF_THREADS - 8.0) / 15.0;
        R.err_sa = sa;
        return R;
    }
    R.mode = mode;
    R.gen = gen && mode == IMPDAR_KIRCH_FAST;
    R.genW = gen_w;
    // One full-aperture walk of a shallow chunk takes ~1.2 ms at config 3 -- as long as the whole step of a rank of
    // an 8-GPU run should be, and such a rank's block has fewer items than the chip has workgroup slots.  Plans
    // of 4+ ranks cut every walk in 2, of 8+ ranks in 4 pieces (kirch_quad_kernel); the pieces are summed in a
    // fixed order, so launches stay bit-reproducible (against whole walks the sum differs by rounding).
    const int parts = K.parts_set ? K.parts : (nranks >= 8 ? 4 : (nranks >= 4 ? 2 : 1));
    R.walk_parts_log2 = parts == 4 ? 2 : (parts == 2 ? 1 : 0);
    R.order = K.order == KirchKnobs::ORDER_CHUNK ? KIRCH_ORDER_CHUNK : (K.order == KirchKnobs::ORDER_PACKED ? KIRCH_ORDER_PACKED : KQ_DEFAULT_ORDER);
    R.gang = (K.g_set && (K.g == 1 || K.g == 2 || K.g == 4)) ? K.g : 0;
    R.nh = nhq;
    R.lk = lkq;
    R.quadW = wq;
    R.quadSH = ring32(xbq, nhq, lkq) <= 65535 ? 0 : 4;
    R.quad = mode == IMPDAR_KIRCH_FAST && !R.gen && quad_ok && !(K.impl == KirchKnobs::IMPL_TAB && tab_ok);
    R.xb = R.gen ? 32 : (R.quad ? xbq : 16);
    // The quad-aligned window keeps a staged trace in use for 3 more steps: routed only where the ring has the rows for
    // that moveout already (the slot size, and with it every recorded route, stays what it was); else the sliding form.
    // The rows must hold it for one, two and three tiles per workgroup alike: the window kind then depends on the geometry
    // and the tile width alone, and the tiles per workgroup still change no bit of an image.
    {
        const int want = K.window == KirchKnobs::WINDOW_SLIDE ? KIRCH_WINDOW_SLIDE
                         : (K.window == KirchKnobs::WINDOW_QUAD ? KIRCH_WINDOW_QUAD : KQ_DEFAULT_WINDOW);
        bool rows_hold = kirch_ring_rows(sa, xbq, nhq, 8, KQ_WIN_EXTRA) == wq;
        for (int nh = 1; nh <= 3; ++nh) rows_hold = rows_hold && kirch_ring_rows(sa, xbq, nh, 8, KQ_WIN_EXTRA) == kirch_ring_rows(sa, xbq, nh, 8);
        if (want == KIRCH_WINDOW_QUAD && R.quad && !nearfield && rows_hold) R.window = KIRCH_WINDOW_QUAD;
    }
    // float64 data in exact mode on uniform grids: the same ring in float64 (20 or 16 output traces per lane, step blocks
    // of 4) when its window fits; otherwise (and for IMPDAR_KIRCH_EXACT_IMPL = tab | pair) the global-memory kernels.
    // The table-driven float64 kernels weight a pair by its trace OFFSET (n dx); the reference by dist[j] - dist[xi].
    // On a profile whose positions are noisy against the grid (a first trace tens of kilometres along the line:
    // ulp(dist) / dx ~ 1e-10; 100000 traces from 0: 4.5e-11) the two weights differ by that much relative, and the
    // result differs from the reference's by up to ~0.03 xnoise of the image maximum.  The stated bar of the float64 path
    // is  max(1e-12, 0.1 xnoise)  of the image maximum (impdar_kirch_plan_xnoise reports xnoise; picks are not affected:
    // every pick within the noise of a tie is re-done pair by pair, kirch_tiefix_kernel).
    // IMPDAR_KIRCH_EXACT_IMPL=pair still forces the reference's arithmetic pair by pair.
    if (mode == IMPDAR_KIRCH_EXACT && dtype == IMPDAR_F64 && G.uniform && aperture_ok && !caller_tables &&
        (2.0 * G.hest + 400.0) / 4.0 * (double)snum * 32.0 < 2147483648.0 && K.exact_impl == KirchKnobs::EXACT_DEFAULT) {
        auto fits = [&](int xb, int nh) {
            const size_t b = (size_t)(kirch_ring_rows(sa, xb, nh, 4) / 32) * kd_piece_bytes(xb);
            return b <= 80 * 1024 && (nh == 1 || b > 65535);
        };
        // Whole radargrams: TWO tiles of 20 traces per workgroup on one ring when that ring fits half a CU's LDS, as the
        // float32 kernel does (same-box A/B at config 3: 17.71 -> 16.91 ms; two tiles of 16: 19.2)
        int nhd = K.nhd_set ? K.nhd : ((!K.xbd_set && fits(20, 2) && whole) ? 2 : KD_DEFAULT_NH);
        if (nhd != 2 || nearfield) nhd = 1;
        int xbd = (K.xbd_set && (K.xbd == 16 || K.xbd == 20)) ? K.xbd : ((nhd == 2 && K.nhd_set) ? KD_DEFAULT_XB2 : 20);
        if (nhd == 2 && !fits(xbd, 2)) nhd = 1;
        if (!fits(xbd, nhd)) xbd = 16;
        if (fits(xbd, nhd)) {
            R.dquad = true;
            R.xb = xbd;
            R.nh = nhd;
            R.quadW = kirch_ring_rows(sa, xbd, nhd, 4);
            R.quadSH = ((size_t)(R.quadW / 32) * kd_piece_bytes(xbd) <= 65535) ? 0 : 4;
        }
    }
    R.exact_tab = G.uniform && K.exact_impl != KirchKnobs::EXACT_PAIR;
    R.xtab_off = caller_tables;
    // Picks that rounding noise decides (kirch_tiescan_kernel): the table-driven kernels would break those ties one way per
    // offset, the reference breaks them pair by pair.  (kirch_gen_kernel needs no list: it re-does every pair on a half-way
    // point in the reference's own arithmetic by itself, kg_ref_upper.)
    R.want_tie_scan = G.uniform && !R.gen && !caller_tables && (mode == IMPDAR_KIRCH_FAST || K.exact_impl != KirchKnobs::EXACT_PAIR);
    return R;
}

// The one step that needs a device result: `count` flagged picks against a list of `cap`.  More ties than the list holds
// (or the correction switched off): the float32 ring kernels stay available when asked for by name; everything the
// library chooses itself goes per pair.
static inline void kirch_route_after_ties(KirchRoute &R, long long count, long long cap)
{
    R.want_tie_groups = count > 0 && count <= cap && !R.tiefix_off;
    R.tie_ambiguous = count > cap || (count > 0 && R.tiefix_off);
    if (!R.tie_ambiguous) return;
    if (R.mode == IMPDAR_KIRCH_FAST && R.requested_mode == IMPDAR_KIRCH_AUTO) {
        R.mode = IMPDAR_KIRCH_EXACT;
        R.quad = false;
        R.xb = 16;
    }
    R.dquad = false;
    R.xtab_off = true;
}

// ---- host tables (the stages of the plan upload them) ------------------------------------------------------------
// aperture half width per sample (uniform grids): largest n with t <= tmax; -1: no pair at all
static inline std::vector<int> kirch_half_widths(const KirchGeometry &G, const double *tt_sec, int snum)
{
    std::vector<int> h(snum);
    const double um = G.tmax / G.dt;
    for (int k = 0; k < snum; ++k) {
        const double a = tt_sec[k] / G.dt;
        const double rem = um * um - a * a;
        h[k] = rem < 0 ? -1 : (int)std::min(std::floor(std::sqrt(rem / G.alpha) + 1e-12), 1073741824.0);
    }
    return h;
}

// Per-sample factors of the ring kernels.
// float32, with a = tt/dt (samples) and rs = half * sqrt(a^2 + alpha n^2):
//   cos(theta)        = a / sqrt(a^2 + alpha n^2) = sign(a) * rsq(1 + c1 n^2),  c1 = alpha / a^2
//   far-field weight  = cos / (2 pi v)            = fin * |cos|,                 fin = sign(a) / (2 pi v)
//   near-field weight = cos / (2 pi rs^2)         = fin * c2 * |cos|^3,          c2 = v / (half a)^2
// a = 0 (a sample at t = 0): cos = 0 for every n != 0 and the apex is 0/0 (dropped) -> fin = 0
// float64, from the reference's own zs = v t / 2 (mig_python.py:101): c1 = (dx / zs)^2, c2 = v / zs^2, fin = sign(zs) / (2 pi v);
// zs = 0: the whole output row is 0
template <typename T>
struct KirchFactors {
    std::vector<T> c1, c2, fin;
};
template <typename T>
static inline KirchFactors<T> kirch_factors(const KirchGeometry &G, const double *tt_sec, int snum, double vel)
{
    constexpr bool dbl = sizeof(T) == 8;
    KirchFactors<T> F{std::vector<T>(snum), std::vector<T>(snum), std::vector<T>(snum)};
    const double half = vel * G.dt / 2.0, big = dbl ? 1e300 : 1e30;         // metres per sample of two-way time
    for (int k = 0; k < snum; ++k) {
        const double a = tt_sec[k] / G.dt, zs = vel * tt_sec[k] / 2.0, s = dbl ? zs : a;
        if (s == 0.0) {
            F.c1[k] = F.c2[k] = F.fin[k] = (T)0;
            continue;
        }
        F.c1[k] = (T)std::min(dbl ? (G.dx / zs) * (G.dx / zs) : G.alpha / (a * a), big);
        F.c2[k] = (T)std::min(dbl ? vel / (zs * zs) : vel / (half * half * a * a), big);
        F.fin[k] = (T)((s > 0 ? 1.0 : -1.0) / (2.0 * M_PI * vel));
    }
    return F;
}

// kirch_gen_kernel: per-sample float32 factors, the squared half-way radii of the float64 re-decision, per-chunk bounds
struct KirchGenTables {
    std::vector<float> a, a2, alo2;
    std::vector<double> zs2min;
};
static inline KirchGenTables kirch_gen_tables(const KirchGeometry &G, const double *tt_sec, int snum, double vel, int genW)
{
    const int nch = (snum + KF_THREADS - 1) / KF_THREADS;
    KirchGenTables T{std::vector<float>(snum), std::vector<float>(snum), std::vector<float>(nch, 3.0e38f), std::vector<double>(nch, 1e300)};
    for (int k = 0; k < snum; ++k) {
        const double ak = tt_sec[k] / G.dt;
        T.a[k] = (float)ak;
        T.a2[k] = (float)(ak * ak / ((double)(genW - 1) * (double)(genW - 1)));    // normalised to the slot (kirch_gen_kernel)
        T.alo2[k / KF_THREADS] = std::min(T.alo2[k / KF_THREADS], (float)(ak * ak) * (1.0f - 1.0e-6f));
        const double zs = vel * tt_sec[k] / 2.0;
        T.zs2min[k / KF_THREADS] = std::min(T.zs2min[k / KF_THREADS], zs * zs);
    }
    return T;
}

// The per-chunk tables of the ring kernels (quad, dquad, tab).
struct KirchRingTables {
    int nchunks = 0, nb = 0, ntab = 0;
    int nrows = 0, mrow0 = 0;   // ring kernels: tables by step block, row r <-> offsets n = S (r - mrow0) + 1 .. + S
    size_t tkbytes = 0;         // the pick table (the kernels address it as one raw buffer: under 2 GiB)
    std::vector<int> hmax;      // aperture half widths per chunk (+ 1)
    std::vector<int> klo, khi;  // staging windows: smallest / largest sample index any lane of chunk c can pick at offset |n|
    std::vector<int> win;       // ... per step block of a ring kernel
};
static inline KirchRingTables kirch_ring_tables(const KirchGeometry &G, const KirchRoute &R, const double *tt_sec, int snum, int tnum,
                                                const std::vector<int> &h_half)
{
    KirchRingTables T;
    const int ringS = R.dquad ? 4 : 8;            // steps per block of the ring kernels (traces per 32-byte row)
    const bool ring = R.quad || R.dquad;
    const int nch = T.nchunks = (snum + KF_THREADS - 1) / KF_THREADS, nb0 = 64;
    T.hmax.assign(nch, 0);
    int hglob = 0;
    std::vector<double> cmin(nch), cmax(nch);
    for (int c = 0; c < nch; ++c) {
        double amin = 1e300, amax = 0;
        for (int k = c * KF_THREADS; k < std::min(snum, (c + 1) * KF_THREADS); ++k) {
            const double a = tt_sec[k] / G.dt;
            amin = std::min(amin, a * a);
            amax = std::max(amax, a * a);
            T.hmax[c] = std::max(T.hmax[c], h_half[k] + 1);
        }
        hglob = std::max(hglob, T.hmax[c]);
        cmin[c] = amin;
        cmax[c] = amax;
    }
    // offsets beyond the profile length can only meet traces outside the profile (zero rows), so the tables need not
    // extend past tnum even when the aperture does
    hglob = std::min(hglob, tnum + 128);
    for (int c = 0; c < nch; ++c) T.hmax[c] = std::min(T.hmax[c], hglob);
    const int nb = T.nb = hglob + nb0;
    T.ntab = hglob + 1;       // offsets 0..hglob-1 (hmax carries a guard) + one all-zero row
    T.mrow0 = hglob / ringS + 8;
    T.nrows = 2 * (hglob / ringS) + 64;
    T.tkbytes = ring ? (size_t)T.nrows * kq_tkb_stride(snum) * 2 * ringS : (size_t)T.ntab * snum * 2;
    if (T.tkbytes >= ((size_t)1 << 31)) return T;
    // (one guard sample each side)
    T.klo.resize((size_t)nch * nb);
    T.khi.resize((size_t)nch * nb);
    const double u0 = tt_sec[0] / G.dt;
    for (int c = 0; c < nch; ++c)
        for (int n = 0; n < nb; ++n) {
            const double bn = G.alpha * (double)n * (double)n;
            const double ulo = std::sqrt(cmin[c] + bn) - u0, uhi = std::sqrt(cmax[c] + bn) - u0;
            T.klo[(size_t)c * nb + n] = std::max(0, (int)std::floor(ulo) - 1);
            T.khi[(size_t)c * nb + n] = std::min(snum - 1, (int)std::ceil(uhi) + 1);
        }
    if (!ring) return T;
    // the S traces block r adds are read by the steps n = S (r - mrow0) + 1 .. + XB + S - 2 (they enter the XB-trace
    // window of a lane at its last slot and leave it XB - 1 steps later)
    T.win.resize((size_t)nch * T.nrows * 2);
    for (int r = 0; r < T.nrows; ++r) {
        // (with nh tiles on one ring the later tiles read the same traces (nh - 1) xb offsets earlier)
        // (the quad-aligned window reads a trace up to 3 steps after the sliding one dropped it)
        const long long nz = (long long)ringS * (r - T.mrow0) + 1 + R.xb + ringS - 2 + (R.window == KIRCH_WINDOW_QUAD ? KQ_WIN_EXTRA : 0);
        const long long na = (long long)ringS * (r - T.mrow0) + 1 - (long long)(R.nh - 1) * R.xb;
        const long long lo = (na <= 0 && nz >= 0) ? 0 : std::min(std::llabs(na), std::llabs(nz));
        const long long hi = std::max(std::llabs(na), std::llabs(nz));
        for (int c = 0; c < nch; ++c) {
            const int kmin = T.klo[(size_t)c * nb + std::min<long long>(lo, nb - 1)];
            const int kmax = T.khi[(size_t)c * nb + std::min<long long>(hi, nb - 1)];
            T.win[((size_t)c * T.nrows + r) * 2 + 0] = kmin | ((kmin % R.quadW) << 16);
            T.win[((size_t)c * T.nrows + r) * 2 + 1] = kmax;
        }
    }
    return T;
}

// The tie list of kirch_tiescan_kernel, (sample, offset) pairs in any order, grouped by sample (sorted: the correction adds
// them in a fixed order): samples g_ti, their ranges g_off[i] .. g_off[i + 1] of the offsets g_n.
struct KirchTie {
    int ti, n;
};
struct KirchTieGroups {
    std::vector<int> g_ti, g_off, g_n;
};
static inline KirchTieGroups kirch_group_ties(std::vector<KirchTie> &list)
{
    std::sort(list.begin(), list.end(), [](const KirchTie &a, const KirchTie &b) { return a.ti < b.ti || (a.ti == b.ti && a.n < b.n); });
    KirchTieGroups T;
    T.g_n.resize(list.size());
    for (size_t i = 0; i < list.size(); ++i) {
        if (i == 0 || list[i].ti != list[i - 1].ti) {
            T.g_ti.push_back(list[i].ti);
            T.g_off.push_back((int)i);
        }
        T.g_n[i] = list[i].n;
    }
    T.g_off.push_back((int)list.size());
    return T;
}

// Which output tile a workgroup of a ring kernel takes: blocks are dealt round-robin over the 8 XCDs (block b -> XCD b & 7),
// so slot q of chunk c on XCD x is block ((c * tiles_per_xcd + q) * 8 + x).  The arithmetic rule (groups of G adjacent tiles
// per XCD in turn) leaves the XCDs up to +-3 % apart in work at config 3: tiles near the ends of the profile walk
// clipped apertures, and which XCD gets them depends on the tile count.  Here the groups of G adjacent tiles (they
// share staging lines in the XCD's L2) are handed out per chunk, longest first, each to the XCD with the least
// accumulated walk so far (steps rounded up to ring revolutions, plus a prologue's worth).  -1 = empty slot.
// An empty map: keep the arithmetic rule.
// (first tile start and tile count of a launch: kirch_tile_origin / kirch_tile_count; `window`: KIRCH_WINDOW_*)
static inline int kirch_tile_origin(int xlo, int tile_w, int align_mask, int window)
{
    return window == KIRCH_WINDOW_QUAD ? (xlo / tile_w) * tile_w : (xlo & ~align_mask);
}
// (the quad-aligned window: the tile right of the block's last column holds part of its last three columns' sums)
static inline int kirch_tile_count(int xlo, int xhi, int tile_w, int align_mask, int window)
{
    return (xhi + (window == KIRCH_WINDOW_QUAD ? KQ_WIN_EXTRA : 0) - kirch_tile_origin(xlo, tile_w, align_mask, window) + tile_w - 1) / tile_w;
}
static inline std::vector<short> kirch_tilemap(const std::vector<int> &h_hmax, int tnum, int xlo, int xhi, int tile_w, int align_mask,
                                               int ring_blocks, int step_block, int G, int tiles_per_xcd, int nchunks,
                                               int window = KIRCH_WINDOW_SLIDE)
{
    const int x00 = kirch_tile_origin(xlo, tile_w, align_mask, window), nxt = kirch_tile_count(xlo, xhi, tile_w, align_mask, window);
    const int wx = window == KIRCH_WINDOW_QUAD ? KQ_WIN_EXTRA : 0;
    const int units = (nxt + G - 1) / G, cap = tiles_per_xcd / G;
    if (nxt > 32767 || units > 8 * cap || (int)h_hmax.size() != nchunks) return {};
    std::vector<short> map((size_t)nchunks * tiles_per_xcd * 8, (short)-1);
    std::vector<double> load(8, 0.0);
    std::vector<std::pair<double, int>> cost(units);
    for (int c = 0; c < nchunks; ++c) {
        const int hm = h_hmax[c];
        for (int u = 0; u < units; ++u) {
            double w = 0;
            for (int t = u * G; t < std::min((u + 1) * G, nxt); ++t) {
                const int x0 = x00 + t * tile_w;
                const int nlo = std::max(-hm, -(x0 + tile_w - 1)), nhi = std::min(hm, tnum - 1 - x0 + wx);
                const int blocks = std::max(0, nhi - nlo + step_block) / step_block;
                w += ((blocks + ring_blocks - 1) / ring_blocks) * ring_blocks + 8;
            }
            cost[u] = {w, u};
        }
        std::sort(cost.begin(), cost.end(), [](const std::pair<double, int> &a, const std::pair<double, int> &b) {
            return a.first > b.first || (a.first == b.first && a.second < b.second);
        });
        int used[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (const auto &cu : cost) {
            int best = -1;
            for (int x = 0; x < 8; ++x)
                if (used[x] < cap && (best < 0 || load[x] < load[best])) best = x;
            for (int g = 0; g < G; ++g) {
                const int t = cu.second * G + g;
                map[((size_t)c * tiles_per_xcd + (size_t)used[best] * G + g) * 8 + best] = (short)(t < nxt ? t : -1);
            }
            ++used[best];
            load[best] += cu.first;
        }
    }
    return map;
}

// The order of the queue lists of a launch of `ntiles` tiles per chunk under route R (the knob's, else packed where the
// launch gets gangs), and its adjacent tiles per gang.  The chunk order keeps the rule the tile map
// always had (groups of 4 from 256 tiles).  The packed order gangs KQ_DEFAULT_GANG tiles where every XCD still gets
// KQ_GANG_MIN_GROUPS gangs of each chunk (config 3: 157 tiles -> 4.9 gangs of 4), else none: with fewer, whole gangs are
// too coarse a unit to balance the XCDs' lists, and stealing moves a gang's tiles off the XCD that shares their lines.
static inline int kirch_queue_order(const KirchRoute &R, int ntiles)
{
    if (R.order != KIRCH_ORDER_AUTO) return R.order;
    return ntiles >= 8 * KQ_DEFAULT_GANG * KQ_GANG_MIN_GROUPS ? KIRCH_ORDER_PACKED : KIRCH_ORDER_CHUNK;
}
static inline int kirch_gang_size(const KirchRoute &R, int ntiles)
{
    if (R.gang) return R.gang;
    if (kirch_queue_order(R, ntiles) == KIRCH_ORDER_CHUNK) return ntiles >= 256 ? 4 : 1;
    return ntiles >= 8 * KQ_DEFAULT_GANG * KQ_GANG_MIN_GROUPS ? KQ_DEFAULT_GANG : 1;
}

// The work lists of the persistent ring kernels: one list of items (chunk << 16 | tile) per XCD, pulled front to back by the
// workgroups running there (kirch_ring_queue_item), then stolen by the others.  The tiles of a chunk form gangs of G
// adjacent tiles; a gang goes whole to one XCD and sits in consecutive positions, so the workgroups that pull it start
// together, walk in phase, and meet each other's pick rows and staged trace groups in that XCD's L2.
// KIRCH_ORDER_CHUNK: the order of kirch_tilemap read slot by slot -- chunk by chunk, longest first inside a chunk.
// KIRCH_ORDER_PACKED: all gangs of all chunks in ONE order, longest first by the tile map's cost model (ties: chunk, then
// tile), each dealt to the XCD with the least accumulated cost.  Costs then never rise along a list, the lists' costs differ
// by at most one gang's, and what the XCDs pull last are the shortest items of the launch (the tail of the chunk order is a
// whole chunk's mix).  No list at all: no queue (more tiles or chunks than an item encodes).
struct __attribute__((visibility("hidden"))) KirchGangMap {
    std::vector<int> list[8];
    size_t items() const
    {
        size_t n = 0;
        for (const auto &l : list) n += l.size();
        return n;
    }
};
static inline KirchGangMap kirch_gangmap(const std::vector<int> &h_hmax, int tnum, int xlo, int xhi, int tile_w, int align_mask, int ring_blocks,
                                         int step_block, int G, int order, int nchunks, int window = KIRCH_WINDOW_SLIDE)
{
    KirchGangMap M;
    const int x00 = kirch_tile_origin(xlo, tile_w, align_mask, window), nxt = kirch_tile_count(xlo, xhi, tile_w, align_mask, window);
    const int wx = window == KIRCH_WINDOW_QUAD ? KQ_WIN_EXTRA : 0;
    if (G < 1 || nxt < 1 || nxt > 32767 || nchunks < 1 || nchunks > 32767 || (int)h_hmax.size() != nchunks) return M;
    const int units = (nxt + G - 1) / G;
    if (order != KIRCH_ORDER_PACKED) {
        const int tpx = ((units + 7) / 8) * G;
        const std::vector<short> map = kirch_tilemap(h_hmax, tnum, xlo, xhi, tile_w, align_mask, ring_blocks, step_block, G, tpx, nchunks, window);
        for (size_t i = 0; i < map.size(); ++i)
            if (map[i] >= 0) M.list[i & 7].push_back((int)((i / 8 / tpx) << 16) | map[i]);
        return M;
    }
    // A gang's tiles run side by side, so it is as long as its longest tile (`len`: the order -- a short gang at the profile's
    // end, or one with clipped apertures, must not wait among the short walks of shallow chunks); its weight `w` on the XCD's
    // list is the sum.
    struct Gang {
        double len, w;
        int c, u;
    };
    std::vector<Gang> gangs;
    gangs.reserve((size_t)nchunks * units);
    for (int c = 0; c < nchunks; ++c) {
        const int hm = h_hmax[c];
        for (int u = 0; u < units; ++u) {
            double w = 0, len = 0;
            for (int t = u * G; t < std::min((u + 1) * G, nxt); ++t) {      // (the cost of a tile as kirch_tilemap counts it)
                const int x0 = x00 + t * tile_w;
                const int nlo = std::max(-hm, -(x0 + tile_w - 1)), nhi = std::min(hm, tnum - 1 - x0 + wx);
                const int blocks = std::max(0, nhi - nlo + step_block) / step_block;
                const double wt = ((blocks + ring_blocks - 1) / ring_blocks) * ring_blocks + 8;
                w += wt;
                len = std::max(len, wt);
            }
            gangs.push_back({len, w, c, u});
        }
    }
    std::sort(gangs.begin(), gangs.end(), [](const Gang &a, const Gang &b) {
        return a.len > b.len || (a.len == b.len && (a.c < b.c || (a.c == b.c && a.u < b.u)));
    });
    double load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (const Gang &g : gangs) {
        int best = 0;
        for (int x = 1; x < 8; ++x)
            if (load[x] < load[best]) best = x;
        for (int t = g.u * G; t < std::min((g.u + 1) * G, nxt); ++t) M.list[best].push_back((g.c << 16) | t);
        load[best] += g.w;
    }
    return M;
}

// How the one-shot entry point (impdar_kirchhoff, kirch_oneshot.hip) takes a large radargram through in pieces.  OUTPUT
// traces in blocks [cut[i], cut[i + 1]), one launch each; block i reads the input traces up to its right edge + the
// aperture half width `halo` only, so its launch starts when input traces [0, need[i]) are on the device and the rest of
// the upload runs under it.  Four blocks [0, .10, .40, .70, 1] tnum when the aperture leaves something to overlap (the
// second block's need stays below 9/10 of the input; sweeps of the cuts: profiles/r03_oneshot_pipeline.txt,
// r05_oneshot_cuts.txt), else -- or with `two`, the round-3 first form kept for A/B -- two (5/8 + 3/8, download overlap
// only; with `two` every block waits for the whole input).  Interior cuts and needs are multiples of 8 (whole image groups).
#ifndef KOS_PCT
#define KOS_PCT {10, 40, 70}
#endif
struct __attribute__((visibility("hidden"))) KirchOneShotCuts {      // (hidden: no weak symbol of it in the library's dynamic table)
    std::vector<int> cut;       // nblk + 1 output cuts, 0 .. tnum
    std::vector<int> need;      // per block: input traces [0, need) its launch reads
};
static inline KirchOneShotCuts kirch_oneshot_cuts(int tnum, int halo, bool two)
{
    auto r8 = [](long long x) { return (int)(x / 8 * 8); };
    KirchOneShotCuts C;
    const std::vector<int> pct = KOS_PCT;              // interior cuts in percent of tnum
    if (!two && (long long)tnum * pct[pct.size() > 1 ? 1 : 0] / 100 + halo < (long long)tnum * 9 / 10) {
        C.cut = {0};
        for (int q : pct) C.cut.push_back(r8((long long)tnum * q / 100));
        C.cut.push_back(tnum);
    } else {
        C.cut = {0, r8((long long)tnum * 5 / 8), tnum};
    }
    for (size_t i = 0; i + 1 < C.cut.size(); ++i)
        C.need.push_back(two ? tnum : (int)std::min<long long>(tnum, ((long long)C.cut[i + 1] + halo + 7) / 8 * 8));
    return C;
}

#ifdef KIRCH_ROUTE_PROBE
// The route and the tables as flat arrays (tests/test_kirch_route.py compiles this header by itself).
// knobs[15]: xb_set, xb, nh_set, nh, lk_set, lk, parts_set, parts, nhd_set, nhd, xbd_set, xbd, impl, exact_impl, tiefix_off.
// tie_count >= 0: kirch_route_after_ties(route, tie_count, tie_cap) is applied.
// ints[32]: status, mode, kernel, tnum_pad, gen, genW, quad, dquad, xb, nh, lk, quadW, quadSH, walk_parts_log2, want_tie_scan, xtab_off,
// tie_ambiguous, want_tie_groups, increasing, uni_t, uni_t11, uni_x, dist_sorted, order, gang (the probe's knobs leave both at their defaults),
// window (KIRCH_WINDOW_* under the probe's window kind, impdar_kirch_window_probe); dbls[16]: tmax, dt, dx, xnoise, sa, alpha, hest,
// gen_need, err_limit, err_sa.
// The window kind of the probe's routes: KirchKnobs::WINDOW_*.  It starts as the sliding window (the tables of a route are
// then what they were before the aligned window existed) until impdar_kirch_window_probe names another.
static inline int *kirch_probe_window()
{
    static int v = KirchKnobs::WINDOW_SLIDE;
    return &v;
}
extern "C" int impdar_kirch_window_probe(int window)
{
    if (window < KirchKnobs::WINDOW_DEFAULT || window > KirchKnobs::WINDOW_QUAD) return -1;
    *kirch_probe_window() = window;
    return 0;
}

static inline KirchKnobs kirch_probe_knobs(const int *k)
{
    KirchKnobs K;
    K.window = *kirch_probe_window();
    K.xb_set = k[0], K.xb = k[1], K.nh_set = k[2], K.nh = k[3], K.lk_set = k[4], K.lk = k[5], K.parts_set = k[6], K.parts = k[7];
    K.nhd_set = k[8], K.nhd = k[9], K.xbd_set = k[10], K.xbd = k[11], K.impl = k[12], K.exact_impl = k[13], K.tiefix_off = k[14];
    return K;
}

extern "C" int impdar_kirch_route_probe(int dtype, int snum, int tnum, const double *dist_m, const double *tt_sec, double vel, int nearfield,
                                        int mode, int nranks, const double *tmax_override, int caller_tables, const int *knobs,
                                        long long tie_count, long long tie_cap, int *ints, double *dbls)
{
    const KirchGeometry G = kirch_geometry(snum, tnum, dist_m, tt_sec, vel, tmax_override);
    KirchRoute R = kirch_route(G, dtype, snum, tnum, nranks, nearfield, mode, kirch_probe_knobs(knobs), caller_tables != 0);
    if (R.status == IMPDAR_OK && tie_count >= 0) kirch_route_after_ties(R, tie_count, tie_cap);
    const int I[23] = {R.status, R.mode, R.status == IMPDAR_OK ? R.kernel() : -1, R.tnum_pad, R.gen, R.genW, R.quad, R.dquad, R.xb, R.nh, R.lk, R.quadW,
                       R.quadSH, R.walk_parts_log2, R.want_tie_scan, R.xtab_off, R.tie_ambiguous, R.want_tie_groups, G.increasing, G.uni_t,
                       G.uni_t11, G.uni_x, G.dist_sorted};
    const double D[10] = {G.tmax, G.dt, G.dx, G.xnoise, G.sa, G.alpha, G.hest, G.gen_need, R.err_limit, R.err_sa};
    std::copy(I, I + 23, ints);
    ints[23] = R.order, ints[24] = R.gang, ints[25] = R.window;
    std::copy(D, D + 10, dbls);
    return 0;
}

// The tables of a plan whose route the probe above reports.  sizes[8]: nchunks, nb, ntab, nrows, mrow0, the pick table refused
// (2 GiB), entries of win, -.  Every output array may be null; h_half / c32 / c64 / gen4 hold snum entries per table (gen4: a,
// a2, then alo2 and zs2min of nchunks entries each go to gen_chunk).
extern "C" int impdar_kirch_tables_probe(int dtype, int snum, int tnum, const double *dist_m, const double *tt_sec, double vel, int nearfield,
                                         int mode, int nranks, const int *knobs, int *sizes, int *h_half, float *c32 /* [3 snum] */,
                                         double *c64 /* [3 snum] */, float *gen2 /* [2 snum] */, double *gen_chunk /* [2 nchunks] */,
                                         int *hmax, int *klo, int *khi, int *win)
{
    const KirchGeometry G = kirch_geometry(snum, tnum, dist_m, tt_sec, vel, nullptr);
    const KirchRoute R = kirch_route(G, dtype, snum, tnum, nranks, nearfield, mode, kirch_probe_knobs(knobs), false);
    if (R.status != IMPDAR_OK || !G.increasing) return -1;
    const std::vector<int> h = G.uniform ? kirch_half_widths(G, tt_sec, snum) : std::vector<int>();
    if (h_half) std::copy(h.begin(), h.end(), h_half);
    auto put3 = [&](const auto &F, auto *dst) {
        std::copy(F.c1.begin(), F.c1.end(), dst);
        std::copy(F.c2.begin(), F.c2.end(), dst + snum);
        std::copy(F.fin.begin(), F.fin.end(), dst + 2 * snum);
    };
    if (c32) put3(kirch_factors<float>(G, tt_sec, snum, vel), c32);
    if (c64) put3(kirch_factors<double>(G, tt_sec, snum, vel), c64);
    if (gen2 && gen_chunk && R.gen) {
        const KirchGenTables T = kirch_gen_tables(G, tt_sec, snum, vel, R.genW);
        std::copy(T.a.begin(), T.a.end(), gen2);
        std::copy(T.a2.begin(), T.a2.end(), gen2 + snum);
        std::copy(T.alo2.begin(), T.alo2.end(), gen_chunk);
        std::copy(T.zs2min.begin(), T.zs2min.end(), gen_chunk + T.alo2.size());
    }
    if (G.uniform && ((R.mode == IMPDAR_KIRCH_FAST && !R.gen) || R.dquad)) {
        const KirchRingTables T = kirch_ring_tables(G, R, tt_sec, snum, tnum, h);
        const int S[8] = {T.nchunks, T.nb, T.ntab, T.nrows, T.mrow0, T.tkbytes >= ((size_t)1 << 31), (int)T.win.size(), 0};
        std::copy(S, S + 8, sizes);
        if (hmax) std::copy(T.hmax.begin(), T.hmax.end(), hmax);
        if (klo) std::copy(T.klo.begin(), T.klo.end(), klo);
        if (khi) std::copy(T.khi.begin(), T.khi.end(), khi);
        if (win) std::copy(T.win.begin(), T.win.end(), win);
    }
    return 0;
}

// ties: n (sample, offset) pairs, sorted in place; returns the number of groups (g_ti[groups], g_off[groups + 1], g_n[n])
extern "C" int impdar_kirch_ties_probe(int *ties, int n, int *g_ti, int *g_off, int *g_n)
{
    std::vector<KirchTie> list(n);
    if (n) memcpy(list.data(), ties, (size_t)n * sizeof(KirchTie));
    const KirchTieGroups T = kirch_group_ties(list);
    std::copy(T.g_ti.begin(), T.g_ti.end(), g_ti);
    std::copy(T.g_off.begin(), T.g_off.end(), g_off);
    std::copy(T.g_n.begin(), T.g_n.end(), g_n);
    return (int)T.g_ti.size();
}

// returns the number of entries of the map (0: the arithmetic rule); map[nchunks * tiles_per_xcd * 8]
extern "C" int impdar_kirch_tilemap_probe(const int *h_hmax, int nchunks, int tnum, int xlo, int xhi, int tile_w, int align_mask, int ring_blocks,
                                          int step_block, int G, int tiles_per_xcd, short *map)
{
    const std::vector<short> m = kirch_tilemap(std::vector<int>(h_hmax, h_hmax + nchunks), tnum, xlo, xhi, tile_w, align_mask, ring_blocks,
                                               step_block, G, tiles_per_xcd, nchunks);
    std::copy(m.begin(), m.end(), map);
    return (int)m.size();
}

// The queue lists of a launch: lens[8], and the lists one behind the other in items[] (at most nchunks * tiles entries);
// returns the number of items (0: no queue).  G = 0 / order = -1: what kirch_gang_size / kirch_queue_order give a route that
// leaves them to the launch.
extern "C" int impdar_kirch_gangmap_probe(const int *h_hmax, int nchunks, int tnum, int xlo, int xhi, int tile_w, int align_mask, int ring_blocks,
                                          int step_block, int G, int order, int *lens, int *items)
{
    KirchRoute R;
    R.order = order;
    R.gang = G;
    const int ntiles = (xhi - (xlo & ~align_mask) + tile_w - 1) / tile_w;
    const KirchGangMap M = kirch_gangmap(std::vector<int>(h_hmax, h_hmax + nchunks), tnum, xlo, xhi, tile_w, align_mask, ring_blocks, step_block,
                                         kirch_gang_size(R, ntiles), kirch_queue_order(R, ntiles), nchunks);
    for (int x = 0; x < 8; ++x) {
        lens[x] = (int)M.list[x].size();
        items = std::copy(M.list[x].begin(), M.list[x].end(), items);
    }
    return (int)M.items();
}

// The cover of a launch of kirch_quad_kernel (far field), step by step as the kernel walks it: every tile of the block
// [xlo, xhi) of a tnum-trace profile, chunk aperture hmax (with its guard), tiles of xb traces, nh per workgroup, lk extra ring
// groups, walks in 1 << parts_log2 pieces, window KIRCH_WINDOW_*.  Per step: the quads read (kq_win_first_quad, or the sliding
// window's run), the accumulator and with it the output each component feeds (kq_win_acc), and the ring group each read slot
// lies in -- which must hold the trace the (output, offset) pair needs, staged by a DMA whose barrier the reading wave has
// passed, and not be re-filled while the read is in flight (the model of the ring: groups staged in the prologue, block k's by
// the DMA issued behind the barrier of block k - 2 - lk and landed by the barrier of block k - 1).
//   count[(xhi - xlo) * (2 hmax + 1)]: how many (tile, step, accumulator) take the pair (output x, offset n), |n| <= hmax
//   written[xhi - xlo]: how often the column is written -- by a tile's whole columns, or by the fix-up of a tile start
//   stats[8]: tiles, steps, quad reads, components that feed no accumulator, reads off a staged group (must be 0), components
//             whose slot holds another trace than their pair's (must be 0), largest accumulator index, tile starts fixed up
// Returns 0, or -1 for arguments the kernel has no instantiation for.
extern "C" int impdar_kirch_quadwin_cover_probe(int tnum, int xlo, int xhi, int xb, int nh, int lk, int hmax, int parts_log2, int window,
                                                int *count, int *written, long long *stats)
{
    if (!(xb == 24 || xb == 32 || xb == 40) || nh < 1 || nh > 3 || lk < 0 || lk > 1 || parts_log2 < 0 || parts_log2 > 2 || hmax < 0 ||
        tnum < 1 || xlo < 0 || xhi <= xlo || xhi > tnum || (parts_log2 && nh != 1))
        return -1;
    const int S = 8, RG = kq_ring_slots(xb) + 8 * lk, NB = RG / S, NQ = RG / 4, G0 = xb / 8, TW = xb * nh;
    const int wx = window == KIRCH_WINDOW_QUAD ? KQ_WIN_EXTRA : 0;
    const int x00 = kirch_tile_origin(xlo, TW, 7, window), nxt = kirch_tile_count(xlo, xhi, TW, 7, window);
    const long long span = 2LL * hmax + 1;
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    for (int part = 0; part < (1 << parts_log2); ++part)
        for (int xt = 0; xt < nxt; ++xt) {
            const int x0w = x00 + xt * TW;
            int nlo, nhi;
            if (kirch_walk_range(hmax, x0w, tnum, S, NB, xb, nh, parts_log2, part, wx, nlo, nhi)) continue;
            ++stats[0];
            const int nblocks = (nhi - nlo + 1 + S - 1) / S, nrev = (nblocks + NB - 1) / NB;
            // ring group -> image group (relative to the group of trace jbase - 1) it holds, and the barriers a reader must have passed
            std::vector<long long> holds(NB, -1), ready(NB, 0);
            auto dma = [&](int blk_for) {
                const int g = ((blk_for + G0) % NB + NB) % NB;
                holds[g] = blk_for + G0;
                ready[g] = std::max(blk_for, 0);
            };
            for (int pb = -G0; pb <= 0; ++pb) dma(pb);
            for (int j = 0; j <= lk; ++j) dma(1 + j);
            // one step's reads; `check_only`: the reads are in flight while the ring changes -- they must still find their traces
            auto step = [&](long long p, bool check_only) {
                const int pm = (int)(p % RG), blk = (int)(p / S);
                for (int h = 0; h < nh; ++h) {
                    const int x0 = x0w + h * xb, n = nlo - h * xb + (int)p;
                    for (int qd = 0; qd < NQ; ++qd) {
                        const int t = (qd - kq_win_first_quad(pm, NQ) + NQ) % NQ;
                        bool any = false;
                        int acc[4];
                        for (int c = 0; c < 4; ++c) {
                            if (window == KIRCH_WINDOW_QUAD) {
                                acc[c] = t < xb / 4 ? kq_win_acc(pm, t, c) : -1;
                            } else {
                                const int i = (4 * qd + c - pm - 1 + 2 * RG) % RG;       // fma_step's i0 .. i3
                                acc[c] = i < xb ? i + 3 : -1;                            // (numbered like the aligned window's)
                            }
                            any = any || acc[c] >= 0;
                        }
                        if (!any) continue;
                        if (!check_only && h == 0) ++stats[2];
                        for (int c = 0; c < 4; ++c) {
                            if (acc[c] < 0) {
                                if (!check_only && h == 0) ++stats[3];
                                continue;
                            }
                            const int x = x0 - 3 + acc[c];
                            // the relative trace the pair (x, n) needs, and the one ring slot 4 qd + c stands for at this step
                            const long long q = (long long)x + n - (x0w + nlo);
                            if (((q + 1) % RG + RG) % RG != 4 * qd + c) {
                                ++stats[5];
                                continue;
                            }
                            const int g = (4 * qd + c) / 8;
                            if (q + 1 < 0 || holds[g] != (q + 1) / 8 || ready[g] > blk) ++stats[4];
                            if (check_only) continue;
                            stats[6] = std::max<long long>(stats[6], acc[c]);
                            if (blk < nblocks && x >= xlo && x < xhi && n >= -hmax && n <= hmax) ++count[(x - xlo) * span + n + hmax];
                        }
                    }
                }
            };
            step(0, false);
            for (int blk = 0; blk < nrev * NB; ++blk) {
                for (int s = 1; s < S; ++s) step((long long)blk * S + s, false);      // issued in front of the block's barrier
                dma(blk + 2 + lk);                                                    // behind it
                step((long long)blk * S + 7, true);                                   // step 7's reads cross the barrier
                if (blk + 1 < nrev * NB) step((long long)(blk + 1) * S, false);
            }
            stats[1] += (long long)nrev * NB * S;
            for (int h = 0; h < nh; ++h) {
                const int x0 = x0w + h * xb;
                for (int i = 0; i < xb - wx; ++i)      // (the aligned window: the last three are the next tile start's)
                    if (x0 + i >= xlo && x0 + i < xhi) ++written[x0 + i - xlo];
            }
        }
    if (wx)
        for (int b = 1; b < nxt * nh; ++b) {
            ++stats[7];
            for (int c = 0; c < 3; ++c) {
                const int x = x00 + b * xb - 3 + c;
                if (x >= xlo && x < xhi) written[x - xlo] += 1 << parts_log2;
            }
        }
    return 0;
}

// returns the number of blocks; cut[blocks + 1], need[blocks] (at most 8 blocks)
extern "C" int impdar_kirch_oneshot_cuts_probe(int tnum, int halo, int two, int *cut, int *need)
{
    const KirchOneShotCuts C = kirch_oneshot_cuts(tnum, halo, two != 0);
    std::copy(C.cut.begin(), C.cut.end(), cut);
    std::copy(C.need.begin(), C.need.end(), need);
    return (int)C.need.size();
}
#endif
