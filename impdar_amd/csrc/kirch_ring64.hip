// The float64 LDS-ring kernel of the Kirchhoff migration (uniform grids), its pick table and its launches.  What it shares
// with the float32 ring (kirch_ring32.hip; the LDS image is described at kirch_quad_kernel there) is kirch_ring.h;
// kirch_launch_ring64 and kirch_table_ring64 at the end are what kirchhoff.hip calls.
#include "kirch_ring.h"

// ---------------------------------------------------------------------------
// dquad kernel: the quad kernel's ring in float64 -- the float64 parity path on uniform grids (what
// RadarData.migrate('kirch') runs on a float64 radargram, mig_python.py:35-60,118).
//
// Same LDS image byte for byte (a ring row is 32 bytes: here 4 traces x 8 bytes, so the image is kept in groups
// of FOUR traces and a step block is 4 steps), same LDS-DMA staging, same fp64 pick table (the reference's
// picks, t > t_max test and 0/0 skip, kirch_tabled_kernel below); a ds_read_b128 now carries the samples of two
// traces.  What differs from the float32 kernel:
//   * XB = 20 (or 16) outputs per lane in float64 accumulators (XB/2 register quads, as many as the 40 floats);
//   * the obliquity factor cos(theta) = zs/rs = rsqrt(1 + (n dx / zs)^2) is evaluated in float64 per (lane,
//     step): a float32 v_rsq seed and ONE third-order correction y0 (1 + r/2 + 3 r^2/8), r = 1 - x y0^2, which
//     leaves < 1e-20 of truncation on top of float64 rounding -- far inside the 1e-12 bar, without the 113 MB
//     float64 weight table of kirch_exact_tab_kernel or an IEEE sqrt + divide per step;
//   * the factor sign(zs)/(2 pi v) is applied once at the end, in float64 (the near-field weight cos/rs^2 is
//     carried in those units: y^3 v / zs^2);
//   * non-finite input: only NaNs are zeroed by prep (they are what nansum drops, :53,:58); infinities travel
//     through the sum as in the reference.  Rows with zs = 0 are written as exact zeros (:60 with cos = 0).
// The kernel is bound by the float64 vector rate (20 v_fma_f64 + ~10 for the weight per lane and step against
// 11 ds_read_b128), not by the LDS port.
// ---------------------------------------------------------------------------
// picks for the dquad kernel: rows of FOUR offsets, n = 4 (r - mrow0) + 1 + s, 16 bits each (see kirch_tableq_kernel)
__global__ __launch_bounds__(256) void kirch_tabled_kernel(TableQParams P)
{
    const int ti = blockIdx.x * 256 + threadIdx.x;
    const int a = blockIdx.y;
    if (ti >= P.snum) return;
    const unsigned zero_row = 1024u >> P.sh;         // KQ_ZERO
    unsigned pk[5];
    bool out = false;
    const double zs = P.zs[ti], zs2 = P.zs2[ti];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int n = 4 * a + s;
        unsigned kb = zero_row;
        if (n < P.nmax && !out) {
            const double dx = (double)n * P.dx;
            const double q = dx * dx + zs2;                       // mig_python.py:44
            const double rs = sqrt(q);
            const double cost = zs / rs;                          // :47
            const double t = 2.0 * rs / P.vel;                    // :49
            if (t > P.tmax) {                                     // :52
                out = true;
            } else if (cost == cost) {
                const int ns = P.snum;
                int k0 = (int)floor((t - P.tt0) * P.inv_dt);
                k0 = min(max(k0, 0), ns - 1);
                while (k0 < ns - 1 && P.tt[k0 + 1] <= t) ++k0;
                while (k0 > 0 && P.tt[k0] > t) --k0;
                const int k1 = min(k0 + 1, ns - 1);
                const int k = (fabs(P.tt[k1] - t) < fabs(P.tt[k0] - t)) ? k1 : k0;
                kb = kq_row_offset(k % P.wmod, P.ps) >> P.sh;
            }
        }
        pk[s] = kb;
    }
    uint2 *T = reinterpret_cast<uint2 *>(P.TKB);
    const int rp = a + P.mrow0, rn = P.mrow0 - a - 1;
    if (rp < P.nrows) T[(size_t)rp * kq_tkb_stride(P.snum) + ti] = make_uint2(pk[1] | (pk[2] << 16), pk[3] | (pk[4] << 16));
    if (rn >= 0) T[(size_t)rn * kq_tkb_stride(P.snum) + ti] = make_uint2(pk[3] | (pk[2] << 16), pk[1] | (pk[0] << 16));
}

template <int XB, bool NEAR, int OCC, int SH, int NH>
__global__ __launch_bounds__(KF_THREADS * NH, OCC) void kirch_dquad_kernel(FastParams P, int W)
{   // NH tiles of XB traces per workgroup on one ring, tile h walking h XB offsets behind tile 0 (as kirch_quad_kernel does)
    constexpr int S = 4;
    constexpr int RG = kd_ring_slots(XB);     // ring slots (traces)
    constexpr int KQ_PS = kd_piece_bytes(XB);
    constexpr int G0 = XB / 4;                // a block's new traces belong to image / ring group blk + G0
    constexpr int KQ_PARTS = (XB / 2 + 1 + KQ_PER - 1) / KQ_PER;   // interleave slices per step
    constexpr int NB = RG / S;                // step blocks per ring revolution (unroll length)
    constexpr int NQ = RG / 2;                // 16-byte slot pairs
    static_assert(XB + 2 * S - 1 <= RG && RG % S == 0 && XB % 4 == 0, "ring too small");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int npieces = W >> 5;
    const unsigned img_bytes = (unsigned)npieces * KQ_PS;

    const int tid = threadIdx.x & (KF_THREADS - 1);
    const int half = NH > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 8) : 0;
    // persistent workgroups pull (chunk, tile) items from per-XCD queues until none is left: kirch_ring_queue_item
    bool first_item = true;
    int *item_slot = reinterpret_cast<int *>(lds) + (size_t)(img_bytes / 4) * (NEAR ? 2 : 1);
    for (;;) {
    int chunk, xt;
    int part = 0;            // which piece of the tile's aperture walk this item is (plans of 4+ ranks: kirch_ring_walk)
    if (P.queue) {
        const int it = kirch_ring_queue_item(P, item_slot, part);
        if (it < 0) break;
        chunk = it >> 16;
        xt = it & 0xffff;
    } else if (!kirch_ring_block_item(P, chunk, xt)) {
        return;
    }
    const int s0 = chunk * KF_THREADS;
    const int x0w = (P.xlo & ~3) + xt * (XB * NH);   // workgroup tiles start at a multiple of 4 (outputs left of xlo are not stored)
    const int x0 = x0w + half * XB;
    const int snum = P.snum;
    const int lane = tid & 63;
    const int sigma = kirch_ring_sigma(lane);        // the 16 lanes a ds_read_b128 services together hold 16 consecutive samples
    const int ti_raw = s0 + (tid & ~63) + sigma;
    const int ti = min(ti_raw, snum - 1);

    const int hmax = P.hmax[chunk];
    int nlo, nhi;                                // tile 0's offsets: the ring clock; x0w + nlo = 1 mod 4
    if (kirch_ring_walk<S, NB, XB, NH>(P, hmax, x0w, part, nlo, nhi)) continue;      // uniform; the partial images are zeroed before the launch
    const int nsteps = nhi - nlo + 1;
    const int nblocks = (nsteps + S - 1) / S;
    const int nrev = (nblocks + NB - 1) / NB;
    const int jbase = x0w + nlo;
    const int mrow = ((nlo - 1) >> 2) + P.mrow0;
    auto row_of = [&](int blk) { return min(mrow + blk, P.nrows - 1); };
    const int mrow_h = mrow - half * (XB / 4);   // this tile's pick rows: half * XB offsets behind the clock
    auto prow_of = [&](int blk) { return blk >= nblocks ? P.nrows - 1 : max(min(mrow_h + blk, P.nrows - 1), 0); };

    const int2 *WIN = P.WIN + (size_t)chunk * P.nrows;
    auto fetch_for = [&](int blk_for, int &a, int &b) {
        const int2 w = WIN[max(row_of(blk_for), 0)];
        a = w.x;
        b = w.y;
    };
    const unsigned grp_bytes = (unsigned)snum * 32u;
    const kq_u4 gdesc = kirch_ring_desc(reinterpret_cast<const double *>(P.GT), jbase, snum);
    const kq_u4 ddesc = kirch_ring_desc(reinterpret_cast<const double *>(NEAR ? P.DT : P.GT), jbase, snum);
    const __amdgpu_buffer_rsrc_t tkres =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(P.TKB), 0, 0x7fffffff, 0x00020000);
    const unsigned tioff = (unsigned)ti * 8u;
    const unsigned rowbytes = (unsigned)kq_tkb_stride(snum) * 8u;
    typedef unsigned kd_u2 __attribute__((ext_vector_type(2)));
    auto picks = [&](int blk) -> kd_u2 {
        return __builtin_amdgcn_raw_buffer_load_b64(tkres, tioff, (unsigned)prow_of(blk) * rowbytes, 0);
    };
#define KD_TK(q, s) (((q)[(s) >> 1] >> (16 * ((s) & 1))) & 0xffffu)
    const double c1 = P.c1d[ti], c2 = NEAR ? P.c2d[ti] : 0.0, fin = P.find[ti];
    const int nlo_h = nlo - half * XB;
    auto n2_of = [&](int step) {
        const int n = nlo_h + step;
        return (double)((unsigned)n * (unsigned)n);
    };
    // cos(theta) = rsqrt(1 + c1 n^2) in float64: float32 seed + one third-order correction (see the header)
    auto cosine = [&](double n2) {
        const double x = fma(c1, n2, 1.0);
        const double y0 = (double)__builtin_amdgcn_rsqf((float)x);
        const double h = x * y0;
        const double rr = fma(-h, y0, 1.0);
        const double pp = fma(rr, 0.375, 0.5) * rr;
        return fma(y0, pp, y0);
    };

    if (first_item) {
        if ((unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)lds != 0u) __builtin_trap();
        for (int e = threadIdx.x; e < (int)(img_bytes / 4) * (NEAR ? 2 : 1); e += KF_THREADS * NH) lds[e] = 0.f;
        __syncthreads();
        first_item = false;
    }
    kd_u2 tkc = picks(0);

    kd_d2 acc2[XB / 2];
#pragma unroll
    for (int i = 0; i < XB / 2; ++i) acc2[i] = kd_d2{0.0, 0.0};
#define KD_ACC(i) acc2[(i) >> 1][(i) & 1]

    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rl = lane >> 1;
    const unsigned hsel = ((unsigned)(lane & 1) ^ ((unsigned)(rl >> 3) & 1u)) * 16u;
    auto dma_issue = [&](int blk_for, int wa) {     // the 4 traces that block `blk_for` adds to the ring
        const int kmin = wa & 0xffff, kmod = (int)((unsigned)wa >> 16);
        const int gidx = ((blk_for + G0) % NB + NB) % NB;
        const unsigned so = (unsigned)(blk_for + G0) * grp_bytes;
        for (int pc = wv; pc < npieces; pc += 4 * NH) {
            int t = pc * 32 + rl - kmod;
            t += (t < 0) ? W : 0;
            const int c = min(kmin + t, snum - 1);
            const unsigned vo = (unsigned)c * 32u + hsel;
            kirch_ring_dma16((unsigned)(pc * KQ_PS + gidx * KQ_GS), vo, gdesc, so);
            if (NEAR) kirch_ring_dma16(img_bytes + (unsigned)(pc * KQ_PS + gidx * KQ_GS), vo, ddesc, so);
        }
    };
    int wa, wb, wn = 0;
    for (int pb = -G0; pb <= 0; ++pb) {
        fetch_for(pb, wa, wb);
        dma_issue(pb, wa);
    }
    fetch_for(1, wa, wb);
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
    __syncthreads();
    dma_issue(1, wa);
    fetch_for(2, wa, wb);

    kq_f4 va[NQ], vb[NQ], ua[NEAR ? NQ : 1], ub[NEAR ? NQ : 1];
    auto needed = [](int pm, int qd) {
        bool any = false;
        for (int c = 0; c < 2; ++c) any = any || ((2 * qd + c - pm - 1 + 2 * RG) % RG) < XB;
        return any;
    };
    auto run_pos = [](int pm, int qd) { return (qd - ((pm + 1) % RG) / 2 + NQ) % NQ; };
    auto load_step = [&](int pm, unsigned tk, kq_f4 (&v)[NQ], kq_f4 (&u)[NEAR ? NQ : 1], int part) {
        typedef const __attribute__((address_space(3))) kq_f4 *lds_f4p;
        const unsigned a0 = tk << SH, a1 = a0 ^ 16u;
#pragma unroll
        for (int qd = 0; qd < NQ; ++qd)
            if (needed(pm, qd) && (part < 0 || run_pos(pm, qd) / KQ_PER == part)) {
                const unsigned src = ((qd & 1) ? a1 : a0) + (qd >> 1) * KQ_GS;
                v[qd] = *(lds_f4p)(uintptr_t)src;
                if (NEAR) u[qd] = *(lds_f4p)(uintptr_t)(src + img_bytes);
            }
    };
    auto fma_step = [&](int pm, double w, double w2, const kq_f4 (&v)[NQ], const kq_f4 (&u)[NEAR ? NQ : 1], int part) {
#pragma unroll
        for (int qd = 0; qd < NQ; ++qd) {
            if (part >= 0 && run_pos(pm, qd) / KQ_PER != part) continue;
            const int i0 = (2 * qd + 0 - pm - 1 + 2 * RG) % RG;
            const int i1 = (2 * qd + 1 - pm - 1 + 2 * RG) % RG;
            if (i0 < XB || i1 < XB) {
                const kd_d2 dv = __builtin_bit_cast(kd_d2, v[qd]);
                const kd_d2 du = __builtin_bit_cast(kd_d2, u[NEAR ? qd : 0]);
#define KD_FMA(a, b, c_) fma(a, b, c_)
#define KD_COMP(ix, c)                                                              \
    if (ix < XB) {                                                                  \
        KD_ACC(ix < XB ? ix : 0) = KD_FMA(w, dv[c], KD_ACC(ix < XB ? ix : 0));         \
        if (NEAR) KD_ACC(ix < XB ? ix : 0) = fma(w2, du[c], KD_ACC(ix < XB ? ix : 0)); \
    } else {                                                                        \
        asm volatile("" ::"v"(dv[c]));                                              \
        if (NEAR) asm volatile("" ::"v"(du[c]));                                    \
    }
                KD_COMP(i0, 0)
                KD_COMP(i1, 1)
#undef KD_COMP
            }
        }
    };
#define KD_PIN()                                                                                          \
    do {                                                                                                  \
        static_assert(XB == 16 || XB == 20, "KD_PIN lists XB/2 accumulator pairs");                       \
        if (XB == 16)                                                                                     \
            asm volatile("" : "+v"(acc2[0]), "+v"(acc2[1]), "+v"(acc2[2]), "+v"(acc2[3]), "+v"(acc2[4]), \
                              "+v"(acc2[5]), "+v"(acc2[6]), "+v"(acc2[7]) :: "memory");                   \
        else                                                                                              \
            asm volatile("" : "+v"(acc2[0]), "+v"(acc2[1]), "+v"(acc2[2]), "+v"(acc2[3]), "+v"(acc2[4]), \
                              "+v"(acc2[5]), "+v"(acc2[6]), "+v"(acc2[7]), "+v"(acc2[XB >= 20 ? 8 : 0]),  \
                              "+v"(acc2[XB >= 20 ? 9 : 0]) :: "memory");                                  \
    } while (0)

    double n2c[S];
#pragma unroll
    for (int s = 0; s < S; ++s) n2c[s] = n2_of(s);
    load_step(0, KD_TK(tkc, 0), va, ua, -1);
    for (int rev = 0; rev < nrev; ++rev) {
#pragma clang loop unroll(full)
        for (int bb = 0; bb < NB; ++bb) {
            const int blk = rev * NB + bb;
            const int pm0 = bb * S;
            const kd_u2 tkn = picks(blk + 1);
            fetch_for(blk + 3, wn, wb);
            double twc[S], tw2c[NEAR ? S : 1];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double y = cosine(n2c[s]);
                twc[s] = y;
                if (NEAR) tw2c[s] = (y * c2) * (y * y);        // near-field weight in units of fin: c2 = v / zs^2
            }
#pragma unroll
            for (int s = 0; s < S; ++s) n2c[s] = n2_of((blk + 1) * S + s);
#define KD_W2(s) (NEAR ? tw2c[NEAR ? (s) : 0] : 0.0)
#define KD_UNPACK(...) __VA_ARGS__
#define KD_STEP(L, F)                                                                          \
    do {                                                                                       \
        _Pragma("unroll") for (int part = 0; part < KQ_PARTS; ++part) {                      \
            load_step(KD_UNPACK L, part); KD_PIN();                                            \
            fma_step(KD_UNPACK F, part); KD_PIN();                                             \
        }                                                                                      \
    } while (0)
            KD_STEP((pm0 + 1, KD_TK(tkc, 1), vb, ub), (pm0 + 0, twc[0], KD_W2(0), va, ua));
            KD_STEP((pm0 + 2, KD_TK(tkc, 2), va, ua), (pm0 + 1, twc[1], KD_W2(1), vb, ub));
            KD_STEP((pm0 + 3, KD_TK(tkc, 3), vb, ub), (pm0 + 2, twc[2], KD_W2(2), va, ua));
            // barrier after step S - 2: the ring group the next DMA overwrites was last read there
            __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0)
            asm volatile("s_barrier" ::: "memory");
            dma_issue(blk + 2, wa);
            wa = wn;
            KD_STEP(((pm0 + 4) % RG, KD_TK(tkn, 0), va, ua), (pm0 + 3, twc[3], KD_W2(3), vb, ub));
#undef KD_W2
#undef KD_STEP
#undef KD_UNPACK
            tkc = tkn;
        }
    }
#undef KD_PIN
#undef KD_TK
    asm volatile("" ::"v"(va[0].x), "v"(va[NQ - 1].w));
    __builtin_amdgcn_s_waitcnt(0x0F70);

    if (ti_raw < snum) {
        double *o = (P.parts_log2 ? reinterpret_cast<double *>(P.partial) + (size_t)part * P.part_stride
                                  : reinterpret_cast<double *>(P.out)) + (size_t)ti_raw * P.ldo + (x0 - P.xlo);
#pragma unroll
        for (int i = 0; i < XB; ++i)
            if (x0 + i >= P.xlo && x0 + i < P.xhi) o[i] = (fin == 0.0) ? 0.0 : KD_ACC(i) * fin;
    }
#undef KD_ACC
    if (!P.queue) break;
    }   // item loop
}

// ===========================================================================
// host side
// ===========================================================================
// a kirch_dquad_kernel instantiation as launch_ring (kirch_ring.h) takes it
template <int XB_, int SH, int NH_ = 1>
struct RingF64 {
    typedef double elem;
    static constexpr int XB = XB_, NH = NH_, window = KIRCH_WINDOW_SLIDE;
    static constexpr int align_mask = 3, step_block = 4, ring_blocks = kd_ring_slots(XB) / 4, piece_bytes = kd_piece_bytes(XB);
    static auto near_kernel() { return kirch_dquad_kernel<XB, true, 1, SH, 1>; }
    static auto far_kernel() { return kirch_dquad_kernel<XB, false, (NH > 1 ? 4 : 2), SH, NH>; }
};

// the diffraction sum in the instantiation of the plan's tile width, tiles per workgroup and table shift
int kirch_launch_ring64(impdar_kirch_plan *p, void *d_out, int xlo, int xhi, hipStream_t st)
{
    const FastParams P = kirch_ring_params(p, d_out, xlo, xhi);
    if (p->nh == 2 && p->quadSH == 4)
        return p->xb == 20 ? launch_ring<RingF64<20, 4, 2>>(p, P, st) : launch_ring<RingF64<16, 4, 2>>(p, P, st);
    return p->quadSH == 0 ? (p->xb == 20 ? launch_ring<RingF64<20, 0>>(p, P, st) : launch_ring<RingF64<16, 0>>(p, P, st))
                          : (p->xb == 20 ? launch_ring<RingF64<20, 4>>(p, P, st) : launch_ring<RingF64<16, 4>>(p, P, st));
}

int kirch_table_ring64(impdar_kirch_plan *p, int b, hipStream_t st)
{
    return prep_table_ring(p, b, st, kirch_tabled_kernel, kd_piece_bytes(p->xb));
}
