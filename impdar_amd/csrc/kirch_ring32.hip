// The float32 LDS-ring kernels of the Kirchhoff migration (uniform grids) and their launches:
//   kirch_tableq_kernel  fp64 pick per (sample, trace offset) in the reference's operation order, stored by step
//                        block as the LDS offset of the picked row.
//   kirch_quad_kernel    the MI355X hot path.  A workgroup owns 256 output samples x 24-40 output traces; input
//                        traces stream by LDS-DMA through an LDS ring read with ds_read_b128; picks come from the table.
//   kirch_fixup_kernel   the columns two tiles of kirch_quad_kernel share under its quad-aligned window.
//   kirch_table_kernel / kirch_tab_kernel
//                        same idea with a trace-major ring, ds_read_b32 and an fp32 weight table, for geometries
//                        whose moveout does not fit the quad ring.
// What they share with the float64 ring (kirch_ring64.hip) is kirch_ring.h; kirch_launch_ring32 and kirch_table_ring32 at
// the end are what kirchhoff.hip calls.
#include "kirch_ring.h"

// pick / weight table of kirch_tab_kernel (TableParams, kirch_ring.h)
__global__ __launch_bounds__(256) void kirch_table_kernel(TableParams P)
{
    const int ti = blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (ti >= P.snum) return;
    const size_t o = (size_t)n * P.snum + ti;
    unsigned short kb = P.sentinel;      // pair dropped by the reference
    float w = 0.f, w2 = 0.f;
    if (n < P.ntab - 1) {
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
            const int k = (fabs(P.tt[k1] - t) < fabs(P.tt[k0] - t)) ? k1 : k0;
            kb = (unsigned short)((k % P.wmod) * P.kscale);
            const double c2pi = 1.0 / (2.0 * 3.141592653589793);
            w = (float)(c2pi * (cost / P.vel));
            if (P.near) w2 = (float)(c2pi * (cost / (rs * rs)));
        }
    }
    P.TK[o] = kb;
    if (P.write_w) {
        P.TW[o] = w;
        if (P.near) P.TW2[o] = w2;
    }
}

__global__ __launch_bounds__(256) void kirch_tableq_kernel(TableQParams P)
{
    // One thread evaluates the 9 picks |n| = 8a .. 8a+8 of one sample and fills TWO rows with them: the
    // block right of the apex n = 8a+1 .. 8a+8 (row a + mrow0) and its mirror n = -8a-7 .. -8a
    // (row mrow0 - a - 1, picks in reverse order): 9 evaluations instead of 16.  A pick beyond the
    // sample's own aperture (t > t_max) is the all-zero row; so is everything once t exceeded t_max
    // (t grows with |n|), which skips the fp64 work for the outer part of the table.
    const int ti = blockIdx.x * 256 + threadIdx.x;
    const int a = blockIdx.y;
    if (ti >= P.snum) return;
    const unsigned zero_row = 1024u >> P.sh;         // KQ_ZERO
    unsigned pk[9];
    bool out = false;                                // t already beyond t_max at a smaller offset
    const double zs = P.zs[ti], zs2 = P.zs2[ti];
#pragma unroll
    for (int s = 0; s < 9; ++s) {
        const int n = 8 * a + s;
        unsigned kb = zero_row;
        if (n < P.nmax && !out) {
            const double dx = (double)n * P.dx;
            const double q = dx * dx + zs2;
            const double rs = sqrt(q);
            const double cost = zs / rs;
            const double t = 2.0 * rs / P.vel;
            if (t > P.tmax) {
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
    const int rp = a + P.mrow0, rn = P.mrow0 - a - 1;
    if (rp < P.nrows)
        P.TKB[(size_t)rp * kq_tkb_stride(P.snum) + ti] =
            make_uint4(pk[1] | (pk[2] << 16), pk[3] | (pk[4] << 16), pk[5] | (pk[6] << 16), pk[7] | (pk[8] << 16));
    if (rn >= 0)
        P.TKB[(size_t)rn * kq_tkb_stride(P.snum) + ti] =
            make_uint4(pk[7] | (pk[6] << 16), pk[5] | (pk[4] << 16), pk[3] | (pk[2] << 16), pk[1] | (pk[0] << 16));
}

// ---------------------------------------------------------------------------
// table-driven ring kernel, trace-major LDS layout: a 256-sample x XB-trace tile walks the
// trace offset n; the XB+8 input traces in use sit in an LDS ring of 512-sample circular
// slots, the per-(sample, offset) pick and weight come from the table (two coalesced loads
// per lane per step, prefetched a block ahead), one conflict-free ds_read_b32 + FMA per pair.
// ---------------------------------------------------------------------------
template <int XB, int S, bool NEAR, int OCC>
__global__ __launch_bounds__(KF_THREADS, OCC) void kirch_tab_kernel(FastParams P)
{
    constexpr int R = XB + 2 * S;
    constexpr int W = KF_W;
    static_assert(R % S == 0, "ring must be a whole number of step blocks");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *ldsG = lds;
    float *ldsD = lds + R * W;

    const int b = blockIdx.x;
    const int xcd = b & 7, r = b >> 3;
    const int chunk = r / P.tiles_per_xcd;
    const int qx = r - chunk * P.tiles_per_xcd;
    const int xt = ((qx / P.G) * 8 + xcd) * P.G + (qx % P.G);
    if (chunk >= P.nchunks || xt >= P.nxt) return;

    const int tid = threadIdx.x;
    const int s0 = chunk * KF_THREADS;
    const int x0 = P.xlo + xt * XB;
    const int snum = P.snum, tnum = P.tnum;
    const int ti_raw = s0 + tid;
    const int ti = min(ti_raw, snum - 1);

    const int hmax = P.hmax[chunk];
    const int *klo = P.klo + (size_t)chunk * P.nb;
    const int *khi = P.khi + (size_t)chunk * P.nb;
    const int nlo = max(-hmax, -(x0 + XB - 1));
    const int nhi = min(hmax, tnum - 1 - x0);
    const int nsteps = nhi - nlo + 1;
    const int nblocks = (nsteps + S - 1) / S;
    const int nsteps_pad = nblocks * S;
    const int jbase = x0 + nlo;
    const int ntab1 = P.ntab - 1;

    auto window = [&](int q, int &kmin, int &kmax) {
        const int pmin = max(0, q - (XB - 1)), pmax = min(q, nsteps_pad - 1);
        const int na = nlo + pmin, nb = nlo + pmax;
        const int lo = (na <= 0 && nb >= 0) ? 0 : min(abs(na), abs(nb));
        const int hi = max(abs(na), abs(nb));
        kmin = klo[min(lo, P.nb - 1)];
        kmax = min(khi[min(hi, P.nb - 1)], kmin + W - 1);
    };

    for (int e = tid; e < R * W * (NEAR ? 2 : 1); e += KF_THREADS) lds[e] = 0.f;
    __syncthreads();
    for (int q = 0; q < XB + S - 1; ++q) {
        int kmin, kmax;
        window(q, kmin, kmax);
        const int j = jbase + q;
        const int jr = (j >= 0 && j < tnum) ? j : P.zero_row;
        const int slot = q % R;
        for (int e = kmin + tid; e <= kmax; e += KF_THREADS) {
            ldsG[slot * W + (e & (W - 1))] = P.GT[(size_t)jr * snum + e];
            if (NEAR) ldsD[slot * W + (e & (W - 1))] = P.DT[(size_t)jr * snum + e];
        }
    }
    // table entries of block 0
    unsigned short tkc[S];
    float twc[S], tw2c[NEAR ? S : 1];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const size_t o = (size_t)min(abs(nlo + s), ntab1) * snum + ti;
        tkc[s] = P.TK[o];
        twc[s] = P.TW[o];
        if (NEAR) tw2c[s] = P.TW2[o];
    }
    __syncthreads();

    float acc[XB];
#pragma unroll
    for (int i = 0; i < XB; ++i) acc[i] = 0.f;

    for (int blk0 = 0; blk0 < nblocks; blk0 += R / S) {
#pragma unroll
        for (int bb = 0; bb < R / S; ++bb) {
            const int blk = blk0 + bb;
            if (blk >= nblocks) break;
            float pfG[S][2], pfD[S][2];
            int pk[S];
            unsigned short tkn[S];
            float twn[S], tw2n[NEAR ? S : 1];
            const bool more = (blk + 1 < nblocks);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                pfG[s][0] = pfG[s][1] = 0.f;
                pfD[s][0] = pfD[s][1] = 0.f;
                pk[s] = 0;
                tkn[s] = 0;
                twn[s] = 0.f;
                if (NEAR) tw2n[s] = 0.f;
                if (more) {
                    const int q = (blk + 1) * S + XB - 1 + s;
                    int kmin, kmax;
                    window(q, kmin, kmax);
                    pk[s] = kmin;
                    const int j = jbase + q;
                    const int jr = (j >= 0 && j < tnum) ? j : P.zero_row;
                    const float *src = P.GT + (size_t)jr * snum;
                    const int e0 = min(kmin + tid, snum - 1), e1 = min(kmin + tid + KF_THREADS, snum - 1);
                    pfG[s][0] = src[e0];
                    pfG[s][1] = src[e1];
                    if (NEAR) {
                        const float *srd = P.DT + (size_t)jr * snum;
                        pfD[s][0] = srd[e0];
                        pfD[s][1] = srd[e1];
                    }
                    const size_t o = (size_t)min(abs(nlo + (blk + 1) * S + s), ntab1) * snum + ti;
                    tkn[s] = P.TK[o];
                    twn[s] = P.TW[o];
                    if (NEAR) tw2n[s] = P.TW2[o];
                }
            }
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int pm = bb * S + s;
                const float w = twc[s];
                const float w2 = NEAR ? tw2c[s] : 0.f;
                const char *base = reinterpret_cast<const char *>(ldsG) + tkc[s];
                const char *based = reinterpret_cast<const char *>(ldsD) + tkc[s];
#pragma unroll
                for (int i = 0; i < XB; ++i) {
                    const int slot = (pm + i) % R;
                    acc[i] = fmaf(w, *reinterpret_cast<const float *>(base + slot * W * 4), acc[i]);
                    if (NEAR) acc[i] = fmaf(w2, *reinterpret_cast<const float *>(based + slot * W * 4), acc[i]);
                }
            }
            if (more) {
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const int slot = ((bb + 1) * S + XB - 1 + s) % R;
                    const int e0 = pk[s] + tid, e1 = e0 + KF_THREADS;
                    ldsG[slot * W + (e0 & (W - 1))] = pfG[s][0];
                    ldsG[slot * W + (e1 & (W - 1))] = pfG[s][1];
                    if (NEAR) {
                        ldsD[slot * W + (e0 & (W - 1))] = pfD[s][0];
                        ldsD[slot * W + (e1 & (W - 1))] = pfD[s][1];
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < S; ++s) {
                tkc[s] = tkn[s];
                twc[s] = twn[s];
                if (NEAR) tw2c[s] = tw2n[s];
            }
            __syncthreads();
        }
    }

    if (ti_raw < snum) {
        float *o = P.out + (size_t)ti_raw * P.ldo + (x0 - P.xlo);
#pragma unroll
        for (int i = 0; i < XB; ++i)
            if (x0 + i < P.xhi) o[i] = acc[i];
    }
}

// ---------------------------------------------------------------------------
// quad kernel: table-driven ring of 40 trace slots (5 groups of 8 traces) in LDS.
// At one step every output i of a lane reads the SAME sample k from XB consecutive ring slots:
// 6-7 aligned ds_read_b128 per step instead of 24 ds_read_b32.
//
// LDS image (filled by LDS-DMA, which writes 1 KiB contiguously per wave instruction):
//   piece  = 32 consecutive ring rows (row = sample mod W, W a multiple of 32)
//   byte(row, group g, half h) = (row >> 5) * KQ_PS + g * KQ_GS + (row & 31) * 32 + 16 * (h ^ ((row >> 3) & 1))
// i.e. per (piece, group) a contiguous [32 rows][8 traces] block of 1 KiB plus one spare 32-byte row; KQ_PS is a
// multiple of 256 B, which keeps rows of neighbouring pieces on distinct banks (15 % conflict cycles otherwise)
// (the spare row of piece 0 stays zero: it is what dropped pairs pick).  The two 16-byte halves of a
// row are swapped in rows with bit 3 set: the 16 lanes a ds_read_b128 services together hold 16
// consecutive samples (lane permutation below), whose rows r and r+8 would otherwise share banks.
// The DMA keeps the image linear and applies the swap on its per-lane SOURCE address; the pick table
// holds the byte offset of half 0 of the picked row, half 1 is that offset ^ 16.
// ---------------------------------------------------------------------------
// NH > 1: NH tiles of XB output traces share ONE ring in one workgroup of 256 NH threads (waves 4h .. 4h+3 own
// tile h = outputs x0 + h XB ...).  Tile h walks the trace offset XB steps BEHIND tile h - 1
// (n_h = n_0 - h XB), so that at every step all tiles read the same XB + 16 ring slots: the staged traces, the
// DMA that brings them and the barrier are shared, only the pick row (h XB / 8 rows behind, re-read from L2 a few
// blocks after the neighbour tile fetched it) and the obliquity factor differ.  The staging window grows by the
// moveout over (NH - 1) XB traces.  Per output this stages NH x fewer image bytes and puts 4 NH waves on the CU.
//
// LK = 1: one more 8-trace group in the ring, and the staging DMA runs one block further ahead (it then has two
// blocks, ~2.6 us, to land instead of one).  What the kernel loses to vector memory is not bytes (NH = 2 halves
// the fabric traffic and gains nothing) but the tail of the load latency: s_waitcnt vmcnt retires loads in issue
// order and every wave must see its DMA landed in front of each block's barrier, so one slow fetch parks four
// (or 4 NH) waves.  The extra group only fits with NH >= 2 (one workgroup per CU, LDS to spare).  The pick rows
// and window lookups are ordinary loads the compiler counts; their pipeline is deepened to PD blocks so that
// each is older than everything the block's wait leaves in flight (the compiler then adds no waits of its own,
// which would drain the younger DMA as well).
//
// WK = KIRCH_WINDOW_QUAD (far field): the output window moves instead of the read window.  At step pm (offset n, pm + 1 = n
// mod 8) a tile reads the ALIGNED XB slots from slot pm + 1 - phi, phi = n & 3 -- XB/4 whole quads, none with an unused
// component -- into the outputs [x0 - phi, x0 - phi + XB): XB + 3 accumulators, accumulator a = output x0 - 3 + a
// (kq_win_first_quad, kq_win_acc, kirch_route.h).  phi is the same for every tile of a launch (tile starts and XB are multiples
// of 8, every walk and walk piece starts at 1 mod 8), so at every offset the tiles still partition the output axis.  The
// XB - 3 columns a tile holds at every phase go to the image; of the three on either side it holds the offsets of some
// phases only, and those sums go to side_r / side_l for kirch_fixup_kernel.  The walk is 3 steps longer (outputs x0 - 3 ..
// x0 - 1 at their last offsets; the traces beyond the profile are zero rows).
// Ring safety of the aligned window: it begins up to 3 slots before the sliding one and ends with it or before.  Step
// pm0 + 6 of a block reads from slot pm0 + 4, in the group this block's DMA re-fills -- issued behind the barrier that every
// wave passes after its FMAs of step 6; steps pm0 + 7 .. pm0 + 10 (the first of them in flight across that barrier) read from
// slot pm0 + 8, step 0 of an item from slot 0, the first trace of the first staged group.  A staged trace is read for up to
// XB + 2 steps: its staging window covers them (kirch_ring_tables), and the route takes this form only where the ring's
// rows hold that moveout (kirch_route).
template <int XB, bool NEAR, int OCC, int SH, int NH, int LK, int WK = KIRCH_WINDOW_SLIDE>
__global__ __launch_bounds__(KF_THREADS * NH, OCC) void kirch_quad_kernel(FastParams P, int W)
{
    static_assert(WK == KIRCH_WINDOW_SLIDE || (WK == KIRCH_WINDOW_QUAD && !NEAR && XB % 8 == 0), "the quad-aligned window is the far field's");
    constexpr int NA4 = XB / 4 + WK;          // accumulator quads
    constexpr int S = 8;
    constexpr int RG = kq_ring_slots(XB) + 8 * LK;     // ring slots
    constexpr int KQ_PS = kq_piece_bytes_lk(XB, LK);
    constexpr int PD = 2 * LK + 1;            // blocks between the issue of a pick row / window lookup and its first use
    static_assert(LK == 0 || LK == 1, "staging lookahead of one or two blocks");
    static_assert(LK == 0 || !NEAR, "the deeper ring is not laid out for the second (near field) image");
    constexpr int G0 = XB / 8;                // a block's new traces belong to image / ring group blk + G0
    constexpr int PER = WK ? KQ_PER_WIN : KQ_PER;            // quads per interleave slice
    constexpr int KQ_PARTS = (XB / 4 + (WK ? 0 : 1) + PER - 1) / PER;   // interleave slices per step
    constexpr int NB = RG / S;                // step blocks per ring revolution (unroll length)
    constexpr int NQ = RG / 4;                // slot quads
    static_assert(XB + 2 * S - 1 <= RG && RG % S == 0 && XB % 4 == 0, "ring too small");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int npieces = W >> 5;               // W is a multiple of 32
    const unsigned img_bytes = (unsigned)npieces * KQ_PS;      // one image (gradient; data image behind it)

    const int tid = threadIdx.x & (KF_THREADS - 1);                  // lane-and-wave index inside the tile
    const int half = NH > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 8) : 0;   // which tile of the workgroup
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
    const int x0w = (WK ? P.x00 : (P.xlo & ~7)) + xt * (XB * NH);   // workgroup's first output trace: a multiple of 8 (outputs left of xlo are not stored)
    const int x0 = x0w + half * XB;
    const int snum = P.snum;
    const int lane = tid & 63;
    const int sigma = kirch_ring_sigma(lane);        // the 16 lanes a ds_read_b128 services together hold 16 consecutive samples
    const int ti_raw = s0 + (tid & ~63) + sigma;
    const int ti = min(ti_raw, snum - 1);

    const int hmax = P.hmax[chunk];
    int nlo, nhi;                                // tile 0's offsets: the ring clock
    if (kirch_ring_walk<S, NB, XB, NH, WK ? KQ_WIN_EXTRA : 0>(P, hmax, x0w, part, nlo, nhi)) continue;      // uniform; the partial images are zeroed before the launch
    const int nsteps = nhi - nlo + 1;
    const int nblocks = (nsteps + S - 1) / S;
    // the main loop always runs whole ring revolutions (NB blocks); steps past the
    // aperture pick the table's all-zero row, so they add nothing
    const int nrev = (nblocks + NB - 1) / NB;
    const int jbase = x0w + nlo;
    // table row of block 0 (block b covers n = nlo + 8 b .. + 7); rows past the tables' end (only the
    // padding blocks of the last revolution can get there) are clamped to the last, all-dropped row
    const int mrow = ((nlo - 1) >> 3) + P.mrow0;
    auto row_of = [&](int blk) { return min(mrow + blk, P.nrows - 1); };
    // this tile's pick rows: half * XB offsets behind the clock (the table keeps 8 all-dropped rows at its start)
    const int mrow_h = mrow - half * (XB / 8);
    // (blocks past the walk -- the padding of the last ring revolution -- read the table's last, all-dropped row: after
    // a piece of a walk they would otherwise be offsets that the next piece owns)
    auto prow_of = [&](int blk) { return blk >= nblocks ? P.nrows - 1 : max(min(mrow_h + blk, P.nrows - 1), 0); };

    // Staging window of the 8 traces block `blk_for` adds: one 8-byte lookup, issued ONE BLOCK EARLIER
    // than its use: s_waitcnt vmcnt counts in order, so waiting for a lookup issued in the same block
    // would also wait for the pick loads just in front of it (a full miss latency per block).
    const int2 *WIN = P.WIN + (size_t)chunk * P.nrows;
    auto fetch_for = [&](int blk_for, int &a, int &b) {
        const int2 w = WIN[max(row_of(blk_for), 0)];
        a = w.x;
        b = w.y;
    };
    // The image is stored in groups of 8 traces, sample-major inside a group (see PrepParams::i8):
    // sample k of the 8 traces of a step block is 32 contiguous bytes.  Raw buffers based at this
    // workgroup's first group: scalar group offset + per-lane sample offset, no address arithmetic
    // in vector registers; traces outside the profile are zero rows of the padded image.
    const unsigned grp_bytes = (unsigned)snum * 32u;
    const kq_u4 gdesc = kirch_ring_desc(P.GT, jbase, snum);
    const kq_u4 ddesc = kirch_ring_desc(NEAR ? P.DT : P.GT, jbase, snum);
    // Pick table entry = LDS offset of the picked sample's ring row (bytes >> SH); pairs the reference
    // drops (t > t_max, or the 0/0 apex of a t = 0 sample) point at the all-zero row, so they need no
    // compare/select.  The 8 picks of a step block are 16 contiguous bytes per lane: one raw-buffer load
    // (scalar row offset + lane offset) per block.
    const __amdgpu_buffer_rsrc_t tkres =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(P.TKB), 0, 0x7fffffff, 0x00020000);
    const unsigned tioff = (unsigned)ti * 16u;
    const unsigned rowbytes = (unsigned)kq_tkb_stride(snum) * 16u;
    auto picks = [&](int blk) -> kq_u4 {
        return __builtin_amdgcn_raw_buffer_load_b128(tkres, tioff, (unsigned)prow_of(blk) * rowbytes, 0);
    };
#define KQ_TK(q, s) (((q)[(s) >> 1] >> (16 * ((s) & 1))) & 0xffffu)
    const float c1 = P.c1[ti], c2 = NEAR ? P.c2[ti] : 0.f, fin = P.fin[ti];
    // n^2 of a step: scalar multiply + one conversion (in-aperture offsets are < 65536, so the product
    // fits 32 bits; padding steps may wrap, they only ever meet the all-zero row)
    const int nlo_h = nlo - half * XB;
    auto n2_of = [&](int step) {
        const int n = nlo_h + step;
        return (float)((unsigned)n * (unsigned)n);
    };

    if (first_item) {
        // (later items of a persistent workgroup keep the image: every row a pick can point at is re-staged before
        // it is read, and the all-zero spare row is never written)
        if ((unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)lds != 0u) __builtin_trap();
        for (int e = threadIdx.x; e < (int)(img_bytes / 4) * (NEAR ? 2 : 1); e += KF_THREADS * NH) lds[e] = 0.f;
        __syncthreads();
        first_item = false;
    }
    // Pick rows are requested TWO blocks ahead (KQ_PICK_AHEAD = 2): a row that misses the XCD's L2 (the table is
    // 61 MB, a chunk's slice 3.8 MB) takes longer than one block (~1.3 us) to arrive, and with one block of
    // lookahead that latency sat in front of every barrier (a build whose pick rows were always L2-hot ran
    // 0.74 ms faster at config 3).  The wait in front of the barrier then leaves the two youngest loads (the
    // pick row and the staging window issued at the top of the block) in flight: s_waitcnt vmcnt counts in
    // order, so vmcnt(2) still retires the staging DMA issued behind the previous barrier.
    kq_u4 tkc = picks(0);                          // picks of the current block
    kq_u4 tkp[PD + 1];                             // ... of the next one (tkp[0]) and of those behind it
#pragma unroll
    for (int j = 0; j < PD; ++j) tkp[j] = picks(1 + j);

    // accumulators in quads: the ordering pin below takes them as XB/4 operands of ONE asm statement
    kq_f4 acc4[NA4];
#pragma unroll
    for (int i = 0; i < NA4; ++i) acc4[i] = kq_f4{0.f, 0.f, 0.f, 0.f};
#define KQ_ACC(i) acc4[(i) >> 2][(i) & 3]

    // ---- staging by LDS-DMA: the 8 traces a block adds (one 8-row group of the image) go straight from
    // memory into their ring group, 1 KiB (32 rows) per wave instruction, no staging registers and no
    // ds_write.  Lane l of a piece writes bytes [16 l, 16 l + 16) of the piece: row 32 piece + l/2,
    // half (l & 1); its SOURCE is the sample congruent to that row in [kmin, kmin + W) and the half
    // the row's swap puts there.  Pieces are dealt to the four waves round robin.
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // wave index in the workgroup, in a scalar register
    const int rl = lane >> 1;                                  // row of this lane inside a piece
    const unsigned hsel = ((unsigned)(lane & 1) ^ ((unsigned)(rl >> 3) & 1u)) * 16u;
    auto dma_issue = [&](int blk_for, int wa) {     // traces that block `blk_for` adds to the ring
        const int kmin = wa & 0xffff, kmod = (int)((unsigned)wa >> 16);
        const int gidx = ((blk_for + G0) % NB + NB) % NB;      // ring group of these traces
        const unsigned so = (unsigned)(blk_for + G0) * grp_bytes;     // image group of trace jbase + q0
        for (int pc = wv; pc < npieces; pc += 4 * NH) {
            int t = pc * 32 + rl - kmod;
            t += (t < 0) ? W : 0;
            const int c = min(kmin + t, snum - 1);
            const unsigned vo = (unsigned)c * 32u + hsel;
            kirch_ring_dma16((unsigned)(pc * KQ_PS + gidx * KQ_GS), vo, gdesc, so);
            if (NEAR) kirch_ring_dma16(img_bytes + (unsigned)(pc * KQ_PS + gidx * KQ_GS), vo, ddesc, so);
        }
    };
    // ring position of ring-relative trace q is (q + 1) % RG: the 8 traces a block adds are one ring
    // group; the ring starts with the four groups q = -1 .. 30
    int wa, wb;
    for (int pb = -G0; pb <= 0; ++pb) {
        fetch_for(pb, wa, wb);
        dma_issue(pb, wa);
    }
    int wl[LK + 1], wp[PD];                        // windows of the DMAs issued in the prologue / in the first PD blocks
#pragma unroll
    for (int j = 0; j <= LK; ++j) fetch_for(1 + j, wl[j], wb);
#pragma unroll
    for (int j = 0; j < PD; ++j) fetch_for(2 + LK + j, wp[j], wb);
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
    __syncthreads();
#pragma unroll
    for (int j = 0; j <= LK; ++j) dma_issue(1 + j, wl[j]);     // block 1's (and 2's) traces land during block 0
    // DMA instructions this wave issues per block (its share of the pieces): the in-order wait in front of the
    // barrier leaves one block's worth of them in flight when LK = 1
    const int dma_c = __builtin_amdgcn_readfirstlane((npieces - wv + 4 * NH - 1) / (4 * NH));

    // ---- the resident ring is read software pipelined: the ds_read_b128 of step s+1 are in flight
    // while the FMAs of step s run (two statically indexed quad buffers), also across block ends
    kq_f4 va[NQ], vb[NQ], ua[NEAR ? NQ : 1], ub[NEAR ? NQ : 1];
    // position of quad qd in the step's run of needed quads (they are consecutive, cyclically; the aligned run starts at
    // the same quad: kq_win_first_quad)
    auto run_pos = [](int pm, int qd) { return (qd - ((pm + 1) % RG) / 4 + NQ) % NQ; };
    static_assert(kq_win_first_quad(5, NQ) == 1 && kq_win_first_quad(RG - 1, NQ) == 0 && kq_win_first_quad(RG - 2, NQ) == NQ - 1, "");
    auto needed = [&](int pm, int qd) {
        if constexpr (WK) return run_pos(pm, qd) < XB / 4;
        bool any = false;
        for (int c = 0; c < 4; ++c) any = any || ((4 * qd + c - pm - 1 + 2 * RG) % RG) < XB;
        return any;
    };
    // pm = step index mod RG (a compile-time constant after unrolling), tk = the step's table entry =
    // byte offset of half 0 of the picked row; quad qd = ring slots 4 qd .. 4 qd + 3 = half qd & 1 of group qd >> 1
    // `part` selects a slice of the run (KQ_PARTS slices; -1 = all): reads and FMAs are interleaved slice
    // by slice so that a wave's ds_read_b128 do not arrive at the LDS queue as one burst of 7
    auto load_step = [&](int pm, unsigned tk, kq_f4 (&v)[NQ], kq_f4 (&u)[NEAR ? NQ : 1], int part) {
        // LDS pointers built from the table's byte offsets directly: the dynamic LDS block of this kernel
        // starts at LDS address 0 (no static __shared__; checked once in the prologue), so no base is added
        typedef const __attribute__((address_space(3))) kq_f4 *lds_f4p;
        const unsigned a0 = tk << SH, a1 = a0 ^ 16u;
#pragma unroll
        for (int qd = 0; qd < NQ; ++qd)
            if (needed(pm, qd) && (part < 0 || run_pos(pm, qd) / PER == part)) {
                // must stay a whole ds_read_b128 also for the partly used quads at the ends of
                // the window: fma_step marks the unused components as used (empty asm)
                const unsigned src = ((qd & 1) ? a1 : a0) + (qd >> 1) * KQ_GS;
                v[qd] = *(lds_f4p)(uintptr_t)src;
                if (NEAR) u[qd] = *(lds_f4p)(uintptr_t)(src + img_bytes);
            }
    };
    auto fma_step = [&](int pm, float w, float w2, const kq_f4 (&v)[NQ], const kq_f4 (&u)[NEAR ? NQ : 1], int part) {
#pragma unroll
        for (int qd = 0; qd < NQ; ++qd) {
            if (part >= 0 && run_pos(pm, qd) / PER != part) continue;
            if constexpr (WK) {
                // every component of the run's quads feeds an accumulator
                const int t = run_pos(pm, qd);
                if (t < XB / 4) {
                    KQ_ACC(kq_win_acc(pm, t, 0)) = fmaf(w, v[qd].x, KQ_ACC(kq_win_acc(pm, t, 0)));
                    KQ_ACC(kq_win_acc(pm, t, 1)) = fmaf(w, v[qd].y, KQ_ACC(kq_win_acc(pm, t, 1)));
                    KQ_ACC(kq_win_acc(pm, t, 2)) = fmaf(w, v[qd].z, KQ_ACC(kq_win_acc(pm, t, 2)));
                    KQ_ACC(kq_win_acc(pm, t, 3)) = fmaf(w, v[qd].w, KQ_ACC(kq_win_acc(pm, t, 3)));
                }
                continue;
            }
            // outputs served by slots 4qd .. 4qd+3 at this step
            const int i0 = (4 * qd + 0 - pm - 1 + 2 * RG) % RG;
            const int i1 = (4 * qd + 1 - pm - 1 + 2 * RG) % RG;
            const int i2 = (4 * qd + 2 - pm - 1 + 2 * RG) % RG;
            const int i3 = (4 * qd + 3 - pm - 1 + 2 * RG) % RG;
            const bool any = i0 < XB || i1 < XB || i2 < XB || i3 < XB;
            if (any) {
                // components of an edge quad that serve no output are handed to an empty asm: the
                // load stays a whole ds_read_b128 (split into b32 pieces it bank-conflicts 4-way)
                // at no instruction cost
#define KQ_COMP(ix, c)                                                              \
    if (ix < XB) {                                                                  \
        KQ_ACC(ix < XB ? ix : 0) = fmaf(w, v[qd].c, KQ_ACC(ix < XB ? ix : 0));            \
        if (NEAR) KQ_ACC(ix < XB ? ix : 0) = fmaf(w2, u[qd].c, KQ_ACC(ix < XB ? ix : 0)); \
    } else {                                                                        \
        asm volatile("" ::"v"(v[qd].c));                                            \
        if (NEAR) asm volatile("" ::"v"(u[qd].c));                                  \
    }
                KQ_COMP(i0, x)
                KQ_COMP(i1, y)
                KQ_COMP(i2, z)
                KQ_COMP(i3, w)
#undef KQ_COMP
            }
        }
    };
    // The FMAs carry no chain, so instruction selection is free to sink a whole block's
    // FMAs below all of its LDS reads (which then spill).  Passing the accumulators
    // through an empty volatile asm (with a memory clobber) after every group of reads and every
    // step's FMAs pins the order reads(s+1) -> FMAs(s) without consuming any load result early.
#define KQ_PIN()                                                                                          \
    do {                                                                                                  \
        static_assert(XB == 24 || XB == 32 || XB == 40, "KQ_PIN lists XB/4 accumulator quads");           \
        if (XB == 24)                                                                                     \
            asm volatile("" : "+v"(acc4[0]), "+v"(acc4[1]), "+v"(acc4[2]), "+v"(acc4[3]), "+v"(acc4[4]), \
                              "+v"(acc4[5]) :: "memory");                                                 \
        else if (XB == 32)                                                                                \
            asm volatile("" : "+v"(acc4[0]), "+v"(acc4[1]), "+v"(acc4[2]), "+v"(acc4[3]), "+v"(acc4[4]), \
                              "+v"(acc4[5]), "+v"(acc4[XB >= 32 ? 6 : 0]), "+v"(acc4[XB >= 32 ? 7 : 0])   \
                         :: "memory");                                                                    \
        else                                                                                              \
            asm volatile("" : "+v"(acc4[0]), "+v"(acc4[1]), "+v"(acc4[2]), "+v"(acc4[3]), "+v"(acc4[4]), \
                              "+v"(acc4[5]), "+v"(acc4[XB >= 32 ? 6 : 0]), "+v"(acc4[XB >= 32 ? 7 : 0]),  \
                              "+v"(acc4[XB >= 40 ? 8 : 0]), "+v"(acc4[XB >= 40 ? 9 : 0]) :: "memory");    \
        if (WK) asm volatile("" : "+v"(acc4[NA4 - 1]) :: "memory");       /* the quad of accumulators XB .. XB + 2 */    \
    } while (0)

    float n2c[S];                                  // n^2 of the current block's steps
#pragma unroll
    for (int s = 0; s < S; ++s) n2c[s] = n2_of(s);
    load_step(0, KQ_TK(tkc, 0), va, ua, -1);       // step 0 of block 0
    for (int rev = 0; rev < nrev; ++rev) {
#pragma clang loop unroll(full)
        for (int bb = 0; bb < NB; ++bb) {              // block index within the ring revolution
            const int blk = rev * NB + bb;
            const int pm0 = bb * S;                    // step index mod RG of the block's first step
            // ---- loads: the next block's table entries and, by DMA, its 8 new traces.  Their ring group
            // held traces last read at step 6 of the previous block, and every wave is past that block's
            // barrier, which sits after step 6: no wave can still be reading them.
            tkp[PD] = picks(blk + PD + 1);
            int wn = 0;
            fetch_for(blk + 2 + LK + PD, wn, wb);      // staging window of a DMA issued PD blocks from now
            // obliquity cos(theta) of this block's steps
            float twc[S], tw2c[NEAR ? S : 1];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const float y = __builtin_amdgcn_rsqf(fmaf(c1, n2c[s], 1.0f));
                twc[s] = y;
                if (NEAR) tw2c[s] = (y * c2) * (y * y);
            }
            {
#pragma unroll
                for (int s = 0; s < S; ++s) n2c[s] = n2_of((blk + 1) * S + s);
            }
#define KQ_W2(s) (NEAR ? tw2c[NEAR ? (s) : 0] : 0.f)
#define KQ_UNPACK(...) __VA_ARGS__
#define KQ_STEP(L, F)                                                                          \
    do {                                                                                       \
        _Pragma("unroll") for (int part = 0; part < KQ_PARTS; ++part) {                      \
            load_step(KQ_UNPACK L, part); KQ_PIN();                                            \
            fma_step(KQ_UNPACK F, part); KQ_PIN();                                             \
        }                                                                                      \
    } while (0)
            KQ_STEP((pm0 + 1, KQ_TK(tkc, 1), vb, ub), (pm0 + 0, twc[0], KQ_W2(0), va, ua));
            KQ_STEP((pm0 + 2, KQ_TK(tkc, 2), va, ua), (pm0 + 1, twc[1], KQ_W2(1), vb, ub));
            KQ_STEP((pm0 + 3, KQ_TK(tkc, 3), vb, ub), (pm0 + 2, twc[2], KQ_W2(2), va, ua));
            KQ_STEP((pm0 + 4, KQ_TK(tkc, 4), va, ua), (pm0 + 3, twc[3], KQ_W2(3), vb, ub));
            KQ_STEP((pm0 + 5, KQ_TK(tkc, 5), vb, ub), (pm0 + 4, twc[4], KQ_W2(4), va, ua));
            KQ_STEP((pm0 + 6, KQ_TK(tkc, 6), va, ua), (pm0 + 5, twc[5], KQ_W2(5), vb, ub));
            KQ_STEP((pm0 + 7, KQ_TK(tkc, 7), vb, ub), (pm0 + 6, twc[6], KQ_W2(6), va, ua));
            // ---- barrier after step 6.  The new traces are first read by step 0 of the next block, whose
            // reads are issued below; each wave retires its own DMA (and the pick load) first.  The LDS
            // reads of step 7 stay in flight across the barrier, so the read pipeline never drains.
            // a builtin so that hipcc's own wait counting sees it
            if (LK == 0) {
                __builtin_amdgcn_s_waitcnt(0x0F72);    // vmcnt(2): all but this block's pick row + window lookup
            } else if (blk < LK || dma_c == 0) {
                __builtin_amdgcn_s_waitcnt(0x0F70);    // pipeline not yet full (or a wave without a DMA share): everything
            } else if (dma_c == 1) {
                __builtin_amdgcn_s_waitcnt(0x0F75);    // vmcnt(5): two blocks of pick + window lookups and one DMA
            } else {
                __builtin_amdgcn_s_waitcnt(0x0F76);    // vmcnt(6): ... and two DMAs
            }
            asm volatile("s_barrier" ::: "memory");
            // every wave is past step 6 of this block: the ring group of the traces last read there is free
            dma_issue(blk + 2 + LK, wp[0]);
#pragma unroll
            for (int j = 0; j + 1 < PD; ++j) wp[j] = wp[j + 1];
            wp[PD - 1] = wn;
#define KQ_NEXT tkp[0]
            KQ_STEP(((pm0 + 8) % RG, KQ_TK(KQ_NEXT, 0), va, ua), (pm0 + 7, twc[7], KQ_W2(7), vb, ub));
#undef KQ_W2
#undef KQ_STEP
#undef KQ_UNPACK
            tkc = KQ_NEXT;
#undef KQ_NEXT
#pragma unroll
            for (int j = 0; j < PD; ++j) tkp[j] = tkp[j + 1];
        }
    }
#undef KQ_PIN
#undef KQ_TK
    asm volatile("" ::"v"(va[0].x), "v"(va[NQ - 1].w));   // the look-ahead reads of the step after the last
    __builtin_amdgcn_s_waitcnt(0x0F70);                    // the look-ahead DMA must land before the LDS is released

    if (ti_raw < snum) {
        float *o = (P.parts_log2 ? reinterpret_cast<float *>(P.partial) + (size_t)part * P.part_stride : P.out) +
                   (size_t)ti_raw * P.ldo + (x0 - P.xlo);
        if constexpr (WK) {
            // accumulators 3 .. XB - 1 are whole columns; 0 .. 2 (left of x0) and XB .. XB + 2 lack the offsets the neighbour
            // tile took: raw sums, sample-major (lanes = consecutive samples), for kirch_fixup_kernel
#pragma unroll
            for (int i = 0; i < XB - 3; ++i)
                if (x0 + i >= P.xlo && x0 + i < P.xhi) o[i] = KQ_ACC(i + 3) * fin;
            const size_t so = (size_t)part * P.side_stride + (size_t)(xt * NH + half) * 3 * snum + ti_raw;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                P.side_l[so + (size_t)c * snum] = KQ_ACC(c);
                P.side_r[so + (size_t)c * snum] = KQ_ACC(XB + c);
            }
        } else {
#pragma unroll
            for (int i = 0; i < XB; ++i)
                if (x0 + i >= P.xlo && x0 + i < P.xhi) o[i] = KQ_ACC(i) * fin;
        }
    }
#undef KQ_ACC
    if (!P.queue) break;
    }   // item loop
}

// The three columns left of every tile start under the quad-aligned window: the tile left of the start summed the offsets at
// which its window still reached them (side_r), the tile right of it the rest (side_l).  One thread per (sample, tile start,
// piece): out = (right tile's sum of the left tile + left-edge sum of the right tile) * fin, always in this order and without
// atomics, so an image is the same from run to run and under any queue order.  `out`: the image, or the partial images of
// the pieces of a walk (stride part_stride) in front of kirch_combine_kernel.
__global__ __launch_bounds__(256) void kirch_fixup_kernel(FastParams P, int xb, int ntt, float *out)
{
    const int ti = blockIdx.y * 256 + threadIdx.x, b = blockIdx.x + 1, part = blockIdx.z;
    if (ti >= P.snum || b >= ntt) return;
    const float *r = P.side_r + (size_t)part * P.side_stride + (size_t)(b - 1) * 3 * P.snum + ti;
    const float *l = P.side_l + (size_t)part * P.side_stride + (size_t)b * 3 * P.snum + ti;
    const float fin = P.fin[ti];
    float *o = out + (size_t)part * P.part_stride + (size_t)ti * P.ldo;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int x = P.x00 + b * xb - 3 + c;
        if (x >= P.xlo && x < P.xhi) o[x - P.xlo] = (r[(size_t)c * P.snum] + l[(size_t)c * P.snum]) * fin;
    }
}

// ===========================================================================
// host side
// ===========================================================================
// a kirch_quad_kernel instantiation as launch_ring (kirch_ring.h) takes it
template <int XB_, int OCC, int SH, int NH_ = 1, int LK = 0, int WK = KIRCH_WINDOW_SLIDE>
struct RingF32 {
    typedef float elem;
    static constexpr int XB = XB_, NH = NH_, window = WK;
    static constexpr int align_mask = 7, step_block = 8, ring_blocks = (kq_ring_slots(XB) + 8 * LK) / 8, piece_bytes = kq_piece_bytes_lk(XB, LK);
    static auto near_kernel() { return kirch_quad_kernel<XB, true, 1, SH, 1, 0>; }
    static auto far_kernel() { return kirch_quad_kernel<XB, false, OCC, SH, NH, LK, WK>; }
    static void launch_fixup(const FastParams &P, int ntt, hipStream_t st)      // ntt: tiles of the launch
    {
        hipLaunchKernelGGL(kirch_fixup_kernel, dim3(ntt - 1, (P.snum + 255) / 256, 1 << P.parts_log2), dim3(256), 0, st, P, XB, ntt,
                           P.parts_log2 ? reinterpret_cast<float *>(P.partial) : P.out);
    }
};

// kirch_tab_kernel: geometry-only pick/weight table, rebuilt with every prep (counted in prep time)
static int prep_table_tab(impdar_kirch_plan *p, int b, hipStream_t st)
{
    TableParams T;
    T.TK = p->d_TK[b].as<unsigned short>();
    T.TW = p->d_TW[b].as<float>();
    T.TW2 = p->d_TW2[b].as<float>();
    kirch_fill_axes(T, p);
    T.dx = p->dx;
    T.ntab = p->ntab;
    T.near = p->nearfield;
    T.wmod = KF_W;
    T.kscale = 4;
    T.sentinel = 0;
    T.write_w = 1;
    hipLaunchKernelGGL(kirch_table_kernel, dim3((p->snum + 255) / 256, p->ntab), dim3(256), 0, st, T);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

template <int XB, int S, int OCC>
static int launch_tab(impdar_kirch_plan *p, const FastParams &P0, int nx, hipStream_t st)
{
    constexpr int R = XB + 2 * S;
    FastParams P = P0;
    const int ntiles = (nx + XB - 1) / XB;
    P.nxt = ntiles;
    P.G = 4;
    const int per = 8 * P.G;
    const int nxt_pad = ((ntiles + per - 1) / per) * per;
    P.tiles_per_xcd = nxt_pad / 8;
    const int nblk = P.nchunks * nxt_pad;
    const size_t shmem = (size_t)R * KF_W * 4 * (p->nearfield ? 2 : 1);
    if (p->nearfield) {
        auto k = kirch_tab_kernel<XB, S, true, 1>;
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL(k, dim3(nblk), dim3(KF_THREADS), shmem, st, P);
    } else {
        auto k = kirch_tab_kernel<XB, S, false, OCC>;
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL(k, dim3(nblk), dim3(KF_THREADS), shmem, st, P);
    }
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

// the diffraction sum by the plan's route: kirch_quad_kernel in the instantiation of its tile width, tiles per workgroup and
// table shift, or kirch_tab_kernel
int kirch_launch_ring32(impdar_kirch_plan *p, void *d_out, int xlo, int xhi, hipStream_t st)
{
    const FastParams P = kirch_ring_params(p, d_out, xlo, xhi);
    // (the window kind is the route's: KIRCH_WINDOW_QUAD only for far-field plans)
#define KQ_RING(...) (p->window == KIRCH_WINDOW_QUAD ? launch_ring<RingF32<__VA_ARGS__, KIRCH_WINDOW_QUAD>>(p, P, st) : launch_ring<RingF32<__VA_ARGS__>>(p, P, st))
    if (p->quad && p->quadSH == 0)
        return p->xb == 40 ? KQ_RING(40, 2, 0, 1, 0) : p->xb == 32 ? KQ_RING(32, 2, 0, 1, 0) : KQ_RING(24, 3, 0, 1, 0);
    if (p->quad && p->nh == 2 && p->xb == 32) return KQ_RING(32, 4, 4, 2, 0);      // 70 KB of LDS: two workgroups of 8 waves per CU
    if (p->quad && p->nh == 2 && p->xb == 40) return p->lk ? KQ_RING(40, 2, 4, 2, 1) : KQ_RING(40, 2, 4, 2, 0);
    if (p->quad && p->nh == 3 && p->xb == 40) return p->lk ? KQ_RING(40, 3, 4, 3, 1) : KQ_RING(40, 3, 4, 3, 0);
    if (p->quad)      // steep moveout: two workgroups per CU
        return p->xb == 40 ? KQ_RING(40, 2, 4, 1, 0) : p->xb == 32 ? KQ_RING(32, 2, 4, 1, 0) : KQ_RING(24, 2, 4, 1, 0);
#undef KQ_RING
    return launch_tab<16, 4, 4>(p, P, xhi - xlo, st);
}

int kirch_table_ring32(impdar_kirch_plan *p, int b, hipStream_t st)
{
    if (p->quad) return prep_table_ring(p, b, st, kirch_tableq_kernel, kq_piece_bytes_lk(p->xb, p->lk));
    return prep_table_tab(p, b, st);
}
