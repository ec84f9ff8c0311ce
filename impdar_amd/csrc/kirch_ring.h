// What the two LDS-ring units share -- kirch_ring32.hip (kirch_quad_kernel, kirch_tab_kernel: float32) and kirch_ring64.hip
// (kirch_dquad_kernel: float64): the kernels' parameter structs, the device fragments that are the same in both ring kernels
// apart from the step block S (8 / 4 traces), and the host code of a ring launch (tile map, persistent-workgroup queue,
// walk pieces and their sum).  The LDS image both kernels read is described at kirch_quad_kernel.
#pragma once
#include "kirch_plan.h"
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

struct FastParams {
    const float *GT, *DT;
    float *out;
    int ldo;
    int snum, tnum, xlo, xhi;
    const int *hmax;               // per sample-chunk aperture half width (+1 guard)     [nchunks]
    int nchunks, nxt, tiles_per_xcd, G;
    int parts_log2;                // persistent ring kernels: every tile's walk as 1 << parts_log2 queue items (pieces)
    void *partial;                 // ... their partial images [piece][snum][ldo] (element type = image type)
    size_t part_stride;            // ... elements per partial image
    // quad kernel, quad-aligned window (KIRCH_WINDOW_QUAD): tiles start at x00 + multiples of the tile; what a tile holds of the
    // three columns left of its own start and of the next tile's -- raw sums [piece][tile][3][snum], sample-major -- goes to
    // side_l / side_r; kirch_fixup_kernel adds the two.  Null under the sliding window.
    int x00;
    float *side_l, *side_r;
    size_t side_stride;            // ... elements per piece
    int *queue;                    // ring kernels, persistent workgroups: 8 item counters (one per XCD, 64 bytes apart), zeroed
                                   // before the launch; null = one item per block
    const int *items;              // ... and the XCDs' lists of items (chunk << 16 | tile, kirch_gangmap): [0..7] their lengths,
                                   // [8..15] where each starts, then the lists
    const short *tilemap;          // one item per block: [nchunks][tiles_per_xcd][8] output tile of (chunk, slot, XCD), -1 = none
                                   // (host-balanced over the XCDs by step count, build_tilemap); null: arithmetic rule
    // tab kernel only:
    const int *klo, *khi;          // per (chunk, |n|) first / last sample a trace at offset n is asked for
    int nb;                        // entries per chunk in klo/khi
    int zero_row;                  // index of an all-zero image row (out-of-profile traces)
    const unsigned short *TK;      // pick table (|n|, ti): offset of the picked sample inside a ring slot [ntab][snum]
    const float *TW, *TW2;         // far / near weights (0 where the reference drops the pair)
    // quad kernel: cos(theta) = sign(a) * rsq(1 + c1 n^2) with a = tt/dt, c1 = alpha / a^2; the far-field sum is
    // scaled by fin = sign(a) / (2 pi v) once at the end, the near-field weight is c2 * cos^3 in those units
    const float *c1, *c2, *fin;    // per sample [snum]
    const double *c1d, *c2d, *find;   // the same in float64 (dquad kernel): c1 = (dx/zs)^2, fin = 1/(2 pi v), c2: see kirch_dquad_kernel
    // quad kernel, step-block tables.  Every workgroup walks the trace offset n in blocks of 8 steps
    // n = 8 m + 1 .. 8 m + 8 (tiles start at multiples of 8, so the alignment is the same for all);
    // table row = m + mrow0:
    const void *TKB;               // [nrows][snum] x 8 picks of 16 bits: one 16-byte load per lane per block
    const int2 *WIN;               // [nchunks][nrows] staging window of the 8 traces a block adds:
                                   //   x = kmin | (kmin mod W) << 16, y = kmax
    int nrows, mrow0;
    int ntab;                      // tab kernel: table rows; the last row is all zero (|n| beyond every aperture)
};

// ---------------------------------------------------------------------------
// pick / weight table.  For a uniform trace spacing the sample picked by the
// pair (output sample ti, input trace xi+n) and its obliquity weight depend on
// (ti, |n|) only.  One thread per entry evaluates them in fp64 in the
// reference's operation order (mig_python.py:44-58), so the diffraction-sum
// kernel below inherits the reference's picks, its t>tmax test and its NaN
// skipping exactly; the table is rebuilt by every prep (it is cheap: ~1e7
// entries) so nothing about it is cached across migrations.
// ---------------------------------------------------------------------------
struct TableParams {
    unsigned short *TK;
    float *TW, *TW2;
    const double *zs, *zs2, *tt;
    double dx, vel, tmax, inv_dt, tt0;
    int snum, ntab, near;
    int wmod, kscale;          // slot byte offset of sample k = (k % wmod) * kscale
    unsigned short sentinel;   // TK value for dropped pairs (0xFFFF for the quad kernel, 0 for tab: its weight is 0)
    int write_w;
};

// Same picks for the quad kernel, laid out by step block: row r holds, per sample, the 8 picks of the
// offsets n = 8 (r - mrow0) + 1 + s, s = 0..7 (|n| decides the pick; blocks left of the apex are stored
// mirrored, so the kernel never computes |n|).  One thread per (row, sample), one 16-byte store.
struct TableQParams {
    uint4 *TKB;
    const double *zs, *zs2, *tt;
    double dx, vel, tmax, inv_dt, tt0;
    int snum, nrows, mrow0, nmax;   // offsets |n| >= nmax are outside every aperture
    int wmod, sh;                   // ring rows; entries are LDS byte offsets >> sh
    int ps;                         // bytes per 32-row piece of the LDS image (kq_piece_bytes)
};

// byte offset of half 0 of ring row r in the quad kernel's LDS image (layout: see kirch_quad_kernel)
__host__ __device__ static inline unsigned kq_row_offset(int r, int ps)
{
    return (unsigned)(r >> 5) * (unsigned)ps + (unsigned)(r & 31) * 32u + (((unsigned)(r >> 3) & 1u) << 4);
}

#define KQ_ZERO 1024        // byte offset of the all-zero row (spare row of piece 0, group 0; + g * KQ_GS)
#ifndef KQ_PER
#define KQ_PER 4            // quads per interleave slice (1..7 all measure within 2 %; 4 keeps 97 VGPRs)
#endif
#ifndef KQ_PER_WIN
#define KQ_PER_WIN 2        // ... under the quad-aligned window: with slices of 4 the two-tile kernel of 32 traces (128 VGPRs at 4
                            // waves per SIMD) spills pick rows inside the step loop, and each reload drains the staging DMA
#endif
typedef float kq_f4 __attribute__((ext_vector_type(4)));
typedef unsigned kq_u4 __attribute__((ext_vector_type(4)));
typedef double kd_d2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------
// device fragments of kirch_quad_kernel and kirch_dquad_kernel
// ---------------------------------------------------------------------------
// The next (chunk, tile) item of a workgroup and which piece `part` of the tile's aperture walk it is: chunk << 16 | tile
// from the queue, -1 when it is empty; (chunk, tile) by the block rule, false when the block has none.
// (Two functions, and the kernels leave differently after each -- the item loop after the queue, the kernel after the block
// rule: one function with one way out is the same program but not the same instruction stream.)
// P.queue != null: persistent workgroups.  As many workgroups as fit the chip are launched, and each keeps
// pulling (chunk, tile) items: first from the list of the XCD it runs on (kirch_gangmap: gangs of adjacent tiles
// in consecutive positions, so the workgroups of an XCD that pull together walk neighbouring tiles of one chunk
// in phase), then, when that is empty, the next unread item of the other XCDs' lists in turn.  The XCDs of one
// MI355X differ by ~3 % in speed on this loop and blocks are dealt to them statically, so with one item per block
// the slowest XCD set the kernel's end; the queue also closes the gaps between workgroups and shortens the tail.
// The item is what the list holds: lists differ in length and say nothing about the chunk by position.
// `item_slot`: three ints of LDS behind the image(s).
__device__ __forceinline__ int kirch_ring_queue_item(const FastParams &P, int *item_slot, int &part)
{
    __syncthreads();                       // every wave is done with the previous item (ring reads, the slot)
    if (threadIdx.x == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        int it = -1;
        for (int v = 0; v < 8 && it < 0; ++v) {
            const int x = (int)((xcc + v) & 7u);
            const int i2 = atomicAdd(P.queue + x * 16, 1);
            const int i = i2 >> P.parts_log2;                // many-rank plans: 2 or 4 queue items per tile
            if (i >= P.items[x]) continue;
            item_slot[2] = i2 & ((1 << P.parts_log2) - 1);
            it = P.items[P.items[8 + x] + i];
        }
        item_slot[0] = it;
    }
    __syncthreads();
    const int it = item_slot[0];
    part = item_slot[2];
    return it;
}

// P.queue == null: one item per block, by the tile map or the arithmetic rule.
__device__ __forceinline__ bool kirch_ring_block_item(const FastParams &P, int &chunk, int &xt)
{
    const int b = blockIdx.x;
    const int xcd = b & 7, r = b >> 3;
    chunk = r / P.tiles_per_xcd;
    const int qx = r - chunk * P.tiles_per_xcd;
    if (chunk >= P.nchunks) return false;
    xt = P.tilemap ? (int)P.tilemap[((size_t)chunk * P.tiles_per_xcd + qx) * 8 + xcd]
                   : ((qx / P.G) * 8 + xcd) * P.G + (qx % P.G);
    if (xt < 0 || xt >= P.nxt) return false;
    return true;
}

// lane -> sample permutation inside a wave.
// ds_read_b128 is serviced in four groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31},
// {32-35,44-47,52-59}, {36-43,48-51,60-63}).  Give every group 16 CONSECUTIVE samples: their
// picks then span < 16 rows and row*11 mod 16 is a bijection, i.e. no bank conflicts.
__device__ __forceinline__ int kirch_ring_sigma(int lane)
{
    const int l32 = lane & 31;
    const int grp = ((l32 >= 4 && l32 < 12) || (l32 >= 16 && l32 < 20) || l32 >= 28) ? 1 : 0;
    const int idx = grp ? (l32 < 12 ? l32 - 4 : (l32 < 20 ? l32 - 8 : l32 - 16))
                        : (l32 < 4 ? l32 : (l32 < 16 ? l32 - 8 : l32 - 12));
    return (lane & 32) + grp * 16 + idx;
}

// The trace offsets nlo .. nhi an item walks (tile 0's: the ring clock.  Tile h is at offset n - h XB and needs the clock
// to run until its own last offset, (NH - 1) XB steps longer); returns true for an empty piece.
// First offset: the S traces a step block adds must be one aligned S-row group of the image
// (ring-relative trace q0 = S blk + XB - 1  ->  x0w + nlo = 1 mod S, i.e. nlo = 1 mod S); the up to
// S - 1 extra leading steps lie outside every aperture of the chunk and pick the all-zero row.
// Plans of 4+ ranks cut every walk into 2 or 4 pieces at fixed offsets (n = 1 and n = 1 -+ U k, U = NB S: whole ring
// revolutions, the same for every tile of a chunk) -- one walk of a shallow chunk is as long as such a rank's whole step
// should be.  A piece writes its sums to its own partial image; kirch_combine_kernel adds the pieces in a fixed order.
// (The arithmetic is kirch_walk_range's, kirch_route.h: the host-side cover of the quad-aligned window walks by it too.  WX: the
// 3 further steps of that window, else 0.)
template <int S, int NB, int XB, int NH, int WX = 0>
__device__ __forceinline__ bool kirch_ring_walk(const FastParams &P, int hmax, int x0w, int part, int &nlo, int &nhi)
{
    return kirch_walk_range(hmax, x0w, P.tnum, S, NB, XB, NH, P.parts_log2, part, WX, nlo, nhi);
}

// Raw buffer over an image, based at the group of trace jbase - 1 (the workgroup's first group), as four scalar words
// (the DMA below is inline asm): base, no stride, 2 GiB range, raw dword format
template <typename T>
__device__ __forceinline__ kq_u4 kirch_ring_desc(const T *img, int jbase, int snum)
{
    const unsigned long long a = (unsigned long long)(img + (ptrdiff_t)(jbase - 1) * snum);
    kq_u4 d;
    d.x = __builtin_amdgcn_readfirstlane((unsigned)a);
    d.y = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);
    d.z = 0x7fffffffu;
    d.w = 0x00020000u;
    return d;
}

// 16 bytes per lane from the buffer (lane offset vo, scalar offset so) straight into LDS at lds_dst + 16 lane.
// The DMA is inline asm on purpose: hipcc treats its own LDS-DMA as a pending LDS write and drains it
// (s_waitcnt vmcnt) in front of the next ds_read, which would expose the whole load latency in
// every block.  Here the order is the kernel's: each wave retires its DMA with the vmcnt wait in front of the
// block's barrier, and the new traces are only read after that barrier.  M0 (the LDS destination)
// is saved and restored inside the statement.
__device__ __forceinline__ void kirch_ring_dma16(unsigned lds_dst, unsigned vo, kq_u4 desc, unsigned so)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lds_dst), "v"(vo), "s"(desc), "s"(so)
                 : "memory");
}

// sum of the pieces of every aperture walk, in piece order (many-rank plans, see kirch_quad_kernel)
template <typename T, int K>
__global__ __launch_bounds__(256) void kirch_combine_kernel(const T *__restrict__ partial, T *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T v = partial[i] + partial[n + i];
    if (K == 4) v = (v + partial[2 * n + i]) + partial[3 * n + i];
    out[i] = v;
}

// The tile map of a launch (kirch_tilemap, kirch_route.h), kept with the plan under the key it was built for.
static int build_tilemap(impdar_kirch_plan *p, FastParams &P, int tile_w, int align_mask, int ring_blocks, int step_block,
                         hipStream_t st)
{
    P.tilemap = nullptr;
    const int key[5] = {P.xlo, P.xhi, tile_w, P.G, P.tiles_per_xcd};
    const size_t n = (size_t)P.nchunks * P.tiles_per_xcd * 8;
    if (memcmp(key, p->tm_key, sizeof(key)) != 0 || p->h_tilemap.size() != n) {
        std::vector<short> map = kirch_tilemap(p->h_hmax, p->tnum, P.xlo, P.xhi, tile_w, align_mask, ring_blocks, step_block, P.G,
                                               P.tiles_per_xcd, P.nchunks, p->window);
        if (map.empty()) return IMPDAR_OK;
        p->h_tilemap.swap(map);
        memcpy(p->tm_key, key, sizeof(key));
        IMPDAR_HIP_CHECK(p->d_tilemap.ensure(n * sizeof(short)));
        IMPDAR_HIP_CHECK(hipMemcpyAsync(p->d_tilemap.p, p->h_tilemap.data(), n * sizeof(short), hipMemcpyHostToDevice, st));
    }
    P.tilemap = p->d_tilemap.as<short>();
    return IMPDAR_OK;
}

// The queue lists of a launch (kirch_gangmap, kirch_route.h) in the layout of FastParams::items, kept with the plan under the
// key they were built for: the output block, the tile width and the plan's two queue knobs as this launch resolves them.
static int build_gangmap(impdar_kirch_plan *p, FastParams &P, int tile_w, int align_mask, int ring_blocks, int step_block, hipStream_t st)
{
    P.items = nullptr;
    const int key[5] = {P.xlo, P.xhi, tile_w, kirch_gang_size(*p, P.nxt), kirch_queue_order(*p, P.nxt)};
    if (memcmp(key, p->gm_key, sizeof(key)) != 0 || p->h_items.empty()) {
        const KirchGangMap M = kirch_gangmap(p->h_hmax, p->tnum, P.xlo, P.xhi, tile_w, align_mask, ring_blocks, step_block, key[3], key[4], P.nchunks, p->window);
        if (M.items() == 0) return IMPDAR_OK;
        std::vector<int> flat(16);
        for (int x = 0; x < 8; ++x) {
            flat[x] = (int)M.list[x].size();
            flat[8 + x] = (int)flat.size();
            flat.insert(flat.end(), M.list[x].begin(), M.list[x].end());
        }
        p->h_items.swap(flat);
        memcpy(p->gm_key, key, sizeof(key));
        IMPDAR_HIP_CHECK(p->d_items.ensure(p->h_items.size() * sizeof(int)));
        IMPDAR_HIP_CHECK(hipMemcpyAsync(p->d_items.p, p->h_items.data(), p->h_items.size() * sizeof(int), hipMemcpyHostToDevice, st));
    }
    P.items = p->d_items.as<int>();
    return IMPDAR_OK;
}

// Workgroup slots the persistent ring kernels leave EMPTY in a multi-rank plan.  They launch exactly as many
// workgroups as are resident at once and keep them until the diffraction sum ends; RCCL's send/recv and all-gather
// are kernels too (ncclDevKernel_Generic: workgroups of their own, with LDS).  Measured on one GPU with a rank of an
// 8-rank plan emulated and its exchange done as a self send/recv (profiles/r03_exchange_overlap.txt, kernel trace
// profiles/r03_exchange_trace_*.txt): queued on the producer stream behind a full chip the RCCL kernel is dispatched
// 0.1 ms into the diffraction sum but ENDS with it (4.5 of 4.7 ms; 1.06 of 1.08 ms) -- the exchange of radargram
// s+1 serialises behind the sum of radargram s instead of hiding under it.  With 32 of the 512 slots left free it
// completes in 0.15-0.3 ms while the sum runs (8 and 16 free slots do not change anything); the diffraction sum pays
// 2.7-2.9 % (4.665 -> 4.800 ms, 1.081 -> 1.110 ms), 5.7 % with 64.  IMPDAR_KIRCH_RESERVE=<R> overrides (0: none).
#ifndef KQ_DEFAULT_RESERVE
#define KQ_DEFAULT_RESERVE 32
#endif
static int kirch_reserved_slots(const impdar_kirch_plan *p)
{
    const char *re = getenv("IMPDAR_KIRCH_RESERVE");
    const int r = re ? atoi(re) : (p->nranks > 1 ? KQ_DEFAULT_RESERVE : 0);
    return std::min(std::max(r, 0), 256);
}

// the pieces of every walk of a many-rank plan, summed in piece order
template <typename T>
static void kirch_launch_combine(const FastParams &P, hipStream_t st)
{
    const size_t nout = (size_t)P.snum * P.ldo;
    const dim3 cg((unsigned)((nout + 255) / 256));
    if (P.parts_log2 == 2)
        hipLaunchKernelGGL((kirch_combine_kernel<T, 4>), cg, dim3(256), 0, st, (const T *)P.partial, (T *)P.out, nout);
    else
        hipLaunchKernelGGL((kirch_combine_kernel<T, 2>), cg, dim3(256), 0, st, (const T *)P.partial, (T *)P.out, nout);
}

// The pick table of the ring kernels depends on the plan's geometry only (like an FFT plan's twiddles): it is built by the
// first prep into each of the two buffer sets and kept.  (Round 1 rebuilt it with every prep -- 0.06-0.13 ms on the producer
// stream, hidden behind a whole-radargram diffraction sum but a tenth of the step of an 8-rank block.)
// `kernel`: kirch_tableq_kernel or kirch_tabled_kernel; piece_bytes: of the plan's ring (kq_piece_bytes_lk / kd_piece_bytes).
template <typename Kernel>
static int prep_table_ring(impdar_kirch_plan *p, int b, hipStream_t st, Kernel kernel, int piece_bytes)
{
    if (p->table_built[b]) return IMPDAR_OK;
    p->table_built[b] = true;
    ++p->diag_tables_built;
    TableQParams T;
    T.TKB = p->d_TK[b].as<uint4>();
    kirch_fill_axes(T, p);
    T.dx = p->dx;
    T.nrows = p->nrows;
    T.mrow0 = p->mrow0;
    T.nmax = p->ntab - 1;
    T.wmod = p->quadW;
    T.sh = p->quadSH;
    T.ps = piece_bytes;
    // rows a + mrow0 (a >= 0) and mrow0 - a - 1: a runs over the larger of the two sides
    const int na = std::max(p->nrows - p->mrow0, p->mrow0);
    hipLaunchKernelGGL(kernel, dim3((p->snum + 255) / 256, na), dim3(256), 0, st, T);
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

// What launch_ring needs of a ring kernel's instantiation K (RingF32 / RingF64 of the two units): the element type, the kernel
// in its near-field (one tile per workgroup, one workgroup per CU) and far-field forms, where tiles may start, and the ring
// as the tile map's cost model sees it; its window kind and, for KIRCH_WINDOW_QUAD, the launch of the fix-up behind the kernel.
template <typename K>
static int launch_ring(impdar_kirch_plan *p, const FastParams &P0, hipStream_t st)
{
    constexpr int XB = K::XB, NH = K::NH;
    FastParams P = P0;
    // workgroup tiles start at a multiple of 8 (4); under the quad-aligned window at multiples of the workgroup tile, and the
    // tile right of the block's last column is part of the launch (kirch_tile_origin, kirch_tile_count)
    const int window = K::window;
    const int ntiles = kirch_tile_count(P.xlo, P.xhi, XB * NH, K::align_mask, window);
    P.nxt = ntiles;
    P.x00 = kirch_tile_origin(P.xlo, XB * NH, K::align_mask, window);
    // P.G: the groups of the one-item-per-block launch (tile map / arithmetic rule) and the padding of its grid.
    // Groups of 4 adjacent tiles per XCD share staging lines in L2 (same-box A/B at config 3 with 250 tiles of 40: 1.2-1.6 %
    // faster than 1, L2 misses -36 %; 6 / 8 / 12 are slower), but with blocks dealt statically the XCDs only stay balanced
    // when each gets many groups: with the 45-70 tiles of an 8-rank block groups of 4 leave half of the XCDs with twice
    // the work (-16 %).  The persistent launch has its own gangs and order: kirch_gang_size, kirch_gangmap
    // (profiles/kirch_gangs.txt).
    P.G = ntiles >= 256 ? 4 : 1;
    const int per = 8 * P.G;
    const int nxt_pad = ((ntiles + per - 1) / per) * per;
    P.tiles_per_xcd = nxt_pad / 8;
    const int nblk = P.nchunks * nxt_pad;
    const int W = p->quadW;
    {
        const int trc = build_tilemap(p, P, XB * NH, K::align_mask, K::ring_blocks, K::step_block, st);
        if (trc) return trc;
    }
    const size_t shmem = (size_t)(W / 32) * K::piece_bytes * (p->nearfield ? 2 : 1) + 16;   // + the item slot
    if (p->nearfield) {
        auto k = K::near_kernel();
        IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL(k, dim3(nblk), dim3(KF_THREADS), shmem, st, P, W);
        IMPDAR_HIP_CHECK(hipGetLastError());
        return IMPDAR_OK;
    }
    auto k = K::far_kernel();
    IMPDAR_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    int grid = nblk;
    if (window == KIRCH_WINDOW_QUAD) {
        // the side sums of every tile of the launch, per piece of a walk; an empty piece writes none, so they start as zeros
        const size_t np = (size_t)1 << (NH == 1 ? p->walk_parts_log2 : 0), side = (size_t)ntiles * NH * 3 * P.snum;
        if (p->d_side_l.ensure(side * np * sizeof(float)) != hipSuccess || p->d_side_r.ensure(side * np * sizeof(float)) != hipSuccess) {
            impdar_set_error("hipMalloc of the %zu-byte side sums failed", side * np * sizeof(float));
            return IMPDAR_ERR_HIP;
        }
        P.side_l = p->d_side_l.as<float>();
        P.side_r = p->d_side_r.as<float>();
        P.side_stride = side;
        if (np > 1) {
            IMPDAR_HIP_CHECK(hipMemsetAsync(p->d_side_l.p, 0, side * np * sizeof(float), st));
            IMPDAR_HIP_CHECK(hipMemsetAsync(p->d_side_r.p, 0, side * np * sizeof(float), st));
        }
    }
    if (P.tilemap) {
        // persistent workgroups: as many as are resident at once, each pulling items from the per-XCD queues
        if (p->slots <= 0) {        // resident workgroups of this plan's kernel on this device: asked once
            int per_cu = 0, ncu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k, KF_THREADS * NH, shmem) == hipSuccess &&
                hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, p->ctx->device) == hipSuccess &&
                per_cu > 0 && ncu > 0)
                p->slots = per_cu * ncu;
            else
                (void)hipGetLastError();
        }
        // many-rank plans: every walk in 2 or 4 pieces with partial images of their own (p->walk_parts_log2)
        const int pl2 = NH == 1 ? p->walk_parts_log2 : 0;
        const size_t nout = (size_t)P.snum * P.ldo, esz = impdar_dtype_size(p->dtype);
        const bool pieces = pl2 > 0 && p->slots > 0 && p->d_partial.ensure((nout << pl2) * esz) == hipSuccess;
        if (p->slots > 0 && (p->slots < nblk || pieces)) {
            const int grc = build_gangmap(p, P, XB * NH, K::align_mask, K::ring_blocks, K::step_block, st);
            if (grc) return grc;
        }
        if (P.items && p->d_queue.ensure(8 * 64) == hipSuccess) {
            IMPDAR_HIP_CHECK(hipMemsetAsync(p->d_queue.p, 0, 8 * 64, st));
            P.queue = p->d_queue.as<int>();
            if (pieces) {
                P.parts_log2 = pl2;
                P.partial = p->d_partial.p;
                P.part_stride = nout;
                // a piece no workgroup reaches (tiles beyond the block's end) must read as zero
                IMPDAR_HIP_CHECK(hipMemsetAsync(p->d_partial.p, 0, (nout << pl2) * esz, st));
            }
            grid = (int)std::min<long long>(std::max(p->slots - kirch_reserved_slots(p), 1), (long long)nblk << P.parts_log2);
        }
    }
    hipLaunchKernelGGL(k, dim3(grid), dim3(KF_THREADS * NH), shmem, st, P, W);
    // the columns two tiles share under the quad-aligned window (kirch_fixup_kernel), in front of the sum of the pieces
    if constexpr (K::window == KIRCH_WINDOW_QUAD)
        if (ntiles * NH > 1) K::launch_fixup(P, ntiles * NH, st);
    if (P.parts_log2) kirch_launch_combine<typename K::elem>(P, st);      // (a ring's element type is its plan's dtype)
    IMPDAR_HIP_CHECK(hipGetLastError());
    return IMPDAR_OK;
}

// the plan's tables and buffer set and the output block [xlo, xhi) as a ring launch takes them
static FastParams kirch_ring_params(impdar_kirch_plan *p, void *d_out, int xlo, int xhi)
{
    const int b = p->buf, nx = xhi - xlo;
    FastParams P;
    P.GT = reinterpret_cast<const float *>(img_row0(p, p->GT[b]));
    P.DT = p->nearfield ? reinterpret_cast<const float *>(img_row0(p, p->DT[b])) : nullptr;
    P.out = reinterpret_cast<float *>(d_out);
    P.ldo = nx;
    P.snum = p->snum;
    P.tnum = p->tnum;
    P.xlo = xlo;
    P.xhi = xhi;
    P.hmax = p->d_hmax.as<int>();
    P.klo = p->d_klo.as<int>();
    P.khi = p->d_khi.as<int>();
    P.nb = p->nb;
    P.zero_row = p->tnum_pad;          // first zero row after the data rows
    P.nchunks = p->nchunks;
    P.TK = p->d_TK[b].as<unsigned short>();
    P.TW = p->d_TW[b].as<float>();
    P.TW2 = p->d_TW2[b].as<float>();
    P.ntab = p->ntab;
    P.c1 = p->d_c1.as<float>();
    P.c2 = p->d_c2.as<float>();
    P.fin = p->d_fin.as<float>();
    P.c1d = p->d_c1d.as<double>();
    P.c2d = p->d_c2d.as<double>();
    P.find = p->d_find.as<double>();
    P.TKB = p->d_TK[b].p;
    P.WIN = p->d_WIN.as<int2>();
    P.nrows = p->nrows;
    P.mrow0 = p->mrow0;
    P.tilemap = nullptr;
    P.queue = nullptr;
    P.items = nullptr;
    P.x00 = 0;
    P.side_l = P.side_r = nullptr;
    P.side_stride = 0;
    P.parts_log2 = 0;
    P.partial = nullptr;
    P.part_stride = 0;
    return P;
}
