// The host-side decisions of the display unit (display.hip): the ranks of a percentile, how many histogram passes a dtype
// takes, the launch shape over a window, and the step from one pass's histograms to the next pass's prefixes -- plain
// C++, no HIP include, compiled by itself in tests/test_display_cpu.py.  display.hip decides nothing that this header does not.
//
// Order statistics are a radix select on order-preserving integer keys (disp_key32 / disp_key64: negatives have all bits
// flipped, non-negatives the top bit set), most significant digit first, DISP_DIGIT_BITS bits per pass.  A rank is followed
// as (prefix, rank within the prefix): the digits found so far and the position among the elements that carry them.  Ranks
// with the same prefix share one histogram, so a pass holds at most DISP_MAX_RANKS of them.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

enum {
    DISP_MAX_Q = 8,                     // percentages of one call
    DISP_MAX_RANKS = 2 * DISP_MAX_Q,    // a lower and an upper rank each
    DISP_DIGIT_BITS = 8,
    DISP_BINS = 1 << DISP_DIGIT_BITS,
    DISP_THREADS = 256,                 // one thread per bin when a workgroup merges its histograms
    DISP_MAX_WGS = 2048,                // 256 compute units x 8
    DISP_HIST_WORDS = DISP_MAX_RANKS * DISP_BINS + 1    // 64-bit counters of one pass: the histograms, then the NaN count
};

constexpr int disp_passes(int key_bits) { return key_bits / DISP_DIGIT_BITS; }

static inline uint32_t disp_key32(float v)
{
    uint32_t b;
    memcpy(&b, &v, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static inline float disp_unkey32(uint32_t k)
{
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    memcpy(&v, &b, 4);
    return v;
}
static inline uint64_t disp_key64(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
static inline double disp_unkey64(uint64_t k)
{
    const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &b, 8);
    return v;
}

// NumPy's linear method: the virtual index (n - 1) * (q / 100) in float64, its floor, and the neighbour above clipped to n - 1
static inline void disp_ranks(long long n, double q, long long *lo, long long *hi)
{
    const double v = (double)(n - 1) * (q / 100.0);
    long long l = (long long)std::floor(v);
    if (l < 0) l = 0;
    if (l > n - 1) l = n - 1;
    *lo = l;
    *hi = l + 1 < n - 1 ? l + 1 : n - 1;
}

// The window [y0, y1) x [x0, x1) as rows of `units` accesses of V elements; a workgroup of DISP_THREADS threads is
// (1 << log_tx) accesses wide and DISP_THREADS >> log_tx rows high, grid_x of them cover a row and grid_y of them stride over the
// rows.  per_wg bounds the elements one workgroup counts (its LDS counters are 32 bits).
struct DispGrid {
    int log_tx = 0, grid_x = 0, grid_y = 0;
    long long rows = 0, units = 0, per_wg = 0;
    bool ok = false;
};

static inline DispGrid disp_grid(long long rows, long long width, int V)
{
    DispGrid G;
    if (rows < 1 || width < 1 || V < 1 || width % V) return G;
    G.rows = rows;
    G.units = width / V;
    while ((1 << G.log_tx) < DISP_THREADS && (1LL << G.log_tx) < G.units) ++G.log_tx;
    const long long tx = 1LL << G.log_tx, ty = DISP_THREADS / tx;
    const long long gx = (G.units + tx - 1) / tx, row_blocks = (rows + ty - 1) / ty;
    if (gx > 0x7fffffffLL) return G;
    long long gy = DISP_MAX_WGS / gx;
    if (gy < 1) gy = 1;
    if (gy > row_blocks) gy = row_blocks;
    if (gy > 65535) gy = 65535;
    G.grid_x = (int)gx;
    G.grid_y = (int)gy;
    const long long rows_per_wg = ((row_blocks + gy - 1) / gy) * ty;
    G.per_wg = rows_per_wg * tx * V;
    G.ok = G.per_wg < (1LL << 32);
    return G;
}

// What the select follows from pass to pass.  group[r]: which of the ngroups distinct prefixes rank r carries.
struct DispSelect {
    int nranks = 0, ngroups = 0;
    uint64_t prefix[DISP_MAX_RANKS] = {};     // per group
    long long rank[DISP_MAX_RANKS] = {};      // per rank: its position among the elements of its prefix
    int group[DISP_MAX_RANKS] = {};
};

// before the first pass: every rank carries the empty prefix
static inline void disp_select_start(DispSelect &S, const long long *ranks, int nranks)
{
    S.nranks = nranks;
    S.ngroups = 1;
    S.prefix[0] = 0;
    for (int r = 0; r < nranks; ++r) {
        S.rank[r] = ranks[r];
        S.group[r] = 0;
    }
}

// hist[g][b]: how many elements of group g's prefix have digit b.  Every rank moves into the bin that holds it; the ranks
// are regrouped by their new prefixes.  False where a rank lies beyond its histogram (the counts disagree with n).
static inline bool disp_select_step(DispSelect &S, const uint64_t *hist)
{
    uint64_t np[DISP_MAX_RANKS];
    for (int r = 0; r < S.nranks; ++r) {
        const uint64_t *h = hist + (size_t)S.group[r] * DISP_BINS;
        uint64_t below = 0;
        int b = 0;
        while (b < DISP_BINS && below + h[b] <= (uint64_t)S.rank[r]) below += h[b++];
        if (b == DISP_BINS) return false;
        S.rank[r] -= (long long)below;
        np[r] = (S.prefix[S.group[r]] << DISP_DIGIT_BITS) | (uint64_t)b;
    }
    S.ngroups = 0;
    for (int r = 0; r < S.nranks; ++r) {
        int g = 0;
        while (g < S.ngroups && S.prefix[g] != np[r]) ++g;
        if (g == S.ngroups) S.prefix[S.ngroups++] = np[r];
        S.group[r] = g;
    }
    return true;
}

#ifdef DISPLAY_ROUTE_PROBE
// what tests/test_display_cpu.py calls: the whole select on a host array of keys, pass by pass, with the histograms counted
// here -- the library's host code around a stand-in for its kernel
extern "C" int impdar_display_ranks_probe(long long n, double q, long long *lo, long long *hi)
{
    disp_ranks(n, q, lo, hi);
    return 0;
}
extern "C" int impdar_display_grid_probe(long long rows, long long width, int V, long long *out)
{
    const DispGrid G = disp_grid(rows, width, V);
    out[0] = G.log_tx;
    out[1] = G.grid_x;
    out[2] = G.grid_y;
    out[3] = G.per_wg;
    return G.ok ? 0 : 1;
}
extern "C" int impdar_display_select_probe(const double *vals, long long n, int as_f32, const long long *ranks, int nranks, double *out)
{
    const int bits = as_f32 ? 32 : 64;
    DispSelect S;
    disp_select_start(S, ranks, nranks);
    static uint64_t hist[DISP_MAX_RANKS * DISP_BINS];
    for (int p = 0; p < disp_passes(bits); ++p) {
        const int shift = bits - DISP_DIGIT_BITS * (p + 1);
        memset(hist, 0, sizeof(hist));
        for (long long i = 0; i < n; ++i) {
            const uint64_t k = as_f32 ? (uint64_t)disp_key32((float)vals[i]) : disp_key64(vals[i]);
            for (int g = 0; g < S.ngroups; ++g)
                if (p == 0 || (k >> (shift + DISP_DIGIT_BITS)) == S.prefix[g]) ++hist[g * DISP_BINS + ((k >> shift) & (DISP_BINS - 1))];
        }
        if (!disp_select_step(S, hist)) return 1;
    }
    for (int r = 0; r < nranks; ++r)
        out[r] = as_f32 ? (double)disp_unkey32((uint32_t)S.prefix[S.group[r]]) : disp_unkey64(S.prefix[S.group[r]]);
    return 0;
}
#endif
