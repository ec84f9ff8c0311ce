// Layer slopes of a (snum, tnum) radargram (slope.hip; an extension: the reference has no slope field): the structure-tensor
// dip field and the dip-steered mean.  This header holds the contract, every refusal with its reason, the weight table, every
// block size and the launch geometry, LDS bytes and scratch sizes of each pass.  Plain C++, no HIP include: compiled into the
// library by slope.hip and, by itself with g++, into the CPU suite's checker (tests/test_slope_route.py).  slope.hip decides
// nothing that this header does not.
//
// THE CONTRACT.  n = snum, m = tnum, x[k][j] is sample k of trace j; float64 arithmetic for both dtypes.
//   1. load       a sample that is not finite is read as NaN; from there NaN propagates by IEEE arithmetic alone (no flag pass).
//   2. gradients  in index units: gz[k][j] = (x[k+1][j] - x[k-1][j]) / 2 inside, x[1] - x[0] and x[n-1] - x[n-2] at the two ends,
//                 0 on an axis of length 1; gx the same along the traces (np.gradient where that is defined).
//   3. products   A = gz gz, B = gz gx, C = gx gx.
//   4. smoothing  each product by a separable Gaussian, sigma_x along the traces FIRST, then sigma_z along the samples.  Radius
//                 r = int(4 sigma + 0.5), weights w[i] = e[i] / sum e, e[i] = exp(-i^2 / (2 sigma^2)), -r <= i <= r, made on the
//                 host (slope_weights: e in float64, its sum with i rising and the quotients in long double, each weight rounded
//                 to float64 once) and uploaded as a table.  Each pass is
//                 (s, t) = (0, 0); for i = -r .. r rising: the exact product w[i] * P[clamp(index + i)] is added to the two-term
//                 float64 sum (s, t) -- the product's rounding error from one fused multiply-add, the sum's from Knuth's two-sum,
//                 both collected in t -- and the pass gives s + t, rounded once; the index is clamped to the axis
//                 (mode='nearest').  A pass is therefore the correctly rounded weighted sum but for a second-order term, in an
//                 order fixed by r alone.  sigma = 0: r = 0, w = {1}, the axis is left alone, bit for bit.  Products that
//                 overflow give a value that is not finite, not necessarily an infinity.
//                 So two calls give the same bits, and an output sample whose unclamped window lies inside the radargram gets the
//                 same bits from any radargram that contains that window.  a, b, c are the smoothed A, B, C;
//                 d = a - c, D = sqrt(d d + 4 b b).
//   5. kinds      float64 (snum, tnum) fields for either data dtype:
//                 0 slope      p = -2b / (d + D) where d >= 0, p = -(D - d) / (2b) where d < 0, p = 0 where D = 0, then clamped to
//                              [-max_slope, max_slope] (samples per trace along the layer; each form where it does not cancel)
//                 1 dip        atan2(-2b, d) / 2 in radians, not clamped (tan(dip) is the unclamped slope)
//                 2 coherence  D / (a + c) where a + c > 0, else 0: (l1 - l2) / (l1 + l2) of the tensor's eigenvalues, in [0, 1]
//                 3 jzz a, 4 jzx b, 5 jxx c
//                 a NaN in a, b or c gives NaN in kinds 0 .. 2 (said in code where a comparison would drop it).
//   6. dipsmooth  half = h.  With p = slope[k][j] at the centre: y[k][j] = (sum_i v_i) / (number of i summed), i rising from -h to h
//                 over the i with 0 <= j + i < m; v_i the linear interpolation of trace j + i at s = min(max(k + p i, 0), n - 1):
//                 k0 = floor(s), k1 = min(k0 + 1, n - 1), f = s - k0, v = x[k0] + f (x[k1] - x[k0]).  A NaN p gives a NaN y (said
//                 in code: fmin / fmax drop a NaN).  y is rounded once to the radargram's dtype.  The slope is a float64
//                 (snum, tnum) array of the caller's or, with none given, kind 0 of this radargram at (sigma_z, sigma_x,
//                 max_slope), computed first, in float64 and never rounded.  In place (d_out == d_data) the gather writes a
//                 scratch copy that is copied over the data afterwards: the same bits as out of place.
//   7. refused before any device work (IMPDAR_ERR_ARG, the reason below): an unknown kind; a sigma that is not finite, negative
//      or above 16 (r <= 64); a max_slope that is not finite or not positive; half outside 1 .. 32; an empty radargram; another
//      dtype; a shape whose grid would pass 2^31 blocks.
//   8. flags are left alone; no floating-point atomics; no environment variable.
//
// THE PASSES.  The radargram keeps its [snum][tnum] layout; nothing is transposed.
//   row pass     one workgroup of SLOPE_ROW_TX threads per row k and block of SLOPE_ROW_TX traces: the products at the
//                SLOPE_ROW_TX + 2 r_x clamped trace indices of its window go into LDS (each from x[k-1], x[k+1] and the two
//                neighbours in row k, indices clamped or one-sided as rule 2 says), then every thread sums one trace's window and
//                writes the three float64 planes.
//   column pass  one workgroup of SLOPE_COL_THREADS threads per SLOPE_COL_SEG x SLOPE_COL_TX tile: plane after plane, the
//                (SLOPE_COL_SEG + 2 r_z) x SLOPE_COL_TX rows of the tile with clamped row indices go into LDS, every thread sums
//                SLOPE_COL_SEG / SLOPE_COL_GROUPS samples of one trace; then the 2 x 2 eigen-analysis and the float64 field.
//   gather       one output sample per thread, SLOPE_GATHER_THREADS per workgroup.
#pragma once
#include <cmath>
#include <cstddef>

enum { SLOPE_KIND_SLOPE = 0, SLOPE_KIND_DIP = 1, SLOPE_KIND_COHERENCE = 2, SLOPE_KIND_JZZ = 3, SLOPE_KIND_JZX = 4, SLOPE_KIND_JXX = 5 };
enum {
    SLOPE_MAX_R = 64,               // int(4 * 16 + 0.5)
    SLOPE_MAX_HALF = 32,
    SLOPE_ROW_TX = 256,             // row pass: traces (and threads) per workgroup
    SLOPE_COL_TX = 32,              // column pass: traces per tile
    SLOPE_COL_SEG = 64,             //              samples per tile
    SLOPE_COL_GROUPS = 8,           //              row groups of a workgroup: SLOPE_COL_SEG / SLOPE_COL_GROUPS samples per thread
    SLOPE_COL_THREADS = SLOPE_COL_TX * SLOPE_COL_GROUPS,
    SLOPE_COL_PER_THREAD = SLOPE_COL_SEG / SLOPE_COL_GROUPS,
    SLOPE_GATHER_THREADS = 256,
    SLOPE_LDS_MAX = 160 * 1024
};
constexpr double SLOPE_MAX_SIGMA = 16.0;

static inline bool slope_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

static inline const char *slope_sigma_refusal(double sigma_z, double sigma_x, double max_slope)
{
    if (!(slope_finite(sigma_z) && sigma_z >= 0.0 && sigma_z <= SLOPE_MAX_SIGMA) || !(slope_finite(sigma_x) && sigma_x >= 0.0 && sigma_x <= SLOPE_MAX_SIGMA))
        return "sigma must be finite and lie in 0 .. 16";
    if (!(slope_finite(max_slope) && max_slope > 0.0)) return "max_slope must be finite and positive";
    return nullptr;
}

static inline const char *slope_shape_refusal(int snum, int tnum)
{
    if (snum < 1 || tnum < 1) return "empty radargram";
    const long long bx = ((long long)tnum + SLOPE_ROW_TX - 1) / SLOPE_ROW_TX;
    const long long cx = ((long long)tnum + SLOPE_COL_TX - 1) / SLOPE_COL_TX, cz = ((long long)snum + SLOPE_COL_SEG - 1) / SLOPE_COL_SEG;
    const long long g = ((long long)snum * tnum + SLOPE_GATHER_THREADS - 1) / SLOPE_GATHER_THREADS;
    if (bx * snum >= (1LL << 31) || cx * cz >= (1LL << 31) || g >= (1LL << 31)) return "radargram too large: a grid would pass 2^31 blocks";
    return nullptr;
}

// Null for a call impdar_slope takes, else what is wrong with it.
static inline const char *slope_refusal(int snum, int tnum, int kind, double sigma_z, double sigma_x, double max_slope)
{
    if (kind < SLOPE_KIND_SLOPE || kind > SLOPE_KIND_JXX) return "kind must be 0 (slope), 1 (dip), 2 (coherence), 3 (jzz), 4 (jzx) or 5 (jxx)";
    if (const char *why = slope_sigma_refusal(sigma_z, sigma_x, max_slope)) return why;
    return slope_shape_refusal(snum, tnum);
}

// ... and for impdar_dipsmooth; the sigmas and max_slope are read only when no slope is given
static inline const char *dipsmooth_refusal(int snum, int tnum, int half, bool given, double sigma_z, double sigma_x, double max_slope)
{
    if (half < 1 || half > SLOPE_MAX_HALF) return "half must lie in 1 .. 32";
    if (!given)
        if (const char *why = slope_sigma_refusal(sigma_z, sigma_x, max_slope)) return why;
    return slope_shape_refusal(snum, tnum);
}

static inline int slope_radius(double sigma) { return (int)(4.0 * sigma + 0.5); }

// the 2 r + 1 weights of rule 4 into w (room for 2 SLOPE_MAX_R + 1), r into *r
static inline void slope_weights(double sigma, double *w, int *r)
{
    const int R = slope_radius(sigma);
    *r = R;
    if (R == 0) {
        w[0] = 1.0;
        return;
    }
    // e in float64; its sum and the quotients in long double, each quotient rounded once: the table then sums to 1 within
    // the roundings of its entries alone, and a plane that is constant along the axis comes out of the pass as it went in
    long double sum = 0.0L;
    for (int i = -R; i <= R; ++i) {
        w[i + R] = std::exp(-(double)(i * i) / (2.0 * sigma * sigma));
        sum += (long double)w[i + R];
    }
    for (int i = 0; i <= 2 * R; ++i) w[i] = (double)((long double)w[i] / sum);
}

struct SlopeRoute {
    int rz = 0, rx = 0;
    long long row_blocks_x = 0, row_blocks = 0;                     // blocks of traces per row; workgroups of the row pass
    size_t row_lds = 0;
    long long col_blocks_x = 0, col_blocks_z = 0, col_blocks = 0;   // tiles along the traces, along the samples; workgroups
    size_t col_lds = 0;
    long long gather_blocks = 0;
    // scratch in bytes: the three float64 planes; the float64 slope field of a dipsmooth with no slope given; the copy an
    // in-place dipsmooth gathers into (of the data's dtype: `elem` bytes per sample)
    size_t plane_bytes = 0, field_bytes = 0, inplace_bytes = 0;
    bool ok = false;
};

// for a shape and sigmas the refusals have passed; elem: bytes per sample of the data
static inline SlopeRoute slope_route(int snum, int tnum, double sigma_z, double sigma_x, size_t elem)
{
    SlopeRoute S;
    S.rz = slope_radius(sigma_z);
    S.rx = slope_radius(sigma_x);
    if (S.rz > SLOPE_MAX_R || S.rx > SLOPE_MAX_R || slope_shape_refusal(snum, tnum)) return S;
    S.row_blocks_x = ((long long)tnum + SLOPE_ROW_TX - 1) / SLOPE_ROW_TX;
    S.row_blocks = S.row_blocks_x * snum;
    S.row_lds = (size_t)3 * (SLOPE_ROW_TX + 2 * S.rx) * sizeof(double);
    S.col_blocks_x = ((long long)tnum + SLOPE_COL_TX - 1) / SLOPE_COL_TX;
    S.col_blocks_z = ((long long)snum + SLOPE_COL_SEG - 1) / SLOPE_COL_SEG;
    S.col_blocks = S.col_blocks_x * S.col_blocks_z;
    S.col_lds = (size_t)(SLOPE_COL_SEG + 2 * S.rz) * SLOPE_COL_TX * sizeof(double);
    S.gather_blocks = ((long long)snum * tnum + SLOPE_GATHER_THREADS - 1) / SLOPE_GATHER_THREADS;
    const size_t count = (size_t)snum * (size_t)tnum;
    S.plane_bytes = 3 * count * sizeof(double);
    S.field_bytes = count * sizeof(double);
    S.inplace_bytes = count * elem;
    S.ok = S.row_lds <= (size_t)SLOPE_LDS_MAX && S.col_lds <= (size_t)SLOPE_LDS_MAX;
    return S;
}

#ifdef SLOPE_ROUTE_PROBE
// what tests/test_slope_route.py calls.  ints[8]: rz, rx, ok, row threads, column threads, gather threads, column tile traces,
// column tile samples; longs[11]: row_blocks_x, row_blocks, row_lds, col_blocks_x, col_blocks_z, col_blocks, col_lds, gather_blocks,
// plane_bytes, field_bytes, inplace_bytes
extern "C" const char *slope_probe_refusal(int snum, int tnum, int kind, double sigma_z, double sigma_x, double max_slope)
{
    return slope_refusal(snum, tnum, kind, sigma_z, sigma_x, max_slope);
}
extern "C" const char *dipsmooth_probe_refusal(int snum, int tnum, int half, int given, double sigma_z, double sigma_x, double max_slope)
{
    return dipsmooth_refusal(snum, tnum, half, given != 0, sigma_z, sigma_x, max_slope);
}
extern "C" int slope_probe_weights(double sigma, double *w)
{
    int r = 0;
    slope_weights(sigma, w, &r);
    return r;
}
extern "C" int slope_probe_route(int snum, int tnum, double sigma_z, double sigma_x, int elem, int *ints, long long *longs)
{
    const SlopeRoute S = slope_route(snum, tnum, sigma_z, sigma_x, (size_t)elem);
    const int i[8] = {S.rz, S.rx, S.ok ? 1 : 0, SLOPE_ROW_TX, SLOPE_COL_THREADS, SLOPE_GATHER_THREADS, SLOPE_COL_TX, SLOPE_COL_SEG};
    const long long l[11] = {S.row_blocks_x, S.row_blocks, (long long)S.row_lds, S.col_blocks_x, S.col_blocks_z, S.col_blocks, (long long)S.col_lds,
                             S.gather_blocks, (long long)S.plane_bytes, (long long)S.field_bytes, (long long)S.inplace_bytes};
    for (int k = 0; k < 8; ++k) ints[k] = i[k];
    for (int k = 0; k < 11; ++k) longs[k] = l[k];
    return S.ok ? 1 : 0;
}
#endif
