// What a deconvolution or autocorrelation call (decon.hip) decides on the host before its first HIP call: whether its arguments
// are a call at all (the reason is the text of the argument error), the lag table, and the plan -- grids, workgroup sizes,
// dynamic LDS, scratch bytes and the kernel string of the metrics line.  Plain C++, no device code: compiled into the library
// by decon.hip and, by itself with g++, into the CPU suite's checker (tests/test_decon_route.py).  No launch argument is
// computed anywhere else.
#pragma once
#include "decon_core.h"

constexpr int DECON_TG = 32;                       // traces of a workgroup of the two sliding kernels: lane % 32 is the trace
constexpr int DECON_SLICES = 8;                    // ... and lane / 32 one of 8 runs of DECON_LPT lags (or output samples)
constexpr int DECON_LPT = DECON_C / DECON_SLICES;  // 8
constexpr int DECON_THREADS = DECON_TG * DECON_SLICES;
constexpr int DECON_SOLVE_TRACES = 64 / DECON_G;   // traces of one (single-wave) workgroup of the recursion
static_assert(DECON_LPT * DECON_SLICES == DECON_C && DECON_G * DECON_SOLVE_TRACES == 64, "decon tiles");

static inline bool decon_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

// Null for a window every call takes, else what is wrong with it.
static inline const char *decon_window_refusal(int snum, int tnum, int s0, int s1)
{
    if (snum < 1 || tnum < 1) return "empty radargram";
    if (!(0 <= s0 && s0 < s1 && s1 <= snum)) return "the window must satisfy 0 <= s0 < s1 <= snum";
    return nullptr;
}
// Null for a deconvolution the entries take, else what is wrong with it.
static inline const char *decon_refusal(int snum, int tnum, int s0, int s1, int oplen, int gap, double prewhiten, int design)
{
    if (const char *why = decon_window_refusal(snum, tnum, s0, s1)) return why;
    if (oplen < 1 || oplen > DECON_MAX_OPLEN) return "oplen must lie in 1 .. 256";
    if (gap < 1) return "gap must be at least 1";
    if ((long long)gap + oplen > (long long)s1 - s0) return "gap + oplen must not exceed the window's length";
    if (!(decon_finite(prewhiten) && prewhiten >= 0.0)) return "prewhiten must be finite and not negative";
    if (design != DECON_EACH && design != DECON_MEAN) return "design must be 0 (each) or 1 (mean)";
    return nullptr;
}
// Null for an autocorrelogram the entries take.
static inline const char *acorr_refusal(int snum, int tnum, int s0, int s1, int maxlag)
{
    if (const char *why = decon_window_refusal(snum, tnum, s0, s1)) return why;
    if (maxlag < 0) return "maxlag must not be negative";
    if (maxlag >= s1 - s0) return "maxlag must be below the window's length";
    if (maxlag >= DECON_C * 65535) return "maxlag is too large";      // (one grid row per chunk of lags)
    return nullptr;
}

// The launches of a call.  Both sliding kernels take DECON_TG traces per workgroup and walk the samples in blocks of DECON_C
// themselves (the autocorrelation upwards from s0, the apply downwards from the trace's end, which is what makes it safe in
// place); the autocorrelation's grid has one row per chunk of lags.
struct DeconPlan {
    DeconLags lags;
    int nlags;                 // rows of the lag table
    int groups;                // ceil(tnum / DECON_TG): grid.x of both sliding kernels
    int lag_chunks;            // grid.y of the autocorrelation
    int tap_chunks;            // chunks of taps the apply walks per block (0: no apply)
    int sample_blocks;         // blocks of the window (autocorrelation)
    int apply_blocks;          // blocks of the whole trace (apply)
    int solve_systems;         // tnum, or 1 for design 'mean'
    int solve_groups;          // ceil(systems / DECON_SOLVE_TRACES): grid.x of the recursion
    int mean_blocks;           // ceil(tnum / DECON_MEAN_BLOCK), design 'mean' only
    size_t acorr_lds, apply_lds, solve_lds;     // dynamic LDS bytes
    // scratch: the lag table and the operators, (nlags + oplen) * tnum doubles; then what design 'mean' adds (block sums, R,
    // its operator) and one flag per trace and one for the mean system
    size_t off_op, off_mean, off_dead, scratch_bytes;
    const char *label;
};
static inline size_t decon_round16(size_t n) { return (n + 15) & ~(size_t)15; }
static inline DeconPlan decon_plan(int snum, int tnum, int s0, int s1, int oplen, int gap, int design)
{
    DeconPlan P;
    P.lags = decon_lags(oplen, gap);
    P.nlags = decon_lag_count(P.lags);
    P.groups = (tnum + DECON_TG - 1) / DECON_TG;
    P.lag_chunks = decon_chunk_count(P.lags);
    P.tap_chunks = (oplen + DECON_C - 1) / DECON_C;
    P.sample_blocks = (s1 - s0 + DECON_C - 1) / DECON_C;
    P.apply_blocks = (snum + DECON_C - 1) / DECON_C;
    P.solve_systems = design == DECON_MEAN ? 1 : tnum;
    P.solve_groups = (P.solve_systems + DECON_SOLVE_TRACES - 1) / DECON_SOLVE_TRACES;
    P.mean_blocks = design == DECON_MEAN ? (tnum + DECON_MEAN_BLOCK - 1) / DECON_MEAN_BLOCK : 0;
    // a block of base samples and a block plus the chunk's reach of shifted ones (autocorrelation); the shifted ones and a
    // chunk of taps (apply); c, rhs, a and two generations of p for each trace of the group (recursion)
    P.acorr_lds = (size_t)(DECON_C + 2 * DECON_C - 1) * DECON_TG * sizeof(double);
    P.apply_lds = (size_t)(2 * DECON_C - 1 + DECON_C) * DECON_TG * sizeof(double);
    P.solve_lds = (size_t)5 * oplen * DECON_SOLVE_TRACES * sizeof(double);
    P.off_op = (size_t)P.nlags * tnum * sizeof(double);
    P.off_mean = P.off_op + (size_t)oplen * tnum * sizeof(double);
    P.off_dead = P.off_mean + decon_round16((size_t)(design == DECON_MEAN ? (P.mean_blocks + 1) * P.nlags + oplen : 0) * sizeof(double));
    P.scratch_bytes = P.off_dead + decon_round16((size_t)(tnum + 1) * sizeof(int));
    P.label = design == DECON_MEAN ? "decon_acorr_kernel + decon_mean_kernel + decon_solve_kernel (one system) + decon_apply_kernel"
                                   : "decon_acorr_kernel + decon_solve_kernel + decon_apply_kernel";
    return P;
}
// The autocorrelogram writes its table straight into the caller's array: no scratch.
static inline DeconPlan acorr_plan(int snum, int tnum, int s0, int s1, int maxlag)
{
    DeconPlan P = decon_plan(snum, tnum, s0, s1, 1, 1, DECON_EACH);
    P.lags.n0 = maxlag + 1;
    P.lags.n1 = 0;
    P.lags.b1 = maxlag + 1;
    P.nlags = maxlag + 1;
    P.lag_chunks = decon_chunk_count(P.lags);
    P.tap_chunks = P.apply_blocks = P.solve_systems = P.solve_groups = 0;
    P.apply_lds = P.solve_lds = 0;
    P.off_op = P.off_mean = P.off_dead = P.scratch_bytes = 0;
    P.label = "decon_acorr_kernel";
    return P;
}
