// Which row lengths the library's own transforms (own_fft.h) take: plain C++, for the host-only planners too (ps_route.h).
#pragma once
// complex length M the kernel supports: a power of two, 16 ... 8192 (float64 rows of 8192 take 132 KB of LDS)
static inline bool own_fft_len_ok(long long m) { return m >= 16 && m <= 8192 && (m & (m - 1)) == 0; }
