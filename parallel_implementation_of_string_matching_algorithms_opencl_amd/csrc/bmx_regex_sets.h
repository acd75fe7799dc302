// bmx_regex_sets.h -- what the compiler of the regular-expression search (bmx_regex_compile.cpp) and its entries
// (bmx_internal.h) both need of a position automaton (struct bmx_regex, include/bmx.h), in plain C++ with no HIP: the
// validity rule and the shortest and the longest match.
#pragma once

#include <stdint.h>

#include "bmx.h"

// 1 <= m <= 64, first and last non-zero, no bit at or above m anywhere, follow[i] holds only bits j > i.
inline bool bmx_regex_sets_ok(int32_t m, uint64_t first, uint64_t last, const uint64_t *follow)
{
    if (m < 1 || m > BMX_MAX_REGEX_POSITIONS || first == 0 || last == 0) return false;
    const uint64_t all = m == 64 ? ~0ull : (1ull << m) - 1;
    if ((first | last) & ~all) return false;
    for (int32_t i = 0; i < m; ++i) {
        const uint64_t above = i == 63 ? 0 : ~0ull << (i + 1);
        if (follow[i] & ~(all & above)) return false;
    }
    return true;
}

// Shortest and longest path from `first` to `last` in bytes, of valid sets (the classes play no part); 0 and 0 where no
// position of `last` can be reached.  Follow sets point upward, so one ascending sweep settles every position.
inline void bmx_regex_lengths(int32_t m, uint64_t first, uint64_t last, const uint64_t *follow, int32_t *min_len, int32_t *max_len)
{
    int32_t lo[BMX_MAX_REGEX_POSITIONS], hi[BMX_MAX_REGEX_POSITIONS];
    int32_t best_lo = 0, best_hi = 0;
    for (int32_t i = 0; i < m; ++i) lo[i] = hi[i] = 0;
    for (int32_t i = 0; i < m; ++i) {
        if ((first >> i) & 1u) lo[i] = 1, hi[i] = hi[i] > 1 ? hi[i] : 1;
        if (hi[i] == 0) continue; // no path reaches it
        if ((last >> i) & 1u) {
            best_lo = best_lo == 0 || lo[i] < best_lo ? lo[i] : best_lo;
            best_hi = hi[i] > best_hi ? hi[i] : best_hi;
        }
        for (uint64_t f = follow[i]; f != 0; f &= f - 1) {
            const int j = __builtin_ctzll(f);
            lo[j] = lo[j] == 0 || lo[i] + 1 < lo[j] ? lo[i] + 1 : lo[j];
            hi[j] = hi[i] + 1 > hi[j] ? hi[i] + 1 : hi[j];
        }
    }
    *min_len = best_lo;
    *max_len = best_hi;
}
