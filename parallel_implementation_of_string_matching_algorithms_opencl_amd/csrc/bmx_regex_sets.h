// bmx_regex_sets.h -- what the compiler of the regular-expression search (bmx_regex_compile.cpp) and its entries
// (bmx_internal.h) both need of a position automaton (struct bmx_regex, include/bmx.h), in plain C++ with no HIP: the
// validity rule and the shortest and the longest match; for the entries that take unbounded repetition
// (bmx_search_regex_star_device) the same with a cycle in follow[].
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

// The rule of the entries that take unbounded repetition: as above, but follow[i] may hold any bit below m (back edges
// and self-loops).
inline bool bmx_regex_star_sets_ok(int32_t m, uint64_t first, uint64_t last, const uint64_t *follow)
{
    if (m < 1 || m > BMX_MAX_REGEX_POSITIONS || first == 0 || last == 0) return false;
    const uint64_t all = m == 64 ? ~0ull : (1ull << m) - 1;
    if ((first | last) & ~all) return false;
    for (int32_t i = 0; i < m; ++i)
        if (follow[i] & ~all) return false;
    return true;
}

// The positions a match can use: reachable from `first` and with a path to `last` (both by a fixed point over follow[]).
inline uint64_t bmx_regex_star_useful(int32_t m, uint64_t first, uint64_t last, const uint64_t *follow)
{
    uint64_t fwd = first, bwd = last;
    for (bool grown = true; grown;) {
        grown = false;
        for (int32_t i = 0; i < m; ++i) {
            if (((fwd >> i) & 1u) && (follow[i] & ~fwd)) fwd |= follow[i], grown = true;
            if (!((bwd >> i) & 1u) && (follow[i] & bwd)) bwd |= 1ull << i, grown = true;
        }
    }
    return fwd & bwd;
}

// Shortest and longest match in bytes of sets valid by the rule above; 0 and 0 where no match exists.  Rounds of
// relaxation over the useful positions: the shortest paths are settled after m rounds, and so are the longest unless a
// cycle lies among the useful positions, in which case *max_len is BMX_REGEX_UNBOUNDED.  *useful (may be NULL): the
// positions a match can use.
inline void bmx_regex_star_lengths(int32_t m, uint64_t first, uint64_t last, const uint64_t *follow, int32_t *min_len,
                                   int32_t *max_len, uint64_t *useful)
{
    const uint64_t use = bmx_regex_star_useful(m, first, last, follow);
    if (useful) *useful = use;
    int32_t lo[BMX_MAX_REGEX_POSITIONS], hi[BMX_MAX_REGEX_POSITIONS];
    for (int32_t i = 0; i < m; ++i) lo[i] = hi[i] = ((first & use) >> i) & 1u ? 1 : 0;
    bool changed = true;
    int32_t rounds = 0;
    for (; changed && rounds <= m; ++rounds) {
        changed = false;
        for (int32_t i = 0; i < m; ++i) {
            if (hi[i] == 0) continue;
            for (uint64_t f = follow[i] & use; f != 0; f &= f - 1) {
                const int j = __builtin_ctzll(f);
                if (lo[j] == 0 || lo[i] + 1 < lo[j]) lo[j] = lo[i] + 1, changed = true;
                if (hi[i] + 1 > hi[j]) hi[j] = hi[i] + 1, changed = true;
            }
        }
    }
    int32_t best_lo = 0, best_hi = 0;
    for (int32_t i = 0; i < m; ++i) {
        if (!(((last & use) >> i) & 1u)) continue;
        best_lo = best_lo == 0 || lo[i] < best_lo ? lo[i] : best_lo;
        best_hi = hi[i] > best_hi ? hi[i] : best_hi;
    }
    *min_len = best_lo;
    *max_len = changed ? BMX_REGEX_UNBOUNDED : best_hi; // still moving after m + 1 rounds: a cycle
}
