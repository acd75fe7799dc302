// bmx_regex_sets.h -- what the compiler of the regular-expression search (bmx_regex_compile.cpp) and its entries
// (bmx_internal.h) both need of a position automaton (struct bmx_regex and struct bmx_regex_long, include/bmx.h), in plain
// C++ with no HIP: the validity rule and the shortest and the longest match; for the entries that take unbounded
// repetition (bmx_search_regex_star_device) the same with a cycle in follow[].  The rules of the star-free automaton are
// written once over the set type S: uint64_t for the 64 positions of struct bmx_regex, bmx_set128 for the 128 of struct
// bmx_regex_long (whose two-word sets are loaded into and stored from it), and with them the split of the positions into
// lin and nl that the kernels step by and the reversed automaton that the starts passes run.
#pragma once

#include <stdint.h>
#include <string.h>

#include "bmx.h"

typedef unsigned __int128 bmx_set128;

inline int bmx_set_low_bit(uint64_t s) { return __builtin_ctzll(s); }
inline int bmx_set_low_bit(bmx_set128 s) { return (uint64_t)s ? __builtin_ctzll((uint64_t)s) : 64 + __builtin_ctzll((uint64_t)(s >> 64)); }
inline bmx_set128 bmx_set128_load(const uint64_t w[2]) { return (bmx_set128)w[0] | ((bmx_set128)w[1] << 64); }
inline void bmx_set128_store(bmx_set128 s, uint64_t w[2]) { w[0] = (uint64_t)s, w[1] = (uint64_t)(s >> 64); }

// 1 <= m <= MAX (the bits of S at the most), first and last non-zero, no bit at or above m anywhere, follow[i] holds only
// bits j > i.
template <typename S, int MAX>
inline bool bmx_regex_sets_ok_t(int32_t m, S first, S last, const S *follow)
{
    if (m < 1 || m > MAX || first == 0 || last == 0) return false;
    const S all = m == (int32_t)(8 * sizeof(S)) ? ~(S)0 : ((S)1 << m) - 1;
    if ((first | last) & ~all) return false;
    for (int32_t i = 0; i < m; ++i) {
        const S above = i == (int32_t)(8 * sizeof(S)) - 1 ? (S)0 : ~(S)0 << (i + 1);
        if (follow[i] & ~(all & above)) return false;
    }
    return true;
}

inline bool bmx_regex_sets_ok(int32_t m, uint64_t first, uint64_t last, const uint64_t *follow)
{
    return bmx_regex_sets_ok_t<uint64_t, BMX_MAX_REGEX_POSITIONS>(m, first, last, follow);
}

// Shortest and longest path from `first` to `last` in bytes, of valid sets (the classes play no part); 0 and 0 where no
// position of `last` can be reached.  Follow sets point upward, so one ascending sweep settles every position.
template <typename S>
inline void bmx_regex_lengths_t(int32_t m, S first, S last, const S *follow, int32_t *min_len, int32_t *max_len)
{
    int32_t lo[8 * sizeof(S)], hi[8 * sizeof(S)];
    int32_t best_lo = 0, best_hi = 0;
    for (int32_t i = 0; i < m; ++i) lo[i] = hi[i] = 0;
    for (int32_t i = 0; i < m; ++i) {
        if ((first >> i) & 1u) lo[i] = 1, hi[i] = hi[i] > 1 ? hi[i] : 1;
        if (hi[i] == 0) continue; // no path reaches it
        if ((last >> i) & 1u) {
            best_lo = best_lo == 0 || lo[i] < best_lo ? lo[i] : best_lo;
            best_hi = hi[i] > best_hi ? hi[i] : best_hi;
        }
        for (S f = follow[i]; f != 0; f &= f - 1) {
            const int j = bmx_set_low_bit(f);
            lo[j] = lo[j] == 0 || lo[i] + 1 < lo[j] ? lo[i] + 1 : lo[j];
            hi[j] = hi[i] + 1 > hi[j] ? hi[i] + 1 : hi[j];
        }
    }
    *min_len = best_lo;
    *max_len = best_hi;
}

inline void bmx_regex_lengths(int32_t m, uint64_t first, uint64_t last, const uint64_t *follow, int32_t *min_len, int32_t *max_len)
{
    bmx_regex_lengths_t<uint64_t>(m, first, last, follow, min_len, max_len);
}

// lin: the positions whose only successor is the next one (they move by a shift); nl: the other positions with a successor.
template <typename S>
inline void bmx_regex_lin_nl_t(int32_t m, const S *follow, S *lin, S *nl)
{
    *lin = *nl = 0;
    for (int32_t i = 0; i < m; ++i) {
        if (follow[i] == 0) continue;
        if (i + 1 < (int32_t)(8 * sizeof(S)) && follow[i] == (S)1 << (i + 1)) *lin |= (S)1 << i;
        else *nl |= (S)1 << i;
    }
}

// The automaton of struct bmx_regex_long with its sets as bmx_set128: what the entries compute on.
struct bmx_regex_long_sets {
    int32_t m;
    bmx_set128 first, last, follow[BMX_MAX_REGEX_LONG_POSITIONS];
};

inline void bmx_regex_long_load(const bmx_regex_long *re, bmx_regex_long_sets *s)
{
    s->m = re->m;
    s->first = bmx_set128_load(re->first);
    s->last = bmx_set128_load(re->last);
    const int32_t m = re->m < 0 ? 0 : re->m > BMX_MAX_REGEX_LONG_POSITIONS ? BMX_MAX_REGEX_LONG_POSITIONS : re->m;
    for (int32_t i = 0; i < BMX_MAX_REGEX_LONG_POSITIONS; ++i) s->follow[i] = i < m ? bmx_set128_load(re->follow[i]) : 0;
}

inline bool bmx_regex_long_sets_ok(const bmx_regex_long *re)
{
    if (!re) return false;
    bmx_regex_long_sets s;
    bmx_regex_long_load(re, &s);
    return bmx_regex_sets_ok_t<bmx_set128, BMX_MAX_REGEX_LONG_POSITIONS>(s.m, s.first, s.last, s.follow);
}

// The reversed automaton of valid sets: bit i stands for position m - 1 - i, first and last swap, follow is transposed
// (upward again).  classes / rev_classes: BMX_CLASS_BYTES per position, mirrored (either may be NULL).
template <typename S>
inline void bmx_regex_reverse_t(int32_t m, S first, S last, const S *follow, const uint8_t *classes, S *rev_first, S *rev_last,
                                S *rev_follow, uint8_t *rev_classes)
{
    const auto flip = [m](S set) {
        S r = 0;
        for (; set != 0; set &= set - 1) r |= (S)1 << (m - 1 - bmx_set_low_bit(set));
        return r;
    };
    *rev_first = flip(last);
    *rev_last = flip(first);
    for (int32_t i = 0; i < m; ++i) rev_follow[i] = 0;
    for (int32_t i = 0; i < m; ++i) {
        for (S f = follow[i]; f != 0; f &= f - 1) rev_follow[m - 1 - bmx_set_low_bit(f)] |= (S)1 << (m - 1 - i);
        if (classes && rev_classes)
            memcpy(rev_classes + (size_t)(m - 1 - i) * BMX_CLASS_BYTES, classes + (size_t)i * BMX_CLASS_BYTES, BMX_CLASS_BYTES);
    }
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
