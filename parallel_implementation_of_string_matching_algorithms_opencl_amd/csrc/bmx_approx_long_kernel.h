// bmx_approx_long_kernel.h -- approximate search for patterns of 65 to 512 bytes (bmx_search_approx_long_device): the
// semantics of bmx_approx_kernel.h -- every end j with min over s of ED(P, T[s..j]) <= k, ascending, with that minimum --
// with a column of W = 2, 4 or 8 64-bit words per lane (bmx_myers_words.h) where that file has one.
//
// The tile loop, the ordered output and the argument block are bmx_tile_frame.h's; this file is the lane's walk and the
// policy.  As there, a lane walks the m + k - 1 bytes in front of its ends without reporting, text comes in 16 bytes per
// lane per load, and a parked hit is {position in tile, ordinal in lane << 32, distance << 48}: a lane has at most 2^12
// ends (bmx_internal_approx_long_piece_shift) and k <= 255, so both fit.  The pattern is a further kernel argument; the
// workgroup builds the Peq table from it (a.peq is not used).  The 16 bytes of a load are walked one dword at a time in a
// loop that is unrolled only at W = 2: a fully unrolled chunk of 16 eight-word columns, in four variants, would not fit
// the instruction cache.
#pragma once

#include "bmx_myers_words.h"
#include "bmx_tile_frame.h"

namespace bmx {

// 16 bytes of one chunk at aligned coordinate c.  HEAD: the chunk that holds view byte 0, walked from byte `skip` on.
// Bit i of rmask: end c + i belongs to this lane.
template <int W, int PASS, bool HEAD>
__device__ __forceinline__ void approx_long_chunk(const TileArgs &a, const words_u64x2 *tab, WordsColumn<W> &s, tile_u32x4 v,
                                                  uint64_t c, uint32_t rmask, uint32_t skip, uint32_t lw, uint32_t hb,
                                                  uint32_t words, uint32_t &cnt, uint64_t tile0, uint64_t *stage,
                                                  uint32_t *stage_n, uint64_t base)
{
#pragma clang loop unroll_count(W <= 2 ? 4 : 1)
    for (int q = 0; q < 4; ++q) {
        const uint32_t dw = q == 0 ? v[0] : q == 1 ? v[1] : q == 2 ? v[2] : v[3];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t i = 4 * q + r;
            if (HEAD && i < skip) continue;
            const uint32_t byte = __builtin_amdgcn_ubfe(dw, 8 * r, 8);
            words_column<W>(s, tab + (size_t)byte * (W / 2), 0, lw, hb, words);
            if (s.score <= a.k) { // rare on sparse results: the branch is skipped by the whole wave
                // (approx_chunk's compiler barrier between this test and the next is not here: with a column of several words
                // it changes no VALU instruction of the three kernels -- 12,094 in all either way -- and adds 64 scalar branches)
                if ((rmask >> i) & 1u) {
                    const uint32_t ord = cnt++;
                    if (PASS == TILE_PARK) {
                        if (a.out != nullptr) {
                            const uint32_t slot = atomicAdd(stage_n, 1u);
                            if (slot < (uint32_t)TILE_STAGE)
                                stage[slot] = (uint64_t)(uint32_t)(c + i - tile0) | ((uint64_t)ord << 32) | ((uint64_t)s.score << 48);
                        }
                    } else {
                        const uint64_t idx = base + ord;
                        if (idx < a.cap) {
                            a.out[idx] = c + i + a.out_bias;
                            if (a.dist != nullptr) a.dist[idx] = (uint8_t)s.score;
                        }
                    }
                }
            }
        }
    }
}

// One lane: the ends [lo, hi) (aligned coordinates), after a warm-up of a.warm bytes (clipped at view byte 0).
// Returns the number of hits.  Every 16-byte load holds at least one byte of the view.
template <int W, int PASS>
__device__ __forceinline__ uint32_t approx_long_walk(const TileArgs &a, const words_u64x2 *tab, uint64_t lo, uint64_t hi,
                                                     uint64_t tile0, uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
    const uint64_t want = lo >= a.first + a.warm ? lo - a.warm : a.first;
    uint64_t c = want & ~15ull;
    const uint32_t lw = (a.m - 1) >> 6, hb = (a.m - 1) & 63, words = lw + 1;
    WordsColumn<W> s;
    words_init<W>(s, a.m);
    uint32_t cnt = 0;
    auto rmask_at = [&](uint64_t cc) -> uint32_t {
        const uint32_t rlo = lo <= cc ? 0u : (lo - cc >= 16 ? 16u : (uint32_t)(lo - cc));
        const uint32_t rhi = hi - cc >= 16 ? 16u : (uint32_t)(hi - cc);
        return ((1u << rhi) - 1u) & ~((1u << rlo) - 1u);
    };
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16);
    tile_u32x4 cur = src[c >> 4];
    tile_u32x4 nxt = cur;
    if (c + 16 < hi) nxt = src[(c >> 4) + 1];
    approx_long_chunk<W, PASS, true>(a, tab, s, cur, c, rmask_at(c), c < a.first ? (uint32_t)(a.first - c) : 0u, lw, hb, words, cnt,
                                     tile0, stage, stage_n, base);
    for (c += 16; c < hi; c += 16) {
        cur = nxt;
        if (c + 16 < hi) nxt = src[(c >> 4) + 1]; // one chunk ahead
        approx_long_chunk<W, PASS, false>(a, tab, s, cur, c, rmask_at(c), 0u, lw, hb, words, cnt, tile0, stage, stage_n, base);
    }
    return cnt;
}

template <int W>
struct ApproxLongPolicy {
    typedef words_u64x2 Elem;
    static constexpr int TAB = 256 * W / 2;
    static constexpr bool FILL_TAKES_X = true; // the table comes from the pattern argument, not from a.peq
    static __device__ __forceinline__ void fill(words_u64x2 *tab, const TileArgs &a, uint32_t tid, const LongPattern &pat)
    {
        words_fill<W>(tab, pat, a.m, tid); // TILE_BLOCK == 256
    }
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const words_u64x2 *tab, uint64_t lo, uint64_t hi,
                                                    uint64_t tile0, uint64_t *stage, uint32_t *stage_n, uint64_t base,
                                                    const LongPattern &)
    {
        return approx_long_walk<W, PASS>(a, tab, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32) & 0xffffu; }
    static __device__ __forceinline__ void also(const TileArgs &a, uint64_t idx, uint64_t e)
    {
        if (a.dist != nullptr) a.dist[idx] = (uint8_t)(e >> 48);
    }
};

} // namespace bmx
