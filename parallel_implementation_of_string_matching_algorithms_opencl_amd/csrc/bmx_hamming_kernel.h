// bmx_hamming_kernel.h -- k-mismatch search (bmx_search_hamming_device): every start p of the text view at which at most k
// of the m positions have text[p + i] outside class i, none of them a position of `must`, in ascending order, with the
// number of mismatches.  Substitutions only: no insertions or deletions.  No counterpart in the reference.
//
// The recurrence is Shift-Add (Baeza-Yates and Gonnet, CACM 35(10), 1992) with bit-sliced counters: bit i of the slice
// words S_0..S_{B-1} is a B-bit counter of the mismatches of the last i + 1 bytes against classes 0..i, and bit i of the
// sticky word V says that this counter has overflowed or that a `must` position mismatched.  A window's counter starts at
// bias = 2^B - 1 - k, so "more than k mismatches" is the carry out of the top slice and the hit test is one bit.  Per byte c
// with M[c] = the positions whose class does NOT hold c:
//     carry = M[c]
//     for t in 0..B-1:  s = (S_t << 1) | (bit t of bias ? seed : 0);  S_t = s ^ carry;  carry = s & carry
//     V = (V << 1) | carry | (M[c] & must)
// End j is a hit iff bit m - 1 of V is clear, and its distance is bit m - 1 of S_{B-1}..S_0 read as a number, minus bias.
// Bit i of every word depends on the last i + 1 bytes only, so a lane that starts from all zeros m - 1 bytes before its
// first end is exact from there on, whatever lay before -- the class search's warm-up (bmx_classes_kernel.h), with the
// same shift of bit m - 1 into the TOP bit of the word (32 bits for m <= 32, two halves for 33..64).
//
// The tile loop, the ordered output and the argument block are bmx_tile_frame.h's, in end coordinates with lead = m - 1;
// the LDS table is the class search's policy's.  The walk is the class search's: whole 128-byte lines per lane, a chunk's
// 16 table words gathered before its 16 steps, no branch, LDS atomic or store inside the chain, the 16 hit bits (the top
// bit of V, inverted once per chunk) funnelled with v_alignbit_b32 and ANDed with ownership once.  The top bit of every
// slice is funnelled into a 16-bit mask of its own alongside (B more VALU per byte), so the hit code reads the distance
// off the masks; stepping a chunk with a hit a second time instead was measured and is no faster on sparse results and
// up to 1.5 times slower on dense ones.
// A parked hit is {position in tile, ordinal in lane << 32, distance << 48}.
#pragma once

#include "bmx_classes_kernel.h"

namespace bmx {

constexpr int MAX_HAMMING_PATTERN = 64; // == BMX_MAX_HAMMING_PATTERN
constexpr int MAX_HAMMING_K = 15;       // == BMX_MAX_HAMMING_K

// The kernel's further arguments: both uniform.
struct HammingConsts {
    uint64_t must; // the positions that may not mismatch, shifted up like the table
    uint32_t bias; // 2^B - 1 - k
};

// Slices 0..B-1 and V (index B) of one lane; hi is the whole word when m <= 32.
template <bool WIDE, int B>
struct HammingState {
    uint32_t lo[B + 1], hi[B + 1];
};

// The table words M[c] of a chunk's 16 bytes.
template <bool WIDE>
struct HammingWords {
    uint32_t lo[16], hi[16];
};

template <bool WIDE, int B>
struct HammingStep {
    uint32_t seed[B];          // the seed bit of position 0 where bit t of the bias is set (WIDE: in the low half)
    uint32_t must_lo, must_hi; // (hi: the whole word when m <= 32)
    uint32_t bias;
    __device__ __forceinline__ HammingStep(const TileArgs &a, const HammingConsts &c) : bias(c.bias)
    {
        const uint32_t bit0 = 1u << ((WIDE ? 64u : 32u) - a.m);
#pragma unroll
        for (int t = 0; t < B; ++t) seed[t] = ((c.bias >> t) & 1u) ? bit0 : 0u;
        must_lo = WIDE ? (uint32_t)c.must : 0u;
        must_hi = WIDE ? (uint32_t)(c.must >> 32) : (uint32_t)c.must;
    }

    __device__ __forceinline__ void gather(const uint32_t *tab, tile_u32x4 v, HammingWords<WIDE> &w) const
    {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t byte = __builtin_amdgcn_ubfe(v[i >> 2], 8 * (i & 3), 8);
            if (WIDE) {
                const uint2 x = reinterpret_cast<const uint2 *>(tab)[byte];
                w.lo[i] = x.x;
                w.hi[i] = x.y;
            } else {
                w.hi[i] = tab[byte];
            }
        }
    }

    // The 16 steps of one chunk.  Returns the hit bits, bit i = the step of byte i; dm[t] gets the top bit of slice t of
    // every step the same way.
    __device__ __forceinline__ uint32_t steps(const HammingWords<WIDE> &w, HammingState<WIDE, B> &s, uint32_t (&dm)[B]) const
    {
        uint32_t over = 0; // step i lands in bit 15 - i, turned round below
#pragma unroll
        for (int t = 0; t < B; ++t) dm[t] = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint32_t clo = WIDE ? w.lo[i] : 0u, chi = w.hi[i];
#pragma unroll
            for (int t = 0; t < B; ++t) {
                if (WIDE) {
                    const uint32_t shi = __builtin_amdgcn_alignbit(s.hi[t], s.lo[t], 31); // (hi << 1) | (lo >> 31)
                    const uint32_t slo = (s.lo[t] << 1) | seed[t];
                    s.lo[t] = slo ^ clo;
                    s.hi[t] = shi ^ chi;
                    clo &= slo;
                    chi &= shi;
                } else {
                    const uint32_t shi = (s.hi[t] << 1) | seed[t];
                    s.hi[t] = shi ^ chi;
                    chi &= shi;
                }
                dm[t] = __builtin_amdgcn_alignbit(dm[t], s.hi[t], 31);
            }
            if (WIDE) {
                const uint32_t vhi = __builtin_amdgcn_alignbit(s.hi[B], s.lo[B], 31);
                s.lo[B] = (s.lo[B] << 1) | clo | (w.lo[i] & must_lo);
                s.hi[B] = vhi | chi | (w.hi[i] & must_hi);
            } else {
                s.hi[B] = (s.hi[B] << 1) | chi | (w.hi[i] & must_hi);
            }
            over = __builtin_amdgcn_alignbit(over, s.hi[B], 31); // (over << 1) | top bit of V
        }
#pragma unroll
        for (int t = 0; t < B; ++t) dm[t] = __builtin_bitreverse32(dm[t]) >> 16;
        return ~__builtin_bitreverse32(over) >> 16;
    }

    // the distance of the hit at byte i of the chunk
    __device__ __forceinline__ uint32_t distance(const uint32_t (&dm)[B], uint32_t i) const
    {
        uint32_t d = 0;
#pragma unroll
        for (int t = 0; t < B; ++t) d |= ((dm[t] >> i) & 1u) << t;
        return d - bias;
    }
};

// One lane: bmx_classes_kernel.h's shift_and_walk with the distance beside every hit.  The ends [lo, hi) (aligned
// coordinates), after a warm-up of a.warm bytes (clipped at view byte 0), line by line; returns the number of hits.
// Every 16-byte load holds at least one byte of the view.  The bytes in front of an unaligned view are stepped through
// like any others: a window of exactly m bytes that ends inside the view begins inside it.
template <bool WIDE, int B, int PASS>
__device__ __forceinline__ uint32_t hamming_walk(const TileArgs &a, const HammingStep<WIDE, B> &step, const uint32_t *tab, uint64_t lo,
                                                 uint64_t hi, uint64_t tile0, uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
    const uint64_t want = lo >= a.first + a.warm ? lo - a.warm : a.first;
    const uint64_t origin = want & ~127ull;                      // the line of the first byte walked
    const int32_t r_begin = (int32_t)((want & ~15ull) - origin); // everything below is relative to origin (< 2^12)
    const int32_t r_lo = (int32_t)(lo - origin);
    const int32_t r_hi = (int32_t)(hi - origin);
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16) + (origin >> 4);
    HammingState<WIDE, B> s;
#pragma unroll
    for (int t = 0; t <= B; ++t) s.lo[t] = s.hi[t] = 0;
    uint32_t cnt = 0;
    for (int32_t line = 0; line < r_hi; line += 128, src += 8) {
        tile_u32x4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int32_t r = line + 16 * q;
            if (r >= r_begin && r < r_hi) v[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int32_t r = line + 16 * q;
            if (r < r_begin || r >= r_hi) continue;
            HammingWords<WIDE> w;
            step.gather(tab, v[q], w);
            uint32_t dm[B];
            uint32_t hits = step.steps(w, s, dm);
            const int32_t own_from = min(max(r_lo - r, 0), 16), own_to = min(r_hi - r, 16);
            hits &= ((1u << own_to) - 1u) & ~((1u << own_from) - 1u);
            if (hits == 0) continue; // the usual case, for the whole wave
            const uint32_t ord0 = cnt;
            const uint32_t pc = __builtin_popcount(hits);
            cnt += pc;
            if (PASS == TILE_PARK) {
                if (a.out == nullptr) continue;
                uint32_t slot = atomicAdd(stage_n, pc);
                const uint32_t pos0 = (uint32_t)(origin - tile0) + (uint32_t)r; // mod 2^32: origin may lie in front of the tile, a hit never
                uint32_t ord = ord0;
                for (uint32_t h = hits; h != 0; h &= h - 1u, ++slot, ++ord) {
                    const uint32_t i = (uint32_t)__builtin_ctz(h);
                    if (slot < (uint32_t)TILE_STAGE)
                        stage[slot] = (uint64_t)(pos0 + i) | ((uint64_t)ord << 32) | ((uint64_t)step.distance(dm, i) << 48);
                }
            } else {
                uint64_t idx = base + ord0;
                const uint64_t end0 = origin + (uint64_t)r + a.out_bias;
                for (uint32_t h = hits; h != 0; h &= h - 1u, ++idx) {
                    const uint32_t i = (uint32_t)__builtin_ctz(h);
                    if (idx < a.cap) {
                        a.out[idx] = end0 + i;
                        if (a.dist != nullptr) a.dist[idx] = (uint8_t)step.distance(dm, i);
                    }
                }
            }
        }
    }
    return cnt;
}

// The frame's policy: the class search's table (here M: the complement, masked to the pattern's bits, built by the host)
// and the walk above; a parked entry carries the distance as the approximate search's does.
template <bool WIDE, int B>
struct HammingPolicy : ShiftAndPolicy<WIDE, HammingStep<WIDE, B>> {
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base, const HammingConsts &c)
    {
        return hamming_walk<WIDE, B, PASS>(a, HammingStep<WIDE, B>(a, c), tab, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32) & 0xffffu; }
    static __device__ __forceinline__ void also(const TileArgs &a, uint64_t idx, uint64_t e)
    {
        if (a.dist != nullptr) a.dist[idx] = (uint8_t)(e >> 48);
    }
};

} // namespace bmx
