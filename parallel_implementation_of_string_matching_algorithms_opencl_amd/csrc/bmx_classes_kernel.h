// bmx_classes_kernel.h -- class-pattern search (bmx_search_classes_device): every start p of the text view at which
// text[p + i] belongs to class i for all i in [0, m), in ascending order.  A class is a set of byte values, so one
// pattern covers wildcards, sets, case folding and IUPAC codes.  No counterpart in the reference.
//
// The recurrence is Shift-And (Baeza-Yates and Gonnet, CACM 35(10), 1992): bit i of D says that the last i + 1 bytes
// belong to classes 0..i, and per byte D = ((D << 1) | 1) & B[byte], where bit i of B[c] says that c is in class i.  End
// j is a hit iff bit m - 1 of D is set; the reported start is j - m + 1.  Bit m - 1 depends on the last m bytes only, so
// a lane that starts with D = 0 at least m - 1 bytes before its first end is exact from there on -- whatever lay before.
// The host shifts B up so that bit m - 1 is the TOP bit of the word (32 bits for m <= 32, 64 for 33..64): the hit bit of
// every step is then funnelled into a mask with one v_alignbit_b32.
//
// The tile loop, the ordered output and the argument block are bmx_tile_frame.h's, in end coordinates
// with lead = m - 1.  This file is the recurrence, the policy that plugs it into the frame, and the lane's walk, which the
// gapped search (bmx_gaps_kernel.h) uses with its own step.  Against the approximate search's walk:
//  * gather first, then step: a 16-byte chunk reads its 16 B words into registers, then runs its 16 steps with no
//    branch, LDS atomic or store between them; the chunk's 16 hit bits are ANDed with its ownership mask once and only a
//    non-zero mask enters the hit code;
//  * text comes in whole 128-byte lines per lane (eight 16-byte loads issued together), so a line is fetched once.
// A parked hit is {position in tile, ordinal in lane << 32}.
#pragma once

#include "bmx_tile_frame.h"

namespace bmx {

constexpr int MAX_CLASS_PATTERN = 64; // == BMX_MAX_CLASS_PATTERN

// Shift-And state of one lane; hi is the whole word when m <= 32.
template <bool WIDE>
struct ShiftAndState {
    uint32_t lo, hi;
};

// One 16-byte chunk: gather, then 16 steps.  Returns the hit bits, bit i = the step of byte i.
template <bool WIDE>
__device__ __forceinline__ uint32_t classes_chunk(const uint32_t *tab, ShiftAndState<WIDE> &s, tile_u32x4 v, uint32_t seed)
{
    uint32_t blo[16], bhi[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t byte = __builtin_amdgcn_ubfe(v[i >> 2], 8 * (i & 3), 8);
        if (WIDE) {
            const uint2 w = reinterpret_cast<const uint2 *>(tab)[byte];
            blo[i] = w.x;
            bhi[i] = w.y;
        } else {
            bhi[i] = tab[byte];
        }
    }
    uint32_t hits = 0; // step i lands in bit 15 - i, turned round below
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (WIDE) {
            const uint32_t nhi = __builtin_amdgcn_alignbit(s.hi, s.lo, 31); // (hi << 1) | (lo >> 31)
            s.lo = ((s.lo << 1) | seed) & blo[i];
            s.hi = nhi & bhi[i];
        } else {
            s.hi = ((s.hi << 1) | seed) & bhi[i];
        }
        hits = __builtin_amdgcn_alignbit(hits, s.hi, 31); // (hits << 1) | top bit of the word
    }
    return __builtin_bitreverse32(hits) >> 16;
}

// The class search's step: the chunk above, with the bit of class 0 as the seed.  It steps through the bytes in front of
// an unaligned view like through any others (`skip`): a window of exactly m bytes that ends inside the view begins inside it.
template <bool WIDE>
struct ClassesStep {
    uint32_t seed;
    __device__ __forceinline__ explicit ClassesStep(const TileArgs &a) : seed(1u << ((WIDE ? 64u : 32u) - a.m)) {}
    __device__ __forceinline__ uint32_t chunk(const uint32_t *tab, ShiftAndState<WIDE> &s, tile_u32x4 v, uint32_t /*skip*/) const
    {
        return classes_chunk<WIDE>(tab, s, v, seed);
    }
};

// One lane: the ends [lo, hi) (aligned coordinates), after a warm-up of a.warm bytes (clipped at view byte 0), line by
// line.  Returns the number of hits.  Every 16-byte load holds at least one byte of the view: chunks lie between the one
// that holds the first warm-up byte and the one that holds end hi - 1.  step.chunk(tab, s, v, skip) runs one chunk and
// returns its 16 hit bits; skip is the number of its bytes that lie in front of the view (non-zero for the chunk at
// aligned byte 0 of an unaligned view only).
// State: what a lane carries from byte to byte, all zero in front of the first byte walked (ShiftAndState, or the four
// dwords of the long regular-expression search); Tab: the element type of the policy's LDS table.
template <typename State, int PASS, typename Step, typename Tab>
__device__ __forceinline__ uint32_t shift_and_walk_state(const TileArgs &a, const Step &step, const Tab *tab, uint64_t lo, uint64_t hi,
                                                         uint64_t tile0, uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
    const uint64_t want = lo >= a.first + a.warm ? lo - a.warm : a.first;
    const uint64_t origin = want & ~127ull;                  // the line of the first byte walked
    const int32_t r_begin = (int32_t)((want & ~15ull) - origin); // everything below is relative to origin (< 2^12)
    const int32_t r_lo = (int32_t)(lo - origin);
    const int32_t r_hi = (int32_t)(hi - origin);
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16) + (origin >> 4);
    State s = State();
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
            const bool at_zero = q == 0 && (origin | (uint64_t)line) == 0; // (aligned byte 0: the one chunk with bytes in front)
            uint32_t hits = step.chunk(tab, s, v[q], at_zero ? (uint32_t)a.first : 0u);
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
                for (uint32_t h = hits; h != 0; h &= h - 1u, ++slot, ++ord)
                    if (slot < (uint32_t)TILE_STAGE)
                        stage[slot] = (uint64_t)(pos0 + (uint32_t)__builtin_ctz(h)) | ((uint64_t)ord << 32);
            } else {
                uint64_t idx = base + ord0;
                const uint64_t end0 = origin + (uint64_t)r + a.out_bias;
                for (uint32_t h = hits; h != 0; h &= h - 1u, ++idx)
                    if (idx < a.cap) a.out[idx] = end0 + (uint32_t)__builtin_ctz(h);
            }
        }
    }
    return cnt;
}

// The walk on a Shift-And word of 32 or 64 bits.
template <bool WIDE, int PASS, typename Step>
__device__ __forceinline__ uint32_t shift_and_walk(const TileArgs &a, const Step &step, const uint32_t *tab, uint64_t lo, uint64_t hi,
                                                   uint64_t tile0, uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
    return shift_and_walk_state<ShiftAndState<WIDE>, PASS>(a, step, tab, lo, hi, tile0, stage, stage_n, base);
}

// The frame's policy of a Shift-And search: B in LDS with bit m - 1 in the top bit (WIDE: {low, high} pairs), the walk
// above with Step made from the argument block and the kernel's further arguments.
template <bool WIDE, typename Step>
struct ShiftAndPolicy {
    typedef uint32_t Elem;
    static constexpr int TAB = WIDE ? 512 : 256;
    static __device__ __forceinline__ void fill(uint32_t *tab, const TileArgs &a, uint32_t tid)
    {
        if (WIDE) {
            tab[2 * tid] = (uint32_t)a.peq[tid]; // TILE_BLOCK == 256
            tab[2 * tid + 1] = (uint32_t)(a.peq[tid] >> 32);
        } else {
            tab[tid] = (uint32_t)a.peq[tid];
        }
    }
    template <int PASS, typename... X>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base, const X &...x)
    {
        return shift_and_walk<WIDE, PASS>(a, Step(a, x...), tab, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32); }
    static __device__ __forceinline__ void also(const TileArgs &, uint64_t, uint64_t) {}
};

} // namespace bmx
