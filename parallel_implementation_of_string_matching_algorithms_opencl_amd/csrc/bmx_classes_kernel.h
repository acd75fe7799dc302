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
// Geometry, tile ticket, tagged status words, look-back, parking pool, second walk of a dense tile and the pinned total
// are the approximate search's (bmx_approx_kernel.h), in end coordinates with lead = m - 1: the argument
// block is shared with it, the look-back is bmx_ordered_out.h.  Two things differ:
//  * gather first, then step: a 16-byte chunk reads its 16 B words into registers, then runs its 16 steps with no
//    branch, LDS atomic or store between them; the chunk's 16 hit bits are ANDed with its ownership mask once and only a
//    non-zero mask enters the hit code;
//  * text comes in whole 128-byte lines per lane (eight 16-byte loads issued together), so a line is fetched once.
#pragma once

#include "bmx_approx_kernel.h"

namespace bmx {

constexpr int CLASSES_BLOCK = APPROX_BLOCK;
constexpr int CLASSES_STAGE = APPROX_STAGE;
constexpr int MAX_CLASS_PATTERN = 64; // == BMX_MAX_CLASS_PATTERN

// Shift-And state of one lane; hi is the whole word when m <= 32.
template <bool WIDE>
struct ShiftAndState {
    uint32_t lo, hi;
};

// One 16-byte chunk: gather, then 16 steps.  Returns the hit bits, bit i = the step of byte i.
template <bool WIDE>
__device__ __forceinline__ uint32_t classes_chunk(const uint32_t *tab, ShiftAndState<WIDE> &s, approx_u32x4 v, uint32_t seed)
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

// One lane: the ends [lo, hi) (aligned coordinates), after a warm-up of a.warm = m - 1 bytes (clipped at view byte 0),
// line by line.  Returns the number of hits.  Every 16-byte load holds at least one byte of the view: chunks lie between
// the one that holds the first warm-up byte and the one that holds end hi - 1.
template <bool WIDE, int PASS>
__device__ __forceinline__ uint32_t classes_walk(const ApproxArgs &a, const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                 uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
    const uint64_t want = lo >= a.first + a.warm ? lo - a.warm : a.first;
    const uint64_t origin = want & ~127ull;                  // the line of the first byte walked
    const int32_t r_begin = (int32_t)((want & ~15ull) - origin); // everything below is relative to origin (< 2^12)
    const int32_t r_lo = (int32_t)(lo - origin);
    const int32_t r_hi = (int32_t)(hi - origin);
    const uint32_t seed = 1u << ((WIDE ? 64u : 32u) - a.m);
    const approx_u32x4 *src = reinterpret_cast<const approx_u32x4 *>(a.text16) + (origin >> 4);
    ShiftAndState<WIDE> s;
    s.lo = s.hi = 0;
    uint32_t cnt = 0;
    for (int32_t line = 0; line < r_hi; line += 128, src += 8) {
        approx_u32x4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int32_t r = line + 16 * q;
            if (r >= r_begin && r < r_hi) v[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int32_t r = line + 16 * q;
            if (r < r_begin || r >= r_hi) continue;
            uint32_t hits = classes_chunk<WIDE>(tab, s, v[q], seed);
            const int32_t own_from = min(max(r_lo - r, 0), 16), own_to = min(r_hi - r, 16);
            hits &= ((1u << own_to) - 1u) & ~((1u << own_from) - 1u);
            if (hits == 0) continue; // the usual case, for the whole wave
            const uint32_t ord0 = cnt;
            const uint32_t pc = __builtin_popcount(hits);
            cnt += pc;
            if (PASS == APPROX_PARK) {
                if (a.out == nullptr) continue;
                uint32_t slot = atomicAdd(stage_n, pc);
                const uint32_t pos0 = (uint32_t)(origin - tile0) + (uint32_t)r; // mod 2^32: origin may lie in front of the tile, a hit never
                uint32_t ord = ord0;
                for (uint32_t h = hits; h != 0; h &= h - 1u, ++slot, ++ord)
                    if (slot < (uint32_t)CLASSES_STAGE)
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

template <bool WIDE>
__global__ __launch_bounds__(CLASSES_BLOCK) void classes_kernel(const ApproxArgs a)
{
    __shared__ uint32_t tab[WIDE ? 512 : 256]; // B, bit m - 1 in the top bit (WIDE: {low, high} pairs)
    __shared__ uint64_t stage[CLASSES_STAGE];
    __shared__ uint32_t lane_base[CLASSES_BLOCK]; // hits per lane, then their exclusive scan
    __shared__ uint32_t stage_n;
    __shared__ uint64_t sh_tile, sh_prefix;
    const uint32_t tid = threadIdx.x;
    if (WIDE) {
        tab[2 * tid] = (uint32_t)a.peq[tid]; // CLASSES_BLOCK == 256
        tab[2 * tid + 1] = (uint32_t)(a.peq[tid] >> 32);
    } else {
        tab[tid] = (uint32_t)a.peq[tid];
    }
    const uint32_t ps = a.p_shift;
    for (;;) {
        if (tid == 0) {
            sh_tile = atomicAdd(a.ticket, 1ull) - a.ticket_base; // tiles in ascending order: every predecessor is owned
            stage_n = 0;
        }
        __syncthreads(); // (also: tab, and the previous tile's last reads of the LDS are done)
        const uint64_t t = sh_tile;
        if (t >= a.n_tiles) break;
        const uint64_t tile0 = (a.tile_begin + t) << (ps + 8);
        const uint64_t lo = max(tile0 + ((uint64_t)tid << ps), a.own_lo);
        const uint64_t hi = min(tile0 + ((uint64_t)(tid + 1) << ps), a.own_hi);
        uint32_t cnt = 0;
        if (lo < hi) cnt = classes_walk<WIDE, APPROX_PARK>(a, tab, lo, hi, tile0, stage, &stage_n, 0);
        lane_base[tid] = cnt;
        __syncthreads();
        if (tid < 64) { // wave 0: exclusive scan of the 256 lane counts, then the look-back
            uint32_t v[4], sum = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = lane_base[4 * tid + q], sum += v[q];
            uint32_t incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if ((int)tid >= d) incl += o;
            }
            uint32_t run = incl - sum;
#pragma unroll
            for (int q = 0; q < 4; ++q) lane_base[4 * tid + q] = run, run += v[q];
            const uint64_t agg = (uint64_t)__shfl(incl, 63);
            if (tid == 0) {
                const uint64_t prefix = ordered_lookback(a, t, agg);
                ordered_publish_total(a, t, prefix + agg);
                sh_prefix = prefix;
            }
        }
        __syncthreads();
        const uint64_t prefix = sh_prefix;
        const uint32_t parked = stage_n;
        if (a.out != nullptr && prefix < a.cap) { // (a tile that starts at or past the capacity stores nothing)
            if (parked <= (uint32_t)CLASSES_STAGE) {
                for (uint32_t j = tid; j < parked; j += CLASSES_BLOCK) {
                    const uint64_t e = stage[j];
                    const uint32_t pos = (uint32_t)e;
                    const uint64_t idx = prefix + lane_base[pos >> ps] + (uint32_t)(e >> 32);
                    if (idx < a.cap) a.out[idx] = tile0 + pos + a.out_bias;
                }
            } else if (lo < hi) { // dense tile: walk it again, writing every hit to its slot
                (void)classes_walk<WIDE, APPROX_WRITE>(a, tab, lo, hi, tile0, stage, &stage_n, prefix + lane_base[tid]);
            }
        }
        __syncthreads(); // the pool, the lane bases and stage_n are the next tile's
    }
}

} // namespace bmx
