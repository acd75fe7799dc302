// bmx_gaps_kernel.h -- gapped pattern search (bmx_search_gaps_device, bmx_gaps_starts_device): class patterns whose
// positions may be OPTIONAL, so that a{2,4}, x(3,5) and colou?r are one pattern.  Every END j of the view at which some
// text[s..j] matches is reported once, ascending.  No counterpart in the reference.
//
// The recurrence is the extended Shift-And of Navarro and Raffinot (Flexible Pattern Matching in Strings, 2002, s4.3),
// restricted to bounded repetition: bit i of D says "position i has just been consumed, or is reachable from such a
// position over optional ones".  Per text byte c
//     D  = ((D << 1) | S) & B[c]
//     Df = D | F
//     D  = D | (O & ~((Df - I) ^ Df))
// with B[c] the positions whose class holds c, O the optional positions, F the last position of every maximal block of
// consecutive optional positions, I the position just below every block (position 0 itself for a block that starts there)
// and S the positions 0..b, b the first mandatory one: those a match may begin with.  The subtraction runs a borrow from
// I upwards to the lowest active bit of its block (or to F, which stops it), and the XOR marks what it passed: every
// optional position above an active one, within the block only.  End j is a hit iff bit M - 1 of D is set.
//
// A match spans at most M bytes, so bit M - 1 depends on the last M bytes only and a lane that starts with D = 0 at least
// M - 1 bytes before its first end is exact from there on.  Geometry, tile ticket, look-back, parking pool, second walk of
// a dense tile and the pinned total are therefore the class kernel's (bmx_classes_kernel.h) with the
// same argument block; the four mask words come as a second kernel argument.  As there, everything is shifted up so that
// bit M - 1 is the TOP bit of the word (32 bits for M <= 32, two halves for 33..64), a chunk gathers its 16 B words and then
// runs 16 steps with no branch, LDS atomic or store between them, and text comes in whole 128-byte lines per lane.
//
// Starts (gaps_starts_kernel): one list entry per lane.  The lane runs the same recurrence over the REVERSED positions
// against text[j], text[j - 1], ... for at most M bytes, anchored: S enters at the first step only.  The top bit after L
// bytes says that text[j - L + 1 .. j] matches.  Text comes as aligned 8-byte words, downwards, one word ahead; a word
// below text[0]'s 16-byte line is never loaded and an entry whose end is outside the view reads no byte.
#pragma once

#include "bmx_classes_kernel.h"

namespace bmx {

constexpr int MAX_GAPS_PATTERN = 64; // == BMX_MAX_GAPS_PATTERN
constexpr int GAPS_STARTS_BLOCK = 256;
constexpr uint64_t GAPS_BAD_END = 1, GAPS_BAD_START = 2; // status bits of the starts kernel (ws[0])

// O, I, F, S of the recurrence, shifted up like B (the low word is the whole word when M <= 32).
struct GapsMasks {
    uint64_t opt, below, last, seed;
};

// One text byte: the three lines above on the B word {blo, bhi} of the byte (bhi alone when M <= 32).
template <bool WIDE>
__device__ __forceinline__ void gaps_step(const GapsMasks &k, ShiftAndState<WIDE> &s, uint32_t blo, uint32_t bhi)
{
    if (WIDE) {
        const uint32_t nhi = __builtin_amdgcn_alignbit(s.hi, s.lo, 31) | (uint32_t)(k.seed >> 32);
        const uint32_t lo = ((s.lo << 1) | (uint32_t)k.seed) & blo;
        const uint32_t hi = nhi & bhi;
        const uint32_t dflo = lo | (uint32_t)k.last, dfhi = hi | (uint32_t)(k.last >> 32);
        const uint64_t x = (((uint64_t)dfhi << 32) | dflo) - k.below; // (the borrow crosses the halves: one carry chain)
        s.lo = lo | ((uint32_t)k.opt & ~((uint32_t)x ^ dflo));
        s.hi = hi | ((uint32_t)(k.opt >> 32) & ~((uint32_t)(x >> 32) ^ dfhi));
    } else {
        const uint32_t d = ((s.hi << 1) | (uint32_t)k.seed) & bhi;
        const uint32_t df = d | (uint32_t)k.last;
        s.hi = d | ((uint32_t)k.opt & ~((df - (uint32_t)k.below) ^ df));
    }
}

// One 16-byte chunk: gather, then 16 steps.  Returns the hit bits, bit i = the step of byte i.
template <bool WIDE>
__device__ __forceinline__ uint32_t gaps_chunk(const uint32_t *tab, const GapsMasks &k, ShiftAndState<WIDE> &s, approx_u32x4 v)
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
            blo[i] = 0;
            bhi[i] = tab[byte];
        }
    }
    uint32_t hits = 0; // step i lands in bit 15 - i, turned round below
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        gaps_step<WIDE>(k, s, blo[i], bhi[i]);
        hits = __builtin_amdgcn_alignbit(hits, s.hi, 31); // (hits << 1) | top bit of the word
    }
    return __builtin_bitreverse32(hits) >> 16;
}

// The chunk that holds view byte 0 when the view does not begin on a 16-byte line: its first `skip` bytes lie in front of
// the view.  A class search may walk them (a window of exactly m bytes that ends inside the view begins inside it), this
// one may not: a shorter match that begins out there could end on one of the first ends.  One chunk per call, so a plain
// loop: the bytes in front of the view are stepped with an empty B word, which leaves D = 0.
template <bool WIDE>
__device__ __forceinline__ uint32_t gaps_chunk_head(const uint32_t *tab, const GapsMasks &k, ShiftAndState<WIDE> &s, approx_u32x4 v,
                                                    uint32_t skip)
{
    uint32_t hits = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t byte = v[0] & 0xFFu;
        v[0] = __builtin_amdgcn_alignbit(v[1], v[0], 8);
        v[1] = __builtin_amdgcn_alignbit(v[2], v[1], 8);
        v[2] = __builtin_amdgcn_alignbit(v[3], v[2], 8);
        v[3] >>= 8;
        uint32_t blo = 0, bhi;
        if (WIDE) {
            const uint2 w = reinterpret_cast<const uint2 *>(tab)[byte];
            blo = w.x;
            bhi = w.y;
        } else {
            bhi = tab[byte];
        }
        if (i < skip) blo = bhi = 0;
        gaps_step<WIDE>(k, s, blo, bhi);
        hits |= (s.hi >> 31) << i;
    }
    return hits;
}

// gaps_walk and gaps_kernel below are COPIES of classes_walk and classes_kernel (bmx_classes_kernel.h) that differ in the
// step, the head chunk and the second kernel argument only: a fix to the parking, the second walk or the scan of the lane
// counts there has to be made here too, and the other way round, until the two share one template.
//
// One lane: the ends [lo, hi) (aligned coordinates), after a warm-up of a.warm = M - 1 bytes (clipped at view byte 0),
// line by line: classes_walk with the step above and the head chunk.  Returns the number of hits.  Every 16-byte load
// holds at least one byte of the view: chunks lie between the one that holds the first warm-up byte and the one that
// holds end hi - 1.  A warm-up that begins earlier inside the view is harmless (D = 0 there is a subset of the truth).
template <bool WIDE, int PASS>
__device__ __forceinline__ uint32_t gaps_walk(const ApproxArgs &a, const GapsMasks &k, const uint32_t *tab, uint64_t lo, uint64_t hi,
                                              uint64_t tile0, uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
    const uint64_t want = lo >= a.first + a.warm ? lo - a.warm : a.first;
    const uint64_t origin = want & ~127ull;                  // the line of the first byte walked
    const int32_t r_begin = (int32_t)((want & ~15ull) - origin); // everything below is relative to origin (< 2^12)
    const int32_t r_lo = (int32_t)(lo - origin);
    const int32_t r_hi = (int32_t)(hi - origin);
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
            uint32_t hits;
            if (q == 0 && (origin | (uint64_t)line) == 0 && a.first != 0) // (aligned byte 0: the one chunk with bytes in front)
                hits = gaps_chunk_head<WIDE>(tab, k, s, v[0], (uint32_t)a.first);
            else
                hits = gaps_chunk<WIDE>(tab, k, s, v[q]);
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
__global__ __launch_bounds__(CLASSES_BLOCK) void gaps_kernel(const ApproxArgs a, const GapsMasks k)
{
    __shared__ uint32_t tab[WIDE ? 512 : 256]; // B, bit M - 1 in the top bit (WIDE: {low, high} pairs)
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
        if (lo < hi) cnt = gaps_walk<WIDE, APPROX_PARK>(a, k, tab, lo, hi, tile0, stage, &stage_n, 0);
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
                (void)gaps_walk<WIDE, APPROX_WRITE>(a, k, tab, lo, hi, tile0, stage, &stage_n, prefix + lane_base[tid]);
            }
        }
        __syncthreads(); // the pool, the lane bases and stage_n are the next tile's
    }
}

struct GapsStartsArgs {
    const uint8_t *text16; // the 16-byte line that holds text[0]
    uint64_t first;        // text[0] is text16[first]
    uint64_t n, base;
    const uint64_t *ends;
    uint64_t count;
    uint64_t *starts;
    uint64_t *ws;          // [0]: status bits
    uint32_t m, chunks;    // chunks = ceil(M / 8)
    uint32_t longest;
    GapsMasks k;           // of the REVERSED positions, bit M - 1 in the top bit of the word
    uint64_t peq[256];     // bit i + up set: byte belongs to position M - 1 - i (low word used when M <= 32)
};

template <typename W>
__global__ __launch_bounds__(GAPS_STARTS_BLOCK) void gaps_starts_kernel(const GapsStartsArgs a)
{
    __shared__ W peq[256];
    const uint32_t tid = threadIdx.x;
    peq[tid] = (W)a.peq[tid]; // GAPS_STARTS_BLOCK == 256
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * GAPS_STARTS_BLOCK + tid;
    if (i >= a.count) return;

    const uint64_t e = a.ends[i];
    const uint64_t j = e - a.base;
    const bool valid = e >= a.base && j < a.n;
    uint32_t steps = 0, b = 0;
    int64_t wi = -1; // index of the 8-byte word that holds text[j], counted from text16
    if (valid) {
        steps = (uint32_t)min(j + 1, (uint64_t)a.m); // the window is clipped at text[0]
        const uint64_t q = a.first + j;
        wi = (int64_t)(q >> 3);
        b = (uint32_t)(q & 7);
    } else {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)GAPS_BAD_END); // no byte is read for this entry
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t hi = valid ? words[wi] : 0;               // text[j] is byte b of hi
    uint64_t lo = valid && wi > 0 ? words[wi - 1] : 0; // word 0 lies in text[0]'s line: nothing below it is loaded

    const W opt = (W)a.k.opt, below = (W)a.k.below, last = (W)a.k.last;
    const uint32_t top = 8 * sizeof(W) - 1;
    W d = 0, seed = (W)a.k.seed; // anchored at text[j]: the seed enters the first step only
    uint32_t first_len = 0, last_len = 0, len = 0;
    for (uint32_t c = 0; c < a.chunks; ++c) {
        // the next 8 bytes downwards from text[j - 8c], the first of them in the top byte
        const uint64_t cur = (hi << (8 * (7 - b))) | ((lo >> (8 * b)) >> 8);
        hi = lo;
        --wi;
        lo = valid && wi > 0 ? words[wi - 1] : 0; // one word ahead of its use
        W eq[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) eq[t] = peq[(uint32_t)(cur >> (8 * (7 - t))) & 0xFFu];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            d = ((W)(d << 1) | seed) & eq[t];
            seed = 0;
            const W df = d | last;
            d |= opt & ~((W)(df - below) ^ df);
            ++len;
            if (len <= steps && ((d >> top) & 1)) { // text[j - len + 1 .. j] matches
                if (first_len == 0) first_len = len;
                last_len = len;
            }
        }
    }
    if (!valid) return;
    if (first_len == 0) {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)GAPS_BAD_START);
        a.starts[i] = e;
        return;
    }
    a.starts[i] = e - ((a.longest ? last_len : first_len) - 1);
}

} // namespace bmx
