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
// M - 1 bytes before its first end is exact from there on.  The tile loop, the ordered output and the argument block are
// therefore bmx_tile_frame.h's and the lane's walk and the policy are the class search's (bmx_classes_kernel.h, DESIGN.md
// s13, s20, s21) with the step below; the four mask words come as a second kernel argument.  As there, everything is
// shifted up so that bit M - 1 is the TOP bit of the word (32 bits for M <= 32, two halves for 33..64), a chunk gathers its
// 16 B words and then runs 16 steps with no branch, LDS atomic or store between them.
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
__device__ __forceinline__ uint32_t gaps_chunk(const uint32_t *tab, const GapsMasks &k, ShiftAndState<WIDE> &s, tile_u32x4 v)
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
__device__ __forceinline__ uint32_t gaps_chunk_head(const uint32_t *tab, const GapsMasks &k, ShiftAndState<WIDE> &s, tile_u32x4 v,
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

// The gapped search's step for the shared walk: the head chunk where bytes lie in front of the view, the unrolled one
// everywhere else.  (A warm-up that begins earlier inside the view is harmless: D = 0 there is a subset of the truth.)
template <bool WIDE>
struct GapsStep {
    const GapsMasks &k;
    __device__ __forceinline__ GapsStep(const TileArgs &, const GapsMasks &masks) : k(masks) {}
    __device__ __forceinline__ uint32_t chunk(const uint32_t *tab, ShiftAndState<WIDE> &s, tile_u32x4 v, uint32_t skip) const
    {
        return skip != 0 ? gaps_chunk_head<WIDE>(tab, k, s, v, skip) : gaps_chunk<WIDE>(tab, k, s, v);
    }
};

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
