// bmx_regex_kernel.h -- regular-expression search (bmx_search_regex_device, bmx_regex_starts_device): the star-free
// expressions, given as their Glushkov (position) automaton: `first`, `last`, follow[] and one class per position.  Every
// END j of the view at which some text[s..j] matches is reported once, ascending.  No counterpart in the reference.
//
// Bit i of D says "position i has just consumed the current byte on some path that began in `first`".  Per text byte c
//     D = (first | Follow(D)) & B[c]            end j is a hit iff (D & last) != 0
//     Follow(D) = ((D & lin) << 1) | OR over the bytes b of the word with nl != 0 there:  T_b[ byte b of (D & nl) ]
// with B[c] the positions whose class holds c, lin the positions i with follow[i] == {i + 1}, nl the other positions with
// a successor, and T_b[v] the OR of follow[8b + t] over the bits t of v (Navarro and Raffinot, Flexible Pattern Matching in
// Strings, 2002, s5.4, with the table cut into bytes and the regular part taken out as a shift).  A literal or a class
// pattern has nl == 0 and steps like the class search; an alternation or an optional group costs one LDS read per byte of
// the word that holds one of its irregular positions.  Which bytes those are is the same for the whole grid: a scalar
// branch.  In front of the reads stands one test per step and wave, "does any lane stand on an irregular position": in
// sparse text none does almost always, and the step then costs the shift, the test and the branch.  Position i is bit i
// of the word (32 bits for m <= 32, two halves for 33..64); the hit is a mask test, so nothing needs to sit in the top bit.
//
// follow[] points upward only, so a match visits a position at most once and spans at most max_len <= m bytes: a lane
// that starts with D = 0 at least max_len - 1 bytes before its first end is exact from there on.  The tile loop, the
// ordered output and the argument block are bmx_tile_frame.h's and the lane's walk is the class search's
// (bmx_classes_kernel.h) with the step below.  B travels in TileArgs::peq; the sets travel as a second kernel argument
// and the workgroup builds the T_b tables in LDS from them, lane tid entry tid of each.  As in the gapped search a chunk
// gathers its 16 B words first; the T_b reads depend on D and sit inside the chain of steps.  The bytes in front of an
// unaligned view are stepped with an empty B word: a match shorter than max_len that begins out there must not end on
// one of the first ends.
//
// Starts (regex_starts_kernel): one list entry per lane.  The lane runs the REVERSED automaton (position i becomes
// m - 1 - i, first and last swap, follow is transposed: upward again) against text[j], text[j - 1], ... for at most
// max_len bytes, anchored: `first` enters at the first step only.  (D & last) != 0 after L bytes says that
// text[j - L + 1 .. j] matches.  Text comes as aligned 8-byte words, downwards, one word ahead; a word below text[0]'s
// 16-byte line is never loaded and an entry whose end is outside the view reads no byte.
#pragma once

#include "bmx_classes_kernel.h"

namespace bmx {

constexpr int MAX_REGEX_POSITIONS = 64; // == BMX_MAX_REGEX_POSITIONS
constexpr int REGEX_STARTS_BLOCK = 256;
constexpr uint64_t REGEX_BAD_END = 1, REGEX_BAD_START = 2; // status bits of the starts kernel (ws[0])

// The sets of the automaton, bit i = position i (the low word is the whole word when m <= 32).
struct RegexSets {
    uint64_t first, last, lin, nl;
    uint32_t nl_bytes; // bit b: byte b of nl is non-zero
    uint32_t pad;
    uint64_t follow[MAX_REGEX_POSITIONS];
};

// entry v of T_b: the OR of follow[8b + t] over the bits t of v
__device__ __forceinline__ uint64_t regex_table_entry(const uint64_t *follow, uint32_t b, uint32_t v)
{
    uint64_t f = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t)
        if ((v >> t) & 1u) f |= follow[8 * b + t];
    return f;
}

// One text byte on the B word {blo, bhi} of the byte (bhi alone when !WIDE).  tt: the T_b tables, 256 words each (WIDE:
// 256 {low, high} pairs), for b = 0..3 (WIDE: 0..7).  Returns D & last, folded into one word.
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_step(const RegexSets &k, const uint32_t *tt, ShiftAndState<WIDE> &s, uint32_t blo, uint32_t bhi)
{
    if (WIDE) {
        const uint32_t llo = s.lo & (uint32_t)k.lin, lhi = s.hi & (uint32_t)(k.lin >> 32);
        uint32_t flo = (llo << 1) | (uint32_t)k.first;
        uint32_t fhi = __builtin_amdgcn_alignbit(lhi, llo, 31) | (uint32_t)(k.first >> 32);
        if (NL) {
            const uint32_t xlo = s.lo & (uint32_t)k.nl, xhi = s.hi & (uint32_t)(k.nl >> 32);
            if (__builtin_amdgcn_ballot_w64((xlo | xhi) != 0) != 0) { // some lane of the wave stands on an irregular position
                const uint2 *t2 = reinterpret_cast<const uint2 *>(tt);
#pragma unroll
                for (uint32_t b = 0; b < 8; ++b) {
                    if ((k.nl_bytes >> b) & 1u) { // (the same for every lane of the grid)
                        const uint2 w = t2[256 * b + __builtin_amdgcn_ubfe(b < 4 ? xlo : xhi, 8 * (b & 3), 8)];
                        flo |= w.x;
                        fhi |= w.y;
                    }
                }
            }
        }
        s.lo = flo & blo;
        s.hi = fhi & bhi;
        return (s.lo & (uint32_t)k.last) | (s.hi & (uint32_t)(k.last >> 32));
    } else {
        uint32_t f = ((s.hi & (uint32_t)k.lin) << 1) | (uint32_t)k.first;
        if (NL) {
            const uint32_t x = s.hi & (uint32_t)k.nl;
            if (__builtin_amdgcn_ballot_w64(x != 0) != 0) { // some lane of the wave stands on an irregular position
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b)
                    if ((k.nl_bytes >> b) & 1u) f |= tt[256 * b + __builtin_amdgcn_ubfe(x, 8 * b, 8)];
            }
        }
        s.hi = f & bhi;
        return s.hi & (uint32_t)k.last;
    }
}

// One 16-byte chunk: gather, then 16 steps.  Returns the hit bits, bit i = the step of byte i.
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_chunk(const uint32_t *tab, const RegexSets &k, ShiftAndState<WIDE> &s, tile_u32x4 v)
{
    const uint32_t *tt = tab + (WIDE ? 512 : 256);
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
    uint32_t hits = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) hits |= (regex_step<WIDE, NL>(k, tt, s, blo[i], bhi[i]) != 0 ? 1u : 0u) << i;
    return hits;
}

// The chunk that holds view byte 0 when the view does not begin on a 16-byte line: its first `skip` bytes lie in front of
// the view and are stepped with an empty B word, which leaves D = 0.  One chunk per call, so a plain loop.
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_chunk_head(const uint32_t *tab, const RegexSets &k, ShiftAndState<WIDE> &s, tile_u32x4 v,
                                                     uint32_t skip)
{
    const uint32_t *tt = tab + (WIDE ? 512 : 256);
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
        hits |= (regex_step<WIDE, NL>(k, tt, s, blo, bhi) != 0 ? 1u : 0u) << i;
    }
    return hits;
}

// The step for the shared walk: the head chunk where bytes lie in front of the view, the unrolled one everywhere else.
template <bool WIDE, bool NL>
struct RegexStep {
    const RegexSets &k;
    __device__ __forceinline__ RegexStep(const TileArgs &, const RegexSets &sets) : k(sets) {}
    __device__ __forceinline__ uint32_t chunk(const uint32_t *tab, ShiftAndState<WIDE> &s, tile_u32x4 v, uint32_t skip) const
    {
        return skip != 0 ? regex_chunk_head<WIDE, NL>(tab, k, s, v, skip) : regex_chunk<WIDE, NL>(tab, k, s, v);
    }
};

// The frame's policy: B as in ShiftAndPolicy (bit i = position i), behind it the T_b tables where the automaton has
// irregular positions (NL), built from the sets.
template <bool WIDE, bool NL>
struct RegexPolicy {
    typedef uint32_t Elem;
    static constexpr bool FILL_TAKES_X = true;
    static constexpr int B_WORDS = WIDE ? 512 : 256;
    static constexpr int TAB = B_WORDS + (NL ? (WIDE ? 8 * 512 : 4 * 256) : 0);
    static __device__ __forceinline__ void fill(uint32_t *tab, const TileArgs &a, uint32_t tid, const RegexSets &k)
    {
        if (WIDE) {
            tab[2 * tid] = (uint32_t)a.peq[tid]; // TILE_BLOCK == 256
            tab[2 * tid + 1] = (uint32_t)(a.peq[tid] >> 32);
        } else {
            tab[tid] = (uint32_t)a.peq[tid];
        }
        if (NL) {
            uint32_t *tt = tab + B_WORDS;
#pragma unroll 1
            for (uint32_t b = 0; b < (WIDE ? 8u : 4u); ++b) {
                if (!((k.nl_bytes >> b) & 1u)) continue; // (never read)
                const uint64_t f = regex_table_entry(k.follow, b, tid);
                if (WIDE) {
                    tt[512 * b + 2 * tid] = (uint32_t)f;
                    tt[512 * b + 2 * tid + 1] = (uint32_t)(f >> 32);
                } else {
                    tt[256 * b + tid] = (uint32_t)f;
                }
            }
        }
    }
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base, const RegexSets &k)
    {
        return shift_and_walk<WIDE, PASS>(a, RegexStep<WIDE, NL>(a, k), tab, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32); }
    static __device__ __forceinline__ void also(const TileArgs &, uint64_t, uint64_t) {}
};

struct RegexStartsArgs {
    const uint8_t *text16; // the 16-byte line that holds text[0]
    uint64_t first;        // text[0] is text16[first]
    uint64_t n, base;
    const uint64_t *ends;
    uint64_t count;
    uint64_t *starts;
    uint64_t *ws;          // [0]: status bits
    uint32_t max_len, chunks; // chunks = ceil(max_len / 8)
    uint32_t longest, pad;
    RegexSets k;           // of the REVERSED automaton
    uint64_t peq[256];     // bit i set: byte belongs to position m - 1 - i (low word used when m <= 32)
};

template <typename W>
__global__ __launch_bounds__(REGEX_STARTS_BLOCK) void regex_starts_kernel(const RegexStartsArgs a)
{
    constexpr uint32_t NB = sizeof(W); // bytes of the word: one T_b table each
    __shared__ W peq[256];
    __shared__ W tt[NB * 256];
    const uint32_t tid = threadIdx.x;
    peq[tid] = (W)a.peq[tid]; // REGEX_STARTS_BLOCK == 256
#pragma unroll 1
    for (uint32_t b = 0; b < NB; ++b) tt[256 * b + tid] = (W)regex_table_entry(a.k.follow, b, tid);
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * REGEX_STARTS_BLOCK + tid;
    if (i >= a.count) return;

    const uint64_t e = a.ends[i];
    const uint64_t j = e - a.base;
    const bool valid = e >= a.base && j < a.n;
    uint32_t steps = 0, b = 0;
    int64_t wi = -1; // index of the 8-byte word that holds text[j], counted from text16
    if (valid) {
        steps = (uint32_t)min(j + 1, (uint64_t)a.max_len); // the window is clipped at text[0]
        const uint64_t q = a.first + j;
        wi = (int64_t)(q >> 3);
        b = (uint32_t)(q & 7);
    } else {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_BAD_END); // no byte is read for this entry
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t hi = valid ? words[wi] : 0;               // text[j] is byte b of hi
    uint64_t lo = valid && wi > 0 ? words[wi - 1] : 0; // word 0 lies in text[0]'s line: nothing below it is loaded

    const W lin = (W)a.k.lin, nl = (W)a.k.nl, last = (W)a.k.last;
    const uint32_t nl_bytes = a.k.nl_bytes;
    W d = 0, seed = (W)a.k.first; // anchored at text[j]: `first` enters the first step only
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
            W f = (W)((d & lin) << 1) | seed;
            seed = 0;
            const W x = d & nl;
#pragma unroll
            for (uint32_t q = 0; q < NB; ++q)
                if ((nl_bytes >> q) & 1u) f |= tt[256 * q + ((uint32_t)(x >> (8 * q)) & 0xFFu)];
            d = f & eq[t];
            ++len;
            if (len <= steps && (d & last) != 0) { // text[j - len + 1 .. j] matches
                if (first_len == 0) first_len = len;
                last_len = len;
            }
        }
    }
    if (!valid) return;
    if (first_len == 0) {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_BAD_START);
        a.starts[i] = e;
        return;
    }
    a.starts[i] = e - ((a.longest ? last_len : first_len) - 1);
}

} // namespace bmx
