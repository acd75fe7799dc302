// bmx_regex_anchored_kernel.h -- anchored regular-expression search (bmx_search_regex_anchored_device,
// bmx_regex_anchored_starts_device; behind them the mirror image, bmx_search_regex_anchored_begins_device and
// bmx_regex_anchored_ends_device): the star-free automaton of bmx_regex_kernel.h with a condition on the byte BEFORE a
// match for every position of `first` and on the byte AFTER it for every position of `last` (struct bmx_regex_anchors:
// ^ $ \b \B \< \>, grep -w, grep -x).  Every END j of the view at which an anchored match ends, once, ascending.
//
//     D = (Follow(D) | E[previous byte]) & B[c]            end j is a hit iff (D_j & A[text[j + 1]]) != 0
// E[v]: the positions of `first` whose `before` class holds v; A[v]: the positions of `last` whose `after` class holds v
// (so `first` and `last` themselves are no longer in the step).  The gate stands where a path enters through `first` or
// leaves through `last`, not where the same position is reached through follow[].  Follow, the T_b tables and the wave
// test for irregular positions are bmx_regex_kernel.h's; E and A are two more tables of 256 words behind them in LDS
// and a chunk gathers the three words of each of its bytes before its steps, in two halves of eight.
//
//  * The tables do not fit into the kernel arguments: the host puts them into a device buffer on the call's stream and
//    the workgroup copies them to LDS in fill (RegexGate::tabs).
//  * Look-behind.  A lane carries the E word of the byte it has just stepped.  Its warm-up is max_len bytes, one more
//    than the plain search's: the first byte walked enters nothing (the carried word is empty there), and a match that
//    begins on it ends before the lane's first owned end.  A lane whose walk begins at view byte 0 carries E[left].
//  * Look-ahead.  The hit of end j is known at the step of byte j + 1: step i of a chunk returns the hit of the byte
//    BEFORE it, so bit i of a chunk at r belongs to position r - 1 + i, and the ownership mask is laid over those
//    positions: a delayed bit is never given to a position outside [lo, hi) or in front of the tile.  A lane that owns
//    [lo, hi) therefore steps byte hi as well when it lies inside the view (the chunk that holds it holds a view byte).
//    At the view's end `right` stands in: the chunk with bytes past the view takes A[right] for the first of them, and
//    where the view ends on a 16-byte line the lane tests its last state against A[right] after its last chunk.
//  * The bytes in front of an unaligned view are stepped with an empty B word and E[left], the bytes behind it with an
//    empty B word: one chunk at either end of the view takes the plain loop (regex_anchored_chunk_edge).
//
// Starts (regex_anchored_starts_kernel): one list entry per lane over the REVERSED automaton as in regex_starts_kernel.
// The seed is first_rev & A_rev[next(j)]; a length L is accepted where (D & E_rev[byte below the match]) != 0, which the
// lane learns one step later, from the byte it gathers anyway; at the view's first byte `left` stands in.  No byte
// outside the aligned 16-byte lines that hold the view is read.
#pragma once

#include "bmx_regex_begins_kernel.h"

namespace bmx {

// The gate tables in device memory, 256 words of 64 bits each: E, A (bit i = position i), then A and E once more with
// bit i = position m - 1 - i for the passes that run the reversed automaton (where A gates the entry and E the hit).
constexpr int REGEX_GATE_WORDS = 4 * 256;
struct RegexGate {
    const uint64_t *tabs;
    uint32_t left, right; // the bytes next to the view
};

template <bool WIDE>
struct RegexAnchoredState {
    ShiftAndState<WIDE> d;
    uint32_t elo, ehi; // E of the byte stepped last (ehi alone when !WIDE)
};

// One text byte with the words {blo, bhi}, {eclo, echi}, {alo, ahi} of B, E and A at it (the high ones alone when !WIDE).
// Returns the hit of the byte BEFORE it: D & A[this byte], folded into one word.
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_anchored_step(const RegexSets &k, const uint32_t *tt, RegexAnchoredState<WIDE> &s, uint32_t blo,
                                                        uint32_t bhi, uint32_t eclo, uint32_t echi, uint32_t alo, uint32_t ahi)
{
    if (WIDE) {
        const uint32_t hit = (s.d.lo & alo) | (s.d.hi & ahi);
        const uint32_t llo = s.d.lo & (uint32_t)k.lin, lhi = s.d.hi & (uint32_t)(k.lin >> 32);
        uint32_t flo = (llo << 1) | s.elo;
        uint32_t fhi = __builtin_amdgcn_alignbit(lhi, llo, 31) | s.ehi;
        if (NL) {
            const uint32_t xlo = s.d.lo & (uint32_t)k.nl, xhi = s.d.hi & (uint32_t)(k.nl >> 32);
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
        s.d.lo = flo & blo;
        s.d.hi = fhi & bhi;
        s.elo = eclo;
        s.ehi = echi;
        return hit;
    } else {
        const uint32_t hit = s.d.hi & ahi;
        uint32_t f = ((s.d.hi & (uint32_t)k.lin) << 1) | s.ehi;
        if (NL) {
            const uint32_t x = s.d.hi & (uint32_t)k.nl;
            if (__builtin_amdgcn_ballot_w64(x != 0) != 0) { // some lane of the wave stands on an irregular position
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b)
                    if ((k.nl_bytes >> b) & 1u) f |= tt[256 * b + __builtin_amdgcn_ubfe(x, 8 * b, 8)];
            }
        }
        s.d.hi = f & bhi;
        s.ehi = echi;
        return hit;
    }
}

// The LDS table: B, the T_b tables (NL), E, A.
template <bool WIDE, bool NL>
struct RegexAnchoredTab {
    static constexpr int B_WORDS = WIDE ? 512 : 256;
    static constexpr int E_AT = RegexPolicy<WIDE, NL>::TAB, A_AT = E_AT + B_WORDS, TAB = A_AT + B_WORDS;
    // the word pair of table `at` for byte value v
    static __device__ __forceinline__ void word(const uint32_t *tab, int at, uint32_t v, uint32_t &lo, uint32_t &hi)
    {
        if (WIDE) {
            const uint2 w = reinterpret_cast<const uint2 *>(tab + at)[v];
            lo = w.x;
            hi = w.y;
        } else {
            lo = 0;
            hi = tab[at + v];
        }
    }
};

// One 16-byte chunk: twice gather eight bytes, then their steps.  Returns the delayed hit bits: bit i = the byte before byte i.
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_anchored_chunk(const uint32_t *tab, const RegexSets &k, RegexAnchoredState<WIDE> &s, tile_u32x4 v)
{
    typedef RegexAnchoredTab<WIDE, NL> T;
    const uint32_t *tt = tab + T::B_WORDS;
    uint32_t hits = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t blo[8], bhi[8], elo[8], ehi[8], alo[8], ahi[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t byte = __builtin_amdgcn_ubfe(v[2 * h + (i >> 2)], 8 * (i & 3), 8);
            T::word(tab, 0, byte, blo[i], bhi[i]);
            T::word(tab, T::E_AT, byte, elo[i], ehi[i]);
            T::word(tab, T::A_AT, byte, alo[i], ahi[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            hits |= (regex_anchored_step<WIDE, NL>(k, tt, s, blo[i], bhi[i], elo[i], ehi[i], alo[i], ahi[i]) != 0 ? 1u : 0u) << (8 * h + i);
    }
    return hits;
}

// A chunk at an end of the view: its first `skip` bytes lie in front of the view (an empty B word, and E[left] as the
// word carried into view byte 0), its bytes from `keep` on lie behind it (an empty B word, and A[right] as what the
// view's last byte sees).  At most two chunks per lane and call, so a plain loop.
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_anchored_chunk_edge(const uint32_t *tab, const RegexSets &k, RegexAnchoredState<WIDE> &s,
                                                              tile_u32x4 v, uint32_t skip, uint32_t keep, const RegexGate &g)
{
    typedef RegexAnchoredTab<WIDE, NL> T;
    const uint32_t *tt = tab + T::B_WORDS;
    uint32_t hits = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t byte = v[0] & 0xFFu;
        v[0] = __builtin_amdgcn_alignbit(v[1], v[0], 8);
        v[1] = __builtin_amdgcn_alignbit(v[2], v[1], 8);
        v[2] = __builtin_amdgcn_alignbit(v[3], v[2], 8);
        v[3] >>= 8;
        const bool in_view = i >= skip && i < keep;
        uint32_t blo, bhi, elo, ehi, alo, ahi;
        T::word(tab, 0, byte, blo, bhi);
        T::word(tab, T::E_AT, i < skip ? g.left : byte, elo, ehi);
        T::word(tab, T::A_AT, i >= keep ? g.right : byte, alo, ahi);
        if (!in_view) blo = bhi = 0;
        hits |= (regex_anchored_step<WIDE, NL>(k, tt, s, blo, bhi, elo, ehi, alo, ahi) != 0 ? 1u : 0u) << i;
    }
    return hits;
}

// One lane: the ends [lo, hi) (aligned coordinates), after a warm-up of a.warm = max_len bytes (clipped at view byte 0),
// line by line as in shift_and_walk.  Every 16-byte load holds a byte of the view.
template <bool WIDE, bool NL, int PASS>
__device__ __forceinline__ uint32_t regex_anchored_walk(const TileArgs &a, const RegexSets &k, const RegexGate &g, const uint32_t *tab,
                                                        uint64_t lo, uint64_t hi, uint64_t tile0, uint64_t *stage, uint32_t *stage_n,
                                                        uint64_t base)
{
    typedef RegexAnchoredTab<WIDE, NL> T;
    const uint64_t want = lo >= a.first + a.warm ? lo - a.warm : a.first;
    const uint64_t origin = want & ~127ull;                      // the line of the first byte walked
    const int32_t r_begin = (int32_t)((want & ~15ull) - origin); // everything below is relative to origin (< 2^13)
    const int32_t r_lo = (int32_t)(lo - origin);
    const int32_t r_hi = (int32_t)(hi - origin);
    const bool at_view_end = hi == a.own_hi;                     // no byte hi: `right` stands in
    const int32_t r_end = r_hi + (at_view_end ? 0 : 1);          // one past the last byte stepped
    const int32_t r_view_hi = (int32_t)min(a.own_hi - origin, (uint64_t)0x7fffffff);
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16) + (origin >> 4);
    RegexAnchoredState<WIDE> s;
    s.d.lo = s.d.hi = 0;
    s.elo = s.ehi = 0;
    if (want == a.first) T::word(tab, T::E_AT, g.left, s.elo, s.ehi); // the walk begins on view byte 0
    uint32_t cnt = 0;
    // the hits `hits` of the positions r_at + bit (relative to origin)
    const auto emit = [&](uint32_t hits, int32_t r_at) {
        const uint32_t ord0 = cnt;
        const uint32_t pc = __builtin_popcount(hits);
        cnt += pc;
        if (PASS == TILE_PARK) {
            if (a.out == nullptr) return;
            uint32_t slot = atomicAdd(stage_n, pc);
            const uint32_t pos0 = (uint32_t)(origin - tile0) + (uint32_t)r_at; // mod 2^32: r_at may lie in front of the tile, a hit never
            uint32_t ord = ord0;
            for (uint32_t h = hits; h != 0; h &= h - 1u, ++slot, ++ord)
                if (slot < (uint32_t)TILE_STAGE) stage[slot] = (uint64_t)(pos0 + (uint32_t)__builtin_ctz(h)) | ((uint64_t)ord << 32);
        } else {
            uint64_t idx = base + ord0;
            const uint64_t end0 = origin + (uint64_t)(int64_t)r_at + a.out_bias;
            for (uint32_t h = hits; h != 0; h &= h - 1u, ++idx)
                if (idx < a.cap) a.out[idx] = end0 + (uint32_t)__builtin_ctz(h);
        }
    };
    for (int32_t line = 0; line < r_end; line += 128, src += 8) {
        tile_u32x4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int32_t r = line + 16 * q;
            if (r >= r_begin && r < r_end) v[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int32_t r = line + 16 * q;
            if (r < r_begin || r >= r_end) continue;
            const bool at_zero = q == 0 && (origin | (uint64_t)line) == 0; // (aligned byte 0: the one chunk with bytes in front)
            const uint32_t skip = at_zero ? (uint32_t)a.first : 0u;
            const uint32_t keep = (uint32_t)min(r_view_hi - r, 16);   // (>= 1: the chunk holds a view byte)
            uint32_t hits = skip != 0 || keep < 16 ? regex_anchored_chunk_edge<WIDE, NL>(tab, k, s, v[q], skip, keep, g)
                                                   : regex_anchored_chunk<WIDE, NL>(tab, k, s, v[q]);
            // bit i is position r - 1 + i
            const int32_t own_from = min(max(r_lo - r + 1, 0), 16), own_to = min(max(r_hi - r + 1, 0), 16);
            hits &= ((1u << own_to) - 1u) & ~((1u << own_from) - 1u);
            if (hits == 0) continue; // the usual case, for the whole wave
            emit(hits, r - 1);
        }
    }
    if (at_view_end && (a.own_hi & 15ull) == 0) { // the view's last byte closes a line: its hit has not been seen yet
        uint32_t alo, ahi;
        T::word(tab, T::A_AT, g.right, alo, ahi);
        if (((s.d.lo & alo) | (s.d.hi & ahi)) != 0) emit(1u, r_hi - 1);
    }
    return cnt;
}

template <bool WIDE, bool NL>
struct RegexAnchoredPolicy {
    typedef uint32_t Elem;
    typedef RegexAnchoredTab<WIDE, NL> T;
    static constexpr bool FILL_TAKES_X = true;
    static constexpr int TAB = T::TAB;
    static __device__ __forceinline__ void fill(uint32_t *tab, const TileArgs &a, uint32_t tid, const RegexSets &k, const RegexGate &g)
    {
        RegexPolicy<WIDE, NL>::fill(tab, a, tid, k);
        const uint64_t e = g.tabs[tid], f = g.tabs[256 + tid]; // TILE_BLOCK == 256
        if (WIDE) {
            tab[T::E_AT + 2 * tid] = (uint32_t)e;
            tab[T::E_AT + 2 * tid + 1] = (uint32_t)(e >> 32);
            tab[T::A_AT + 2 * tid] = (uint32_t)f;
            tab[T::A_AT + 2 * tid + 1] = (uint32_t)(f >> 32);
        } else {
            tab[T::E_AT + tid] = (uint32_t)e;
            tab[T::A_AT + tid] = (uint32_t)f;
        }
    }
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base, const RegexSets &k,
                                                    const RegexGate &g)
    {
        return regex_anchored_walk<WIDE, NL, PASS>(a, k, g, tab, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32); }
    static __device__ __forceinline__ void also(const TileArgs &, uint64_t, uint64_t) {}
};

struct RegexAnchoredStartsArgs {
    const uint8_t *text16; // the 16-byte line that holds text[0]
    uint64_t first;        // text[0] is text16[first]
    uint64_t n, base;
    const uint64_t *ends;
    uint64_t count;
    uint64_t *starts;
    uint64_t *ws;          // [0]: status bits (REGEX_BAD_END, REGEX_BAD_START)
    const uint64_t *gate;  // A_rev[256], E_rev[256]: bit i = position m - 1 - i
    uint32_t max_len, chunks; // chunks = ceil((max_len + 1) / 8): a length is accepted one step late
    uint32_t longest, left, right, pad;
    RegexSets k;           // of the REVERSED automaton
    uint64_t peq[256];     // bit i set: byte belongs to position m - 1 - i (low word used when m <= 32)
};

template <typename W>
__global__ __launch_bounds__(REGEX_STARTS_BLOCK) void regex_anchored_starts_kernel(const RegexAnchoredStartsArgs a)
{
    constexpr uint32_t NB = sizeof(W); // bytes of the word: one T_b table each
    __shared__ W peq[256];
    __shared__ W eg[256];
    __shared__ W tt[NB * 256];
    const uint32_t tid = threadIdx.x;
    peq[tid] = (W)a.peq[tid]; // REGEX_STARTS_BLOCK == 256
    eg[tid] = (W)a.gate[256 + tid];
#pragma unroll 1
    for (uint32_t b = 0; b < NB; ++b) tt[256 * b + tid] = (W)regex_table_entry(a.k.follow, b, tid);
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * REGEX_STARTS_BLOCK + tid;
    if (i >= a.count) return;

    const uint64_t e = a.ends[i];
    const uint64_t j = e - a.base;
    const bool valid = e >= a.base && j < a.n;
    uint32_t steps = 0, b = 0, next = a.right;
    int64_t wi = -1; // index of the 8-byte word that holds text[j], counted from text16
    if (valid) {
        steps = (uint32_t)min(j + 1, (uint64_t)a.max_len); // the window is clipped at text[0]
        const uint64_t q = a.first + j;
        wi = (int64_t)(q >> 3);
        b = (uint32_t)(q & 7);
        if (j + 1 < a.n) next = a.text16[q + 1]; // (a byte of the view)
    } else {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_BAD_END); // no byte is read for this entry
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t hi = valid ? words[wi] : 0;               // text[j] is byte b of hi
    uint64_t lo = valid && wi > 0 ? words[wi - 1] : 0; // word 0 lies in text[0]'s line: nothing below it is loaded

    const W lin = (W)a.k.lin, nl = (W)a.k.nl;
    const W e_left = eg[a.left];
    const uint32_t nl_bytes = a.k.nl_bytes;
    W d = 0, seed = (W)(a.k.first & a.gate[next]); // anchored at text[j]: `first` enters the first step only, gated by the byte above
    uint32_t first_len = 0, last_len = 0, len = 0;
    for (uint32_t c = 0; c < a.chunks; ++c) {
        // the next 8 bytes downwards from text[j - 8c], the first of them in the top byte
        const uint64_t cur = (hi << (8 * (7 - b))) | ((lo >> (8 * b)) >> 8);
        hi = lo;
        --wi;
        lo = valid && wi > 0 ? words[wi - 1] : 0; // one word ahead of its use
        W eq[8], ee[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t byte = (uint32_t)(cur >> (8 * (7 - t))) & 0xFFu;
            eq[t] = peq[byte];
            ee[t] = eg[byte];
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            // d is the state after `len` bytes and this byte is the one below them: text[j - len + 1 .. j] matches iff ...
            if (len >= 1 && len <= steps && (d & (len == j + 1 ? e_left : ee[t])) != 0) {
                if (first_len == 0) first_len = len;
                last_len = len;
            }
            W f = (W)((d & lin) << 1) | seed;
            seed = 0;
            const W x = d & nl;
#pragma unroll
            for (uint32_t q = 0; q < NB; ++q)
                if ((nl_bytes >> q) & 1u) f |= tt[256 * q + ((uint32_t)(x >> (8 * q)) & 0xFFu)];
            d = f & eq[t];
            ++len;
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

// ---- the mirror image: every START of an anchored match, and the end of every start of a list ----
// The reversed automaton walks DOWN the text as in bmx_regex_begins_kernel.h.  What enters is first_rev, gated by the byte
// ABOVE (A, in the table slot that the forward walk uses for E); the hit of start s is gated by the byte BELOW (E, in
// A's slot) and known at the step of byte s - 1.  So the step is the forward one, bit i of a chunk at r belongs to
// position r + 1 + i, a lane that owns [lo, hi) steps byte lo - 1 as well when it lies inside the view, a lane whose
// walk begins on the view's last byte carries A[right], and `left` stands in below view byte 0.

// One 16-byte chunk downwards.  Returns the delayed hit bits: bit i = the byte above byte i.
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_anchored_chunk_down(const uint32_t *tab, const RegexSets &k, RegexAnchoredState<WIDE> &s,
                                                              tile_u32x4 v)
{
    typedef RegexAnchoredTab<WIDE, NL> T;
    const uint32_t *tt = tab + T::B_WORDS;
    uint32_t hits = 0;
#pragma unroll
    for (int h = 1; h >= 0; --h) {
        uint32_t blo[8], bhi[8], elo[8], ehi[8], alo[8], ahi[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t byte = __builtin_amdgcn_ubfe(v[2 * h + (i >> 2)], 8 * (i & 3), 8);
            T::word(tab, 0, byte, blo[i], bhi[i]);
            T::word(tab, T::E_AT, byte, elo[i], ehi[i]);
            T::word(tab, T::A_AT, byte, alo[i], ahi[i]);
        }
#pragma unroll
        for (int i = 7; i >= 0; --i)
            hits |= (regex_anchored_step<WIDE, NL>(k, tt, s, blo[i], bhi[i], elo[i], ehi[i], alo[i], ahi[i]) != 0 ? 1u : 0u) << (8 * h + i);
    }
    return hits;
}

// A chunk at an end of the view, downwards: its bytes from `keep` on lie behind the view (an empty B word, and the entry
// word of `right` carried into the view's last byte), its first `skip` bytes in front of it (an empty B word, and the hit
// word of `left` as what view byte 0 sees).
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_anchored_chunk_edge_down(const uint32_t *tab, const RegexSets &k, RegexAnchoredState<WIDE> &s,
                                                                   tile_u32x4 v, uint32_t skip, uint32_t keep, const RegexGate &g)
{
    typedef RegexAnchoredTab<WIDE, NL> T;
    const uint32_t *tt = tab + T::B_WORDS;
    uint32_t hits = 0;
#pragma unroll 1
    for (int32_t i = 15; i >= 0; --i) {
        const uint32_t byte = v[3] >> 24;
        v[3] = __builtin_amdgcn_alignbit(v[3], v[2], 24);
        v[2] = __builtin_amdgcn_alignbit(v[2], v[1], 24);
        v[1] = __builtin_amdgcn_alignbit(v[1], v[0], 24);
        v[0] <<= 8;
        const bool in_view = (uint32_t)i >= skip && (uint32_t)i < keep;
        uint32_t blo, bhi, elo, ehi, alo, ahi;
        T::word(tab, 0, byte, blo, bhi);
        T::word(tab, T::E_AT, (uint32_t)i >= keep ? g.right : byte, elo, ehi);
        T::word(tab, T::A_AT, (uint32_t)i < skip ? g.left : byte, alo, ahi);
        if (!in_view) blo = bhi = 0;
        hits |= (regex_anchored_step<WIDE, NL>(k, tt, s, blo, bhi, elo, ehi, alo, ahi) != 0 ? 1u : 0u) << i;
    }
    return hits;
}

// One lane: the starts [lo, hi) (aligned coordinates), walked downwards from a.warm = max_len bytes above hi - 1 (clipped
// at the view's last byte, view_hi - 1) to byte lo - 1 (clipped at view byte 0).  Ordinals and slots as regex_begins_walk.
template <bool WIDE, bool NL, int PASS>
__device__ __forceinline__ uint32_t regex_anchored_begins_walk(const TileArgs &a, const RegexSets &k, const RegexGate &g, uint64_t view_hi,
                                                               const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                               uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
    typedef RegexAnchoredTab<WIDE, NL> T;
    const uint64_t top = min(hi + a.warm, view_hi);         // one past the first byte walked
    const bool clipped = top == view_hi;                    // the walk begins on the view's last byte
    const bool at_view_begin = lo == a.first;               // no byte lo - 1: `left` stands in
    const uint64_t bottom = at_view_begin ? lo : lo - 1;    // the last byte walked
    const uint64_t origin = bottom & ~127ull;               // its line
    const int32_t r_lo = (int32_t)(lo - origin);            // everything below is relative to origin (< 2^13)
    const int32_t r_hi = (int32_t)(hi - origin);
    const int32_t r_top = (int32_t)(top - origin);
    const int32_t r_begin = (int32_t)(bottom - origin) & ~15;
    const tile_u32x4 *src0 = reinterpret_cast<const tile_u32x4 *>(a.text16) + (origin >> 4);
    RegexAnchoredState<WIDE> s;
    s.d.lo = s.d.hi = 0;
    s.elo = s.ehi = 0;
    if (clipped) T::word(tab, T::E_AT, g.right, s.elo, s.ehi);
    uint32_t cnt = 0;
    // the hits `hits` of the positions r_at + bit (relative to origin), highest first
    const auto emit = [&](uint32_t hits, int32_t r_at) {
        const uint32_t ord0 = cnt;
        const uint32_t pc = __builtin_popcount(hits);
        cnt += pc;
        if (PASS == TILE_PARK) {
            if (a.out == nullptr) return;
            uint32_t slot = atomicAdd(stage_n, pc);
            const uint32_t pos0 = (uint32_t)(origin - tile0) + (uint32_t)r_at; // mod 2^32: origin may lie one line in front of the tile, a hit never
            uint32_t ord = ord0;
            for (uint32_t h = hits; h != 0; ++slot, ++ord) {
                const uint32_t bit = 31u - (uint32_t)__builtin_clz(h);
                h ^= 1u << bit;
                if (slot < (uint32_t)TILE_STAGE) stage[slot] = (uint64_t)(pos0 + bit) | ((uint64_t)ord << 32);
            }
        } else {
            uint64_t idx = base - 1 - ord0;
            const uint64_t start0 = origin + (uint64_t)(int64_t)r_at + a.out_bias;
            for (uint32_t h = hits; h != 0; --idx) {
                const uint32_t bit = 31u - (uint32_t)__builtin_clz(h);
                h ^= 1u << bit;
                if (idx < a.cap) a.out[idx] = start0 + bit;
            }
        }
    };
    for (int32_t line = (r_top - 1) & ~127; line >= 0; line -= 128) {
        const tile_u32x4 *src = src0 + (line >> 4);
        tile_u32x4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int32_t r = line + 16 * q;
            if (r >= r_begin && r < r_top) v[q] = src[q];
        }
#pragma unroll
        for (int q = 7; q >= 0; --q) {
            const int32_t r = line + 16 * q;
            if (r < r_begin || r >= r_top) continue;
            const bool at_zero = q == 0 && (origin | (uint64_t)line) == 0; // (aligned byte 0: the one chunk with bytes in front)
            const uint32_t skip = at_zero ? (uint32_t)a.first : 0u;
            const uint32_t keep = clipped ? (uint32_t)min(r_top - r, 16) : 16u; // (the view's last chunk: the one with bytes past the view)
            uint32_t hits = skip != 0 || keep < 16 ? regex_anchored_chunk_edge_down<WIDE, NL>(tab, k, s, v[q], skip, keep, g)
                                                   : regex_anchored_chunk_down<WIDE, NL>(tab, k, s, v[q]);
            // bit i is position r + 1 + i
            const int32_t own_from = min(max(r_lo - r - 1, 0), 16), own_to = min(max(r_hi - r - 1, 0), 16);
            hits &= ((1u << own_to) - 1u) & ~((1u << own_from) - 1u);
            if (hits == 0) continue; // the usual case, for the whole wave
            emit(hits, r + 1);
        }
    }
    if (at_view_begin && a.first == 0) { // view byte 0 opens a line: its hit has not been seen yet
        uint32_t alo, ahi;
        T::word(tab, T::A_AT, g.left, alo, ahi);
        if (((s.d.lo & alo) | (s.d.hi & ahi)) != 0) emit(1u, r_lo);
    }
    return cnt;
}

// The frame's policy of the begins search: the tables of the REVERSED automaton, g.tabs = {A_rev, E_rev}.
template <bool WIDE, bool NL>
struct RegexAnchoredBeginsPolicy {
    typedef uint32_t Elem;
    static constexpr bool FILL_TAKES_X = true;
    static constexpr bool ORDINAL_DESCENDS = true;
    static constexpr int TAB = RegexAnchoredTab<WIDE, NL>::TAB;
    static __device__ __forceinline__ void fill(uint32_t *tab, const TileArgs &a, uint32_t tid, const RegexSets &k, const RegexGate &g, uint64_t)
    {
        RegexAnchoredPolicy<WIDE, NL>::fill(tab, a, tid, k, g);
    }
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base, const RegexSets &k,
                                                    const RegexGate &g, uint64_t view_hi)
    {
        return regex_anchored_begins_walk<WIDE, NL, PASS>(a, k, g, view_hi, tab, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32); }
    static __device__ __forceinline__ void also(const TileArgs &, uint64_t, uint64_t) {}
};

struct RegexAnchoredEndsArgs {
    const uint8_t *text16; // the 16-byte line that holds text[0]
    uint64_t first;        // text[0] is text16[first]
    uint64_t n, base;
    const uint64_t *starts;
    const uint64_t *limit; // NULL, or the last byte (coordinates of starts) a match of entry i may use
    uint64_t count;
    uint64_t *ends;
    uint64_t *ws;          // [0]: status bits (REGEX_ENDS_BAD_START, REGEX_ENDS_NO_MATCH)
    const uint64_t *gate;  // E[256], A[256]: bit i = position i
    uint32_t max_len, chunks; // chunks = ceil((max_len + 1) / 8): a length is accepted one step late
    uint32_t longest, left, right, pad;
    RegexSets k;           // of the automaton as given
    uint64_t peq[256];     // bit i set: byte belongs to position i (low word used when m <= 32)
};

// One list entry per lane, the mirror of regex_anchored_starts_kernel over the automaton as given: the seed is
// first & E[prev(s)], a length L is accepted where (D & A[byte above the match]) != 0, one step late; above the view's
// last byte `right` stands in.  Reads as regex_ends_kernel: nothing above text[n - 1]'s line.
template <typename W>
__global__ __launch_bounds__(REGEX_STARTS_BLOCK) void regex_anchored_ends_kernel(const RegexAnchoredEndsArgs a)
{
    constexpr uint32_t NB = sizeof(W); // bytes of the word: one T_b table each
    __shared__ W peq[256];
    __shared__ W ag[256];
    __shared__ W tt[NB * 256];
    const uint32_t tid = threadIdx.x;
    peq[tid] = (W)a.peq[tid]; // REGEX_STARTS_BLOCK == 256
    ag[tid] = (W)a.gate[256 + tid];
#pragma unroll 1
    for (uint32_t b = 0; b < NB; ++b) tt[256 * b + tid] = (W)regex_table_entry(a.k.follow, b, tid);
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * REGEX_STARTS_BLOCK + tid;
    if (i >= a.count) return;

    const uint64_t st = a.starts[i];
    const uint64_t j = st - a.base;
    const bool valid = st >= a.base && j < a.n;
    const int64_t w_last = (int64_t)((((a.first + a.n - 1) >> 4) << 1) + 1); // the last 8-byte word of text[n - 1]'s line
    uint32_t steps = 0, b = 0, prev = a.left;
    int64_t wi = w_last; // index of the 8-byte word that holds text[j], counted from text16
    if (valid) {
        uint64_t room = min(a.n - j, (uint64_t)a.max_len); // the window is clipped at text[n - 1] ...
        if (a.limit != nullptr) {                          // ... and at the entry's limit
            const uint64_t lim = a.limit[i];
            room = lim >= st ? min(room, lim - st + 1) : 0;
        }
        steps = (uint32_t)room;
        const uint64_t q = a.first + j;
        wi = (int64_t)(q >> 3);
        b = (uint32_t)(q & 7);
        if (j > 0) prev = a.text16[q - 1]; // (a byte of the view)
    } else {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_ENDS_BAD_START); // no byte is read for this entry
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t lo = valid ? words[wi] : 0;                    // text[j] is byte b of lo
    uint64_t hi = valid && wi < w_last ? words[wi + 1] : 0; // nothing above text[n - 1]'s line is loaded

    const W lin = (W)a.k.lin, nl = (W)a.k.nl;
    const W a_right = ag[a.right];
    const uint32_t nl_bytes = a.k.nl_bytes;
    W d = 0, seed = (W)(a.k.first & a.gate[prev]); // anchored at text[j]: `first` enters the first step only, gated by the byte below
    uint32_t first_len = 0, last_len = 0, len = 0;
    for (uint32_t c = 0; c < a.chunks; ++c) {
        // the next 8 bytes upwards from text[j + 8c], the first of them in the low byte
        const uint64_t cur = (lo >> (8 * b)) | ((hi << (8 * (7 - b))) << 8);
        lo = hi;
        ++wi;
        hi = valid && wi < w_last ? words[wi + 1] : 0; // one word ahead of its use
        W eq[8], aa[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t byte = (uint32_t)(cur >> (8 * t)) & 0xFFu;
            eq[t] = peq[byte];
            aa[t] = ag[byte];
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            // d is the state after `len` bytes and this byte is the one above them: text[j .. j + len - 1] matches iff ...
            if (len >= 1 && len <= steps && (d & (j + len == a.n ? a_right : aa[t])) != 0) {
                if (first_len == 0) first_len = len;
                last_len = len;
            }
            W f = (W)((d & lin) << 1) | seed;
            seed = 0;
            const W x = d & nl;
#pragma unroll
            for (uint32_t q = 0; q < NB; ++q)
                if ((nl_bytes >> q) & 1u) f |= tt[256 * q + ((uint32_t)(x >> (8 * q)) & 0xFFu)];
            d = f & eq[t];
            ++len;
        }
    }
    if (!valid) return;
    if (first_len == 0) {
        if (a.limit == nullptr) {
            atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_ENDS_NO_MATCH);
            a.ends[i] = st;
        } else {
            a.ends[i] = ~0ull; // no match within the limit: the selection skips the entry
        }
        return;
    }
    a.ends[i] = st + ((a.longest ? last_len : first_len) - 1);
}

} // namespace bmx
