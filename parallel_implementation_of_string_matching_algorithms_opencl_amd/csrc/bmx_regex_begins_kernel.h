// bmx_regex_begins_kernel.h -- the mirror image of the regular-expression search (bmx_search_regex_begins_device,
// bmx_regex_ends_device): every START s of the view at which some text[s..j] matches is reported once, ascending, and a
// post-pass gives every start of a list its shortest or its longest end.  No counterpart in the reference.
//
// Begins.  The lane runs the REVERSED automaton (position i becomes m - 1 - i, first and last swap, follow is transposed
// and so points upward again) DOWN the text: bit i of D says "reversed position i has just consumed the current byte on
// some path that began in first_rev", and after text[s]
//     D = (first_rev | Follow_rev(D)) & B_rev[text[s]]          start s is a hit iff (D & last_rev) != 0.
// The sets, the T_b tables and the step are bmx_regex_kernel.h's, fed with the reversed automaton.  A match spans at most
// max_len bytes, so a lane that starts with D = 0 at least max_len - 1 bytes ABOVE its last start, or on the view's last
// byte, is exact from there on.  The tile loop, the ordered output and the argument block are bmx_tile_frame.h's in START
// coordinates: a lane owns the P starts [lo, hi) and walks from min(hi - 1 + warm, last view byte) down to lo.
//  * Text comes in whole 128-byte lines per lane, sixteen bytes a load, as in shift_and_walk; the lines are visited in
//    descending order and the bytes of a chunk are stepped 15..0.  The highest chunk loaded holds the first byte walked,
//    the lowest holds lo: every load holds a byte of the view and none lies above the line of text[n - 1].
//  * The chunk that holds text[n - 1] is this walk's head chunk: its bytes past the view are stepped with an empty B word
//    (a match must end inside the view), the mirror of regex_chunk_head.  The bytes in front of an unaligned view need
//    nothing: they are stepped last and no start among them is owned.
//  * A lane's hits come out in DESCENDING position.  The lane parks {position in tile, descending ordinal << 32}; the
//    frame turns the ordinal round at placement (ORDINAL_DESCENDS: slot = prefix + lane_base[lane + 1] - 1 - ordinal) and
//    hands the second walk of a dense tile the slot one past the lane's last, from which it writes downwards.
//
// Ends (regex_ends_kernel): one list entry per lane, the mirror of regex_starts_kernel.  The lane runs the FORWARD
// automaton against text[s], text[s + 1], ... for at most min(max_len, n - s, limit - s + 1) bytes, anchored: `first`
// enters at the first step only.  Text comes as aligned 8-byte words, upwards, one word ahead; a word above the 16-byte
// line of text[n - 1] is never loaded and an entry whose start is outside the view reads no byte.
#pragma once

#include "bmx_regex_kernel.h"

namespace bmx {

constexpr uint64_t REGEX_ENDS_BAD_START = 1, REGEX_ENDS_NO_MATCH = 2; // status bits of the ends kernel (ws[0])

// One 16-byte chunk downwards: gather, then 16 steps from byte 15 to byte 0.  Returns the hit bits, bit i = the step of byte i.
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_chunk_down(const uint32_t *tab, const RegexSets &k, ShiftAndState<WIDE> &s, tile_u32x4 v)
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
    for (int i = 15; i >= 0; --i) hits |= (regex_step<WIDE, NL>(k, tt, s, blo[i], bhi[i]) != 0 ? 1u : 0u) << i;
    return hits;
}

// The chunk that holds the view's last byte when the view does not end on a 16-byte line: only its first `keep` bytes
// belong to the view, the others are stepped with an empty B word, which leaves D = 0.  One chunk per call, so a plain loop.
template <bool WIDE, bool NL>
__device__ __forceinline__ uint32_t regex_chunk_tail(const uint32_t *tab, const RegexSets &k, ShiftAndState<WIDE> &s, tile_u32x4 v,
                                                     uint32_t keep)
{
    const uint32_t *tt = tab + (WIDE ? 512 : 256);
    uint32_t hits = 0;
#pragma unroll 1
    for (int32_t i = 15; i >= 0; --i) {
        const uint32_t byte = v[3] >> 24;
        v[3] = __builtin_amdgcn_alignbit(v[3], v[2], 24);
        v[2] = __builtin_amdgcn_alignbit(v[2], v[1], 24);
        v[1] = __builtin_amdgcn_alignbit(v[1], v[0], 24);
        v[0] <<= 8;
        uint32_t blo = 0, bhi;
        if (WIDE) {
            const uint2 w = reinterpret_cast<const uint2 *>(tab)[byte];
            blo = w.x;
            bhi = w.y;
        } else {
            bhi = tab[byte];
        }
        if ((uint32_t)i >= keep) blo = bhi = 0;
        hits |= (regex_step<WIDE, NL>(k, tt, s, blo, bhi) != 0 ? 1u : 0u) << i;
    }
    return hits;
}

// One lane: the starts [lo, hi) (aligned coordinates), walked downwards from a.warm bytes above hi - 1 (clipped at the
// view's last byte, view_hi - 1).  Returns the number of hits.  TILE_PARK: as shift_and_walk, with the ordinal counted
// from the lane's HIGHEST hit.  TILE_WRITE: `base` is one past the lane's last slot; hit number i from the top goes to
// slot base - 1 - i if that is below a.cap.
template <bool WIDE, bool NL, int PASS>
__device__ __forceinline__ uint32_t regex_begins_walk(const TileArgs &a, const RegexSets &k, uint64_t view_hi, const uint32_t *tab,
                                                      uint64_t lo, uint64_t hi, uint64_t tile0, uint64_t *stage, uint32_t *stage_n,
                                                      uint64_t base)
{
    const uint64_t top = min(hi + a.warm, view_hi);         // one past the first byte walked
    const bool clipped = top == view_hi;                    // the walk begins on the view's last byte
    const uint64_t origin = lo & ~127ull;                   // the line of the last byte walked
    const int32_t r_lo = (int32_t)(lo - origin);            // everything below is relative to origin (< 2^13)
    const int32_t r_hi = (int32_t)(hi - origin);
    const int32_t r_top = (int32_t)(top - origin);
    const int32_t r_begin = r_lo & ~15;
    const tile_u32x4 *src0 = reinterpret_cast<const tile_u32x4 *>(a.text16) + (origin >> 4);
    ShiftAndState<WIDE> s;
    s.lo = s.hi = 0;
    uint32_t cnt = 0;
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
            const bool at_end = clipped && r + 16 > r_top; // (the view's last chunk: the one with bytes past the view)
            uint32_t hits = at_end ? regex_chunk_tail<WIDE, NL>(tab, k, s, v[q], (uint32_t)(r_top - r))
                                   : regex_chunk_down<WIDE, NL>(tab, k, s, v[q]);
            const int32_t own_from = min(max(r_lo - r, 0), 16), own_to = min(max(r_hi - r, 0), 16);
            hits &= ((1u << own_to) - 1u) & ~((1u << own_from) - 1u);
            if (hits == 0) continue; // the usual case, for the whole wave
            const uint32_t ord0 = cnt;
            const uint32_t pc = __builtin_popcount(hits);
            cnt += pc;
            if (PASS == TILE_PARK) {
                if (a.out == nullptr) continue;
                uint32_t slot = atomicAdd(stage_n, pc);
                const uint32_t pos0 = (uint32_t)(origin - tile0) + (uint32_t)r; // (origin >= tile0: a tile begins on a line)
                uint32_t ord = ord0;
                for (uint32_t h = hits; h != 0; ++slot, ++ord) {
                    const uint32_t bit = 31u - (uint32_t)__builtin_clz(h);
                    h ^= 1u << bit;
                    if (slot < (uint32_t)TILE_STAGE) stage[slot] = (uint64_t)(pos0 + bit) | ((uint64_t)ord << 32);
                }
            } else {
                uint64_t idx = base - 1 - ord0;
                const uint64_t start0 = origin + (uint64_t)r + a.out_bias;
                for (uint32_t h = hits; h != 0; --idx) {
                    const uint32_t bit = 31u - (uint32_t)__builtin_clz(h);
                    h ^= 1u << bit;
                    if (idx < a.cap) a.out[idx] = start0 + bit;
                }
            }
        }
    }
    return cnt;
}

// The frame's policy: RegexPolicy's tables, built from the reversed automaton's sets and classes, the walk above, and the
// trait that makes the frame place descending ordinals.  view_hi: one past the view's last byte, in aligned coordinates.
template <bool WIDE, bool NL>
struct RegexBeginsPolicy {
    typedef uint32_t Elem;
    static constexpr bool FILL_TAKES_X = true;
    static constexpr bool ORDINAL_DESCENDS = true;
    static constexpr int TAB = RegexPolicy<WIDE, NL>::TAB;
    static __device__ __forceinline__ void fill(uint32_t *tab, const TileArgs &a, uint32_t tid, const RegexSets &k, uint64_t)
    {
        RegexPolicy<WIDE, NL>::fill(tab, a, tid, k);
    }
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base, const RegexSets &k,
                                                    uint64_t view_hi)
    {
        return regex_begins_walk<WIDE, NL, PASS>(a, k, view_hi, tab, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32); }
    static __device__ __forceinline__ void also(const TileArgs &, uint64_t, uint64_t) {}
};

struct RegexEndsArgs {
    const uint8_t *text16; // the 16-byte line that holds text[0]
    uint64_t first;        // text[0] is text16[first]
    uint64_t n, base;
    const uint64_t *starts;
    const uint64_t *limit; // NULL, or the last byte (coordinates of starts) a match of entry i may use
    uint64_t count;
    uint64_t *ends;
    uint64_t *ws;          // [0]: status bits
    uint32_t max_len, chunks; // chunks = ceil(max_len / 8)
    uint32_t longest, pad;
    RegexSets k;           // of the automaton as given
    uint64_t peq[256];     // bit i set: byte belongs to position i (low word used when m <= 32)
};

template <typename W>
__global__ __launch_bounds__(REGEX_STARTS_BLOCK) void regex_ends_kernel(const RegexEndsArgs a)
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

    const uint64_t st = a.starts[i];
    const uint64_t j = st - a.base;
    const bool valid = st >= a.base && j < a.n;
    const int64_t w_last = (int64_t)((((a.first + a.n - 1) >> 4) << 1) + 1); // the last 8-byte word of text[n - 1]'s line
    uint32_t steps = 0, b = 0;
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
    } else {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_ENDS_BAD_START); // no byte is read for this entry
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t lo = valid ? words[wi] : 0;                    // text[j] is byte b of lo
    uint64_t hi = valid && wi < w_last ? words[wi + 1] : 0; // nothing above text[n - 1]'s line is loaded

    const W lin = (W)a.k.lin, nl = (W)a.k.nl, last = (W)a.k.last;
    const uint32_t nl_bytes = a.k.nl_bytes;
    W d = 0, seed = (W)a.k.first; // anchored at text[j]: `first` enters the first step only
    uint32_t first_len = 0, last_len = 0, len = 0;
    for (uint32_t c = 0; c < a.chunks; ++c) {
        // the next 8 bytes upwards from text[j + 8c], the first of them in the low byte
        const uint64_t cur = (lo >> (8 * b)) | ((hi << (8 * (7 - b))) << 8);
        lo = hi;
        ++wi;
        hi = valid && wi < w_last ? words[wi + 1] : 0; // one word ahead of its use
        W eq[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) eq[t] = peq[(uint32_t)(cur >> (8 * t)) & 0xFFu];
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
            if (len <= steps && (d & last) != 0) { // text[j .. j + len - 1] matches
                if (first_len == 0) first_len = len;
                last_len = len;
            }
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
