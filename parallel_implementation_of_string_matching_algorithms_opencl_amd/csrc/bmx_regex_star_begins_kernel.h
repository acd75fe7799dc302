// bmx_regex_star_begins_kernel.h -- every START of a match of an automaton with a cycle (bmx_search_regex_star_begins_device)
// and the shortest or longest end of every start of a list within a window (bmx_regex_star_ends_device); DESIGN.md s31.
// It joins two things the project has: the downward walk of bmx_regex_begins_kernel.h (the REVERSED automaton run down the
// text, descending ordinals turned round by the tile frame) and the monotone / linear argument of bmx_regex_star_kernel.h
// (a pair warm-up from the empty and the full set; where the two do not meet, bounds, columns, a sweep and the search again).
//
// Everything is the mirror image of the forward star search.  The state "above byte p" is the reversed automaton's state
// after the bytes view end - 1, ..., p; a lane that owns the starts [lo, hi) needs the state above roundup16(hi).
//  * Fast path (ENTRY = false): the pair (e from the empty set, f from every useful position) walks from
//    min(roundup16(hi) + warm, view end) down to roundup16(hi).  A walk that begins on the view's last byte has f = 0 as
//    well: nothing lies above it.  e == f: exact, and the single-state descending walk takes the state handed in.
//    Otherwise the lane walks from e (a lower bound) and one lane of its wave raises the taint word and the counter.
//  * Slow path: pieces of 2^p_shift aligned bytes are numbered from the TOP of the view, l = p_top - (aligned piece), so
//    that "the piece in front" is l - 1 and RegexStarColumns, the scan and star_sweep_kernel of bmx_regex_star_kernel.h run
//    unchanged (bmx_regex_star.hip launches them for this search too).  The entry state of piece l is the state above its top byte; piece 0 holds the view's last byte and enters
//    with 0; piece 1 has f = 0 because its warm-up, piece 0, begins on the view's end.
//  * The chunk that holds text[n - 1] steps its bytes past the view with an empty B word and no chunk above it is loaded.
//    The bytes in front of an unaligned view are stepped last by whoever reaches them and own no start.
#pragma once

#include "bmx_regex_begins_kernel.h"

namespace bmx {

// (bmx_regex_star_kernel.h is not included: it defines the sweep and the starts fix-up as plain kernels, which one library
// holds once.  The scan and the sweep run through bmx_regex_star.hip's launchers; these three are that header's.)
constexpr int REGEX_STAR_BLOCK = 256; // lanes per workgroup of the slow path's kernels (== TILE_BLOCK: the policy's fill)

template <bool WIDE>
__device__ __forceinline__ void star_state_set(ShiftAndState<WIDE> &s, uint64_t v)
{
    s.lo = WIDE ? (uint32_t)v : 0u;
    s.hi = WIDE ? (uint32_t)(v >> 32) : (uint32_t)v;
}
template <bool WIDE>
__device__ __forceinline__ uint64_t star_state_get(const ShiftAndState<WIDE> &s)
{
    return WIDE ? ((uint64_t)s.hi << 32) | s.lo : (uint64_t)s.hi;
}

// The tile kernel's second argument.
struct RegexStarBeginsX {
    RegexSets k;                 // of the REVERSED automaton, masked to its useful positions
    uint64_t all;                // the positions a match can use: where f starts
    uint64_t *taint;             // pinned, device-visible: [0] becomes 1 when a lane's bounds did not meet
    unsigned long long *taint_n; // device: the waves that held such a lane
    const uint64_t *entry;       // ENTRY: the state above every piece, by piece number counted from the view's top
    uint64_t view_hi;            // one past the view's last byte, aligned coordinates
    uint32_t warm;               // bytes of the pair warm-up, a multiple of 16
    uint32_t pad;
};

// One 16-byte chunk downwards on two states: gather once, then the bytes 15..0 on each (two independent chains).  keep: the
// number of its bytes that belong to the view (16, or fewer in the chunk of text[n - 1]); the others get an empty B word.
template <bool WIDE, bool NL>
__device__ __forceinline__ void star_pair_chunk_down(const uint32_t *tab, const RegexSets &k, ShiftAndState<WIDE> &e,
                                                     ShiftAndState<WIDE> &f, tile_u32x4 v, uint32_t keep)
{
    const uint32_t *tt = tab + (WIDE ? 512 : 256);
    uint32_t blo[16], bhi[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t byte = __builtin_amdgcn_ubfe(v[i >> 2], 8 * (i & 3), 8);
        if (WIDE) {
            const uint2 w = reinterpret_cast<const uint2 *>(tab)[byte];
            blo[i] = (uint32_t)i >= keep ? 0u : w.x;
            bhi[i] = (uint32_t)i >= keep ? 0u : w.y;
        } else {
            blo[i] = 0;
            bhi[i] = (uint32_t)i >= keep ? 0u : tab[byte];
        }
    }
#pragma unroll
    for (int i = 15; i >= 0; --i) {
        (void)regex_step<WIDE, NL>(k, tt, e, blo[i], bhi[i]);
        (void)regex_step<WIDE, NL>(k, tt, f, blo[i], bhi[i]);
    }
}

// The pair walk over the chunks [c0, c1) of the aligned text from the highest down, one load ahead.  c1 is clipped to the
// chunk of the view's last byte, so every chunk loaded holds a byte of the view.
template <bool WIDE, bool NL>
__device__ __forceinline__ void star_pair_walk_down(const TileArgs &a, const RegexSets &k, const uint32_t *tab, uint64_t c0, uint64_t c1,
                                                    uint64_t view_hi, ShiftAndState<WIDE> &e, ShiftAndState<WIDE> &f)
{
    const uint64_t c_top = (view_hi - 1) >> 4;
    c1 = min(c1, c_top + 1);
    if (c0 >= c1) return;
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16);
    tile_u32x4 next = src[c1 - 1];
#pragma unroll 1
    for (uint64_t c = c1; c-- > c0;) {
        const tile_u32x4 v = next;
        if (c > c0) next = src[c - 1];
        star_pair_chunk_down<WIDE, NL>(tab, k, e, f, v, c == c_top ? (uint32_t)(view_hi - (c_top << 4)) : 16u);
    }
}

// One state over the same chunks, with the sets `k` (the caller's, or those with an empty `first`: an unseeded run).
template <bool WIDE, bool NL>
__device__ __forceinline__ void star_single_walk_down(const TileArgs &a, const RegexSets &k, const uint32_t *tab, uint64_t c0, uint64_t c1,
                                                      uint64_t view_hi, ShiftAndState<WIDE> &s)
{
    const uint64_t c_top = (view_hi - 1) >> 4;
    c1 = min(c1, c_top + 1);
    if (c0 >= c1) return;
    const uint32_t keep_top = (uint32_t)(view_hi - (c_top << 4));
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16);
    tile_u32x4 next = src[c1 - 1];
#pragma unroll 1
    for (uint64_t c = c1; c-- > c0;) {
        const tile_u32x4 v = next;
        if (c > c0) next = src[c - 1];
        if (c == c_top && keep_top != 16) (void)regex_chunk_tail<WIDE, NL>(tab, k, s, v, keep_top);
        else (void)regex_chunk_down<WIDE, NL>(tab, k, s, v);
    }
}

// One lane: the starts [lo, hi) (aligned coordinates) from the state s above aligned byte top16 (a multiple of 16, at least
// hi), line by line downwards: regex_begins_walk with the warm-up taken out and the state handed in.  A top16 past the
// view's end is clipped there, and the chunk of text[n - 1] is then the first one stepped.
template <bool WIDE, bool NL, int PASS>
__device__ __forceinline__ uint32_t star_begins_walk(const TileArgs &a, const RegexSets &k, uint64_t view_hi, const uint32_t *tab,
                                                     uint64_t top16, ShiftAndState<WIDE> s, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                     uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
    const uint64_t top = min(top16, view_hi);               // one past the first byte walked
    const uint64_t origin = lo & ~127ull;                   // the line of the last byte walked
    const int32_t r_lo = (int32_t)(lo - origin);            // everything below is relative to origin (< 2^13)
    const int32_t r_hi = (int32_t)(hi - origin);
    const int32_t r_top = (int32_t)(top - origin);
    const int32_t r_begin = r_lo & ~15;
    const tile_u32x4 *src0 = reinterpret_cast<const tile_u32x4 *>(a.text16) + (origin >> 4);
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
            const bool at_end = r + 16 > r_top; // (only the view's last chunk: any other top is a multiple of 16)
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

// The frame's policy: RegexPolicy's table from the reversed automaton, descending ordinals, and a walk that first settles
// the state above the lane's starts -- by the pair warm-up (ENTRY = false) or from the swept array (ENTRY = true).
template <bool WIDE, bool NL, bool ENTRY>
struct RegexStarBeginsPolicy {
    typedef uint32_t Elem;
    static constexpr bool FILL_TAKES_X = true;
    static constexpr bool ORDINAL_DESCENDS = true;
    static constexpr int TAB = RegexPolicy<WIDE, NL>::TAB;
    static __device__ __forceinline__ void fill(uint32_t *tab, const TileArgs &a, uint32_t tid, const RegexStarBeginsX &x)
    {
        RegexPolicy<WIDE, NL>::fill(tab, a, tid, x.k);
    }
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base, const RegexStarBeginsX &x)
    {
        ShiftAndState<WIDE> s;
        uint64_t top16;
        if (ENTRY) {
            const uint64_t piece = (hi - 1) >> a.p_shift; // the lane's starts lie in one aligned piece
            top16 = (piece + 1) << a.p_shift;
            star_state_set<WIDE>(s, x.entry[((x.view_hi - 1) >> a.p_shift) - piece]);
        } else {
            top16 = (hi + 15) & ~15ull;
            ShiftAndState<WIDE> f;
            star_state_set<WIDE>(s, 0);
            uint64_t c1 = (top16 + x.warm) >> 4;
            if (top16 + x.warm >= x.view_hi) {
                star_state_set<WIDE>(f, 0); // from the view's last byte: exact
                c1 = ((x.view_hi - 1) >> 4) + 1;
            } else {
                star_state_set<WIDE>(f, x.all);
            }
            star_pair_walk_down<WIDE, NL>(a, x.k, tab, top16 >> 4, c1, x.view_hi, s, f);
            if (PASS == TILE_PARK) { // (a dense tile's second walk finds what its first one found)
                const bool tainted = ((s.lo ^ f.lo) | (s.hi ^ f.hi)) != 0;
                const uint64_t any = __builtin_amdgcn_ballot_w64(tainted);
                if (tainted && (uint32_t)__builtin_ctzll(any) == (threadIdx.x & 63u)) { // one lane of the wave
                    __hip_atomic_store(&x.taint[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    atomicAdd(x.taint_n, 1ull);
                }
            }
        }
        return star_begins_walk<WIDE, NL, PASS>(a, x.k, x.view_hi, tab, top16, s, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32); }
    static __device__ __forceinline__ void also(const TileArgs &, uint64_t, uint64_t) {}
};

// ---- the slow path's kernels: one lane per piece, piece l = aligned piece p_top - l, pieces [0, n_pieces) ----

// R1, first half: e_out[l] = the state above piece l from the lower bound, u_out[l] = what only the upper bound holds.
template <bool WIDE, bool NL>
__global__ __launch_bounds__(REGEX_STAR_BLOCK) void star_begins_bounds_kernel(const TileArgs a, const RegexStarBeginsX x, uint64_t n_pieces,
                                                                              uint64_t *e_out, uint64_t *u_out)
{
    __shared__ uint32_t tab[RegexPolicy<WIDE, NL>::TAB];
    RegexPolicy<WIDE, NL>::fill(tab, a, threadIdx.x, x.k);
    __syncthreads();
    const uint64_t l = (uint64_t)blockIdx.x * REGEX_STAR_BLOCK + threadIdx.x;
    if (l >= n_pieces) return;
    ShiftAndState<WIDE> e, f;
    star_state_set<WIDE>(e, 0);
    star_state_set<WIDE>(f, l <= 1 ? 0 : x.all); // piece 0 enters empty, and piece 1's warm-up begins on the view's end
    if (l != 0) {
        const uint32_t cs = a.p_shift - 4; // chunks per piece, log2
        const uint64_t p = ((x.view_hi - 1) >> a.p_shift) - (l - 1);
        star_pair_walk_down<WIDE, NL>(a, x.k, tab, p << cs, (p + 1) << cs, x.view_hi, e, f);
    }
    const uint64_t ev = star_state_get<WIDE>(e);
    e_out[l] = ev;
    u_out[l] = star_state_get<WIDE>(f) & ~ev;
}

// R1, second half, for the pieces [0, n_pieces - 1) (nothing is entered below the lowest one): base_out[l] = the state
// below piece l entered with e[l]; cols[off[l] + r] = the unseeded run of the piece from the r-th position of u[l].
// k0: the sets with an empty `first`.
template <bool WIDE, bool NL>
__global__ __launch_bounds__(REGEX_STAR_BLOCK) void star_begins_columns_kernel(const TileArgs a, const RegexStarBeginsX x, const RegexSets k0,
                                                                               uint64_t n_run, const uint64_t *e_in, const uint64_t *u_in,
                                                                               const uint64_t *off, uint64_t *base_out, uint64_t *cols)
{
    __shared__ uint32_t tab[RegexPolicy<WIDE, NL>::TAB];
    RegexPolicy<WIDE, NL>::fill(tab, a, threadIdx.x, x.k);
    __syncthreads();
    const uint64_t l = (uint64_t)blockIdx.x * REGEX_STAR_BLOCK + threadIdx.x;
    if (l >= n_run) return;
    const uint32_t cs = a.p_shift - 4;
    const uint64_t p = ((x.view_hi - 1) >> a.p_shift) - l;
    const uint64_t c0 = p << cs, c1 = (p + 1) << cs;
    ShiftAndState<WIDE> s;
    star_state_set<WIDE>(s, e_in[l]);
    star_single_walk_down<WIDE, NL>(a, x.k, tab, c0, c1, x.view_hi, s);
    base_out[l] = star_state_get<WIDE>(s);
    uint64_t *col = cols + off[l];
#pragma unroll 1
    for (uint64_t u_bits = u_in[l]; u_bits != 0; u_bits &= u_bits - 1, ++col) {
        star_state_set<WIDE>(s, u_bits & (~u_bits + 1)); // the lowest position left
        star_single_walk_down<WIDE, NL>(a, k0, tab, c0, c1, x.view_hi, s);
        *col = star_state_get<WIDE>(s);
    }
}

// ---- the ends pass: regex_ends_kernel with the window in place of max_len, a cyclic follow[] in the same tables, an early
// exit and the count of the entries the window cut short ----

constexpr uint64_t REGEX_STAR_ENDS_BAD_START = 1, REGEX_STAR_ENDS_NO_MATCH = 2; // status bits (ws[0]); ws[1]: clipped entries

// a.max_len is the window.  A wave leaves its chunk loop once every lane's state is empty and its seed spent, or its room
// used up: the run is anchored, so an empty state stays empty.  An entry is CLIPPED when its state after `window` steps
// still holds a position with a successor and neither its limit nor the view's end would have stopped it there: a longer
// match may exist.  (A state of final positions without successors, as behind the d of a[bc]*d, cannot go on.)
template <typename W>
__global__ __launch_bounds__(REGEX_STARTS_BLOCK) void regex_star_ends_kernel(const RegexEndsArgs a, const uint32_t early_exit)
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
    const bool in_list = i < a.count; // (no early return: the wave votes)

    const uint64_t st = in_list ? a.starts[i] : 0;
    const uint64_t j = st - a.base;
    const bool valid = in_list && st >= a.base && j < a.n;
    const int64_t w_last = (int64_t)((((a.first + a.n - 1) >> 4) << 1) + 1); // the last 8-byte word of text[n - 1]'s line
    uint32_t steps = 0, b = 0;
    bool open = false; // neither the limit nor the view's end stops the entry within the window
    int64_t wi = w_last; // index of the 8-byte word that holds text[j], counted from text16
    if (valid) {
        uint64_t room = a.n - j; // the bytes up to text[n - 1] ...
        if (a.limit != nullptr) { // ... and up to the entry's limit
            const uint64_t lim = a.limit[i];
            room = lim >= st ? min(room, lim - st + 1) : 0;
        }
        open = room > (uint64_t)a.max_len;
        steps = (uint32_t)min(room, (uint64_t)a.max_len);
        const uint64_t q = a.first + j;
        wi = (int64_t)(q >> 3);
        b = (uint32_t)(q & 7);
    } else if (in_list) {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_STAR_ENDS_BAD_START); // no byte is read for this entry
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t lo = valid ? words[wi] : 0;                    // text[j] is byte b of lo
    uint64_t hi = valid && wi < w_last ? words[wi + 1] : 0; // nothing above text[n - 1]'s line is loaded

    const W lin = (W)a.k.lin, nl = (W)a.k.nl, last = (W)a.k.last;
    const uint32_t nl_bytes = a.k.nl_bytes;
    W d = 0, seed = (W)a.k.first; // anchored at text[j]: `first` enters the first step only
    uint32_t first_len = 0, last_len = 0, len = 0;
    bool alive = false; // the state after exactly `steps` bytes can be extended
    for (uint32_t c = 0; c < a.chunks; ++c) {
        const bool done = len >= steps || (early_exit && d == 0 && seed == 0);
        if (__builtin_amdgcn_ballot_w64(!done) == 0) break; // the whole wave: nothing more can match
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
            if (len == steps) alive = (d & (lin | nl)) != 0;
        }
    }
    const bool clipped = valid && open && alive;
    const uint64_t clipped_wave = __builtin_amdgcn_ballot_w64(clipped);
    if (clipped_wave != 0 && (tid & 63u) == 0) // one add per wave at most, none on the output
        atomicAdd((unsigned long long *)&a.ws[1], (unsigned long long)__builtin_popcountll(clipped_wave));
    if (!valid) return;
    if (first_len == 0) {
        if (a.limit == nullptr) atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_STAR_ENDS_NO_MATCH);
        a.ends[i] = ~0ull; // no match within the window, the limit and the view: the selection skips the entry
        return;
    }
    a.ends[i] = st + ((a.longest ? last_len : first_len) - 1);
}

} // namespace bmx
