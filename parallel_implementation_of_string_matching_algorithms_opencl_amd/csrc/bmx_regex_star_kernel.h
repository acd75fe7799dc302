// bmx_regex_star_kernel.h -- regular-expression search with unbounded repetition (bmx_search_regex_star_device,
// DESIGN.md s27): bmx_regex_kernel.h's automaton and per-byte step, D = (first | Follow(D)) & B[c], with a cycle in
// follow[].  regex_step does not care where follow[] points; what a cycle breaks is the warm-up: there is no longest
// match, so a lane's state at its first end can depend on text arbitrarily far back.  Two facts about the step repair it.
//   * Follow is built from OR and AND: it is MONOTONE.  A lane that walks the same bytes from a subset and from a superset
//     of the true state keeps the truth between the two, and once the two are equal they stay equal and are the truth.
//   * It is LINEAR over OR: the state after a stretch of text entered with the set X is  c | OR over u in X of col[u],
//     where c is the run from the empty set with `first` seeding every step and col[u] the run from the single position u
//     with NO seeding.
//
// Fast path, one launch (RegexStarPolicy<.., ENTRY = false> on the tile frame).  A lane walks `warm` bytes in front of
// its first end with TWO states, e from the empty set and f from every position; a warm-up that would begin in front of
// view byte 0 begins there with e = f = 0.  e == f at the first end: the lane is exact and walks its piece with one
// state, as the star-free search does.  e != f: it walks from e (a lower bound: every end it reports is a true one) and
// raises the call's taint word.  An untainted call's list is exact.
//
// Slow path, when the call is tainted: the first launch's list is dropped and three passes make an exact one.
//   R1  one lane per piece l of the same geometry.  star_bounds_kernel runs the pair walk over piece l - 1 (the warm-up is
//       the whole piece; piece 0 enters with e = f = 0) and stores e_l and U_l = f_l & ~e_l, the positions the piece's
//       entry state is unsure of.  The popcounts of U go through an exclusive scan to column offsets.  star_columns_kernel
//       stores base_l, the state at the end of piece l entered with e_l, and col_l[u] for every u of U_l (one unseeded
//       run of the piece per set bit), compactly, no atomics.
//   sweep  truth(entry of l + 1) = base_l | OR over u in (truth(entry of l) & U_l) of col_l[u].  A piece with U_l == 0 knows
//       its entry (e_l), so chains are independent: the lane of every such piece walks its chain to the next one.
//   R2  the tile kernel again with the lane's entry state read from the swept array (ENTRY = true).
// No pass spins or waits on another lane beyond what the tile frame's look-back already does.
#pragma once

#include "bmx_regex_kernel.h"

namespace bmx {

constexpr int REGEX_STAR_BLOCK = 256; // lanes per workgroup of the slow path's kernels (== TILE_BLOCK: the policy's fill)

// The tile kernel's second argument.
struct RegexStarX {
    RegexSets k;
    uint64_t all;                // the positions a match can use: where f starts
    uint64_t *taint;             // pinned, device-visible: [0] becomes 1 when a lane's bounds did not meet
    unsigned long long *taint_n; // device: the waves that held such a lane
    const uint64_t *entry;       // ENTRY: the state in front of every piece, by aligned piece index
    uint32_t warm;               // bytes of the pair warm-up, a multiple of 16
    uint32_t pad;
};

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

// One 16-byte chunk on two states: gather once, then 16 steps of each (two independent chains).  skip: the number of its
// bytes in front of the view (the chunk at aligned byte 0 of an unaligned view), stepped with an empty B word.
template <bool WIDE, bool NL>
__device__ __forceinline__ void star_pair_chunk(const uint32_t *tab, const RegexSets &k, ShiftAndState<WIDE> &e, ShiftAndState<WIDE> &f,
                                                tile_u32x4 v, uint32_t skip)
{
    const uint32_t *tt = tab + (WIDE ? 512 : 256);
    uint32_t blo[16], bhi[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t byte = __builtin_amdgcn_ubfe(v[i >> 2], 8 * (i & 3), 8);
        if (WIDE) {
            const uint2 w = reinterpret_cast<const uint2 *>(tab)[byte];
            blo[i] = (uint32_t)i < skip ? 0u : w.x;
            bhi[i] = (uint32_t)i < skip ? 0u : w.y;
        } else {
            blo[i] = 0;
            bhi[i] = (uint32_t)i < skip ? 0u : tab[byte];
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        (void)regex_step<WIDE, NL>(k, tt, e, blo[i], bhi[i]);
        (void)regex_step<WIDE, NL>(k, tt, f, blo[i], bhi[i]);
    }
}

// The pair walk over the chunks [c0, c1) of the aligned text, one load ahead.  Every chunk holds a byte of the view.
template <bool WIDE, bool NL>
__device__ __forceinline__ void star_pair_walk(const TileArgs &a, const RegexSets &k, const uint32_t *tab, uint64_t c0, uint64_t c1,
                                               ShiftAndState<WIDE> &e, ShiftAndState<WIDE> &f)
{
    if (c0 >= c1) return;
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16);
    tile_u32x4 next = src[c0];
#pragma unroll 1
    for (uint64_t c = c0; c < c1; ++c) {
        const tile_u32x4 v = next;
        if (c + 1 < c1) next = src[c + 1];
        star_pair_chunk<WIDE, NL>(tab, k, e, f, v, c == 0 ? (uint32_t)a.first : 0u);
    }
}

// One state over the chunks [c0, c1), with the sets `k` (the caller's, or those with an empty `first`: an unseeded run).
template <bool WIDE, bool NL>
__device__ __forceinline__ void star_single_walk(const TileArgs &a, const RegexSets &k, const uint32_t *tab, uint64_t c0, uint64_t c1,
                                                 ShiftAndState<WIDE> &s)
{
    if (c0 >= c1) return;
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16);
    tile_u32x4 next = src[c0];
#pragma unroll 1
    for (uint64_t c = c0; c < c1; ++c) {
        const tile_u32x4 v = next;
        if (c + 1 < c1) next = src[c + 1];
        if (c == 0 && a.first != 0) (void)regex_chunk_head<WIDE, NL>(tab, k, s, v, (uint32_t)a.first);
        else (void)regex_chunk<WIDE, NL>(tab, k, s, v);
    }
}

// One lane: the ends [lo, hi) (aligned coordinates) from the state s in front of aligned byte start16 (a multiple of 16,
// at most lo), line by line: bmx_classes_kernel.h's shift_and_walk with the warm-up taken out and the state handed in.
template <bool WIDE, bool NL, int PASS>
__device__ __forceinline__ uint32_t star_walk(const TileArgs &a, const RegexSets &k, const uint32_t *tab, uint64_t start16,
                                              ShiftAndState<WIDE> s, uint64_t lo, uint64_t hi, uint64_t tile0, uint64_t *stage,
                                              uint32_t *stage_n, uint64_t base)
{
    const uint64_t origin = start16 & ~127ull;               // the line of the first byte walked
    const int32_t r_begin = (int32_t)(start16 - origin);     // everything below is relative to origin
    const int32_t r_lo = (int32_t)(lo - origin);
    const int32_t r_hi = (int32_t)(hi - origin);
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16) + (origin >> 4);
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
            const uint32_t skip = at_zero ? (uint32_t)a.first : 0u;
            uint32_t hits = skip != 0 ? regex_chunk_head<WIDE, NL>(tab, k, s, v[q], skip) : regex_chunk<WIDE, NL>(tab, k, s, v[q]);
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

// The frame's policy: RegexPolicy's table, and a walk that first settles the lane's entry state -- by the pair warm-up
// (ENTRY = false) or from the swept array (ENTRY = true).
template <bool WIDE, bool NL, bool ENTRY>
struct RegexStarPolicy {
    typedef uint32_t Elem;
    static constexpr bool FILL_TAKES_X = true;
    static constexpr int TAB = RegexPolicy<WIDE, NL>::TAB;
    static __device__ __forceinline__ void fill(uint32_t *tab, const TileArgs &a, uint32_t tid, const RegexStarX &x)
    {
        RegexPolicy<WIDE, NL>::fill(tab, a, tid, x.k);
    }
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const uint32_t *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base, const RegexStarX &x)
    {
        ShiftAndState<WIDE> s;
        uint64_t start16;
        if (ENTRY) {
            const uint64_t piece = lo >> a.p_shift; // lo lies in the lane's piece (the first owned end may be inside it)
            start16 = piece << a.p_shift;
            star_state_set<WIDE>(s, x.entry[piece]);
        } else {
            start16 = lo & ~15ull;
            ShiftAndState<WIDE> f;
            star_state_set<WIDE>(s, 0);
            uint64_t c0 = 0;
            if (start16 <= x.warm) {
                star_state_set<WIDE>(f, 0); // from view byte 0: exact
            } else {
                star_state_set<WIDE>(f, x.all);
                c0 = (start16 - x.warm) >> 4;
            }
            star_pair_walk<WIDE, NL>(a, x.k, tab, c0, start16 >> 4, s, f);
            if (PASS == TILE_PARK) { // (a dense tile's second walk finds what its first one found)
                const bool tainted = ((s.lo ^ f.lo) | (s.hi ^ f.hi)) != 0;
                const uint64_t any = __builtin_amdgcn_ballot_w64(tainted);
                if (tainted && (uint32_t)__builtin_ctzll(any) == (threadIdx.x & 63u)) { // one lane of the wave
                    __hip_atomic_store(&x.taint[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    atomicAdd(x.taint_n, 1ull);
                }
            }
        }
        return star_walk<WIDE, NL, PASS>(a, x.k, tab, start16, s, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32); }
    static __device__ __forceinline__ void also(const TileArgs &, uint64_t, uint64_t) {}
};

// ---- the slow path's kernels: one lane per piece of 2^a.p_shift aligned bytes, pieces [0, n_pieces) ----

// R1, first half: the bounds of every piece's entry state.  e_out[l] = the state in front of piece l from the lower
// bound, u_out[l] = the positions only the upper bound holds.
template <bool WIDE, bool NL>
__global__ __launch_bounds__(REGEX_STAR_BLOCK) void star_bounds_kernel(const TileArgs a, const RegexStarX x, uint64_t n_pieces,
                                                                       uint64_t *e_out, uint64_t *u_out)
{
    __shared__ uint32_t tab[RegexPolicy<WIDE, NL>::TAB];
    RegexPolicy<WIDE, NL>::fill(tab, a, threadIdx.x, x.k);
    __syncthreads();
    const uint64_t l = (uint64_t)blockIdx.x * REGEX_STAR_BLOCK + threadIdx.x;
    if (l >= n_pieces) return;
    ShiftAndState<WIDE> e, f;
    star_state_set<WIDE>(e, 0);
    star_state_set<WIDE>(f, l <= 1 ? 0 : x.all); // piece 0 enters empty, and piece 1's warm-up begins at view byte 0
    if (l != 0) {
        const uint32_t cs = a.p_shift - 4; // chunks per piece, log2
        star_pair_walk<WIDE, NL>(a, x.k, tab, (l - 1) << cs, l << cs, e, f);
    }
    const uint64_t ev = star_state_get<WIDE>(e);
    e_out[l] = ev;
    u_out[l] = star_state_get<WIDE>(f) & ~ev;
}

// the scan's input: the number of columns of piece i (none behind the last piece)
struct RegexStarColumns {
    const uint64_t *u;
    uint64_t n_pieces;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n_pieces ? (uint64_t)__popcll(u[i]) : 0ull; }
};

// R1, second half, for the pieces [0, n_pieces - 1) (nothing enters behind the last one): base_out[l] = the state at the
// end of piece l entered with e[l]; cols[off[l] + r] = the unseeded run of the piece from the r-th position of u[l].
// k0: the sets with an empty `first`.
template <bool WIDE, bool NL>
__global__ __launch_bounds__(REGEX_STAR_BLOCK) void star_columns_kernel(const TileArgs a, const RegexStarX x, const RegexSets k0,
                                                                        uint64_t n_run, const uint64_t *e_in, const uint64_t *u_in,
                                                                        const uint64_t *off, uint64_t *base_out, uint64_t *cols)
{
    __shared__ uint32_t tab[RegexPolicy<WIDE, NL>::TAB];
    RegexPolicy<WIDE, NL>::fill(tab, a, threadIdx.x, x.k);
    __syncthreads();
    const uint64_t l = (uint64_t)blockIdx.x * REGEX_STAR_BLOCK + threadIdx.x;
    if (l >= n_run) return;
    const uint32_t cs = a.p_shift - 4;
    const uint64_t c0 = l << cs, c1 = (l + 1) << cs;
    ShiftAndState<WIDE> s;
    star_state_set<WIDE>(s, e_in[l]);
    star_single_walk<WIDE, NL>(a, x.k, tab, c0, c1, s);
    base_out[l] = star_state_get<WIDE>(s);
    uint64_t *col = cols + off[l];
#pragma unroll 1
    for (uint64_t u_bits = u_in[l]; u_bits != 0; u_bits &= u_bits - 1, ++col) {
        star_state_set<WIDE>(s, u_bits & (~u_bits + 1)); // the lowest position left
        star_single_walk<WIDE, NL>(a, k0, tab, c0, c1, s);
        *col = star_state_get<WIDE>(s);
    }
}

// Sweep: the lane of every piece whose entry state is known (u == 0: piece 0, and wherever the bounds met) stores it and
// carries it through the pieces behind until the next such piece.
__global__ __launch_bounds__(REGEX_STAR_BLOCK) void star_sweep_kernel(uint64_t n_pieces, const uint64_t *e_in, const uint64_t *u_in,
                                                                      const uint64_t *off, const uint64_t *base, const uint64_t *cols,
                                                                      uint64_t *entry)
{
    uint64_t l = (uint64_t)blockIdx.x * REGEX_STAR_BLOCK + threadIdx.x;
    if (l >= n_pieces || u_in[l] != 0) return;
    uint64_t truth = e_in[l], u = 0;
    entry[l] = truth;
    for (;;) {
        if (l + 1 >= n_pieces) return;
        const uint64_t u_next = u_in[l + 1];
        if (u_next == 0) return; // the next chain's
        uint64_t next = base[l];
        const uint64_t *col = cols + off[l];
        for (uint64_t bits = truth & u; bits != 0; bits &= bits - 1) {
            const uint64_t bit = bits & (~bits + 1);
            next |= col[__popcll(u & (bit - 1))];
        }
        ++l;
        truth = next;
        u = u_next;
        entry[l] = truth;
    }
}

// Starts: what regex_starts_kernel stored for an end without a match within the window is the end itself, which is also
// what a match of one byte gives.  Run only where the status word says that some entry had none: an entry whose start
// equals its end and whose byte is in no class of first & last gets the sentinel.
struct RegexStarFixArgs {
    const uint8_t *text;
    uint64_t base;
    const uint64_t *ends;
    uint64_t count;
    uint64_t *starts;
    uint64_t one[4]; // bit c: the one-byte string c matches
};
__global__ __launch_bounds__(REGEX_STAR_BLOCK) void star_starts_fix_kernel(const RegexStarFixArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * REGEX_STAR_BLOCK + threadIdx.x;
    if (i >= a.count) return;
    const uint64_t e = a.ends[i];
    if (a.starts[i] != e) return;
    const uint32_t c = a.text[e - a.base]; // (every end is inside the view: the status word said so)
    if (!((a.one[c >> 6] >> (c & 63)) & 1u)) a.starts[i] = ~0ull;
}

} // namespace bmx
