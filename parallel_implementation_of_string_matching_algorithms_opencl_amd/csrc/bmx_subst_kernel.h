// bmx_subst_kernel.h -- non-overlapping match selection, replace and extract on device lists (bmx_spans_select*,
// bmx_replace*, bmx_extract*, include/bmx.h).  No counterpart in the reference.
//
// Spans.  Entry j of a list is the span [s, e] (e the last byte) in one of three input forms (both lists; starts and a
// length; ends and a length).  subst_span() reads it and says whether the selection skips it.
//
// Select, disjoint.  key[j] = s + 1 (0: skipped), PM = the inclusive prefix maximum of key (rocPRIM).  The list is in
// order iff PM[j-1] <= e[j] + 1 for every entry that is not skipped, and then the entry taken after a taken entry j is
// next[j] = the first i with PM[i] > e[j] + 1 (DESIGN.md s29 has the proof); the first entry taken is the first i with
// PM[i] > 0.  next[j] > j, so the chain from there is resolved in tiles of T = 2^shift entries: X_0 = next, X_l[j] = the
// first element of j's chain at or past the end of j's block of T^l entries.  X_1 comes from shift rounds of pointer
// jumping in LDS, X_l (l >= 2) from shift rounds over X_(l-1) in global memory between two buffers; L is the smallest
// level at which at most T blocks remain.  One lane walks X_L over those blocks and leaves the first chain element of each
// in E_L; then, level by level and one lane per block, a walk of at most T steps over X_(l-1) leaves the first chain
// element of every sub-block in E_(l-1); E_0 is the flag "taken".  No lane follows more than T pointers per level.
//
// Select, merge.  PE = prefix maximum of e + 1, SM = suffix minimum of s (a prefix maximum of ~s over the reversed list).
// Entry j heads a region iff it is not skipped and SM[j] >= PE[j-1]; the region runs from SM[j] to PE[next head - 1] - 1.
//
// Both end in an exclusive sum of the flags (rocPRIM) and a fill in order: no atomics on the output, no sort.
//
// Copy (replace and extract), driven by the output.  The output is a sequence of pieces: piece i begins at output byte
// A[i], opens with `lead` bytes of the replacement (replace: every piece but the first; extract: none) and goes on with the
// text bytes at output position + delta[i].  A workgroup of SUBST_BLOCK lanes takes tiles of SUBST_TILE output bytes;
// wave w of it owns SUBST_LINES KiB of the tile, lane l the aligned 16-byte line at 16 l of each KiB.  The wave finds the
// pieces of its first and of its last byte (64 probes to a step) and every lane searches between the two.  A line that
// lies inside one piece's text is two aligned 16-byte loads, a funnel shift and one 16-byte store, the loads of the lane's
// four lines issued before the first is used; any other line is put together byte by byte.  The replacement sits in LDS.
// Only 16-byte lines that hold a byte of the text are loaded.
//
// Copy with a template (bmx_expand_device): the same body with a wider piece model.  T references make T + 1
// pieces per match; piece r opens with literal r of the template (offset and length from a table in LDS, indexed by the
// piece's number modulo T + 1) and goes on with a run of text that may be empty.  The piece starts are an exclusive sum over
// lengths read from the group table of bmx_regex_groups_device.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmx {

constexpr int SUBST_BLOCK = 256;                       // lanes per workgroup, every kernel of this file
constexpr uint32_t SUBST_TILE_SHIFT = 8;               // production T = 256 entries: one workgroup's LDS round
constexpr uint64_t SUBST_NONE = ~0ull;                 // a skipped start, == BMX_ROW_NONE
constexpr uint32_t SUBST_NO_ENTRY = 0xffffffffu;       // E_l: the block holds no chain element
constexpr int SUBST_WORDS = 4;                         // status words of a call: [0] bad list (the others are spare)
constexpr int SUBST_LINES = 4;                         // 16-byte lines per lane and tile
constexpr uint32_t SUBST_WAVE_BYTES = 1024u * SUBST_LINES;                  // a wave's contiguous piece of the tile
constexpr uint32_t SUBST_TILE = (SUBST_BLOCK / 64) * SUBST_WAVE_BYTES;      // 16 KiB of output

struct SubstList {
    const uint64_t *starts, *ends, *row; // starts or ends may be NULL (then len >= 1); row may be NULL
    uint64_t len, count;
};

// span j of the list; false: the selection skips it (s and e are then unspecified)
__device__ __forceinline__ bool subst_span(const SubstList &l, uint64_t j, uint64_t &s, uint64_t &e)
{
    if (l.starts != nullptr && l.ends != nullptr) {
        s = l.starts[j], e = l.ends[j];
    } else if (l.starts != nullptr) {
        s = l.starts[j], e = s + (l.len - 1);
    } else {
        e = l.ends[j], s = e - (l.len - 1);
        if (e < l.len - 1) return false;
    }
    if (s == SUBST_NONE || e == SUBST_NONE || e < s) return false; // (e >= len - 1: checked above, or s + len - 1 did not wrap)
    return l.row == nullptr || l.row[j] != SUBST_NONE;
}

// the smallest index i in [lo, hi] with a[i] > v, or hi (a[hi] is never read); a is non-decreasing
__device__ __forceinline__ uint64_t subst_upper(const uint64_t *a, uint64_t lo, uint64_t hi, uint64_t v)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] > v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the same for a v that all 64 lanes share, 64 probes to a step; every lane of the wave calls it
__device__ __forceinline__ uint64_t subst_upper_wave(const uint64_t *a, uint64_t lo, uint64_t hi, uint64_t v, uint32_t lane)
{
    while (hi - lo > 64) {
        const uint64_t step = (hi - lo + 63) / 64; // >= 2
        const uint64_t q = lo + (uint64_t)(lane + 1) * step - 1;
        const uint64_t greater = __ballot(q >= hi || a[q] > v);
        const uint32_t f = greater ? (uint32_t)__builtin_ctzll(greater) : 64u; // (lane 63 probes hi - 1 or past it)
        const uint64_t new_hi = f == 64 ? hi : min(lo + (uint64_t)(f + 1) * step - 1, hi);
        lo = f == 0 ? lo : lo + (uint64_t)f * step;
        hi = new_hi;
    }
    const uint64_t q = lo + lane;
    const uint64_t greater = __ballot(q < hi && a[q] > v);
    return greater ? lo + (uint32_t)__builtin_ctzll(greater) : hi;
}

// ---- select, disjoint ----

// key[j] = s + 1, 0 for a skipped entry
__global__ __launch_bounds__(SUBST_BLOCK) void select_key_kernel(const SubstList l, uint64_t *key)
{
    const uint64_t j = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (j >= l.count) return;
    uint64_t s, e;
    key[j] = subst_span(l, j, s, e) ? s + 1 : 0;
}

// next[j] (count: the chain ends) and the order condition.  A skipped entry points at its neighbour, and no pointer goes
// backwards even in a list that breaks the condition: every later walk ends.
__global__ __launch_bounds__(SUBST_BLOCK) void select_next_kernel(const SubstList l, const uint64_t *pm, uint32_t *next,
                                                                 unsigned long long *words)
{
    const uint64_t count = l.count;
    const uint64_t j = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t s = 0, e = 0;
    const bool ok = j < count && subst_span(l, j, s, e);
    const uint64_t e1 = e + 1;
    if (ok && j > 0 && pm[j - 1] > e1) words[0] = 1;
    // the wave's smallest and largest end bound every lane's search (PM is monotone)
    uint64_t mn = ok ? e1 : SUBST_NONE, mx = ok ? e1 : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mn = min(mn, (uint64_t)__shfl_xor((unsigned long long)mn, d));
        mx = max(mx, (uint64_t)__shfl_xor((unsigned long long)mx, d));
    }
    if (mn > mx) { // no lane of the wave has a span
        if (j < count) next[j] = (uint32_t)(j + 1);
        return;
    }
    const uint64_t wave0 = j - lane; // (the same in every lane, below count)
    const uint64_t ub_lo = subst_upper_wave(pm, wave0, count, mn, lane);
    uint64_t ub_hi = ub_lo;
    if (mn != mx) { // ascending lists: the largest end's successor lies a few entries on
        const uint64_t near = min(ub_lo + 4096, count);
        const bool within = near == count || pm[near - 1] > mx; // (near >= 1: count >= 1)
        ub_hi = subst_upper_wave(pm, ub_lo, within ? near : count, mx, lane);
    }
    if (j >= count) return;
    uint64_t nx = j + 1;
    if (ok) nx = max(subst_upper(pm, ub_lo, ub_hi, e1), j + 1);
    next[j] = (uint32_t)nx;
}

// X_1 from X_0: `shift` rounds of pointer jumping in LDS; a workgroup holds SUBST_BLOCK >> shift whole tiles
__global__ __launch_bounds__(SUBST_BLOCK) void select_level1_kernel(const uint32_t *x0, uint32_t *x1, uint64_t count, uint32_t shift)
{
    __shared__ uint32_t sh[SUBST_BLOCK];
    const uint64_t base = (uint64_t)blockIdx.x * SUBST_BLOCK;
    const uint64_t j = base + threadIdx.x;
    const uint64_t tile_end = min(((j >> shift) + 1) << shift, count);
    uint64_t x = j < count ? x0[j] : count;
    for (uint32_t r = 0; r < shift; ++r) {
        sh[threadIdx.x] = (uint32_t)x;
        __syncthreads();
        if (x < tile_end) x = sh[x - base]; // (inside the lane's own tile, so inside the workgroup and below count)
        __syncthreads();
    }
    if (j < count) x1[j] = (uint32_t)x;
}

// one round of pointer jumping inside blocks of 2^block_shift entries, from `in` to `out`
__global__ __launch_bounds__(SUBST_BLOCK) void select_jump_kernel(const uint32_t *in, uint32_t *out, uint64_t count, uint32_t block_shift)
{
    const uint64_t j = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (j >= count) return;
    const uint64_t block_end = min(((j >> block_shift) + 1) << block_shift, count);
    uint32_t x = in[j];
    if (x < block_end) x = in[x];
    out[j] = x;
}

// The top of the chain, one lane: the first entry taken (the first i with PM[i] > 0) and from there X_L over at most T
// blocks of 2^block_shift entries.  Level 0: taken[p] = 1; above: entry[block] = p.
__global__ void select_top_kernel(const uint64_t *pm, const uint32_t *x, uint64_t count, uint32_t block_shift, uint32_t *entry,
                                  uint64_t *taken)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t p = subst_upper(pm, 0, count, 0);
    while (p < count) {
        if (block_shift == 0) taken[p] = 1;
        else entry[p >> block_shift] = (uint32_t)p;
        p = x[p];
    }
}

// One lane per block of 2^block_shift entries that holds a chain element: from its first one, x (the level below) over
// the block's at most T sub-blocks of 2^sub_shift entries, leaving each one's first chain element (level 0: the flag).
__global__ __launch_bounds__(SUBST_BLOCK) void select_descend_kernel(const uint32_t *entry, uint64_t blocks, const uint32_t *x,
                                                                    uint64_t count, uint32_t block_shift, uint32_t sub_shift,
                                                                    uint32_t *sub_entry, uint64_t *taken)
{
    const uint64_t b = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (b >= blocks) return;
    uint64_t q = entry[b];
    if (q == SUBST_NO_ENTRY) return;
    const uint64_t end = min((b + 1) << block_shift, count);
    while (q < end) {
        if (sub_shift == 0) taken[q] = 1;
        else sub_entry[q >> sub_shift] = (uint32_t)q;
        q = x[q];
    }
}

// slot[j] = taken entries in front of j (slot[count]: all of them): every taken entry stores itself below cap
__global__ __launch_bounds__(SUBST_BLOCK) void select_fill_kernel(const SubstList l, const uint64_t *slot, uint64_t *starts_out,
                                                                 uint64_t *ends_out, uint64_t *index_out, uint64_t cap)
{
    const uint64_t j = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (j >= l.count) return;
    const uint64_t k = slot[j];
    if (slot[j + 1] == k || k >= cap) return;
    uint64_t s, e;
    (void)subst_span(l, j, s, e);
    starts_out[k] = s, ends_out[k] = e;
    if (index_out) index_out[k] = j;
}

// ---- select, merge ----

// pe_key[j] = e + 1, sm_key[count - 1 - j] = ~s; 0 for a skipped entry
__global__ __launch_bounds__(SUBST_BLOCK) void merge_key_kernel(const SubstList l, uint64_t *pe_key, uint64_t *sm_key)
{
    const uint64_t j = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (j >= l.count) return;
    uint64_t s, e;
    const bool ok = subst_span(l, j, s, e);
    pe_key[j] = ok ? e + 1 : 0;
    sm_key[l.count - 1 - j] = ok ? ~s : 0;
}

// head[j]; an end below an earlier one raises words[0]
__global__ __launch_bounds__(SUBST_BLOCK) void merge_heads_kernel(const SubstList l, const uint64_t *pe, const uint64_t *sm_rev,
                                                                 uint64_t *head, unsigned long long *words)
{
    const uint64_t j = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (j > l.count) return;
    if (j == l.count) { // (the scan runs over count + 1 flags)
        head[j] = 0;
        return;
    }
    uint64_t s, e;
    const bool ok = subst_span(l, j, s, e);
    const uint64_t before = j ? pe[j - 1] : 0;
    if (ok && e + 1 < before) words[0] = 1;
    head[j] = ok && ~sm_rev[l.count - 1 - j] >= before;
}

// every head stores its region's start and its own index at its slot and the end of the region in front of it; the
// list's last entry stores the end of the last region
__global__ __launch_bounds__(SUBST_BLOCK) void merge_fill_kernel(uint64_t count, const uint64_t *slot, const uint64_t *pe,
                                                                const uint64_t *sm_rev, uint64_t *starts_out, uint64_t *ends_out,
                                                                uint64_t *index_out, uint64_t cap)
{
    const uint64_t j = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (j >= count) return;
    const uint64_t k = slot[j], total = slot[count];
    if (slot[j + 1] != k) {
        if (k < cap) {
            starts_out[k] = ~sm_rev[count - 1 - j];
            if (index_out) index_out[k] = j;
        }
        if (k >= 1 && k - 1 < cap) ends_out[k - 1] = pe[j - 1] - 1; // (k >= 1: an entry with a span lies in front of j)
    }
    if (j == count - 1 && total >= 1 && total - 1 < cap) ends_out[total - 1] = pe[j] - 1;
}

// ---- replace and extract ----

struct SubstView {
    uint64_t base_offset, n;
};

// the spans of a replace or an extract: ascending, pairwise disjoint, inside the view; anything else raises words[0]
__global__ __launch_bounds__(SUBST_BLOCK) void copy_check_kernel(const SubstList l, const SubstView v, unsigned long long *words)
{
    const uint64_t k = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (k >= l.count) return;
    uint64_t s, e;
    bool ok = subst_span(l, k, s, e) && s >= v.base_offset && e - v.base_offset < v.n;
    if (ok && k > 0) {
        uint64_t ps, pe;
        ok = subst_span(l, k - 1, ps, pe) && s > pe;
    }
    if (!ok) words[0] = 1;
}

// the length of span k (0 at k == count, which closes the exclusive sum), for rocPRIM's transform iterator
struct SubstSpanLen {
    SubstList l;
    __device__ uint64_t operator()(uint64_t k) const
    {
        if (k >= l.count) return 0;
        if (l.starts != nullptr && l.ends != nullptr) return l.ends[k] - l.starts[k] + 1;
        return l.len;
    }
};

// The pieces of the output from d = the exclusive sum of the span lengths.  Replace (pieces = count + 1): piece 0 is the
// text in front of span 0; piece k >= 1 begins with the replacement of span k - 1 at s - base - d[k-1] + (k-1) repl_len
// and goes on with the text behind that span.  Extract (pieces = count): piece k is span k at d[k].
__global__ __launch_bounds__(SUBST_BLOCK) void copy_pieces_kernel(const SubstList l, const SubstView v, const uint64_t *d, uint64_t repl_len,
                                                                 int extract, uint64_t *a, uint64_t *delta)
{
    const uint64_t k = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    uint64_t s, e;
    if (extract) {
        if (k >= l.count) return;
        (void)subst_span(l, k, s, e);
        a[k] = d[k];
        delta[k] = s - v.base_offset - d[k];
        return;
    }
    if (k > l.count) return;
    if (k == 0) {
        a[0] = 0, delta[0] = 0;
        return;
    }
    (void)subst_span(l, k - 1, s, e);
    a[k] = s - v.base_offset - d[k - 1] + (k - 1) * repl_len;
    delta[k] = d[k] - k * repl_len;
}

typedef uint32_t subst_u32x4 __attribute__((ext_vector_type(4)));

struct SubstCopyArgs {
    const uint8_t *text;   // the caller's pointer (byte loads of the lines put together piece by piece)
    const uint64_t *a;     // pieces: the first output byte of each, non-decreasing
    const uint64_t *delta; // text position = output position + delta[i] behind the piece's `lead` bytes
    uint64_t pieces;       // >= 1
    const uint8_t *repl;   // device copy of the replacement
    uint32_t lead;         // its bytes in front of every piece but the first (0: extract)
    uint8_t *out16;        // the output pointer rounded down to a multiple of 16
    uint64_t own_lo;       // aligned coordinate of output byte 0 (0..15)
    uint64_t own_hi;       // one past the last byte to store (bytes + own_lo), bytes >= 1
    uint64_t n_tiles;
};

// 16 bytes from byte `sh` (0..15) of the 32 bytes lo, hi
__device__ __forceinline__ subst_u32x4 subst_funnel(subst_u32x4 lo, subst_u32x4 hi, uint32_t sh)
{
    uint64_t q0 = lo[0] | ((uint64_t)lo[1] << 32), q1 = lo[2] | ((uint64_t)lo[3] << 32);
    uint64_t q2 = hi[0] | ((uint64_t)hi[1] << 32), q3 = hi[2] | ((uint64_t)hi[3] << 32);
    if (sh >= 8) q0 = q1, q1 = q2, q2 = q3, sh -= 8;
    if (sh) {
        const uint32_t r = 8 * sh, c = 64 - r;
        q0 = (q0 >> r) | (q1 << c);
        q1 = (q1 >> r) | (q2 << c);
    }
    subst_u32x4 o;
    o[0] = (uint32_t)q0, o[1] = (uint32_t)(q0 >> 32), o[2] = (uint32_t)q1, o[3] = (uint32_t)(q1 >> 32);
    return o;
}

// The piece model of a template (bmx_expand_device): T references make t1 = T + 1 pieces per match.  Piece p >= first
// opens with literal r = (p - first) % t1, len[r] bytes at off[r] of the literal bytes; the pieces below `first` (replace:
// the text in front of the first match) have none.
constexpr int SUBST_MAX_LITERALS = 33; // == BMX_MAX_TEMPLATE_REFS + 1
struct SubstTemplate {
    uint32_t t1, first;
    uint32_t off[SUBST_MAX_LITERALS], len[SUBST_MAX_LITERALS];
};

// TMPL false: the literal replacement, every piece but the first opens with the g.lead bytes of it.  TMPL true: tab holds
// the template's off[] and, SUBST_MAX_LITERALS words on, len[]; g.lead is the number of literal bytes in LDS.
template <bool TMPL>
__device__ __forceinline__ void subst_copy_body(const SubstCopyArgs &g, const uint8_t *sh_repl, const uint32_t *tab, uint32_t t1,
                                                uint32_t first_piece)
{
    // the literal in front of piece p: its length, and (TMPL) where it begins in sh_repl
    const auto lead_of = [&](uint64_t p, uint32_t &off) -> uint64_t {
        if (TMPL) {
            if (p < first_piece) return off = 0, 0;
            const uint32_t r = (uint32_t)((p - first_piece) % t1);
            off = tab[r];
            return tab[SUBST_MAX_LITERALS + r];
        }
        off = 0;
        return p ? g.lead : 0;
    };
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t t = blockIdx.x; t < g.n_tiles; t += gridDim.x) {
        const uint64_t wave0 = t * SUBST_TILE + (uint64_t)wave * SUBST_WAVE_BYTES; // aligned coordinate of the wave's first byte
        if (wave0 >= g.own_hi) continue;                                           // (the same in every lane of the wave)
        // the pieces of the wave's first and last byte: p_lo .. p_hi, both the last piece with a[p] <= the byte
        const uint64_t first = max(wave0, g.own_lo) - g.own_lo, last = min(wave0 + SUBST_WAVE_BYTES, g.own_hi) - 1 - g.own_lo;
        const uint64_t p_lo = subst_upper_wave(g.a, 0, g.pieces, first, lane) - 1; // (a[0] = 0 <= first)
        uint64_t p_hi = p_lo;
        if (p_lo + 1 < g.pieces) {
            const uint64_t near = min(p_lo + 65, g.pieces);
            const bool within = near == g.pieces || g.a[near - 1] > last;
            p_hi = subst_upper_wave(g.a, p_lo + 1, within ? near : g.pieces, last, lane) - 1;
        }
        uint64_t x[SUBST_LINES], src[SUBST_LINES], piece[SUBST_LINES];
        bool fast[SUBST_LINES];
        subst_u32x4 v_lo[SUBST_LINES], v_hi[SUBST_LINES];
#pragma unroll
        for (int i = 0; i < SUBST_LINES; ++i) {
            const uint64_t c = wave0 + (uint32_t)i * 1024u + lane * 16u; // aligned coordinate of the line
            x[i] = c - g.own_lo;                                          // (wraps in front of the output: `whole` is false)
            const bool whole = c >= g.own_lo && c + 16 <= g.own_hi;
            uint64_t p = p_lo;
            if (c < g.own_hi && p_lo != p_hi) p = subst_upper(g.a, p_lo + 1, p_hi + 1, c >= g.own_lo ? x[i] : 0) - 1;
            piece[i] = p;
            uint32_t lead_off = 0;
            const uint64_t lead = TMPL ? lead_of(p, lead_off) : (p ? g.lead : 0);
            fast[i] =whole && x[i] - g.a[p] >= lead && (p + 1 == g.pieces || x[i] + 16 <= g.a[p + 1]);
            src[i] = x[i] + g.delta[p];
        }
#pragma unroll
        for (int i = 0; i < SUBST_LINES; ++i) { // the loads of a lane's lines before the first is used
            if (fast[i]) {                      // (bytes src .. src + 15 are the text's: both lines hold one)
                const uint64_t addr = reinterpret_cast<uint64_t>(g.text) + src[i];
                const subst_u32x4 *line = reinterpret_cast<const subst_u32x4 *>(addr & ~15ull);
                v_lo[i] = line[0];
                v_hi[i] = line[(addr & 15ull) ? 1 : 0];
            }
        }
#pragma unroll
        for (int i = 0; i < SUBST_LINES; ++i) {
            const uint64_t c = wave0 + (uint32_t)i * 1024u + lane * 16u;
            if (fast[i]) {
                const uint32_t sh = (uint32_t)((reinterpret_cast<uint64_t>(g.text) + src[i]) & 15ull);
                *reinterpret_cast<subst_u32x4 *>(g.out16 + c) = subst_funnel(v_lo[i], v_hi[i], sh);
                continue;
            }
            if (c >= g.own_hi) continue;
            // byte by byte: the line holds a piece boundary, a replacement, or the output's first or last bytes
            uint64_t p = piece[i];
            uint8_t b[16];
            const uint32_t from = c >= g.own_lo ? 0u : (uint32_t)(g.own_lo - c);
            const uint32_t to = (uint32_t)min((uint64_t)16, g.own_hi - c);
            if (TMPL) {
                uint32_t lit_off;
                uint64_t lit_len = lead_of(p, lit_off);
                for (uint32_t k = from; k < to; ++k) {
                    const uint64_t y = c + k - g.own_lo;
                    // the last piece with a[p] <= y: in a run of equal a[] (an empty group, an empty literal) the one that holds y
                    if (p + 1 < g.pieces && g.a[p + 1] <= y) {
                        do ++p;
                        while (p + 1 < g.pieces && g.a[p + 1] <= y);
                        lit_len = lead_of(p, lit_off);
                    }
                    const uint64_t in = y - g.a[p];
                    b[k] = in < lit_len ? sh_repl[lit_off + in] : g.text[y + g.delta[p]];
                }
            } else {
                for (uint32_t k = from; k < to; ++k) {
                    const uint64_t y = c + k - g.own_lo;
                    while (p + 1 < g.pieces && g.a[p + 1] <= y) ++p;
                    const uint64_t in = y - g.a[p];
                    b[k] = (p && in < g.lead) ? sh_repl[in] : g.text[y + g.delta[p]];
                }
            }
            if (from == 0 && to == 16) {
                subst_u32x4 o;
#pragma unroll
                for (int w = 0; w < 4; ++w) o[w] = b[4 * w] | ((uint32_t)b[4 * w + 1] << 8) | ((uint32_t)b[4 * w + 2] << 16) | ((uint32_t)b[4 * w + 3] << 24);
                *reinterpret_cast<subst_u32x4 *>(g.out16 + c) = o;
            } else {
                for (uint32_t k = from; k < to; ++k) g.out16[c + k] = b[k];
            }
        }
    }
}

__global__ __launch_bounds__(SUBST_BLOCK) void subst_copy_kernel(const SubstCopyArgs g)
{
    extern __shared__ uint8_t sh_repl[];
    for (uint32_t i = threadIdx.x; i < g.lead; i += SUBST_BLOCK) sh_repl[i] = g.repl[i];
    __syncthreads();
    subst_copy_body<false>(g, sh_repl, nullptr, 1, 0);
}

// ... with a template: the literal bytes in the dynamic LDS, the table of the literals in front of them
__global__ __launch_bounds__(SUBST_BLOCK) void expand_copy_kernel(const SubstCopyArgs g, const SubstTemplate tp)
{
    extern __shared__ uint8_t sh_repl[];
    __shared__ uint32_t tab[2 * SUBST_MAX_LITERALS];
    for (uint32_t i = threadIdx.x; i < g.lead; i += SUBST_BLOCK) sh_repl[i] = g.repl[i];
    if (threadIdx.x < SUBST_MAX_LITERALS) {
        tab[threadIdx.x] = tp.off[threadIdx.x];
        tab[SUBST_MAX_LITERALS + threadIdx.x] = tp.len[threadIdx.x];
    }
    __syncthreads();
    subst_copy_body<true>(g, sh_repl, tab, tp.t1, tp.first);
}

// ---- the pieces of a template expansion (bmx_expand_device) ----

// d_groups of bmx_regex_groups_device: `pairs` = n_groups + 1 half-open (begin, end) pairs per entry
struct ExpandList {
    const uint64_t *groups;
    uint64_t count;
    uint32_t pairs, t1, first; // t1 = T + 1 pieces per match; first: 1 = replace (piece 0 is the text in front), 0 = extract
    int32_t ref[SUBST_MAX_LITERALS - 1];
    uint32_t lit_len[SUBST_MAX_LITERALS];
};

// group 0 of every entry: set, non-empty, inside the view, not below the entry in front; every other group unset or inside
// its entry's group 0.  Anything else raises words[0].
__global__ __launch_bounds__(SUBST_BLOCK) void expand_check_kernel(const ExpandList l, const SubstView v, unsigned long long *words)
{
    const uint64_t k = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (k >= l.count) return;
    const uint64_t *g = l.groups + k * l.pairs * 2;
    const uint64_t b0 = g[0], e0 = g[1];
    bool ok = b0 != SUBST_NONE && e0 != SUBST_NONE && b0 >= v.base_offset && e0 > b0 && e0 - v.base_offset <= v.n;
    if (ok && k > 0) {
        const uint64_t pe = g[1 - (int64_t)l.pairs * 2]; // the end of the entry in front
        ok = pe != SUBST_NONE && pe <= b0;
    }
    for (uint32_t q = 1; ok && q < l.pairs; ++q) {
        const uint64_t gb = g[2 * q], ge = g[2 * q + 1];
        if (gb == SUBST_NONE && ge == SUBST_NONE) continue;
        ok = gb >= b0 && ge >= gb && ge <= e0;
    }
    if (!ok) words[0] = 1;
}

// the bytes of piece p (0 at p == pieces, which closes the exclusive sum), for rocPRIM's transform iterator
struct ExpandPieceLen {
    ExpandList l;
    SubstView v;
    __device__ uint64_t operator()(uint64_t p) const
    {
        if (p < l.first) return l.groups[0] - v.base_offset; // replace: the text in front of the first match
        const uint64_t q = p - l.first, k = q / l.t1;
        const uint32_t r = (uint32_t)(q % l.t1);
        if (k >= l.count) return 0;
        const uint64_t *g = l.groups + k * l.pairs * 2;
        uint64_t len = l.lit_len[r];
        if (r + 1 < l.t1) { // the group of reference r; nothing where it is unset
            const uint64_t gb = g[2 * l.ref[r]], ge = g[2 * l.ref[r] + 1];
            if (gb != SUBST_NONE) len += ge - gb;
        } else if (l.first) { // replace: the text behind the match, up to the next one or the view's end
            len += (k + 1 < l.count ? g[l.pairs * 2] : v.base_offset + v.n) - g[1];
        }
        return len;
    }
};

// delta[p] from a = the exclusive sum of the piece lengths: the run of text behind piece p's literal begins at view byte
// `src`, so text position = output position + (src - a[p] - literal length).  Extract: off[k] = a[k t1], off[count] = a[pieces].
__global__ __launch_bounds__(SUBST_BLOCK) void expand_delta_kernel(const ExpandList l, const SubstView v, const uint64_t *a, uint64_t pieces,
                                                                  uint64_t *delta, uint64_t *off)
{
    const uint64_t p = (uint64_t)blockIdx.x * SUBST_BLOCK + threadIdx.x;
    if (p >= pieces) return;
    if (p < l.first) {
        delta[p] = 0;
        return;
    }
    const uint64_t q = p - l.first, k = q / l.t1;
    const uint32_t r = (uint32_t)(q % l.t1);
    const uint64_t *g = l.groups + k * l.pairs * 2;
    uint64_t src = g[1]; // behind the match
    if (r + 1 < l.t1) {
        const uint64_t gb = g[2 * l.ref[r]];
        src = gb != SUBST_NONE ? gb : g[0]; // (an unset group: an empty run, delta is never used)
    }
    delta[p] = src - v.base_offset - a[p] - l.lit_len[r];
    if (off != nullptr) {
        if (r == 0) off[k] = a[p];
        if (p + 1 == pieces) off[l.count] = a[pieces];
    }
}

} // namespace bmx
