// bmx_align_kernel.h -- kernels of the alignments (bmx_align_device, include/bmx.h): one entry per lane,
// a pattern of 1 .. 512 bytes against a span text[s..j] of a resident text, the canonical edit script out as BAM op words.
//
// Table.  D[i][t] = ED(pat[0..i), span[0..t)), m = the pattern's length, L = the span's.  The script is the walk from
// (m, L) to (0, 0) that takes, at every cell, the first step that keeps the value: diagonal, up (I), left (D).
//
// Forward pass (align_kernel<T, W, BAND>).  Myers' column step in its GLOBAL form (row 0 costs 1 per column, as ed_batch_step)
// over the span's bytes with the state in W words of type T (uint32_t x 1, uint64_t x 1, 2, 4, 8; the longest pattern of
// the call picks the instance).  The pattern stays in registers in the layout of ed_batch_eq32 (bmx_eq_kernel.h), the
// text is read in aligned 8-byte words, one word ahead, none outside the words that hold the span.  Every column step
// also leaves, per row, the two bits the walk needs: whether the diagonal step keeps the value, and whether the bytes are
// equal or else the up step keeps it (align_planes); they go to workspace, and the walk reads neither pattern nor
// text again and does no arithmetic on table values.  (Storing pv / mv with a score per column instead costs the walk two
// byte loads per step and a masked popcount over the column per edit; the planes are no larger.)
// Every lane takes the same number of 8-column chunks (the host passes ceil((M + k) / 8) for the longest pattern M), a
// wave leaves the loop when none of its lanes has a column left, and steps past a lane's own span only stop counting.
//
// Workspace.  Column t of the 64 lanes of wave v, plane p (2 b, 2 b + 1 = the two planes of word b):
// cols[((v C + t) 2W + p) 64 + lane], C = 8 chunks -- one plane of one column of a wave is 64 consecutive words of T.
// A walk of at most k edits stays on rows |i - t| <= k, so where that band is narrower than the words (k <= 63, 64-bit
// words) only the band is stored: 2k + 1 rows from row t - k, cut into ceil((2k + 1) / 32) 32-bit halves h, in the same
// layout with 2 x halves planes of 32-bit words (AlignStore, align_use_band).  The column step shifts the band out of its
// words as it goes; the shifts are uniform over a wave.
//
// Traceback (align_traceback, the same lane, straight after its forward pass).  At cell (i, t) the two bits of row i in
// column t name the step: '=' or 'X' along the diagonal, 'I' up, 'D' left -- the first that keeps the value.  The planes of
// several columns are loaded at once, so the walk waits for memory once per ALIGN_AHEAD columns, not once per step.  Runs
// go from the back of the entry's slot of 2k + 1 words (a script of d edits has at most 2d + 1 runs), so that the slot's
// tail reads from the span's start to its end.
//
// Output.  nruns per entry, rocPRIM's exclusive scan of it into op_off (the host carries the total from batch to batch
// in device memory), and align_fill_kernel copies the slots' tails to ops.  No atomics.
//
// Memory safety: an entry with pid >= pat_count, offsets that decrease or end past the blob, a pattern of 0 or more than
// 64 W (T = uint64_t) / 32 (uint32_t) bytes, a position outside [base_offset, base_offset + n), end < start or exactly
// one position equal to NO_POS raises status[0] and reads neither pattern nor text.  An entry that aligns has
// L <= m + k <= 8 chunks, so every column index is inside the lane's workspace; slot writes are bounded by the slot.
//
// align_column (with align_planes and the band window) and align_traceback are __host__ __device__ so that
// tests/align_check.hip runs them on the CPU against a plain-table walk (tests/test_align_cpu.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bmx_eq_kernel.h"

namespace bmx {

constexpr uint32_t ALIGN_BLOCK = 256;
constexpr uint32_t ALIGN_MAX_PATTERN = 512; // == BMX_ALIGN_MAX_PATTERN
constexpr uint32_t ALIGN_MAX_K = 254;       // == BMX_ALIGN_MAX_K
constexpr uint32_t ALIGN_NONE = 255u;       // == BMX_ALIGN_NONE
constexpr uint64_t ALIGN_NO_POS = ~0ull;    // == BMX_MAP_NO_POS
constexpr uint32_t CIGAR_INS = 1u, CIGAR_DEL = 2u, CIGAR_EQ = 7u, CIGAR_X = 8u;
constexpr uint32_t ALIGN_BAD_WALK = 0xffffffffu; // align_traceback: the walk left its slot or its band, or its edits are not dist

// words of T per column of one wave's lane set: 2 W planes of 64 lanes
template <int W>
__host__ __device__ constexpr size_t align_column_stride() { return (size_t)2 * W * 64; }

// The pattern Q[0..m) into R registers, in the layout ed_batch_eq32 reads: bit 32 h + 8 k + j of Eq belongs to byte k of
// register 8 h + j.  Bytes at and above m stay 0 (and are masked off Eq).
template <int R>
__host__ __device__ __forceinline__ void align_load_pattern(uint32_t *p, const uint8_t *Q, uint32_t m)
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t x = 32u * (uint32_t)(r >> 3) + 8u * (uint32_t)k + (uint32_t)(r & 7);
            if (x < m) v |= (uint32_t)Q[x] << (8 * k);
        }
        p[r] = v;
    }
}

// What the walk needs of cell (i, t), two bits: A = the diagonal step keeps the value (the bytes are equal, or
// D[i][t] == D[i-1][t-1] + 1), B = the bytes are equal if A, else the up step keeps the value (D[i][t] == D[i-1][t] + 1).
// So A B reads 11 '=', 10 'X', 01 'I', 00 'D': the first step that keeps the value, in the order diagonal, up, left.
// eq: the Eq word of the column's byte, d0: Myers' D0 (bit i set: D[i][t] == D[i-1][t-1]), pv: the column's positive
// vertical deltas.
template <typename T>
__host__ __device__ __forceinline__ void align_planes(T eq, T d0, T pv, T &a, T &b)
{
    a = eq | (T)~d0;
    b = eq | ((T)~a & pv);
}

// v >> s for -64 < s < 64 (a negative s shifts left), 0 beyond
__host__ __device__ __forceinline__ uint64_t align_shift(uint64_t v, int s)
{
    return s <= -64 || s >= 64 ? 0ull : s >= 0 ? v >> s : v << -s;
}

// Where a column's planes go.  FULL (band == false): plane 2 b = A, 2 b + 1 = B of word b, words of T.  BAND: only the
// rows i with |i - t| <= k, which hold every cell of a walk of at most k edits: bit x of the window is row t - k + x, the
// window is cut into `halves` = ceil((2k + 1) / 32) <= 4 32-bit words, plane 2 h = A, 2 h + 1 = B of half h.  planes: the
// lane's word of plane 0 of the column, or nullptr (a step past the lane's span).
struct AlignStore {
    void *planes;
    uint32_t halves; // BAND
    int first;       // BAND: the window's first row as a bit of the column, t - k - 1 (may be negative)
};

__host__ __device__ inline uint32_t align_band_halves(uint32_t k) { return (2u * k + 1u + 31u) / 32u; }
// the band is stored when it is smaller than the words (T = uint64_t; the window holds at most 128 rows)
__host__ __device__ inline bool align_use_band(uint32_t k, int word_bytes, int W)
{
    return word_bytes == 8 && k <= 63u && align_band_halves(k) * 4u < (uint32_t)W * 8u;
}

// One column of W words of T in the global form (the horizontal delta that enters row 0 is +1): the word step of
// map_column (bmx_index_map_kernel.h).  lw, hb: word and bit of row m - 1, where the score is read.  words: the words the
// caller needs (uniform over a wave).
template <typename T, int W, bool BAND>
__host__ __device__ __forceinline__ void align_column(T *pv, T *mv, uint32_t &score, const uint32_t *p, uint32_t c, const T *mask,
                                                      uint32_t lw, uint32_t hb, uint32_t words, const AlignStore &st)
{
    constexpr int TOP = 8 * (int)sizeof(T) - 1;
    constexpr int REGS = 2 * (int)sizeof(T); // registers of the pattern per word
    const uint32_t c4 = c * 0x01010101u;
    T hp = 1, hm = 0;
    uint64_t wa[2] = {0, 0}, wb[2] = {0, 0}; // BAND: the window's 128 rows of either plane
#pragma unroll
    for (int b = 0; b < W; ++b) {
        if ((uint32_t)b < words) {
            const T eq0 = ed_batch_eq<T>(p + REGS * b, c4, mask[b]);
            const T xv = eq0 | mv[b];
            const T eq = eq0 | hm;
            const T xh = (T)((T)((T)(eq & pv[b]) + pv[b]) ^ pv[b]) | eq;
            const T d0 = xh | mv[b];
            T ph = mv[b] | (T)~(xh | pv[b]);
            T mh = pv[b] & xh;
            const uint32_t here = (uint32_t)b == lw ? 1u : 0u;
            score += here * ((uint32_t)((ph >> hb) & 1) - (uint32_t)((mh >> hb) & 1));
            const T op = ph >> TOP, om = mh >> TOP;
            ph = (T)(ph << 1) | hp;
            mh = (T)(mh << 1) | hm;
            pv[b] = mh | (T)~(xv | ph);
            mv[b] = ph & xv;
            hp = op, hm = om;
            T pa, pb;
            align_planes<T>(eq0, d0, pv[b], pa, pb);
            if (BAND) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    wa[q] |= align_shift((uint64_t)pa, st.first + 64 * q - 64 * b);
                    wb[q] |= align_shift((uint64_t)pb, st.first + 64 * q - 64 * b);
                }
            } else if (st.planes) {
                T *out = static_cast<T *>(st.planes);
                out[(size_t)(2 * b) * 64] = pa;
                out[(size_t)(2 * b + 1) * 64] = pb;
            }
        }
    }
    if (BAND && st.planes) {
        uint32_t *out = static_cast<uint32_t *>(st.planes);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            if ((uint32_t)h < st.halves) {
                out[(size_t)(2 * h) * 64] = (uint32_t)(wa[h >> 1] >> (32 * (h & 1)));
                out[(size_t)(2 * h + 1) * 64] = (uint32_t)(wb[h >> 1] >> (32 * (h & 1)));
            }
        }
    }
}

// The runs of one walk, written from the back of the slot.
struct AlignRuns {
    uint32_t *slot;
    uint32_t at; // the slot's words [at, size) are written
    uint32_t code, len;
    bool spilled;
    __host__ __device__ __forceinline__ void flush()
    {
        if (len == 0) return;
        if (at == 0) {
            spilled = true;
            return;
        }
        slot[--at] = (len << 4) | code;
    }
    __host__ __device__ __forceinline__ void put(uint32_t c, uint32_t n)
    {
        if (n == 0) return;
        if (c == code) {
            len += n;
            return;
        }
        flush();
        code = c, len = n;
    }
};

constexpr int ALIGN_AHEAD = 8; // columns whose planes a walk loads at once

// words (of T, or of 32 bits with BAND) between one stored column of a wave and the next
template <typename T, int W, bool BAND>
__host__ __device__ __forceinline__ size_t align_stride(uint32_t halves)
{
    return BAND ? (size_t)2 * halves * 64 : align_column_stride<W>();
}

// The walk from (m, L), where the table holds `dist`, to (0, 0).  col: the lane's word of plane 0 of stored column 0
// (span byte t - 1, table column t, is stored column t - 1).  It reads the two planes of the word (BAND: the half) that
// holds row i for ALIGN_AHEAD columns at once (the loads are independent of each other), then steps through those columns
// from registers; a step into another word loads afresh.  Returns the number of runs; they lie in
// slot[slot_words - runs .. slot_words) in the order of the span.  ALIGN_BAD_WALK: more runs than the slot holds, a walk
// whose edits are not `dist`, or one that leaves the band (none happens with dist <= k and a slot of 2k + 1 words).
template <typename T, int W, bool BAND>
__host__ __device__ inline uint32_t align_traceback(const void *colv, uint32_t halves, uint32_t k, uint32_t m, uint32_t L,
                                                    uint32_t dist, uint32_t *slot, uint32_t slot_words)
{
    typedef typename std::conditional<BAND, uint32_t, T>::type E;
    constexpr uint32_t BITS = 8 * (uint32_t)sizeof(E);
    const E *col = static_cast<const E *>(colv);
    const size_t stride = align_stride<T, W, BAND>(halves);
    AlignRuns runs = {slot, slot_words, 0u, 0u, false};
    uint32_t i = m, t = L, edits = 0;
    bool left_band = false;
    while (i > 0 && t > 0 && !left_band) {
        // the bit of cell (i, t) in its column's planes: row i - 1, or with BAND row i - (t - k) of the window
        const uint32_t x0 = BAND ? i + k - t : i - 1u;
        if (BAND && x0 > 2u * k) {
            left_band = true;
            break;
        }
        const uint32_t wb = x0 / BITS;
        E pa[ALIGN_AHEAD], pb[ALIGN_AHEAD];
#pragma unroll
        for (int j = 0; j < ALIGN_AHEAD; ++j) { // table columns t, t - 1, ..
            const bool have = t > (uint32_t)j;
            const E *c = col + (size_t)(have ? t - 1u - (uint32_t)j : 0u) * stride + (size_t)(2u * wb) * 64;
            pa[j] = have ? c[0] : (E)0;
            pb[j] = have ? c[64] : (E)0;
        }
        bool afresh = false;
#pragma unroll
        for (int j = 0; j < ALIGN_AHEAD; ++j) {
            // the steps inside one column: up while that keeps the value, out by a diagonal or a left step
            while (!afresh && i > 0 && t > 0) {
                const uint32_t x = BAND ? i + k - t : i - 1u;
                if ((BAND && x > 2u * k) || x / BITS != wb) {
                    afresh = true; // (outside the band: the outer loop says so)
                    break;
                }
                const uint32_t bit = x % BITS;
                const uint32_t a = (uint32_t)(pa[j] >> bit) & 1u, b = (uint32_t)(pb[j] >> bit) & 1u;
                if (a) {
                    runs.put(b ? CIGAR_EQ : CIGAR_X, 1);
                    edits += 1u - b;
                    --i, --t;
                    break;
                }
                ++edits;
                if (b) {
                    runs.put(CIGAR_INS, 1);
                    --i;
                } else {
                    runs.put(CIGAR_DEL, 1);
                    --t;
                    break;
                }
            }
        }
    }
    runs.put(CIGAR_INS, i); // column 0: D[i][0] = i
    runs.put(CIGAR_DEL, t); // row 0: D[0][t] = t
    edits += i + t;
    runs.flush();
    if (runs.spilled || left_band || edits != dist) return ALIGN_BAD_WALK;
    return slot_words - runs.at;
}

#ifndef BMX_ALIGN_PIECES_ONLY // (tests/align_check.hip builds for the host alone: the pieces above, no kernel)

// bytes of column workspace per entry (the header's formula): C columns of 2 W words of T, or of 2 halves of 32 bits
inline size_t align_entry_col_bytes(uint32_t chunks, int word_bytes, int W, uint32_t k)
{
    const size_t column = align_use_band(k, word_bytes, W) ? (size_t)2 * align_band_halves(k) * 4 : (size_t)2 * W * word_bytes;
    return (size_t)8 * chunks * column;
}

// status[0]: an entry that failed its checks, status[1]: a walk that came back as ALIGN_BAD_WALK
struct AlignArgs {
    const uint8_t *text;
    uint64_t n, base_offset;
    const uint8_t *pat;
    uint64_t pat_bytes;
    const uint64_t *pat_off;
    uint64_t pat_count;
    const uint32_t *pid; // may be nullptr
    const uint64_t *start, *end;
    uint64_t e0, e1; // the entries of this launch; its lanes, nruns, slots and columns count from e0
    uint32_t one;    // pid == nullptr: every entry takes pattern 0
    uint32_t k;
    uint32_t chunks; // 8-column chunks every lane walks: ceil((M + k) / 8)
    uint8_t *dist;   // per entry of the call, may be nullptr
    uint32_t *nruns; // per entry of the launch
    uint32_t *slots; // 2k + 1 words per entry of the launch
    void *cols;      // the column workspace of the launch
    uint64_t *status;
};

// the longest pattern of the column, for the instance and the chunk count (offsets that decrease count as 0)
struct AlignPatLen {
    const uint64_t *pat_off;
    __host__ __device__ uint64_t operator()(uint64_t p) const
    {
        const uint64_t o0 = pat_off[p], o1 = pat_off[p + 1];
        return o1 > o0 ? o1 - o0 : 0ull;
    }
};
struct AlignMax {
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};
struct AlignToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

template <typename T, int W, bool BAND>
__global__ __launch_bounds__(ALIGN_BLOCK) void align_kernel(const AlignArgs a)
{
    constexpr uint32_t BITS = 8 * (uint32_t)sizeof(T);
    constexpr int REGS = 2 * (int)sizeof(T) * W;
    const uint64_t j = (uint64_t)blockIdx.x * ALIGN_BLOCK + threadIdx.x; // the lane's entry within the launch
    const uint64_t e = a.e0 + j;
    const bool listed = e < a.e1;

    // the entry: ok = a table to fill; otherwise it has no alignment (or is bad)
    bool ok = false;
    uint32_t m = 1, L = 0;
    uint64_t s = 0;
    const uint8_t *Q = nullptr;
    if (listed) {
        const uint64_t ps = a.start[e], pe = a.end[e];
        if (ps == ALIGN_NO_POS && pe == ALIGN_NO_POS) {
            // a read without a hit
        } else {
            const uint64_t p = a.pid ? (uint64_t)a.pid[e] : a.one ? 0ull : e;
            bool good = ps != ALIGN_NO_POS && pe != ALIGN_NO_POS && ps >= a.base_offset && pe >= ps && pe - a.base_offset < a.n &&
                        p < a.pat_count;
            uint64_t o0 = 0, o1 = 0;
            if (good) {
                o0 = a.pat_off[p], o1 = a.pat_off[p + 1];
                good = o1 > o0 && o1 <= a.pat_bytes && o1 - o0 <= (uint64_t)BITS * W && o1 - o0 <= ALIGN_MAX_PATTERN;
            }
            if (!good) {
                a.status[0] = 1;
            } else {
                const uint64_t len = pe - ps + 1, mm = o1 - o0;
                if ((len > mm ? len - mm : mm - len) <= a.k) { // (else: no alignment within k, and no byte is read)
                    ok = true;
                    m = (uint32_t)mm, L = (uint32_t)len;
                    s = ps - a.base_offset;
                    Q = a.pat + o0;
                }
            }
        }
    }
    const uint32_t lw = (m - 1u) / BITS, hb = (m - 1u) % BITS;
    uint32_t words = 0;
#pragma unroll
    for (int b = 0; b < W; ++b)
        if (__ballot(ok && lw >= (uint32_t)b)) words = b + 1;

    uint32_t dist = ALIGN_NONE, nruns = 0;
    if (words != 0) { // (uniform)
        uint32_t p[REGS];
        align_load_pattern<REGS>(p, Q, ok ? m : 0u);
        T mask[W], pv[W], mv[W];
#pragma unroll
        for (int b = 0; b < W; ++b) {
            mask[b] = !ok || (uint32_t)b > lw ? (T)0 : (uint32_t)b < lw || hb == BITS - 1u ? (T)~(T)0 : (T)(((T)2 << hb) - 1);
            pv[b] = (T)~(T)0, mv[b] = 0;
        }
        uint32_t score = m;
        typedef typename std::conditional<BAND, uint32_t, T>::type E;
        const uint32_t halves = align_band_halves(a.k);
        const size_t stride = align_stride<T, W, BAND>(halves);
        E *col = static_cast<E *>(a.cols) + (size_t)(j >> 6) * (8u * a.chunks) * stride + (j & 63u);

        // aligned 8-byte words of the span, from the word that holds s to the one that holds s + L - 1
        const uintptr_t t0 = (uintptr_t)a.text;
        const uint64_t *words8 = reinterpret_cast<const uint64_t *>(t0 & ~(uintptr_t)7);
        const uint64_t first = t0 & 7u;
        uint64_t wi = (first + s) >> 3;
        const uint64_t wlast = ok ? (first + s + L - 1u) >> 3 : 0;
        const uint32_t sh = (uint32_t)((first + s) & 7u) * 8u;
        uint64_t lo = ok ? words8[wi] : 0ull;
        uint64_t hi = ok && wi + 1 <= wlast ? words8[wi + 1] : 0ull;
        uint32_t pos = 0;
        for (uint32_t ch = 0; ch < a.chunks; ++ch) {
            if (!__ballot(pos < L)) break; // (uniform: no lane of the wave has a column left)
            const uint64_t cur = sh ? (lo >> sh) | (hi << (64u - sh)) : lo; // span[pos .. pos + 8), the first in the low byte
            lo = hi;
            ++wi;
            hi = ok && wi + 1 <= wlast ? words8[wi + 1] : 0ull; // one word ahead of its use
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const AlignStore st = {pos < L ? col + (size_t)pos * stride : nullptr, halves, (int)pos - (int)a.k};
                align_column<T, W, BAND>(pv, mv, score, p, (uint32_t)(cur >> (8 * t)) & 0xffu, mask, lw, hb, words, st);
                ++pos;
                if (pos == L) dist = score; // D[m][L]
            }
        }
        if (ok && dist <= a.k) {
            const uint32_t slot_words = 2u * a.k + 1u;
            nruns = align_traceback<T, W, BAND>(col, halves, a.k, m, L, dist, a.slots + j * slot_words, slot_words);
            if (nruns == ALIGN_BAD_WALK) a.status[1] = 1, nruns = 0;
        } else {
            dist = ALIGN_NONE;
        }
    }
    if (!listed) return;
    if (a.dist) a.dist[e] = (uint8_t)dist;
    a.nruns[j] = nruns;
}

// Behind the scan of the launch's nruns into op_off[e0 .. e1) (which starts at the total of the launches before it):
// entry e's runs from its slot's tail to ops, if its segment ends at or below `capacity`; the last lane writes the running
// total to op_off[e1] and to *total, where the next launch's scan starts.
__global__ __launch_bounds__(ALIGN_BLOCK) void align_fill_kernel(uint64_t e0, uint64_t e1, uint32_t k, const uint32_t *nruns,
                                                                 const uint32_t *slots, uint64_t *op_off, uint32_t *ops,
                                                                 uint64_t capacity, uint64_t *total)
{
    const uint64_t j = (uint64_t)blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    const uint64_t e = e0 + j;
    if (e >= e1) return;
    const uint32_t n = nruns[j], slot_words = 2u * k + 1u;
    const uint64_t off = op_off[e];
    if (e + 1 == e1) op_off[e1] = off + n, *total = off + n;
    if (n > slot_words || off + n > capacity) return;
    const uint32_t *src = slots + j * slot_words + (slot_words - n);
    for (uint32_t r = 0; r < n; ++r) ops[off + r] = src[r];
}

#endif // BMX_ALIGN_PIECES_ONLY

} // namespace bmx
