// bmx_spans_kernel.h -- match spans for the approximate search (bmx_approx_spans_device): a post-pass over a
// device-resident list of ends that finds the START of every match and, on request, keeps one entry per occurrence.
//
// Definitions.  The view is text[0..n), the pattern has m positions, 0 <= k < m, and the list is
// ends[i] = base_offset + j_i with dist[i] = d(j_i) = min over s of ED(pat, text[s..j_i]) <= k, as the search returns it.
//   start(j)  the LARGEST s with ED(pat, text[s..j]) == d(j): the shortest span that attains the minimum.  Its length
//             L = j - s + 1 lies in [m - d, m + d], so no byte before j - (m + k) + 1 is needed.
//   BEST      entry i is kept iff dist[i] <= dprev and dist[i] < dnext, where dprev = dist[i-1] if ends[i-1] == ends[i] - 1
//             (else k + 1) and dnext = dist[i+1] if ends[i+1] == ends[i] + 1 (else k + 1): the last end of every local
//             minimum of the distance along a run of adjacent ends.  Adjacent ends differ by at most 1 in distance, so a
//             rising plateau (1,2,2,3) also keeps its last 2: the price of a rule that looks at two neighbours only.
// Worked example: text xxabcdxxabxdxxacdxx, pattern abcd, k = 1.  The search returns ends [4,5,6,11,16], dist [1,0,1,1,1].
//   flags 0           (2,4,1) (2,5,0) (2,6,1) (8,11,1) (14,16,1)      as (start, end, dist)
//   BMX_SPANS_BEST    (2,5,0) (8,11,1) (14,16,1)
//
// Selection: three launches, no waiting between workgroups.  spans_select_kernel<false> counts the kept entries of every
// tile of SPANS_TILE list entries, spans_scan_kernel (one workgroup) turns the counts into exclusive prefixes and the
// total, spans_select_kernel<true> evaluates the rule again and writes the kept entries in list order at prefix + rank
// (ballot ranks: no atomics decide an order).  The rule reads the two list neighbours straight from memory, so a tile's
// first and last entry look across the tile boundary like any other.
//
// Starts: one list entry per lane, in list order (lanes of one run of ends read the same lines; the caches are the reuse).
// The lane runs Myers' GLOBAL recurrence (bmx_ed_batch_kernel.h) of the REVERSED pattern against text[j], text[j-1], ...:
// after L bytes the score is ED(pat, text[j-L+1..j]).  It tracks the minimum and the first L that attains it over
// L = 1..min(j + 1, m + k).  Every lane takes the same ceil((m + k) / 8) chunks of 8 steps, steps past a lane's own bound
// only stop counting, so waves stay converged.  A pattern of more than 64 positions (bmx_approx_long_spans_device) takes
// spans_starts_long_kernel: the same lane with a column of W words (bmx_myers_words.h), the reversed pattern a kernel
// argument.  Text comes as aligned 8-byte words, downwards in address, one word
// ahead; a word below text[0]'s 16-byte line is never loaded.  An entry whose end is outside the view reads no byte.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmx_myers_words.h"

namespace bmx {

constexpr int SPANS_BLOCK = 256;                        // lanes per workgroup, all three kernels but the scan
constexpr int SPANS_ITEMS = 8;                          // list entries per lane of the selection
constexpr int SPANS_TILE = SPANS_BLOCK * SPANS_ITEMS;   // list entries per selection workgroup
constexpr int SPANS_SCAN_BLOCK = 1024;
constexpr uint64_t SPANS_BAD_END = 1, SPANS_BAD_MIN = 2, SPANS_BAD_DIST = 4; // status bits (ws[0])

struct SpansSelectArgs {
    const uint64_t *ends;
    const uint8_t *dist;
    uint64_t count;
    uint32_t k;
    uint64_t *tiles;    // per tile: kept entries (count pass), their exclusive prefix (fill pass)
    uint64_t *sel_ends; // fill pass only
    uint8_t *sel_dist;
};

struct SpansArgs {
    const uint8_t *text16; // the 16-byte line that holds text[0]
    uint64_t first;        // text[0] is text16[first]
    uint64_t n, base;
    const uint64_t *ends;
    const uint8_t *dist;   // nullptr: the computed minimum is only checked against k
    uint64_t count;
    uint64_t *starts;
    uint64_t *ws;          // [0]: status bits
    uint32_t m, k, chunks; // chunks = ceil((m + k) / 8)
    uint64_t peq[256];     // bit i set: byte belongs to pattern position m - 1 - i (low word used when m <= 32)
};

__device__ __forceinline__ bool spans_keep(const SpansSelectArgs &a, uint64_t i)
{
    const uint64_t e = a.ends[i];
    const uint32_t d = a.dist[i];
    uint32_t dprev = a.k + 1, dnext = a.k + 1;
    if (i > 0 && a.ends[i - 1] + 1 == e) dprev = a.dist[i - 1];
    if (i + 1 < a.count && a.ends[i + 1] == e + 1) dnext = a.dist[i + 1];
    return d <= dprev && d < dnext;
}

template <bool FILL>
__global__ __launch_bounds__(SPANS_BLOCK) void spans_select_kernel(const SpansSelectArgs a)
{
    __shared__ uint32_t wave_n[SPANS_BLOCK / 64];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t tile0 = (uint64_t)blockIdx.x * SPANS_TILE;
    uint64_t base = FILL ? a.tiles[blockIdx.x] : 0;
    uint32_t mine = 0; // count pass: kept entries of this wave
    for (int r = 0; r < SPANS_ITEMS; ++r) {
        const uint64_t row = tile0 + (uint64_t)r * SPANS_BLOCK;
        if (row >= a.count) break; // (uniform)
        const uint64_t i = row + tid;
        const bool keep = i < a.count && spans_keep(a, i);
        const uint64_t vote = __ballot(keep);
        if (!FILL) {
            mine += (uint32_t)__popcll(vote);
            continue;
        }
        if (lane == 0) wave_n[wave] = (uint32_t)__popcll(vote);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < SPANS_BLOCK / 64; ++w) {
            before += w < wave ? wave_n[w] : 0u;
            all += wave_n[w];
        }
        if (keep) {
            const uint64_t at = base + before + (uint32_t)__popcll(vote & ((1ull << lane) - 1));
            a.sel_ends[at] = a.ends[i];
            a.sel_dist[at] = a.dist[i];
        }
        base += all;
        __syncthreads(); // wave_n is written again in the next row
    }
    if (!FILL) {
        if (lane == 0) wave_n[wave] = mine;
        __syncthreads();
        if (tid == 0) {
            uint64_t all = 0;
            for (uint32_t w = 0; w < SPANS_BLOCK / 64; ++w) all += wave_n[w];
            a.tiles[blockIdx.x] = all;
        }
    }
}

// One workgroup: tiles[t] <- sum of tiles[0..t), *total <- the sum of all.  A tile holds at most SPANS_TILE entries, so
// 32 bits carry a row of SPANS_SCAN_BLOCK tiles; the running total is 64-bit.
__global__ __launch_bounds__(SPANS_SCAN_BLOCK) void spans_scan_kernel(uint64_t *tiles, uint64_t n_tiles, uint64_t *total)
{
    __shared__ uint32_t wave_n[SPANS_SCAN_BLOCK / 64];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint64_t carry = 0;
    for (uint64_t row = 0; row < n_tiles; row += SPANS_SCAN_BLOCK) {
        const uint64_t t = row + tid;
        const uint32_t v = t < n_tiles ? (uint32_t)tiles[t] : 0u;
        uint32_t x = v; // inclusive scan within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= (uint32_t)d) x += y;
        }
        if (lane == 63) wave_n[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < SPANS_SCAN_BLOCK / 64; ++w) {
            before += w < wave ? wave_n[w] : 0u;
            all += wave_n[w];
        }
        if (t < n_tiles) tiles[t] = carry + before + (x - v);
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

template <typename W>
struct SpansState {
    W pv, mv;
    uint32_t score;
};

// Myers' column step, global form: a 1 enters bit 0 of the shifted Ph (row 0 is not free), score read at bit hb = m - 1.
template <typename W>
__device__ __forceinline__ void spans_step(SpansState<W> &s, W eq, uint32_t hb)
{
    const W xv = eq | s.mv;
    const W xh = (((eq & s.pv) + s.pv) ^ s.pv) | eq;
    W ph = s.mv | ~(xh | s.pv);
    W mh = s.pv & xh;
    s.score += (uint32_t)((ph >> hb) & 1) - (uint32_t)((mh >> hb) & 1);
    ph = (ph << 1) | 1;
    mh <<= 1;
    s.pv = mh | ~(xv | ph);
    s.mv = ph & xv;
}

template <typename W>
__global__ __launch_bounds__(SPANS_BLOCK) void spans_starts_kernel(const SpansArgs a)
{
    __shared__ W peq[256];
    const uint32_t tid = threadIdx.x;
    peq[tid] = (W)a.peq[tid]; // SPANS_BLOCK == 256
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * SPANS_BLOCK + tid;
    if (i >= a.count) return;

    const uint64_t e = a.ends[i];
    const uint64_t j = e - a.base;
    const bool valid = e >= a.base && j < a.n;
    uint32_t steps = 0, b = 0;
    int64_t wi = -1; // index of the 8-byte word that holds text[j], counted from text16
    if (valid) {
        steps = (uint32_t)min(j + 1, (uint64_t)(a.m + a.k)); // the window is clipped at text[0]
        const uint64_t q = a.first + j;
        wi = (int64_t)(q >> 3);
        b = (uint32_t)(q & 7);
    } else {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)SPANS_BAD_END); // no byte is read for this entry
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t hi = valid ? words[wi] : 0;                // text[j] is byte b of hi
    uint64_t lo = valid && wi > 0 ? words[wi - 1] : 0;  // word 0 lies in text[0]'s line: nothing below it is loaded

    const uint32_t hb = a.m - 1;
    SpansState<W> s;
    s.pv = ~(W)0;
    s.mv = 0;
    s.score = a.m;
    uint32_t best = 0xFFFFFFFFu, best_len = 0, len = 0;
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
            spans_step<W>(s, eq[t], hb);
            ++len;
            if (len <= steps && s.score < best) { // the first (smallest) length that attains the minimum
                best = s.score;
                best_len = len;
            }
        }
    }
    if (!valid) return;
    if (best > a.k)
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)SPANS_BAD_MIN);
    else if (a.dist && a.dist[i] != best)
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)SPANS_BAD_DIST);
    a.starts[i] = e - (best_len - 1);
}

// The same for a pattern of 65 to 512 positions: a column of W words whose table the workgroup builds from `rev`, the
// REVERSED pattern (a.peq is not used).  The global form: 1 enters word 0.
template <int W>
__global__ __launch_bounds__(SPANS_BLOCK) void spans_starts_long_kernel(const SpansArgs a, const LongPattern rev)
{
    __shared__ words_u64x2 tab[256 * W / 2];
    const uint32_t tid = threadIdx.x;
    words_fill<W>(tab, rev, a.m, tid); // SPANS_BLOCK == 256
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * SPANS_BLOCK + tid;
    if (i >= a.count) return;

    const uint64_t e = a.ends[i];
    const uint64_t j = e - a.base;
    const bool valid = e >= a.base && j < a.n;
    uint32_t steps = 0, b = 0;
    int64_t wi = -1; // index of the 8-byte word that holds text[j], counted from text16
    if (valid) {
        steps = (uint32_t)min(j + 1, (uint64_t)(a.m + a.k)); // the window is clipped at text[0]
        const uint64_t q = a.first + j;
        wi = (int64_t)(q >> 3);
        b = (uint32_t)(q & 7);
    } else {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)SPANS_BAD_END); // no byte is read for this entry
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t hi = valid ? words[wi] : 0;                // text[j] is byte b of hi
    uint64_t lo = valid && wi > 0 ? words[wi - 1] : 0;  // word 0 lies in text[0]'s line: nothing below it is loaded

    const uint32_t lw = (a.m - 1) >> 6, hb = (a.m - 1) & 63, n_words = lw + 1;
    WordsColumn<W> s;
    words_init<W>(s, a.m);
    uint32_t best = 0xFFFFFFFFu, best_len = 0, len = 0;
    for (uint32_t c = 0; c < a.chunks; ++c) {
        // the next 8 bytes downwards from text[j - 8c], the first of them in the top byte
        const uint64_t cur = (hi << (8 * (7 - b))) | ((lo >> (8 * b)) >> 8);
        hi = lo;
        --wi;
        lo = valid && wi > 0 ? words[wi - 1] : 0; // one word ahead of its use
        for (int t = 0; t < 8; ++t) {
            const uint32_t byte = (uint32_t)(cur >> (8 * (7 - t))) & 0xFFu;
            words_column<W>(s, tab + (size_t)byte * (W / 2), 1, lw, hb, n_words);
            ++len;
            if (len <= steps && s.score < best) { // the first (smallest) length that attains the minimum
                best = s.score;
                best_len = len;
            }
        }
    }
    if (!valid) return;
    if (best > a.k)
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)SPANS_BAD_MIN);
    else if (a.dist && a.dist[i] != best)
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)SPANS_BAD_DIST);
    a.starts[i] = e - (best_len - 1);
}

} // namespace bmx
