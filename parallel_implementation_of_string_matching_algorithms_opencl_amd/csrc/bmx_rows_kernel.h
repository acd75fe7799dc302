// bmx_rows_kernel.h -- row-wise results (bmx_rows_*, include/bmx.h): the offsets of the rows of a text
// split at a delimiter byte, the row of every match of a list, and the distinct rows of a list of row ids (or the rows
// that are not in it).  No counterpart in the reference.
//
// Split.  A workgroup of ROWS_BLOCK lanes takes tiles of ROWS_TILE bytes (256 KiB) from an atomic ticket, in ascending
// order (bmx_ordered_out.h).  Wave w of the tile owns ROWS_WAVE_BYTES contiguous bytes and goes through them in
// ROWS_BATCHES batches of eight rounds of 1 KiB: lane l loads the 16-byte line at round * 1024 + 16 l, so a wave's load is
// one contiguous KiB, and a batch's eight loads are issued before the first is used.  A line is compared as four 32-bit
// words against the splatted delimiter (exact zero-byte test), which leaves 16 hit bits; the byte in front of the text's
// end counts as a hit whatever it is (the unterminated tail ends there), bytes outside the text never do.  The hit counts
// of two rounds share one 32-bit word through the wave's inclusive scan; a batch parks its hit bits and scans in LDS (a
// lane reads back only its own words).  The workgroup's total goes through the decoupled look-back (here by a whole wave,
// 64 predecessors to a step), after which every lane knows the final slot of each of its hits and stores base_offset +
// position + 1 there: no staging of positions, no second walk.  The tile is this large because the ticket and the look-back
// cost about 10 ns per tile whatever its size (measured: 16, 32, 64 KiB tiles take 1.02, 0.64, 0.53 ms for 1 GiB).
// Only 16-byte lines that hold a byte of the text are loaded (a lane whose line lies behind the end loads its tile's first).
//
// Row of a match.  ub(e) = the number of offsets <= e is monotone in e, so a wave first finds ub of its smallest and of
// its largest end over all rows + 1 offsets (the 64 lanes probe 64 places to a step) and each lane then searches between
// the two.  Lists in any order give the same answers; ascending ones leave a handful of rows per wave.
//
// Matching rows.  head[i]: entry i is the first of its row: id + 1 exceeds the largest id + 1 in front of it (NONE counts
// as 0).  Three passes over tiles of one entry per lane: every tile's summary, one workgroup that turns the summaries into
// carries, and the fill, which gives every head its output slot and the number of entries with a row in front of it; the
// differences of those are the counts.  The inverted list is filled one output per lane: the j-th absent row is j + k for the
// smallest k with hit[k] - k > j.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmx_ordered_out.h"

namespace bmx {

constexpr int ROWS_BLOCK = 512;                                // lanes per workgroup
constexpr int ROWS_ROUNDS = 8;                                 // 16-byte lines per lane and batch
constexpr uint32_t ROWS_BATCH_BYTES = 64 * 16 * ROWS_ROUNDS;   // 8 KiB: what a wave loads at once
constexpr int ROWS_BATCHES = 4;                                // batches of a wave per tile
constexpr uint32_t ROWS_WAVE_BYTES = ROWS_BATCHES * ROWS_BATCH_BYTES; // 32 KiB: a wave's contiguous piece of the tile
constexpr uint32_t ROWS_TILE = (ROWS_BLOCK / 64) * ROWS_WAVE_BYTES;   // 256 KiB
constexpr uint64_t ROWS_NONE = ~0ull;                          // == BMX_ROW_NONE
constexpr int ROWS_WORDS = 4;                                  // status words of a call: [0] bad list, [1] longest row, [2] distinct rows of the list

struct RowsSplitArgs {
    const uint8_t *text16; // caller's pointer rounded down to a multiple of 16
    uint64_t own_lo;       // aligned coordinate of text byte 0 (0..15)
    uint64_t own_hi;       // one past the last byte (n + own_lo), n >= 1
    uint64_t out_bias;     // offset = aligned position + out_bias (base_offset - own_lo + 1)
    uint64_t *off;         // off[0] = base_offset, off[1 + i] = offset behind hit i (NULL: count only)
    uint64_t cap;          // entries off has room for
    uint64_t base_offset;
    uint32_t splat;        // the delimiter in every byte
    // ordered output (bmx_ordered_out.h)
    uint64_t *status;
    unsigned long long *ticket;
    uint64_t ticket_base;
    uint64_t *host_status;
    uint64_t seq, tag;
    uint64_t n_tiles;
};

typedef uint32_t rows_u32x4 __attribute__((ext_vector_type(4)));

// bit i: byte i of the word equals the splatted byte (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t rows_eq4(uint32_t w, uint32_t splat)
{
    const uint32_t y = w ^ splat;
    const uint32_t t = ~((((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) | 0x7f7f7f7fu); // 0x80 in every zero byte of y
    return (((t >> 7) * 0x01020408u) >> 24) & 0xfu;
}

// sum over the wave's 64 lanes (the same in every lane)
__device__ __forceinline__ uint64_t rows_wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
    return v;
}

// The look-back of bmx_ordered_out.h (the same status words, tags and give-up rule) by a whole wave: lane l reads the word
// of tile top - 1 - l, so one step covers 64 predecessors.  A step ends the walk when the words down to the first inclusive
// prefix are all published; with all 64 published and no prefix among them it moves on; otherwise it reads again.  Tiles
// below 0 count as an empty prefix.  Called by every lane of one wave; returns the exclusive prefix of tile t in all of them.
__device__ __forceinline__ uint64_t rows_lookback_wave(const RowsSplitArgs &a, uint64_t t, uint64_t agg, uint32_t lane)
{
    const uint64_t tagbits = a.tag << ORDERED_TAG_SHIFT;
    if (t == 0) {
        if (lane == 0) ordered_store_status(&a.status[0], tagbits | (ORDERED_KIND_PREFIX << 40) | agg);
        return 0;
    }
    if (lane == 0) ordered_store_status(&a.status[t], tagbits | (ORDERED_KIND_AGG << 40) | agg);
    uint64_t prefix = 0, top = t; // tiles below `top` are still to be summed
    uint32_t spins = 0;
    for (;;) {
        uint64_t value = 0;
        bool ready = true, inclusive = true;
        if (lane < top) {
            const uint64_t w = ordered_load_status(&a.status[top - 1 - lane]);
            const uint64_t kind = (w >> 40) & 3u;
            ready = (w >> ORDERED_TAG_SHIFT) == a.tag && kind != 0;
            inclusive = ready && kind == ORDERED_KIND_PREFIX;
            value = w & ORDERED_VALUE_MASK;
        }
        const uint64_t waiting = __ballot(!ready), found = __ballot(inclusive);
        const uint32_t g = waiting ? (uint32_t)__builtin_ctzll(waiting) : 64u, f = found ? (uint32_t)__builtin_ctzll(found) : 64u;
        if (f < g) { // every word down to the first inclusive prefix is there
            prefix += rows_wave_sum(lane <= f ? value : 0);
            break;
        }
        if (g == 64) { // 64 aggregates (top >= 64: a lane below tile 0 would have been a prefix)
            prefix += rows_wave_sum(value);
            top -= 64;
            continue;
        }
        if (++spins > (1u << 22)) {
            if (lane == 0) __hip_atomic_store(&a.host_status[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    if (lane == 0) ordered_store_status(&a.status[t], tagbits | (ORDERED_KIND_PREFIX << 40) | ((prefix + agg) & ORDERED_VALUE_MASK));
    return prefix;
}

__global__ __launch_bounds__(ROWS_BLOCK, 4) void rows_split_kernel(const RowsSplitArgs a)
{
    constexpr int BATCHES = ROWS_BATCHES;
    constexpr uint32_t BATCH_BYTES = ROWS_BATCH_BYTES, PIECE = ROWS_WAVE_BYTES, TILE = ROWS_TILE;
    // per batch and lane: the hit bits of its eight rounds, two to a word, then the inclusive scan over the lanes of their
    // counts, two to a word (a lane reads only what it wrote: no barrier)
    __shared__ uint32_t sh_state[BATCHES][ROWS_ROUNDS][ROWS_BLOCK];
    __shared__ uint32_t sh_wave[ROWS_BLOCK / 64];
    __shared__ uint64_t sh_tile, sh_prefix;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t rel0 = lane * 16u;
    for (;;) {
        if (tid == 0) sh_tile = atomicAdd(a.ticket, 1ull) - a.ticket_base; // tiles in ascending order: every predecessor is owned
        __syncthreads();
        const uint64_t t = sh_tile;
        if (t >= a.n_tiles) break;
        const uint64_t wave0 = t * TILE + (uint64_t)wave * PIECE; // aligned coordinate of the wave's first byte
        const rows_u32x4 *tile_src = reinterpret_cast<const rows_u32x4 *>(a.text16) + t * (TILE / 16);
        uint32_t wave_total = 0;
#pragma unroll 1
        for (int b = 0; b < BATCHES; ++b) { // (not unrolled: one batch's loads in flight, its results parked in LDS)
            const uint64_t batch0 = wave0 + (uint32_t)b * BATCH_BYTES;
            const rows_u32x4 *src = tile_src + wave * (PIECE / 16) + b * (BATCH_BYTES / 16) + lane;
            // relative to batch0: lim = bytes from there to the text's end (0: the batch has none)
            const uint32_t lim = batch0 >= a.own_hi ? 0u : (uint32_t)min(a.own_hi - batch0, (uint64_t)BATCH_BYTES);
            rows_u32x4 v[ROWS_ROUNDS];
#pragma unroll
            for (int r = 0; r < ROWS_ROUNDS; ++r) { // no branch: a line behind the text's end is replaced by the tile's first
                const uint32_t rel = rel0 + (uint32_t)r * 1024u; // line, which holds a byte of the text (own_lo < 16)
                v[r] = *(rel < lim ? src + r * 64 : tile_src);
            }
            const bool ends_here = batch0 + lim == a.own_hi; // (lim > 0: the text's last byte lies in this batch)
            uint32_t mask[ROWS_ROUNDS];
#pragma unroll
            for (int r = 0; r < ROWS_ROUNDS; ++r) {
                const uint32_t rel = rel0 + (uint32_t)r * 1024u;
                uint32_t h = 0;
                if (rel < lim) {
                    h = rows_eq4(v[r][0], a.splat) | (rows_eq4(v[r][1], a.splat) << 4) | (rows_eq4(v[r][2], a.splat) << 8) |
                        (rows_eq4(v[r][3], a.splat) << 12);
                    const uint32_t left = lim - rel; // bytes of the batch from this line on (>= 1)
                    if (left <= 16) {
                        if (ends_here) h |= 1u << (left - 1); // the text's last byte ends a row whatever it is
                        h &= (1u << left) - 1u;
                    }
                    if (b == 0 && r == 0 && rel == 0 && wave0 == 0) h &= ~((1u << a.own_lo) - 1u); // in front of an unaligned text
                }
                mask[r] = h;
            }
#pragma unroll
            for (int q = 0; q < ROWS_ROUNDS / 2; ++q) { // (a wave's round has at most 1024 hits)
                sh_state[b][q][tid] = mask[2 * q] | (mask[2 * q + 1] << 16);
                uint32_t x = (uint32_t)__builtin_popcount(mask[2 * q]) | ((uint32_t)__builtin_popcount(mask[2 * q + 1]) << 16);
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o = __shfl_up(x, d);
                    if ((int)lane >= d) x += o;
                }
                sh_state[b][ROWS_ROUNDS / 2 + q][tid] = x;
                const uint32_t both = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
                wave_total += (both & 0xffffu) + (both >> 16);
            }
        }
        if (lane == 0) sh_wave[wave] = wave_total;
        __syncthreads();
        if (wave == 0) {
            uint64_t agg = 0;
            for (int w = 0; w < ROWS_BLOCK / 64; ++w) agg += sh_wave[w];
            const uint64_t prefix = rows_lookback_wave(a, t, agg, lane);
            if (lane == 0) {
                ordered_publish_total(a, t, prefix + agg);
                sh_prefix = prefix;
                if (t == 0 && a.off != nullptr && a.cap > 0) a.off[0] = a.base_offset;
            }
        }
        __syncthreads();
        uint64_t slot0 = sh_prefix + 1; // off[0] is the first row's start
        for (uint32_t w = 0; w < wave; ++w) slot0 += sh_wave[w];
        if (a.off != nullptr && slot0 < a.cap) {
            uint32_t run = 0; // hits of the wave in front of the round, in (batch, round, lane) order
#pragma unroll 1
            for (int b = 0; b < BATCHES; ++b) {
#pragma unroll
                for (int r = 0; r < ROWS_ROUNDS; ++r) {
                    const uint32_t sh = 16 * (r & 1);
                    const uint32_t incl = sh_state[b][ROWS_ROUNDS / 2 + (r >> 1)][tid];
                    const uint32_t h0 = (sh_state[b][r >> 1][tid] >> sh) & 0xffffu;
                    const uint32_t mine = (incl >> sh) & 0xffffu;
                    const uint32_t total = ((uint32_t)__builtin_amdgcn_readlane((int)incl, 63) >> sh) & 0xffffu;
                    uint64_t idx = slot0 + run + mine - (uint32_t)__builtin_popcount(h0);
                    const uint64_t p = wave0 + a.out_bias + ((uint32_t)b * BATCH_BYTES + rel0 + (uint32_t)r * 1024u);
                    for (uint32_t h = h0; h != 0; h &= h - 1u, ++idx)
                        if (idx < a.cap) a.off[idx] = p + (uint32_t)__builtin_ctz(h);
                    run += total;
                }
            }
        }
        __syncthreads(); // sh_wave, sh_tile and sh_prefix are the next tile's
    }
}

// The longest row of the offsets the split stored: max of off[i + 1] - off[i] over i < min(rows, cap - 1), where rows is
// the total the split's last tile left in pinned memory (read once per workgroup).  words[1] starts at 0.
__global__ __launch_bounds__(ROWS_BLOCK) void rows_longest_kernel(const uint64_t *off, uint64_t cap, const uint64_t *host_status,
                                                                 unsigned long long *words)
{
    __shared__ uint64_t sh_rows;
    __shared__ uint64_t sh_max[ROWS_BLOCK / 64];
    if (threadIdx.x == 0) sh_rows = __hip_atomic_load(&host_status[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    const uint64_t items = min(sh_rows, cap - 1);
    uint64_t best = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * ROWS_BLOCK + threadIdx.x; i < items; i += (uint64_t)gridDim.x * ROWS_BLOCK)
        best = max(best, off[i + 1] - off[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best = max(best, (uint64_t)__shfl_xor((unsigned long long)best, d));
    if ((threadIdx.x & 63u) == 0) sh_max[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < ROWS_BLOCK / 64; ++w) best = max(best, sh_max[w]);
        if (best) atomicMax(&words[1], (unsigned long long)best);
    }
}

// ---- the row of every match ----

// the number of off[lo..hi) entries ... precisely: the smallest index i in [lo, hi] with off[i] > e, or hi (off[hi] is
// never read).  With lo = 0 and hi = rows + 1 this is ub(e), the number of offsets <= e.
// Eight probes to a step, all loaded before the first is compared: a range of 128 rows takes three dependent steps where
// the binary search takes seven.
__device__ __forceinline__ uint64_t rows_upper(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t e)
{
    while (hi - lo > 8) {
        const uint64_t step = (hi - lo + 7) / 8; // >= 2
        uint64_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = off[min(lo + (uint64_t)(j + 1) * step - 1, hi - 1)];
        uint32_t f = 8;
#pragma unroll
        for (int j = 7; j >= 0; --j)
            if (lo + (uint64_t)(j + 1) * step - 1 >= hi || v[j] > e) f = (uint32_t)j; // (a probe at or past hi counts as greater)
        const uint64_t new_hi = f == 8 ? hi : min(lo + (uint64_t)(f + 1) * step - 1, hi);
        lo = f == 0 ? lo : lo + (uint64_t)f * step;
        hi = new_hi;
    }
    uint64_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = lo + j < hi ? off[lo + j] : ~0ull;
    uint64_t r = hi;
#pragma unroll
    for (int j = 7; j >= 0; --j)
        if (lo + j < hi && v[j] > e) r = lo + j;
    return r;
}

// The same answer for an e that all 64 lanes share, 64 probes to a step: lane l reads off[lo + (l + 1) step - 1], the
// ballot of "greater than e" (a probe at or past hi counts as greater) leaves one of 64 pieces.  Every lane of the wave
// calls it; four steps go through 2^23 rows where the lane's own search takes 23 dependent loads.
__device__ __forceinline__ uint64_t rows_upper_wave(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t e, uint32_t lane)
{
    while (hi - lo > 64) {
        const uint64_t step = (hi - lo + 63) / 64; // >= 2
        const uint64_t q = lo + (uint64_t)(lane + 1) * step - 1;
        const uint64_t greater = __ballot(q >= hi || off[q] > e);
        const uint32_t f = greater ? (uint32_t)__builtin_ctzll(greater) : 64u; // (lane 63 probes hi - 1 or past it)
        const uint64_t new_hi = f == 64 ? hi : min(lo + (uint64_t)(f + 1) * step - 1, hi);
        lo = f == 0 ? lo : lo + (uint64_t)f * step;
        hi = new_hi;
    }
    const uint64_t q = lo + lane;
    const uint64_t greater = __ballot(q < hi && off[q] > e);
    return greater ? lo + (uint32_t)__builtin_ctzll(greater) : hi;
}

__global__ __launch_bounds__(ROWS_BLOCK) void rows_of_kernel(const uint64_t *off, uint64_t rows, const uint64_t *starts,
                                                            const uint64_t *ends, uint64_t len, uint64_t count, uint64_t *row)
{
    const uint64_t i = (uint64_t)blockIdx.x * ROWS_BLOCK + threadIdx.x;
    uint64_t s = ROWS_NONE, e = 0;
    bool ok = false;
    if (i < count) {
        if (starts != nullptr && ends != nullptr) {
            s = starts[i], e = ends[i];
            ok = s != ROWS_NONE && e >= s;
        } else if (starts != nullptr) {
            s = starts[i], e = s + (len - 1);
            ok = s != ROWS_NONE && e >= s;
        } else {
            e = ends[i], s = e - (len - 1);
            ok = e >= len - 1 && s != ROWS_NONE;
        }
    }
    // the wave's smallest and largest end bound every lane's search
    uint64_t mn = ok ? e : ROWS_NONE, mx = ok ? e : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mn = min(mn, (uint64_t)__shfl_xor((unsigned long long)mn, d));
        mx = max(mx, (uint64_t)__shfl_xor((unsigned long long)mx, d));
    }
    if (mn > mx) { // no lane of the wave has a match
        if (i < count) row[i] = ROWS_NONE;
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t ub_lo = rows_upper_wave(off, 0, rows + 1, mn, lane);
    uint64_t ub_hi = ub_lo;
    if (mn != mx) { // ascending lists: the largest end lies a few rows on, so try 4096 rows before all of them
        const uint64_t near = min(ub_lo + 4096, rows + 1);
        const bool within = near == rows + 1 || off[near - 1] > mx; // (near - 1 <= rows; the same load in every lane)
        ub_hi = rows_upper_wave(off, ub_lo, within ? near : rows + 1, mx, lane);
    }
    if (i >= count) return;
    uint64_t r = ROWS_NONE;
    if (ok) {
        const uint64_t ub = rows_upper(off, ub_lo, ub_hi, e);
        if (ub >= 1 && ub <= rows && s >= off[ub - 1]) r = ub - 1; // off[r] <= s and e < off[r + 1]
    }
    row[i] = r;
}

// ---- the distinct rows of a list of row ids ----

struct RowsPair {
    uint64_t heads, valid;
};

// One list entry per lane, ROWS_BLOCK entries per tile.  key = id + 1 (0: NONE, or behind the list).  For the calling lane:
// before = the largest key in front of it (carry: the largest key of all earlier tiles), head = it has a row and is the
// first entry of that row, and the numbers of heads and of entries with a row in front of it inside the tile.  tot[0..3]
// (every lane) = the tile's first key with a row (0: none), its largest key, its heads, its entries with a row.
struct RowsLane {
    uint64_t before;
    bool head;
    uint32_t heads_before, valid_before;
};
__device__ __forceinline__ RowsLane rows_tile_scan(uint64_t key, uint64_t carry, uint64_t tot[4])
{
    __shared__ uint64_t sh_max[ROWS_BLOCK / 64], sh_first[ROWS_BLOCK / 64];
    __shared__ uint32_t sh_heads[ROWS_BLOCK / 64], sh_valid[ROWS_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull; // the lanes in front of this one
    uint64_t incl = key;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)incl, d);
        if ((int)lane >= d) incl = max(incl, o);
    }
    uint64_t excl = (uint64_t)__shfl_up((unsigned long long)incl, 1);
    if (lane == 0) excl = 0;
    const uint64_t vmask = __ballot(key != 0);
    if (lane == 63) sh_max[wave] = incl;
    const uint64_t first_key = vmask ? (uint64_t)__shfl((unsigned long long)key, __builtin_ctzll(vmask)) : 0; // of the wave
    if (lane == 0) {
        sh_valid[wave] = (uint32_t)__builtin_popcountll(vmask);
        sh_first[wave] = first_key;
    }
    __syncthreads();
    RowsLane r;
    r.before = max(excl, carry);
    r.valid_before = (uint32_t)__builtin_popcountll(vmask & below);
    uint64_t first = 0, largest = 0;
    uint32_t valid = 0;
    for (uint32_t w = 0; w < ROWS_BLOCK / 64; ++w) {
        if (w < wave) r.before = max(r.before, sh_max[w]), r.valid_before += sh_valid[w];
        if (first == 0) first = sh_first[w];
        largest = max(largest, sh_max[w]);
        valid += sh_valid[w];
    }
    r.head = key != 0 && key > r.before;
    const uint64_t hmask = __ballot(r.head);
    if (lane == 0) sh_heads[wave] = (uint32_t)__builtin_popcountll(hmask);
    __syncthreads();
    r.heads_before = (uint32_t)__builtin_popcountll(hmask & below);
    uint32_t heads = 0;
    for (uint32_t w = 0; w < ROWS_BLOCK / 64; ++w) {
        if (w < wave) r.heads_before += sh_heads[w];
        heads += sh_heads[w];
    }
    tot[0] = first, tot[1] = largest, tot[2] = heads, tot[3] = valid;
    __syncthreads(); // the arrays are the next call's
    return r;
}

// Pass 1: every tile's summary {first key with a row, largest key, heads as if nothing came before, entries with a row}.
__global__ __launch_bounds__(ROWS_BLOCK) void rows_summary_kernel(const uint64_t *id, uint64_t count, uint64_t *summary)
{
    const uint64_t i = (uint64_t)blockIdx.x * ROWS_BLOCK + threadIdx.x;
    uint64_t tot[4];
    (void)rows_tile_scan(i < count ? id[i] + 1 : 0, 0, tot);
    if (threadIdx.x < 4) summary[4 * (uint64_t)blockIdx.x + threadIdx.x] = tot[threadIdx.x];
}

// Pass 2, one workgroup: the carry of every tile {largest key in front, heads in front, entries with a row in front}.  A
// tile whose first key equals the largest key in front of it has counted one head too many.  total = {heads, entries}
// of the list, first[heads] = the entries (the end of the last row's count).
__global__ __launch_bounds__(ROWS_BLOCK) void rows_carry_kernel(const uint64_t *summary, uint64_t tiles, uint64_t *carry, RowsPair *total,
                                                               uint64_t *first, unsigned long long *words)
{
    __shared__ uint64_t sh_a[ROWS_BLOCK / 64], sh_b[ROWS_BLOCK / 64], sh_c[ROWS_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t run_key = 0, run_heads = 0, run_valid = 0;
    for (uint64_t t0 = 0; t0 < tiles; t0 += ROWS_BLOCK) {
        const uint64_t t = t0 + threadIdx.x;
        const bool in = t < tiles;
        const uint64_t fkey = in ? summary[4 * t] : 0, mkey = in ? summary[4 * t + 1] : 0;
        uint64_t heads = in ? summary[4 * t + 2] : 0, valid = in ? summary[4 * t + 3] : 0;
        // exclusive maximum of the largest keys
        uint64_t incl = mkey;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = (uint64_t)__shfl_up((unsigned long long)incl, d);
            if ((int)lane >= d) incl = max(incl, o);
        }
        uint64_t before = (uint64_t)__shfl_up((unsigned long long)incl, 1);
        if (lane == 0) before = 0;
        if (lane == 63) sh_a[wave] = incl;
        __syncthreads();
        before = max(before, run_key);
        uint64_t chunk_key = run_key;
        for (uint32_t w = 0; w < ROWS_BLOCK / 64; ++w) {
            if (w < wave) before = max(before, sh_a[w]);
            chunk_key = max(chunk_key, sh_a[w]);
        }
        if (fkey != 0 && fkey == before) --heads; // its first row began in an earlier tile
        // exclusive sums of the heads and of the entries with a row
        uint64_t ih = heads, iv = valid;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t oh = (uint64_t)__shfl_up((unsigned long long)ih, d), ov = (uint64_t)__shfl_up((unsigned long long)iv, d);
            if ((int)lane >= d) ih += oh, iv += ov;
        }
        if (lane == 63) sh_b[wave] = ih, sh_c[wave] = iv;
        __syncthreads();
        uint64_t hb = run_heads + ih - heads, vb = run_valid + iv - valid, chunk_heads = run_heads, chunk_valid = run_valid;
        for (uint32_t w = 0; w < ROWS_BLOCK / 64; ++w) {
            if (w < wave) hb += sh_b[w], vb += sh_c[w];
            chunk_heads += sh_b[w], chunk_valid += sh_c[w];
        }
        if (in) carry[3 * t] = before, carry[3 * t + 1] = hb, carry[3 * t + 2] = vb;
        run_key = chunk_key, run_heads = chunk_heads, run_valid = chunk_valid;
        __syncthreads(); // sh_a, sh_b, sh_c are the next chunk's
    }
    if (threadIdx.x == 0) {
        total->heads = run_heads, total->valid = run_valid;
        words[2] = run_heads; // (the host reads it with the status word)
        if (first) first[run_heads] = run_valid;
    }
}

// Pass 3: every head stores its row at its slot (below cap) and the number of entries with a row in front of it in
// first[slot].  An id at or past `rows` (other than NONE) or below an earlier one raises words[0].
__global__ __launch_bounds__(ROWS_BLOCK) void rows_heads_kernel(const uint64_t *id, uint64_t count, uint64_t rows, const uint64_t *carry,
                                                               uint64_t *rows_out, uint64_t *first, uint64_t cap, unsigned long long *words)
{
    const uint64_t i = (uint64_t)blockIdx.x * ROWS_BLOCK + threadIdx.x;
    const uint64_t key = i < count ? id[i] + 1 : 0;
    const uint64_t *c = carry + 3 * (uint64_t)blockIdx.x;
    uint64_t tot[4];
    const RowsLane r = rows_tile_scan(key, c[0], tot);
    if (key == 0) return;
    if (key > rows || key < r.before) words[0] = 1;
    if (!r.head) return;
    const uint64_t slot = c[1] + r.heads_before;
    if (first) first[slot] = c[2] + r.valid_before;
    if (rows_out && slot < cap) rows_out[slot] = key - 1;
}

__global__ __launch_bounds__(ROWS_BLOCK) void rows_counts_kernel(const uint64_t *first, const RowsPair *total, uint64_t *counts,
                                                                uint64_t cap)
{
    const uint64_t k = (uint64_t)blockIdx.x * ROWS_BLOCK + threadIdx.x;
    if (k < total->heads && k < cap) counts[k] = first[k + 1] - first[k];
}

// The rows of [0, rows) that are not among the `total->heads` ascending rows of hit[]: output j is row j + k for the
// smallest k with hit[k] - k > j (hit[k] - k rows are absent in front of hit[k]).
__global__ __launch_bounds__(ROWS_BLOCK) void rows_absent_kernel(const uint64_t *hit, const RowsPair *total, uint64_t rows,
                                                                uint64_t *rows_out, uint64_t cap)
{
    const uint64_t j = (uint64_t)blockIdx.x * ROWS_BLOCK + threadIdx.x;
    const uint64_t nh = total->heads;
    if (j >= rows - nh || j >= cap) return;
    uint64_t lo = 0, hi = nh;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (hit[mid] - mid > j) hi = mid;
        else lo = mid + 1;
    }
    rows_out[j] = j + lo;
}

} // namespace bmx
