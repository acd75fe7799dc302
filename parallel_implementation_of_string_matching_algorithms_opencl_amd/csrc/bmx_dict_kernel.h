// bmx_dict_kernel.h -- dictionary search (bmx_dict_search_device): every pair (p, i) with text[p .. p + m_i) == pattern
// i, ordered by p, then by i, in one pass over the text.
//
// Filter.  Each pattern is keyed on its first min(m, 4) bytes; a length class (1, 2, 3, 4+) has a bitmap in LDS: class
// 1 and 2 exact (128 bits, 16 Kbit, 7 bits per pattern byte), class 3 and class 4+ a two-hash Bloom filter (32 Kbit,
// 1 Mbit).  Every text position probes the classes the dictionary holds (a scalar branch: the flags are launch-uniform)
// with its first hash only; the rare position that passes is tested on the second hash, then verified.
// Verify.  The exact prefix of each class is looked up in an open-addressing table in HBM (L2-resident): it gives the
// ids of the patterns with that prefix, ascending.  The up-to-four lists are merged by id and each pattern's remaining
// bytes are compared against the text from a packed blob.
//
// Text access.  A workgroup of DICT_BLOCK lanes reads rounds of DICT_ROUND bytes: lane l reads bytes [16l, 16l + 16)
// (one coalesced 16-byte load), tests the 16 starts in them and takes the 3 bytes that follow from lane l + 1 (a
// ds_bpermute); lane 63 of a wave loads that dword itself.  Two rounds are in flight ahead of the one being tested.
//
// Ordered output in one pass, as bmx_approx_kernel.h does it: a workgroup takes tiles of 2^rounds_shift rounds from an
// atomic ticket, parks its tile's pairs as ((p - tile0) << 16 | i) in a pool in LDS, publishes the tile's count and
// finds its exclusive prefix by decoupled look-back over tagged status words (bmx_ordered_out.h).  A pair's slot is the
// prefix plus its rank among the tile's parked keys.  A tile with more pairs than the pool walks itself a second time
// round by round: count, workgroup scan, write.  Slots at or past the capacity are dropped: the stored pairs are the
// lowest ones.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmx_ordered_out.h"

namespace bmx {

constexpr int DICT_BLOCK = 512;               // lanes per workgroup
constexpr int DICT_ROUND = DICT_BLOCK * 16;   // bytes per round
constexpr int DICT_STAGE = 2048;              // pairs parked per tile (16 KiB of LDS)
constexpr int DICT_MAX_ROUNDS_SHIFT = 5;      // tile <= 256 KiB: (p - tile0) < 2^18, id < 2^16
constexpr int DICT_MAX = 65536;               // == BMX_MAX_DICT

// LDS bitmaps, in 32-bit words, one array: class 1 | class 2 | class 3 | class 4+
constexpr uint32_t DICT_BM1_WORDS = 4, DICT_BM2_WORDS = 512, DICT_BM3_WORDS = 1024, DICT_BM4_WORDS = 32768;
constexpr uint32_t DICT_BM1 = 0, DICT_BM2 = DICT_BM1 + DICT_BM1_WORDS, DICT_BM3 = DICT_BM2 + DICT_BM2_WORDS,
                   DICT_BM4 = DICT_BM3 + DICT_BM3_WORDS, DICT_BM_WORDS = DICT_BM4 + DICT_BM4_WORDS;
constexpr uint32_t DICT_HAS1 = 1, DICT_HAS2 = 2, DICT_HAS3 = 4, DICT_HAS4 = 8;

// Exact-prefix table: EMPTY is never a key (a class-4 key has no byte >= 0x80; the others carry 0xff in byte 3).
constexpr uint32_t DICT_EMPTY = 0x80808080u;

// The hashes, shared with the host builder.  The multiplies are 24 x 24 bits (full rate); the word comes from the high
// bits of the product, the bit from the low 5 bits of the folded key.  k: the key bytes, little-endian (class 3: 3 bytes).
__host__ __device__ __forceinline__ uint32_t dict_mul24(uint32_t a, uint32_t b)
{
    return (a & 0xffffffu) * (b & 0xffffffu);
}
__host__ __device__ __forceinline__ uint32_t dict_fold1(uint32_t k) { return k ^ (k >> 14); }
__host__ __device__ __forceinline__ uint32_t dict_fold2(uint32_t k) { return k ^ (k >> 9) ^ (k << 3); }
// class 4+: 2^20 bits (word 15 bits)
__host__ __device__ __forceinline__ uint32_t dict_h4a_word(uint32_t f) { return dict_mul24(f, 0x9E3779u) >> 17; }
__host__ __device__ __forceinline__ uint32_t dict_h4b_word(uint32_t f) { return dict_mul24(f, 0xC2B2AEu | 1u) >> 17; }
// class 3: 2^15 bits (word 10 bits)
__host__ __device__ __forceinline__ uint32_t dict_h3a_word(uint32_t f) { return dict_mul24(f, 0x85EBCAu | 1u) >> 22; }
__host__ __device__ __forceinline__ uint32_t dict_h3b_word(uint32_t f) { return dict_mul24(f, 0x27D4EBu) >> 22; }
// the exact-prefix table's slot
__host__ __device__ __forceinline__ uint32_t dict_slot(uint32_t key)
{
    const uint32_t h = (key ^ (key >> 15)) * 0x2C1B3C6Du;
    return h ^ (h >> 16);
}

struct DictArgs {
    const uint8_t *text16; // caller's pointer rounded down to a multiple of 16
    uint64_t first;        // aligned coordinate of view byte 0 (0..15)
    uint64_t own_hi;       // one past the last start to report (aligned coordinates: min(n_own, n) + first)
    uint64_t vend;         // one past the last view byte (n + first)
    uint64_t out_bias;     // reported p = aligned p + out_bias (base_offset - first)
    uint64_t tile_begin;   // first tile index (aligned first / tile bytes)
    uint64_t n_tiles;
    uint64_t *out;         // positions (NULL: count only)
    uint32_t *pid;         // their pattern ids (NULL: not wanted)
    uint64_t cap;
    uint64_t *status;      // n_tiles tile words (tagged: no clearing between calls)
    unsigned long long *ticket; // monotonic across calls: this call's tickets start at ticket_base
    uint64_t ticket_base;
    uint64_t *host_status; // pinned: [0] total, [1] give-up flag, [2] seq (written by the last tile)
    uint64_t seq;
    uint64_t tag;          // seq mod 2^22 (never 0)
    unsigned long long *cand; // positions that reached the exact lookup (zeroed before the launch)
    const uint32_t *bitmaps;  // DICT_BM_WORDS words, copied to LDS
    const uint4 *table;       // {key, first id index, id count, 0}, table_mask + 1 slots
    const uint32_t *ids;      // pattern ids grouped by prefix, ascending in each group
    const uint2 *pats;        // {blob offset, length} per id
    const uint8_t *blob;
    uint32_t table_mask;
    uint32_t classes;         // DICT_HAS*
    uint32_t rounds_shift;
};

__device__ __forceinline__ uint32_t dict_bit(const uint32_t *bm, uint32_t word, uint32_t bit)
{
    return __builtin_amdgcn_ubfe(bm[word], bit & 31u, 1);
}

// The ids of the patterns of class c whose prefix equals the c key bytes of k: [*s, *e) of a.ids (empty if none).
__device__ __forceinline__ void dict_lookup(const DictArgs &a, uint32_t key, uint32_t &s, uint32_t &e)
{
    uint32_t i = dict_slot(key) & a.table_mask;
    s = e = 0;
    for (uint32_t probes = 0; probes <= a.table_mask; ++probes) {
        const uint4 t = a.table[i];
        if (t.x == key) {
            s = t.y;
            e = t.y + t.z;
            return;
        }
        if (t.x == DICT_EMPTY) return;
        i = (i + 1) & a.table_mask;
    }
}

// Every pattern that occurs at aligned position p (k: the 4 bytes from p, garbage past vend), by ascending id:
// emit(id) for each.  Reads text and blob bytes only inside the view.
template <typename Emit>
__device__ __forceinline__ void dict_at(const DictArgs &a, uint64_t p, uint32_t k, Emit &emit)
{
    const uint64_t avail = a.vend - p;
    uint32_t cs[4], ce[4];
#pragma unroll
    for (int c = 1; c <= 4; ++c) {
        cs[c - 1] = ce[c - 1] = 0;
        if (!(a.classes & (1u << (c - 1))) || avail < (uint64_t)c) continue;
        const uint32_t kc = c == 4 ? k : (k & ((1u << (8 * c)) - 1u));
        if (kc & 0x80808080u) continue; // a text byte >= 0x80 is in no pattern
        const uint32_t key = c == 4 ? kc : (kc | (0xffffffffu << (8 * c)));
        dict_lookup(a, key, cs[c - 1], ce[c - 1]);
    }
    const uint8_t *t = a.text16 + p;
    for (;;) {
        uint32_t best = 0xffffffffu;
        int bc = -1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (cs[c] < ce[c]) {
                const uint32_t id = a.ids[cs[c]];
                if (id < best) best = id, bc = c;
            }
        }
        if (bc < 0) break;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c == bc) ++cs[c];
        const uint2 pl = a.pats[best];
        if ((uint64_t)pl.y > avail) continue;
        const uint8_t *q = a.blob + pl.x;
        uint32_t j = pl.y < 4 ? pl.y : 4u; // the prefix is the key
        while (j < pl.y && t[j] == q[j]) ++j;
        if (j == pl.y) emit(best);
    }
}

// The 4 bytes from aligned position p (0 past the view), read again from memory on the rare paths: indexing the lane's
// words with a start that is not a constant would put them in scratch.
__device__ __forceinline__ uint32_t dict_key(const DictArgs &a, uint64_t p)
{
    uint32_t k = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (p + j < a.vend) k |= (uint32_t)a.text16[p + j] << (8 * j);
    return k;
}

// The 16 starts of one lane's bytes: bit i set when position c + i passes the filters and lies in [lo, hi) (both
// relative to c, clipped to 0..16).  w[0..3]: the lane's bytes, w[4]: the next lane's first 4.
__device__ __forceinline__ uint32_t dict_filter(const DictArgs &a, const uint32_t *bm, const uint32_t w[5], uint64_t c,
                                                uint32_t own)
{
    uint32_t first = 0, cand = 0;
    const uint32_t cls = a.classes;
    if (cls & DICT_HAS4) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t k = __builtin_amdgcn_alignbit(w[(i >> 2) + 1], w[i >> 2], 8 * (i & 3));
            const uint32_t f = dict_fold1(k);
            first |= dict_bit(bm + DICT_BM4, dict_h4a_word(f), f) << i;
        }
    }
    if (cls & DICT_HAS3) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t k = __builtin_amdgcn_alignbit(w[(i >> 2) + 1], w[i >> 2], 8 * (i & 3)) & 0xffffffu;
            const uint32_t f = dict_fold1(k);
            first |= dict_bit(bm + DICT_BM3, dict_h3a_word(f), f) << i;
        }
    }
    first &= own;
    // second hash of classes 3 and 4+ (rare: only where the first passed)
    while (first) {
        const int i = __builtin_ctz(first);
        first &= first - 1;
        const uint32_t k = dict_key(a, c + i);
        uint32_t ok = 0;
        if (cls & DICT_HAS4) {
            const uint32_t f1 = dict_fold1(k), f2 = dict_fold2(k);
            ok |= dict_bit(bm + DICT_BM4, dict_h4a_word(f1), f1) & dict_bit(bm + DICT_BM4, dict_h4b_word(f2), f2);
        }
        if (cls & DICT_HAS3) {
            const uint32_t k3 = k & 0xffffffu;
            const uint32_t f1 = dict_fold1(k3), f2 = dict_fold2(k3);
            ok |= dict_bit(bm + DICT_BM3, dict_h3a_word(f1), f1) & dict_bit(bm + DICT_BM3, dict_h3b_word(f2), f2);
        }
        cand |= ok << i;
    }
    if (cls & DICT_HAS2) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t k = __builtin_amdgcn_alignbit(w[(i >> 2) + 1], w[i >> 2], 8 * (i & 3));
            const uint32_t x = (k & 0x7fu) | ((k >> 1) & 0x3f80u); // b0 | b1 << 7 (high bits dropped: verified later)
            cand |= dict_bit(bm + DICT_BM2, x >> 5, x) << i;
        }
    }
    if (cls & DICT_HAS1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0x7fu;
            cand |= dict_bit(bm + DICT_BM1, b >> 5, b) << i;
        }
    }
    return cand & own;
}

// Bits [lo, hi) of 16 for the starts c .. c + 15 that lie in [beg, end) (aligned coordinates).
__device__ __forceinline__ uint32_t dict_own_mask(uint64_t c, uint64_t beg, uint64_t end)
{
    if (c >= end || c + 16 <= beg) return 0;
    const uint32_t lo = beg > c ? (uint32_t)(beg - c) : 0u;
    const uint32_t hi = end - c >= 16 ? 16u : (uint32_t)(end - c);
    return ((1u << hi) - 1u) & ~((1u << lo) - 1u) & 0xffffu;
}

// One round's bytes for this lane: the 16 at c (if c holds a view byte) and the next lane's first 4.
__device__ __forceinline__ void dict_load(const DictArgs &a, uint64_t c, uint32_t lane, uint4 &v, uint32_t &x)
{
    v = make_uint4(0, 0, 0, 0);
    x = 0;
    if (c < a.vend) v = *reinterpret_cast<const uint4 *>(a.text16 + c);
    if (lane == 63 && c + 16 < a.vend) x = *reinterpret_cast<const uint32_t *>(a.text16 + c + 16);
}

__device__ __forceinline__ void dict_words(uint4 v, uint32_t x, uint32_t lane, uint32_t w[5])
{
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    const uint32_t up = __shfl_down(v.x, 1, 64);
    w[4] = lane == 63 ? x : up;
}

// Exclusive scan of one value per lane over the workgroup; *total gets the sum.  Two barriers.
__device__ __forceinline__ uint32_t dict_block_scan(uint32_t v, uint32_t *wave_sums, uint32_t *total)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl += o;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < DICT_BLOCK / 64; ++q) {
        const uint32_t s = wave_sums[q];
        if ((uint32_t)q < wave) before += s;
        all += s;
    }
    *total = all;
    __syncthreads(); // wave_sums is free again
    return before + incl - v;
}

__global__ __launch_bounds__(DICT_BLOCK) void dict_kernel(const DictArgs a)
{
    __shared__ uint32_t bm[DICT_BM_WORDS];
    __shared__ uint64_t stage[DICT_STAGE];
    __shared__ uint32_t wave_sums[DICT_BLOCK / 64];
    __shared__ unsigned long long stage_n; // the tile's pairs: 64 bits (2^18 starts x 2^16 duplicates of one pattern is 2^34)
    __shared__ uint32_t cand_n;
    __shared__ uint64_t sh_tile, sh_prefix;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < DICT_BM_WORDS; i += DICT_BLOCK) bm[i] = a.bitmaps[i];
    const uint32_t rs = a.rounds_shift;
    const uint32_t tile_shift = rs + 13; // DICT_ROUND == 2^13
    for (;;) {
        if (tid == 0) {
            sh_tile = atomicAdd(a.ticket, 1ull) - a.ticket_base; // tiles in ascending order: every predecessor is owned
            stage_n = 0;
            cand_n = 0;
        }
        __syncthreads(); // (also: the bitmaps, and the previous tile's last reads of the pool)
        const uint64_t t = sh_tile;
        if (t >= a.n_tiles) break;
        const uint64_t tile0 = (a.tile_begin + t) << tile_shift;
        const uint64_t tile_end = tile0 + (1ull << tile_shift);
        const uint64_t beg = tile0 > a.first ? tile0 : a.first;
        const uint64_t end = tile_end < a.own_hi ? tile_end : a.own_hi;
        const uint32_t rounds = 1u << rs;

        // first walk: park every pair
        {
            auto park = [&](uint64_t p, uint32_t id) {
                const unsigned long long slot = atomicAdd(&stage_n, 1ull);
                if (a.out != nullptr && slot < (unsigned long long)DICT_STAGE) stage[slot] = ((p - tile0) << 16) | id;
            };
            uint4 v0, v1;
            uint32_t x0, x1;
            uint64_t c = tile0 + 16ull * tid;
            dict_load(a, c, lane, v0, x0);
            dict_load(a, c + DICT_ROUND, lane, v1, x1);
            uint32_t ncand = 0;
            for (uint32_t r = 0; r < rounds; ++r, c += DICT_ROUND) {
                if (tile0 + (uint64_t)r * DICT_ROUND >= end) break; // uniform
                uint4 v2;
                uint32_t x2;
                dict_load(a, c + 2ull * DICT_ROUND, lane, v2, x2); // two rounds ahead (the last ones load nothing)
                uint32_t w[5];
                dict_words(v0, x0, lane, w);
                uint32_t cand = dict_filter(a, bm, w, c, dict_own_mask(c, beg, end));
                while (cand) { // rare on sparse results
                    const int i = __builtin_ctz(cand);
                    cand &= cand - 1;
                    ++ncand;
                    const uint32_t k = dict_key(a, c + i);
                    const uint64_t p = c + i;
                    auto emit = [&](uint32_t id) { park(p, id); };
                    dict_at(a, p, k, emit);
                }
                v0 = v1, x0 = x1, v1 = v2, x1 = x2;
            }
            if (ncand) atomicAdd(&cand_n, ncand);
        }
        __syncthreads();
        if (tid == 0) {
            const uint64_t agg = stage_n;
            if (cand_n) atomicAdd(a.cand, (unsigned long long)cand_n);
            const uint64_t prefix = ordered_lookback(a, t, agg);
            sh_prefix = prefix;
            ordered_publish_total(a, t, prefix + agg);
        }
        __syncthreads();
        const uint64_t prefix = sh_prefix;
        const uint64_t tile_pairs = stage_n;
        if (a.out != nullptr && prefix < a.cap && tile_pairs > 0) { // (a tile that starts at or past the capacity stores nothing)
            if (tile_pairs <= (uint64_t)DICT_STAGE) {
                const uint32_t parked = (uint32_t)tile_pairs;
                // slot = prefix + rank of the key among the parked ones (keys are distinct: one per (p, id))
                for (uint32_t j = tid; j < parked; j += DICT_BLOCK) {
                    const uint64_t e = stage[j];
                    uint32_t rank = 0;
                    for (uint32_t q = 0; q < parked; ++q) rank += stage[q] < e ? 1u : 0u;
                    const uint64_t idx = prefix + rank;
                    if (idx < a.cap) {
                        a.out[idx] = tile0 + (e >> 16) + a.out_bias;
                        if (a.pid != nullptr) a.pid[idx] = (uint32_t)(e & 0xffffu);
                    }
                }
            } else {
                // dense tile: walk it again round by round; each round counts, scans and writes
                uint64_t base = prefix;
                uint64_t c = tile0 + 16ull * tid;
                for (uint32_t r = 0; r < rounds; ++r, c += DICT_ROUND) {
                    if (tile0 + (uint64_t)r * DICT_ROUND >= end || base >= a.cap) break; // uniform
                    uint4 v;
                    uint32_t x;
                    dict_load(a, c, lane, v, x);
                    uint32_t w[5];
                    dict_words(v, x, lane, w);
                    const uint32_t cand0 = dict_filter(a, bm, w, c, dict_own_mask(c, beg, end));
                    uint32_t cnt = 0;
                    for (uint32_t cand = cand0; cand; cand &= cand - 1) {
                        const int i = __builtin_ctz(cand);
                        const uint32_t k = dict_key(a, c + i);
                        auto count = [&](uint32_t) { ++cnt; };
                        dict_at(a, c + i, k, count);
                    }
                    uint32_t round_total;
                    const uint32_t lane_base = dict_block_scan(cnt, wave_sums, &round_total);
                    uint64_t idx = base + lane_base;
                    for (uint32_t cand = cand0; cand && idx < a.cap; cand &= cand - 1) {
                        const int i = __builtin_ctz(cand);
                        const uint32_t k = dict_key(a, c + i);
                        const uint64_t p = c + i;
                        auto write = [&](uint32_t id) {
                            if (idx < a.cap) {
                                a.out[idx] = p + a.out_bias;
                                if (a.pid != nullptr) a.pid[idx] = id;
                            }
                            ++idx;
                        };
                        dict_at(a, p, k, write);
                    }
                    base += round_total;
                }
            }
        }
        __syncthreads(); // the pool and stage_n are the next tile's
    }
}

} // namespace bmx
