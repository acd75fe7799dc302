// bmx_lcp_kernel.h -- kernels of the LCP array (bmx_lcp_*, include/bmx.h): lcp[j] = length of the longest common prefix of
// the suffixes at positions j - 1 and j of a suffix array, for a device-resident text and ANY permutation sa of 0..n-1.
//
// The algorithm is the Phi / irreducible-LCP one of Karkkainen, Manzini and Puglisi (CPM 2009), in text order:
//     phi[sa[j]] = sa[j - 1]                                            lcp_phi_kernel       (a scatter; phi lives in lcp)
//     plcp[i] = common prefix of text[i..) and text[phi[i]..)           lcp_lane_kernel      for the IRREDUCIBLE i only
//     the pairs that share more than LCP_LANE_BYTES bytes              lcp_plan_kernel, lcp_long_kernel
//     plcp[i] = plcp[r] - (i - r), r the nearest irreducible <= i       lcp_carry_kernel, lcp_fill_kernel
//     lcp[j] = plcp[sa[j]]                                              lcp_gather_kernel
// Position i is REDUCIBLE iff i >= 1, phi[i] >= 1, text[i - 1] == text[phi[i] - 1] and phi[i - 1] == phi[i] - 1.  Then the
// pair (i, phi[i]) is the pair (i - 1, phi[i - 1]) with its first byte -- an equal one -- taken off, so plcp[i] =
// plcp[i - 1] - 1 by byte identity alone, whatever the permutation.  The textbook drops the last condition because
// lexicographic order implies it; the order bmx_suffix_array builds outside lower-case text does not (prepending a byte
// flips the parity that decides whether a suffix carries the virtual end symbol, csrc/bmx_index_kernel.h), and an
// arbitrary permutation certainly does not.  For a lexicographic array the irreducible values sum to at most 2 n log n.
//
// Bytes compare as plain bytes and nothing at or past n counts.  Memory safety: a text byte is fetched as part of the
// aligned 8-byte word that holds it, and no word is read that does not hold at least one byte of text[0..n).  An entry of
// sa outside [0, n) is never stored into phi and never used as an index; a slot of phi nobody wrote (an entry that occurs
// twice leaves one) is found by lcp_lane_kernel.  Both raise ws[LCP_WS_BAD]; the outputs are then unspecified, but every
// offset that is used is one that passed its range check.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmx {

constexpr uint32_t LCP_BLOCK = 256;
constexpr uint32_t LCP_PER = 4;                      // text positions per lane and tile
constexpr uint32_t LCP_TILE = LCP_BLOCK * LCP_PER;   // text positions per workgroup turn: the unit of tile_last / carry
constexpr uint32_t LCP_LANE_BYTES = 64;              // == BMX_LCP_LANE_BYTES (a multiple of 8)
constexpr uint32_t LCP_MAX_GRID = 65536;             // workgroups of a grid-stride kernel, as bmx_sa.hip's helpers
constexpr int32_t LCP_NONE = -1;                     // phi of sa[0]
constexpr int32_t LCP_UNSET = -2;                    // phi before the scatter
constexpr int32_t LCP_REDUCIBLE = -1;                // plcp of a reducible position until lcp_fill_kernel
// The long path: one wave per segment, 16 bytes per lane and step, LCP_LONG_UNROLL steps in flight.
constexpr uint32_t LCP_LONG_UNROLL = 4;
constexpr uint32_t LCP_LONG_STEP = 64 * 16;                           // bytes of each stream per wave step
constexpr uint32_t LCP_LONG_ITER = LCP_LONG_STEP * LCP_LONG_UNROLL;   // ... per loop turn
constexpr uint32_t LCP_LONG_GRID = 2048;                              // workgroups of lcp_long_kernel: 8,192 waves,
constexpr uint32_t LCP_LONG_WAVES = LCP_LONG_GRID * (LCP_BLOCK / 64); // the 32 waves per CU that can be resident on 256 CUs
constexpr uint32_t LCP_LONG_MIN_SEG = 16384;                          // no segment shorter than four loop turns
constexpr uint32_t LCP_PLAN_BLOCK = 1024;                             // lcp_plan_kernel, lcp_carry_kernel: ONE workgroup
constexpr uint32_t LCP_STATS_GRID = 1024;                             // partials of bmx_lcp_stats_device at most

// the 32-bit words the kernels share with the host (zeroed before every call)
enum { LCP_WS_BAD = 0, LCP_WS_LONG = 1, LCP_WS_LISTED = 2, LCP_WS_SEGS = 3, LCP_WS_SEG_BYTES = 4, LCP_WS_WORDS = 8 };

// text[at .. at + 8) as one little-endian word: byte at + b in bits 8b .. 8b + 7.  at < n; `last` is the address of the
// aligned word that holds text[n - 1].  Bytes at and behind n come out as anything (the caller counts only valid ones).
__device__ __forceinline__ uint64_t lcp_load8(const uint8_t *text, uint64_t at, uintptr_t last)
{
    const uintptr_t addr = (uintptr_t)text + at;
    const uintptr_t a = addr & ~(uintptr_t)7;
    const uint32_t sh = (uint32_t)(addr & 7u) * 8u;
    uint64_t w = *reinterpret_cast<const uint64_t *>(a);
    if (sh) {
        const uint64_t w1 = a < last ? *reinterpret_cast<const uint64_t *>(a + 8) : 0ull;
        w = (w >> sh) | (w1 << (64u - sh));
    }
    return w;
}

// the same for 16 bytes: three aligned words at most
__device__ __forceinline__ void lcp_load16(const uint8_t *text, uint64_t at, uintptr_t last, uint64_t &lo, uint64_t &hi)
{
    const uintptr_t addr = (uintptr_t)text + at;
    const uintptr_t a = addr & ~(uintptr_t)7;
    const uint32_t sh = (uint32_t)(addr & 7u) * 8u;
    const uint64_t w0 = *reinterpret_cast<const uint64_t *>(a);
    const uint64_t w1 = a + 8 <= last ? *reinterpret_cast<const uint64_t *>(a + 8) : 0ull;
    lo = w0, hi = w1;
    if (sh) {
        const uint64_t w2 = a + 16 <= last ? *reinterpret_cast<const uint64_t *>(a + 16) : 0ull;
        lo = (w0 >> sh) | (w1 << (64u - sh));
        hi = (w1 >> sh) | (w2 << (64u - sh));
    }
}

// Common prefix of text[i..) and text[p..) from byte k on (the first k are known equal), counted up to `lim` bytes
// (lim <= n - max(i, p)): returns the first k' in [k, lim) with text[i + k'] != text[p + k'], or lim.
__device__ __forceinline__ uint32_t lcp_lane_compare(const uint8_t *text, uintptr_t last, uint32_t i, uint32_t p, uint32_t k,
                                                     uint32_t lim)
{
    while (k < lim) {
        const uint64_t x = lcp_load8(text, (uint64_t)i + k, last) ^ lcp_load8(text, (uint64_t)p + k, last);
        const uint32_t valid = lim - k < 8u ? lim - k : 8u;
        const uint32_t same = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
        if (same < valid) return k + same;
        k += valid;
    }
    return lim;
}

__global__ __launch_bounds__(LCP_BLOCK) void lcp_phi_kernel(const int32_t *__restrict__ sa, uint32_t n, int32_t *__restrict__ phi,
                                                            uint32_t *ws)
{
    for (uint64_t j = (uint64_t)blockIdx.x * LCP_BLOCK + threadIdx.x; j < n; j += (uint64_t)gridDim.x * LCP_BLOCK) {
        const uint32_t cur = (uint32_t)sa[j];
        if (cur >= n) {
            ws[LCP_WS_BAD] = 1;
            continue;
        }
        int32_t prev = LCP_NONE;
        if (j > 0) {
            const uint32_t pv = (uint32_t)sa[j - 1];
            if (pv >= n) continue; // (that entry's own lane raises the status word; the slot stays unset)
            prev = (int32_t)pv;
        }
        phi[cur] = prev;
    }
}

// One lane per text position.  plcp[i] = LCP_REDUCIBLE, or the pair's common prefix; a pair whose common prefix is longer
// than LCP_LANE_BYTES goes on the list with plcp[i] = n - max(i, phi[i]), the value it keeps if lcp_long_kernel finds no
// difference either (lcp_long_kernel takes it up at byte LCP_LANE_BYTES again).  The list is filled through a counter (one
// atomic per wave), so its ORDER differs from run to run; no output depends on it.  A pair that finds the list full is
// finished by its lane.  tile_last[t] = the last irreducible position of tile t, or -1.
__global__ __launch_bounds__(LCP_BLOCK) void lcp_lane_kernel(const uint8_t *__restrict__ text, uint32_t n,
                                                             const int32_t *__restrict__ phi, int32_t *__restrict__ plcp,
                                                             int32_t *__restrict__ tile_last, uint32_t *__restrict__ list,
                                                             uint32_t list_cap, uint32_t *ws)
{
    __shared__ int32_t red[LCP_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uintptr_t last_word = ((uintptr_t)text + n - 1) & ~(uintptr_t)7;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + LCP_TILE - 1) / LCP_TILE);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        int32_t last = -1;
#pragma unroll
        for (uint32_t u = 0; u < LCP_PER; ++u) {
            const uint64_t i64 = (uint64_t)t * LCP_TILE + u * LCP_BLOCK + tid;
            const bool in = i64 < n;
            const uint32_t i = (uint32_t)i64;
            const int32_t ph = in ? phi[i] : LCP_NONE;
            if (ph == LCP_UNSET) ws[LCP_WS_BAD] = 1; // no entry of sa names i: another position is named twice
            bool reducible = false;
            if (in && i >= 1 && ph >= 1 && phi[i - 1] == ph - 1) reducible = text[i - 1] == text[ph - 1];
            int32_t v = reducible ? LCP_REDUCIBLE : 0;
            uint32_t maxlen = 0, k = 0;
            const bool pair = in && !reducible && ph >= 0;
            if (pair) {
                maxlen = n - (i > (uint32_t)ph ? i : (uint32_t)ph);
                // (one byte past the budget is looked at: a common prefix of exactly LCP_LANE_BYTES ends here)
                k = lcp_lane_compare(text, last_word, i, (uint32_t)ph, 0, maxlen <= LCP_LANE_BYTES ? maxlen : LCP_LANE_BYTES + 1u);
                v = (int32_t)k;
            }
            const bool lng = pair && k > LCP_LANE_BYTES; // the common prefix is longer than the budget
            const uint64_t mask = __ballot(lng);
            if (mask != 0) { // (wave-uniform)
                uint32_t base = 0;
                if (lane == (uint32_t)(__ffsll((unsigned long long)mask) - 1)) base = atomicAdd(&ws[LCP_WS_LONG], (uint32_t)__popcll(mask));
                base = __shfl(base, __ffsll((unsigned long long)mask) - 1);
                if (lng) {
                    const uint32_t slot = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                    if (slot < list_cap) { // (the counter counts at most n < 2^31 pairs: it does not wrap)
                        list[slot] = i;
                        v = (int32_t)maxlen;
                    } else {
                        v = (int32_t)lcp_lane_compare(text, last_word, i, (uint32_t)ph, k, maxlen);
                    }
                }
            }
            if (in) {
                plcp[i] = v;
                if (!reducible) last = (int32_t)i;
            }
        }
        for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o));
        if (lane == 0) red[tid >> 6] = last;
        __syncthreads();
        if (tid == 0) {
            int32_t m = red[0];
            for (uint32_t w = 1; w < LCP_BLOCK / 64; ++w) m = max(m, red[w]);
            tile_last[t] = m;
        }
        __syncthreads(); // (red is used again)
    }
}

// bytes of listed pair e that lie behind the lane's budget: > 0
__device__ __forceinline__ uint32_t lcp_pair_rest(const int32_t *phi, const uint32_t *list, uint32_t e, uint32_t n)
{
    const uint32_t i = list[e], p = (uint32_t)phi[i];
    return n - (i > p ? i : p) - LCP_LANE_BYTES;
}

// ONE workgroup: cuts the listed pairs into segments for lcp_long_kernel.  The split rule for skewed work lists: a pair
// whose rest (the bytes it MAY have to compare: its length is what is being computed) is above a quarter of one wave's
// share of all rests is cut into segments of that size, and no segment is shorter than LCP_LONG_MIN_SEG.
// seg_start[e] = number of segments of the pairs before e; ws[LCP_WS_LISTED / _SEGS / _SEG_BYTES] = pairs, segments,
// bytes per segment.
__global__ __launch_bounds__(LCP_PLAN_BLOCK) void lcp_plan_kernel(const int32_t *__restrict__ phi, uint32_t n,
                                                                  const uint32_t *__restrict__ list, uint32_t list_cap,
                                                                  uint32_t *__restrict__ seg_start, uint32_t *ws)
{
    __shared__ unsigned long long total;
    __shared__ uint32_t scan[LCP_PLAN_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint32_t m = ws[LCP_WS_LONG] < list_cap ? ws[LCP_WS_LONG] : list_cap;
    if (tid == 0) total = 0;
    __syncthreads();
    const uint32_t per = (m + LCP_PLAN_BLOCK - 1) / LCP_PLAN_BLOCK;
    const uint64_t e0 = (uint64_t)tid * per, e1 = e0 + per < m ? e0 + per : m;
    unsigned long long mine = 0;
    for (uint64_t e = e0; e < e1; ++e) mine += lcp_pair_rest(phi, list, (uint32_t)e, n);
    if (mine != 0) atomicAdd(&total, mine);
    __syncthreads();
    unsigned long long chunk = (total / (4ull * LCP_LONG_WAVES) + LCP_LONG_ITER - 1) / LCP_LONG_ITER * LCP_LONG_ITER;
    if (chunk < LCP_LONG_MIN_SEG) chunk = LCP_LONG_MIN_SEG;
    if (chunk > 0x80000000ull) chunk = 0x80000000ull; // (a rest is below 2^31: one segment per pair from here on)
    const uint32_t seg_bytes = (uint32_t)chunk;
    uint32_t segs = 0;
    for (uint64_t e = e0; e < e1; ++e) segs += (lcp_pair_rest(phi, list, (uint32_t)e, n) + (seg_bytes - 1u)) / seg_bytes;
    scan[tid] = segs;
    __syncthreads();
    for (uint32_t d = 1; d < LCP_PLAN_BLOCK; d *= 2) { // inclusive scan over the threads
        const uint32_t add = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    uint32_t at = scan[tid] - segs;
    for (uint64_t e = e0; e < e1; ++e) {
        seg_start[e] = at;
        at += (lcp_pair_rest(phi, list, (uint32_t)e, n) + (seg_bytes - 1u)) / seg_bytes;
    }
    if (tid == LCP_PLAN_BLOCK - 1) {
        ws[LCP_WS_LISTED] = m;
        ws[LCP_WS_SEGS] = scan[tid];
        ws[LCP_WS_SEG_BYTES] = seg_bytes;
    }
}

// One wave per segment of a listed pair: 16 bytes of both streams per lane and step, LCP_LONG_UNROLL steps loaded before
// the first is looked at, ballot for the first difference.  plcp[i] = the minimum over the pair's segments (atomicMin on
// the value lcp_lane_kernel left: the pair's full length); a segment stops when an earlier one has found a difference.
__global__ __launch_bounds__(LCP_BLOCK) void lcp_long_kernel(const uint8_t *__restrict__ text, uint32_t n,
                                                             const int32_t *__restrict__ phi, int32_t *plcp,
                                                             const uint32_t *__restrict__ list,
                                                             const uint32_t *__restrict__ seg_start, const uint32_t *ws)
{
    const uint32_t m = ws[LCP_WS_LISTED], segs = ws[LCP_WS_SEGS], seg_bytes = ws[LCP_WS_SEG_BYTES];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (LCP_BLOCK / 64);
    const uintptr_t last_word = ((uintptr_t)text + n - 1) & ~(uintptr_t)7;
    for (uint32_t s = blockIdx.x * (LCP_BLOCK / 64) + (threadIdx.x >> 6); s < segs; s += waves) {
        uint32_t lo = 0, hi = m; // the pair: the last e with seg_start[e] <= s
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (seg_start[mid] <= s) lo = mid;
            else hi = mid;
        }
        const uint32_t i = list[lo], p = (uint32_t)phi[i];
        const uint32_t maxlen = n - (i > p ? i : p);
        const uint64_t begin = (uint64_t)LCP_LANE_BYTES + (uint64_t)(s - seg_start[lo]) * seg_bytes; // < maxlen
        const uint32_t end = begin + seg_bytes < maxlen ? (uint32_t)(begin + seg_bytes) : maxlen;
        int32_t *res = &plcp[i];
        for (uint32_t pos = (uint32_t)begin; pos < end; pos += LCP_LONG_ITER) {
            // (one lane's view for the whole wave: the ballots below need every lane in step)
            const uint32_t known = (uint32_t)__shfl(__atomic_load_n(res, __ATOMIC_RELAXED), 0);
            if (known <= pos) break; // nothing here can be the first difference
            uint32_t at[LCP_LONG_UNROLL];
            bool diff[LCP_LONG_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < LCP_LONG_UNROLL; ++u) {
                const uint64_t off = (uint64_t)pos + u * LCP_LONG_STEP + lane * 16u;
                at[u] = 0;
                diff[u] = false;
                if (off < end) {
                    uint64_t a0, a1, b0, b1;
                    lcp_load16(text, (uint64_t)i + off, last_word, a0, a1);
                    lcp_load16(text, (uint64_t)p + off, last_word, b0, b1);
                    const uint64_t x0 = a0 ^ b0, x1 = a1 ^ b1;
                    const uint32_t same = x0 ? (uint32_t)__builtin_ctzll(x0) >> 3 : x1 ? 8u + ((uint32_t)__builtin_ctzll(x1) >> 3) : 16u;
                    const uint32_t valid = end - (uint32_t)off < 16u ? end - (uint32_t)off : 16u;
                    diff[u] = same < valid;
                    at[u] = (uint32_t)off + same;
                }
            }
            bool found = false;
#pragma unroll
            for (uint32_t u = 0; u < LCP_LONG_UNROLL; ++u) {
                const uint64_t mask = __ballot(diff[u]);
                if (!found && mask != 0) {
                    const int first = __ffsll((unsigned long long)mask) - 1;
                    const uint32_t where = __shfl(at[u], first);
                    if (lane == 0) atomicMin(res, (int32_t)where);
                    found = true;
                }
            }
            if (found) break; // (wave-uniform)
        }
    }
}

// ONE workgroup: carry[t] = the last irreducible position of the tiles before t, or -1
__global__ __launch_bounds__(LCP_PLAN_BLOCK) void lcp_carry_kernel(const int32_t *__restrict__ tile_last, uint32_t tiles,
                                                                   int32_t *__restrict__ carry)
{
    __shared__ int32_t scan[LCP_PLAN_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (tiles + LCP_PLAN_BLOCK - 1) / LCP_PLAN_BLOCK;
    const uint64_t t0 = (uint64_t)tid * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    int32_t mine = -1;
    for (uint64_t t = t0; t < t1; ++t) mine = max(mine, tile_last[t]);
    scan[tid] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < LCP_PLAN_BLOCK; d *= 2) { // inclusive prefix maximum over the threads
        const int32_t other = tid >= d ? scan[tid - d] : -1;
        __syncthreads();
        scan[tid] = max(scan[tid], other);
        __syncthreads();
    }
    int32_t run = tid > 0 ? scan[tid - 1] : -1;
    for (uint64_t t = t0; t < t1; ++t) {
        carry[t] = run;
        run = max(run, tile_last[t]);
    }
}

// Streaming: a lane takes LCP_PER consecutive positions.  The nearest irreducible position at or below each comes from
// the lane's own entries, the lanes before it (a prefix maximum over the workgroup) and carry[t]; its value is read
// from plcp (irreducible entries are final and are stored back unchanged).
__global__ __launch_bounds__(LCP_BLOCK) void lcp_fill_kernel(int32_t *plcp, uint32_t n, const int32_t *__restrict__ carry)
{
    __shared__ int32_t red[LCP_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + LCP_TILE - 1) / LCP_TILE);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t i0 = (uint64_t)t * LCP_TILE + tid * LCP_PER;
        const bool whole = i0 + LCP_PER <= n;
        int32_t v[LCP_PER];
        if (whole) {
            const int4 q = *reinterpret_cast<const int4 *>(plcp + i0);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (uint32_t q = 0; q < LCP_PER; ++q) v[q] = i0 + q < n ? plcp[i0 + q] : LCP_REDUCIBLE;
        }
        int32_t mine = -1;
#pragma unroll
        for (uint32_t q = 0; q < LCP_PER; ++q)
            if (v[q] >= 0) mine = (int32_t)(i0 + q);
        // exclusive prefix maximum over the workgroup's lanes
        int32_t incl = mine;
        for (uint32_t d = 1; d < 64; d *= 2) {
            const int32_t other = __shfl_up(incl, d);
            if (lane >= d) incl = max(incl, other);
        }
        if (lane == 63) red[wave] = incl;
        __syncthreads();
        int32_t r = carry[t];
        for (uint32_t w = 0; w < wave; ++w) r = max(r, red[w]);
        const int32_t up = __shfl_up(incl, 1);
        if (lane > 0) r = max(r, up);
        __syncthreads(); // (red is used again)
        int32_t rv = r >= 0 ? plcp[r] : 0; // (position 0 is irreducible: r < 0 only for positions that do not exist)
#pragma unroll
        for (uint32_t q = 0; q < LCP_PER; ++q) {
            const int32_t i = (int32_t)(i0 + q);
            if (v[q] >= 0) r = i, rv = v[q];
            else v[q] = rv - (i - r);
        }
        if (whole) {
            *reinterpret_cast<int4 *>(plcp + i0) = make_int4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (uint32_t q = 0; q < LCP_PER; ++q)
                if (i0 + q < n) plcp[i0 + q] = v[q];
        }
    }
}

__global__ __launch_bounds__(LCP_BLOCK) void lcp_gather_kernel(const int32_t *__restrict__ sa, uint32_t n,
                                                               const int32_t *__restrict__ plcp, int32_t *__restrict__ lcp)
{
    for (uint64_t j = (uint64_t)blockIdx.x * LCP_BLOCK + threadIdx.x; j < n; j += (uint64_t)gridDim.x * LCP_BLOCK) {
        const uint32_t p = (uint32_t)sa[j];
        lcp[j] = j > 0 && p < n ? plcp[p] : 0;
    }
}

// Per workgroup {max, smallest j that attains it, sum, number of entries >= min_len} of the entries its grid-stride loop
// visits: integer arithmetic, a fixed tree within the workgroup; the host combines the workgroups in index order.
__global__ __launch_bounds__(LCP_BLOCK) void lcp_stats_kernel(const int32_t *__restrict__ lcp, uint32_t n, uint32_t min_len,
                                                              uint64_t *__restrict__ partial)
{
    __shared__ uint64_t s_max[LCP_BLOCK], s_arg[LCP_BLOCK], s_sum[LCP_BLOCK], s_cnt[LCP_BLOCK];
    const uint32_t tid = threadIdx.x;
    uint64_t mx = 0, arg = ~0ull, sum = 0, cnt = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * LCP_BLOCK + tid; j < n; j += (uint64_t)gridDim.x * LCP_BLOCK) {
        const uint64_t v = (uint32_t)lcp[j];
        if (v > mx || arg == ~0ull) mx = v, arg = j; // (j ascends: the first one stays)
        sum += v;
        cnt += v >= min_len ? 1u : 0u;
    }
    s_max[tid] = mx, s_arg[tid] = arg, s_sum[tid] = sum, s_cnt[tid] = cnt;
    __syncthreads();
    for (uint32_t d = LCP_BLOCK / 2; d > 0; d /= 2) {
        if (tid < d) {
            const uint64_t om = s_max[tid + d], oa = s_arg[tid + d];
            if (om > s_max[tid] || (om == s_max[tid] && oa < s_arg[tid])) s_max[tid] = om, s_arg[tid] = oa;
            s_sum[tid] += s_sum[tid + d];
            s_cnt[tid] += s_cnt[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        partial[4 * blockIdx.x + 0] = s_max[0];
        partial[4 * blockIdx.x + 1] = s_arg[0];
        partial[4 * blockIdx.x + 2] = s_sum[0];
        partial[4 * blockIdx.x + 3] = s_cnt[0];
    }
}

} // namespace bmx
