// bmx_approx_kernel.h -- approximate search (bmx_search_approx_device): every end j of the text view with
// min over s of ED(P, T[s..j]) <= k (Sellers' k-differences problem), in ascending order, with that minimum.
//
// The recurrence is Myers' bit-parallel column update (J. ACM 46(3), 1999) with the search boundary: row 0 of the
// table is all zeros (an alignment may start anywhere), so no carry enters bit 0 of the horizontal deltas.  The
// reference's closest relative is the anti-diagonal DP of EditDistance-1/EditDistance-1/kernal.cl:5-56 (one cell per
// work-item); its "one report per hit" is BoyreMoore/x64/Debug/kernel1.cl:24.
//
// Geometry.  A workgroup of APPROX_BLOCK lanes takes tiles of APPROX_BLOCK * P end positions from an
// atomic ticket, in ascending order.  Lane l owns the P ends [tile + l*P, tile + (l+1)*P) and first walks the
// m + k - 1 bytes in front of them (rounded down to 16) without reporting: an alignment of cost <= k spans at most
// m + k bytes, so from there on the lane's scores are exact.  Text comes in 16 bytes per lane per load, straight from
// HBM (neighbouring lanes' warm-up bytes are the previous lane's last bytes: L2 serves them).  Peq -- the bit mask of
// the pattern positions holding each byte value -- is in LDS.
//
// Ordered output in one pass.  While it walks, a lane counts its hits and parks (position in tile, ordinal in lane,
// distance) in a pool of APPROX_STAGE entries per tile.  The workgroup then scans the lane counts, publishes the
// tile's aggregate and finds its exclusive prefix by decoupled look-back over per-tile status words
// (bmx_ordered_out.h; the word is its own payload: {epoch tag, kind, value}), so every parked hit goes straight to
// its final slot prefix + lane base + ordinal.  A tile with more hits than the pool walks itself a second time and
// writes directly.  Slots at or past the capacity are dropped: the stored entries are the lowest ends.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmx_ordered_out.h"

namespace bmx {

constexpr int APPROX_BLOCK = 256;  // lanes per workgroup
constexpr int APPROX_STAGE = 2048; // hits parked per tile (16 KiB of LDS)
constexpr int MAX_APPROX_PATTERN = 64; // == BMX_MAX_APPROX_PATTERN

struct ApproxArgs {
    const uint8_t *text16; // caller's pointer rounded down to a multiple of 16
    uint64_t first;        // aligned coordinate of view byte 0 (0..15)
    uint64_t own_lo;       // first end to report (aligned coordinates: lead + first)
    uint64_t own_hi;       // one past the last (n + first)
    uint64_t out_bias;     // reported end = aligned end + out_bias (base_offset - first)
    uint64_t tile_begin;   // first tile index (aligned end / tile bytes)
    uint64_t n_tiles;
    uint64_t *out;         // ends, ascending (NULL: count only)
    uint8_t *dist;         // their distances (NULL: not wanted)
    uint64_t cap;          // entries out / dist have room for
    uint64_t *status;      // n_tiles tile words (tagged: no clearing between calls)
    unsigned long long *ticket; // monotonic across calls: this call's tickets start at ticket_base
    uint64_t ticket_base;
    uint64_t *host_status; // pinned: [0] total, [1] give-up flag, [2] seq (written by the last tile)
    uint64_t seq;
    uint64_t tag;          // seq mod 2^22 (never 0)
    uint32_t m, k, warm;   // warm = m + k - 1
    uint32_t p_shift;      // P = 1 << p_shift ends per lane
    uint64_t peq[256];     // bit i set: pattern[i] == byte (low word used when m <= 32)
};

// Column state of Myers' recurrence for one lane.
template <typename W>
struct MyersState {
    W pv, mv;
    uint32_t score;
};

template <typename W>
__device__ __forceinline__ void myers_step(MyersState<W> &s, W eq, uint32_t hb)
{
    const W xv = eq | s.mv;
    const W xh = (((eq & s.pv) + s.pv) ^ s.pv) | eq;
    W ph = s.mv | ~(xh | s.pv);
    W mh = s.pv & xh;
    // score += bit hb of ph - bit hb of mh (v_bfe_u32 + v_bfe_i32 + v_add3).  The 64-bit word is only used for
    // m = 33..64, so bit hb is in its upper half.
    const uint32_t phw = sizeof(W) == 4 ? (uint32_t)ph : (uint32_t)((uint64_t)ph >> 32);
    const uint32_t mhw = sizeof(W) == 4 ? (uint32_t)mh : (uint32_t)((uint64_t)mh >> 32);
    s.score += __builtin_amdgcn_ubfe(phw, hb, 1) + (uint32_t)__builtin_amdgcn_sbfe((int32_t)mhw, hb, 1);
    ph <<= 1; // row 0 is free: no carry into bit 0
    mh <<= 1;
    s.pv = mh | ~(xv | ph);
    s.mv = ph & xv;
}

typedef uint32_t approx_u32x4 __attribute__((ext_vector_type(4)));

// What a walk does with a hit: PARK it in the tile's pool (first walk) or WRITE it to its final slot (second walk of a
// dense tile, from the lane's output base).
enum ApproxPass { APPROX_PARK = 0, APPROX_WRITE = 1 };

// 16 bytes of one chunk at aligned coordinate c.  HEAD: the chunk that holds view byte 0, walked from byte `skip` on.
// Bit i of rmask: end c + i belongs to this lane.
template <typename W, int PASS, bool HEAD>
__device__ __forceinline__ void approx_chunk(const ApproxArgs &a, const W *peq, MyersState<W> &s, approx_u32x4 v,
                                             uint64_t c, uint32_t rmask, uint32_t skip, uint32_t hb, uint32_t &cnt,
                                             uint64_t tile0, uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (HEAD && (uint32_t)i < skip) continue;
        const uint32_t byte = __builtin_amdgcn_ubfe(v[i >> 2], 8 * (i & 3), 8);
        myers_step<W>(s, peq[byte], hb);
        if (s.score <= a.k) { // rare on sparse results: the branch is skipped by the whole wave
            // (keeps the compiler from folding the test below into the one above: that costs two VALU per byte)
            __asm__ volatile("" ::: "memory");
            if ((rmask >> i) & 1u) {
                const uint32_t ord = cnt++;
                if (PASS == APPROX_PARK) {
                    if (a.out != nullptr) {
                        const uint32_t slot = atomicAdd(stage_n, 1u);
                        if (slot < (uint32_t)APPROX_STAGE)
                            stage[slot] = (uint64_t)(uint32_t)(c + i - tile0) | ((uint64_t)ord << 32) | ((uint64_t)s.score << 48);
                    }
                } else {
                    const uint64_t idx = base + ord;
                    if (idx < a.cap) {
                        a.out[idx] = c + i + a.out_bias;
                        if (a.dist != nullptr) a.dist[idx] = (uint8_t)s.score;
                    }
                }
            }
        }
    }
}

// One lane: the ends [lo, hi) (aligned coordinates), after a warm-up of a.warm bytes (clipped at view byte 0).
// Returns the number of hits.  Every 16-byte load holds at least one byte of the view.
template <typename W, int PASS>
__device__ __forceinline__ uint32_t approx_walk(const ApproxArgs &a, const W *peq, uint64_t lo, uint64_t hi, uint64_t tile0,
                                uint64_t *stage, uint32_t *stage_n, uint64_t base)
{
    const uint64_t want = lo >= a.first + a.warm ? lo - a.warm : a.first;
    uint64_t c = want & ~15ull;
    const uint32_t hb = sizeof(W) == 4 ? a.m - 1 : a.m - 33;
    MyersState<W> s;
    s.pv = ~(W)0;
    s.mv = 0;
    s.score = a.m;
    uint32_t cnt = 0;
    auto rmask_at = [&](uint64_t cc) -> uint32_t {
        const uint32_t rlo = lo <= cc ? 0u : (lo - cc >= 16 ? 16u : (uint32_t)(lo - cc));
        const uint32_t rhi = hi - cc >= 16 ? 16u : (uint32_t)(hi - cc);
        return ((1u << rhi) - 1u) & ~((1u << rlo) - 1u);
    };
    const approx_u32x4 *src = reinterpret_cast<const approx_u32x4 *>(a.text16);
    approx_u32x4 cur = src[c >> 4];
    approx_u32x4 nxt = cur;
    if (c + 16 < hi) nxt = src[(c >> 4) + 1];
    approx_chunk<W, PASS, true>(a, peq, s, cur, c, rmask_at(c), c < a.first ? (uint32_t)(a.first - c) : 0u, hb, cnt, tile0,
                                stage, stage_n, base);
    for (c += 16; c < hi; c += 16) {
        cur = nxt;
        if (c + 16 < hi) nxt = src[(c >> 4) + 1]; // one chunk ahead
        approx_chunk<W, PASS, false>(a, peq, s, cur, c, rmask_at(c), 0u, hb, cnt, tile0, stage, stage_n, base);
    }
    return cnt;
}

template <typename W>
__global__ __launch_bounds__(APPROX_BLOCK) void approx_kernel(const ApproxArgs a)
{
    __shared__ W peq[256];
    __shared__ uint64_t stage[APPROX_STAGE];
    __shared__ uint32_t lane_base[APPROX_BLOCK]; // hits per lane, then their exclusive scan
    __shared__ uint32_t stage_n;
    __shared__ uint64_t sh_tile, sh_prefix;
    const uint32_t tid = threadIdx.x;
    peq[tid] = (W)a.peq[tid]; // APPROX_BLOCK == 256
    const uint32_t ps = a.p_shift;
    for (;;) {
        if (tid == 0) {
            sh_tile = atomicAdd(a.ticket, 1ull) - a.ticket_base; // tiles in ascending order: every predecessor is owned
            stage_n = 0;
        }
        __syncthreads(); // (also: peq, and the previous tile's last reads of the LDS are done)
        const uint64_t t = sh_tile;
        if (t >= a.n_tiles) break;
        const uint64_t tile0 = (a.tile_begin + t) << (ps + 8);
        const uint64_t lo = max(tile0 + ((uint64_t)tid << ps), a.own_lo);
        const uint64_t hi = min(tile0 + ((uint64_t)(tid + 1) << ps), a.own_hi);
        uint32_t cnt = 0;
        if (lo < hi) cnt = approx_walk<W, APPROX_PARK>(a, peq, lo, hi, tile0, stage, &stage_n, 0);
        lane_base[tid] = cnt;
        __syncthreads();
        if (tid < 64) { // wave 0: exclusive scan of the 256 lane counts, then the look-back
            uint32_t v[4], sum = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = lane_base[4 * tid + q], sum += v[q];
            uint32_t incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if ((int)tid >= d) incl += o;
            }
            uint32_t run = incl - sum;
#pragma unroll
            for (int q = 0; q < 4; ++q) lane_base[4 * tid + q] = run, run += v[q];
            const uint64_t agg = (uint64_t)__shfl(incl, 63);
            if (tid == 0) {
                const uint64_t prefix = ordered_lookback(a, t, agg);
                sh_prefix = prefix;
                ordered_publish_total(a, t, prefix + agg);
            }
        }
        __syncthreads();
        const uint64_t prefix = sh_prefix;
        const uint32_t parked = stage_n;
        if (a.out != nullptr && prefix < a.cap) { // (a tile that starts at or past the capacity stores nothing)
            if (parked <= (uint32_t)APPROX_STAGE) {
                for (uint32_t j = tid; j < parked; j += APPROX_BLOCK) {
                    const uint64_t e = stage[j];
                    const uint32_t pos = (uint32_t)e;
                    const uint64_t idx = prefix + lane_base[pos >> ps] + ((e >> 32) & 0xffffu);
                    if (idx < a.cap) {
                        a.out[idx] = tile0 + pos + a.out_bias;
                        if (a.dist != nullptr) a.dist[idx] = (uint8_t)(e >> 48);
                    }
                }
            } else if (lo < hi) { // dense tile: walk it again, writing every hit to its slot
                (void)approx_walk<W, APPROX_WRITE>(a, peq, lo, hi, tile0, stage, &stage_n, prefix + lane_base[tid]);
            }
        }
        __syncthreads(); // the pool, the lane bases and stage_n are the next tile's
    }
}

} // namespace bmx
