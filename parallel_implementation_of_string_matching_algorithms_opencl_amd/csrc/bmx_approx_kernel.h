// bmx_approx_kernel.h -- approximate search (bmx_search_approx_device): every end j of the text view with
// min over s of ED(P, T[s..j]) <= k (Sellers' k-differences problem), in ascending order, with that minimum.
//
// The recurrence is Myers' bit-parallel column update (J. ACM 46(3), 1999) with the search boundary: row 0 of the
// table is all zeros (an alignment may start anywhere), so no carry enters bit 0 of the horizontal deltas.  The
// reference's closest relative is the anti-diagonal DP of EditDistance-1/EditDistance-1/kernal.cl:5-56 (one cell per
// work-item); its "one report per hit" is BoyreMoore/x64/Debug/kernel1.cl:24.
//
// The tile loop, the ordered output and the argument block are bmx_tile_frame.h's; this file is the recurrence, the lane's
// walk and the policy that plugs them into the frame.  A lane walks the m + k - 1 bytes in front of its ends (rounded down
// to 16) without reporting: an alignment of cost <= k spans at most m + k bytes, so from there on the lane's scores are
// exact.  Text comes in 16 bytes per lane per load, straight from HBM (neighbouring lanes' warm-up bytes are the previous
// lane's last bytes: L2 serves them).  Peq -- the bit mask of the pattern positions holding each byte value -- is in LDS.
// A parked hit is {position in tile, ordinal in lane << 32, distance << 48}.
#pragma once

#include "bmx_tile_frame.h"

namespace bmx {

constexpr int MAX_APPROX_PATTERN = 64; // == BMX_MAX_APPROX_PATTERN

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

// 16 bytes of one chunk at aligned coordinate c.  HEAD: the chunk that holds view byte 0, walked from byte `skip` on.
// Bit i of rmask: end c + i belongs to this lane.
template <typename W, int PASS, bool HEAD>
__device__ __forceinline__ void approx_chunk(const TileArgs &a, const W *peq, MyersState<W> &s, tile_u32x4 v,
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
                if (PASS == TILE_PARK) {
                    if (a.out != nullptr) {
                        const uint32_t slot = atomicAdd(stage_n, 1u);
                        if (slot < (uint32_t)TILE_STAGE)
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
__device__ __forceinline__ uint32_t approx_walk(const TileArgs &a, const W *peq, uint64_t lo, uint64_t hi, uint64_t tile0,
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
    const tile_u32x4 *src = reinterpret_cast<const tile_u32x4 *>(a.text16);
    tile_u32x4 cur = src[c >> 4];
    tile_u32x4 nxt = cur;
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
struct ApproxPolicy {
    typedef W Elem;
    static constexpr int TAB = 256;
    static __device__ __forceinline__ void fill(W *peq, const TileArgs &a, uint32_t tid) { peq[tid] = (W)a.peq[tid]; } // TILE_BLOCK == 256
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const W *peq, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base)
    {
        return approx_walk<W, PASS>(a, peq, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32) & 0xffffu; }
    static __device__ __forceinline__ void also(const TileArgs &a, uint64_t idx, uint64_t e)
    {
        if (a.dist != nullptr) a.dist[idx] = (uint8_t)(e >> 48);
    }
};

} // namespace bmx
