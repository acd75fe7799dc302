// bmx_tile_frame.h -- what the approximate, the class-pattern, the gapped and the k-mismatch search share (DESIGN.md s9,
// s21, s23): the argument block, the tile loop of the kernel and the host side of a launch.  A search supplies its
// per-byte recurrence as a policy; everything with an invariant across tiles or calls is here, once.
//
// Geometry.  A workgroup of TILE_BLOCK lanes takes tiles of TILE_BLOCK * P end positions from an atomic ticket, in
// ascending order.  Lane l owns the P ends [tile + l*P, tile + (l+1)*P) and first walks a.warm bytes in front of them
// without reporting, after which its state is exact.  Text comes in 16-byte loads from the caller's pointer rounded down
// to a multiple of 16 ("aligned coordinates").
//
// Ordered output in one pass.  While it walks, a lane counts its hits and parks (position in tile, ordinal in lane, and
// whatever else the search reports) in a pool of TILE_STAGE entries per tile.  The workgroup then scans the lane counts,
// publishes the tile's aggregate and finds its exclusive prefix by decoupled look-back over per-tile status words
// (bmx_ordered_out.h), so every parked hit goes straight to its final slot prefix + lane base + ordinal.  A tile with
// more hits than the pool walks itself a second time and writes directly.  Slots at or past the capacity are dropped:
// the stored entries are the lowest ends.
//
// A policy P has
//   Elem, TAB             the LDS table: TAB elements of type Elem ...
//   fill(tab, a, tid)     ... filled from a.peq by lane tid of TILE_BLOCK; a policy with FILL_TAKES_X = true builds its
//                         table from the further arguments instead: fill(tab, a, tid, x...)
//   walk<PASS>(a, tab, lo, hi, tile0, stage, stage_n, base, x...)
//                         one lane over the ends [lo, hi): returns the number of hits.  TILE_PARK: every hit takes a slot
//                         of the pool with atomicAdd(stage_n, ..) and, if the slot is below TILE_STAGE, parks
//                         {position in tile (low 32 bits), ordinal in lane, ...}; nothing is parked when a.out is NULL.
//                         TILE_WRITE: hit number i of the lane goes to slot base + i if that is below a.cap.
//   ordinal(e)            the ordinal in lane of the parked entry e
//   also(a, idx, e)       what the entry stores at slot idx besides its position (the approximate search: the distance)
//   ORDINAL_DESCENDS      optional, true for a policy whose lanes meet their hits in DESCENDING position (the regex begins
//                         search walks downwards): ordinal(e) then counts from the lane's highest hit, a parked hit goes to
//                         prefix + lane_base[lane + 1] - 1 - ordinal (lane_base[] gets the tile's sum as one more entry),
//                         and walk<TILE_WRITE> gets the slot one past the lane's last as `base` and writes downwards
// and x... are further by-value kernel arguments handed through to walk (the gapped search: its four mask words; the
// k-mismatch search: its `must` mask and counter bias).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>

#include "bmx_ordered_out.h"

namespace bmx {

constexpr int TILE_BLOCK = 256;  // lanes per workgroup
constexpr int TILE_STAGE = 2048; // hits parked per tile (16 KiB of LDS)

struct TileArgs {
    const uint8_t *text16; // caller's pointer rounded down to a multiple of 16
    uint64_t first;        // aligned coordinate of view byte 0 (0..15)
    uint64_t own_lo;       // first end to report (aligned coordinates: lead + first)
    uint64_t own_hi;       // one past the last (n + first)
    uint64_t out_bias;     // reported position = aligned end + out_bias
    uint64_t tile_begin;   // first tile index (aligned end / tile bytes)
    uint64_t n_tiles;
    uint64_t *out;         // positions, ascending (NULL: count only)
    uint8_t *dist;         // approximate and k-mismatch search: their distances (NULL: not wanted)
    uint64_t cap;          // entries out / dist have room for
    uint64_t *status;      // n_tiles tile words (tagged: no clearing between calls)
    unsigned long long *ticket; // monotonic across calls: this call's tickets start at ticket_base
    uint64_t ticket_base;
    uint64_t *host_status; // pinned: [0] total, [1] give-up flag, [2] seq (written by the last tile)
    uint64_t seq;
    uint64_t tag;          // seq mod 2^22 (never 0)
    uint32_t m, k, warm;   // pattern length, edits (k-mismatch search: mismatches); bytes walked in front of a lane's first end
    uint32_t p_shift;      // P = 1 << p_shift ends per lane
    uint64_t peq[256];     // the search's table, bit i for pattern position i (low word used when m <= 32)
};

typedef uint32_t tile_u32x4 __attribute__((ext_vector_type(4)));

// What a walk does with a hit: PARK it in the tile's pool (first walk) or WRITE it to its final slot (second walk of a
// dense tile, from the lane's output base).
enum TilePass { TILE_PARK = 0, TILE_WRITE = 1 };

// Wave 0: lane_base[] holds the hits of the TILE_BLOCK lanes and gets their exclusive scan.  Returns the sum.
__device__ __forceinline__ uint32_t tile_scan_counts(uint32_t *lane_base, uint32_t tid)
{
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
    return __shfl(incl, 63);
}

// P::FILL_TAKES_X, false for a policy that does not say
template <typename P, typename = void>
struct tile_fill_takes_x : std::false_type {};
template <typename P>
struct tile_fill_takes_x<P, typename std::enable_if<P::FILL_TAKES_X>::type> : std::true_type {};

// P::ORDINAL_DESCENDS, false for a policy that does not say
template <typename P, typename = void>
struct tile_ordinal_descends : std::false_type {};
template <typename P>
struct tile_ordinal_descends<P, typename std::enable_if<P::ORDINAL_DESCENDS>::type> : std::true_type {};

template <typename P, typename... X>
__global__ __launch_bounds__(TILE_BLOCK) void tile_kernel(const TileArgs a, const X... x)
{
    __shared__ typename P::Elem tab[P::TAB];
    __shared__ uint64_t stage[TILE_STAGE];
    constexpr int DESC = tile_ordinal_descends<P>::value ? 1 : 0;
    __shared__ uint32_t lane_base[TILE_BLOCK + DESC]; // hits per lane, then their exclusive scan (DESC: and their sum)
    __shared__ uint32_t stage_n;
    __shared__ uint64_t sh_tile, sh_prefix;
    const uint32_t tid = threadIdx.x;
    if constexpr (tile_fill_takes_x<P>::value) P::fill(tab, a, tid, x...);
    else P::fill(tab, a, tid);
    const uint32_t ps = a.p_shift;
    for (;;) {
        if (tid == 0) {
            sh_tile = atomicAdd(a.ticket, 1ull) - a.ticket_base; // tiles in ascending order: every predecessor is owned
            stage_n = 0;
        }
        __syncthreads(); // (also: tab, and the previous tile's last reads of the LDS are done)
        const uint64_t t = sh_tile;
        if (t >= a.n_tiles) break;
        const uint64_t tile0 = (a.tile_begin + t) << (ps + 8);
        const uint64_t lo = max(tile0 + ((uint64_t)tid << ps), a.own_lo);
        const uint64_t hi = min(tile0 + ((uint64_t)(tid + 1) << ps), a.own_hi);
        uint32_t cnt = 0;
        if (lo < hi) cnt = P::template walk<TILE_PARK>(a, tab, lo, hi, tile0, stage, &stage_n, 0, x...);
        lane_base[tid] = cnt;
        __syncthreads();
        if (tid < 64) { // wave 0: exclusive scan of the lane counts, then the look-back
            const uint64_t agg = tile_scan_counts(lane_base, tid);
            if (tid == 0) {
                const uint64_t prefix = ordered_lookback(a, t, agg);
                ordered_publish_total(a, t, prefix + agg);
                sh_prefix = prefix;
                if constexpr (DESC != 0) lane_base[TILE_BLOCK] = (uint32_t)agg;
            }
        }
        __syncthreads();
        const uint64_t prefix = sh_prefix;
        const uint32_t parked = stage_n;
        if (a.out != nullptr && prefix < a.cap) { // (a tile that starts at or past the capacity stores nothing)
            if (parked <= (uint32_t)TILE_STAGE) {
                for (uint32_t j = tid; j < parked; j += TILE_BLOCK) {
                    const uint64_t e = stage[j];
                    const uint32_t pos = (uint32_t)e;
                    const uint64_t idx = DESC ? prefix + lane_base[(pos >> ps) + 1] - 1 - P::ordinal(e)
                                              : prefix + lane_base[pos >> ps] + P::ordinal(e);
                    if (idx < a.cap) {
                        a.out[idx] = tile0 + pos + a.out_bias;
                        P::also(a, idx, e);
                    }
                }
            } else if (lo < hi) { // dense tile: walk it again, writing every hit to its slot
                (void)P::template walk<TILE_WRITE>(a, tab, lo, hi, tile0, stage, &stage_n, prefix + lane_base[tid + DESC], x...);
            }
        }
        __syncthreads(); // the pool, the lane bases and stage_n are the next tile's
    }
}

// ---- host side ----

// What a context keeps between calls of one search.  A search that keeps more has it as the FIRST member of its state.
struct TileState {
    OrderedOut oo; // (first: bmx_ordered_out.h)
    int blocks_per_cu[4] = {0, 0, 0, 0}; // resident workgroups per CU of the search's kernels, by slot (the 32- and the
                                         // 64-bit one; the long approximate search: 2, 4 and 8 words; the k-mismatch search:
                                         // two slices at 32 and 64 bits, then four)
};
static_assert(offsetof(TileState, oo) == 0, "ordered_set_seq");

// The state S behind a context's pointer, made on first use; a call starts with no matches and no kernel time.
template <typename S = TileState>
S *tile_state(void **state_v, uint64_t *n_matches)
{
    static_assert(std::is_standard_layout<S>::value, "S begins with its TileState");
    if (!*state_v) *state_v = new S();
    if (n_matches) *n_matches = 0;
    static_cast<TileState *>(*state_v)->oo.last_ms = 0.0f;
    return static_cast<S *>(*state_v);
}

inline void tile_free(TileState *st)
{
    if (!st) return;
    st->oo.free();
    delete st;
}

inline float tile_last_ms(const void *state_v)
{
    return state_v ? static_cast<const TileState *>(state_v)->oo.last_ms : -1.0f;
}

// bit i + up of peq[c]: byte c belongs to class i (reversed: to class m - 1 - i)
inline void tile_class_table(const uint8_t *classes, int32_t m, uint32_t up, bool reversed, uint64_t peq[256])
{
    for (int32_t i = 0; i < m; ++i) {
        const uint8_t *cls = classes + (size_t)(reversed ? m - 1 - i : i) * BMX_CLASS_BYTES;
        for (uint32_t c = 0; c < 256; ++c)
            if ((cls[c >> 3] >> (c & 7)) & 1u) peq[c] |= 1ull << (i + up);
    }
}

// One call of `kernel` (slot: which of the search's kernels it is, for the occupancy cache) over the ends [lead, n_ends)
// of the view at d_text, each reported as
// end + base_offset (a search that reports starts passes base_offset - lead).  piece(resident lanes) is the search's rule
// for log2 of the ends per lane.  The caller has set a.m, a.k, a.warm, a.peq and a.dist in a block that is otherwise zero;
// x... are the kernel's further arguments.
template <typename K, typename Piece, typename... X>
int tile_launch(TileState *st, const char *where, K kernel, int slot, int num_cu, TileArgs &a, const void *d_text,
                uint64_t n_ends, uint64_t lead, uint64_t base_offset, Piece piece, uint64_t *d_out, uint64_t capacity,
                uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen, const X &...x)
{
    int &bpc = st->blocks_per_cu[slot];
    if (bpc == 0) {
        BMX_HIP(where, hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kernel, TILE_BLOCK, 0));
        bpc = std::max(1, std::min(bpc, 8));
    }
    const uint64_t resident = (uint64_t)num_cu * (uint64_t)bpc * TILE_BLOCK;
    uint32_t ps = piece(resident);
#ifdef BMX_EXPERIMENTS
    if (st->oo.force_piece_shift) ps = st->oo.force_piece_shift; // libbmx_exp.so's knob "tile_piece_shift"
#endif
    const uint32_t tile_shift = ps + 8; // TILE_BLOCK lanes of 2^ps ends
    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.own_lo = lead + a.first;
    a.own_hi = n_ends + a.first;
    a.out_bias = base_offset - a.first;
    a.tile_begin = a.own_lo >> tile_shift;
    a.n_tiles = ((a.own_hi + (1ull << tile_shift) - 1) >> tile_shift) - a.tile_begin;
    a.out = capacity ? d_out : nullptr;
    a.cap = capacity;
    a.p_shift = ps;

    int rc = st->oo.begin(where, stream, a, err, errlen);
    if (rc != BMX_OK) return rc;
    uint64_t grid = std::min<uint64_t>(a.n_tiles, resident / TILE_BLOCK);
#ifdef BMX_EXPERIMENTS
    if (st->oo.force_max_grid) grid = std::min<uint64_t>(grid, st->oo.force_max_grid); // ... "tile_max_grid"
    st->oo.last_piece_shift = ps, st->oo.last_grid = grid, st->oo.last_tiles = a.n_tiles; // (bmx_exp_last_launch)
#endif
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(TILE_BLOCK), 0, stream, a, x...);
    return st->oo.finish(where, grid, a.n_tiles, stream, capacity, n_matches, err, errlen);
}

} // namespace bmx
