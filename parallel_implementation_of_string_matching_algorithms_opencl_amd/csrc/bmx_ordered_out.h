// bmx_ordered_out.h -- ordered output in one pass, shared by the tile frame of the approximate, the
// class-pattern and the gapped search (bmx_tile_frame.h) and by the dictionary search (bmx_dict_kernel.h): tiles are
// handed out in ascending order by an atomic ticket, every tile publishes its count in a tagged status word and finds its
// exclusive prefix by decoupled look-back, the last tile writes the total to pinned memory.  Device side: the status word
// and the look-back.  Host side: what a context keeps between calls for it and the two halves of a call around the
// feature's own launch.
//
// The argument block of a kernel that uses it (TileArgs, DictArgs) has the fields
//   uint64_t *status;            n_tiles tile words (tagged: no clearing between calls)
//   unsigned long long *ticket;  monotonic across calls: this call's tickets start at ticket_base
//   uint64_t ticket_base;
//   uint64_t *host_status;       pinned: [0] total, [1] give-up flag, [2] seq (written by the last tile)
//   uint64_t seq, tag;           tag = seq mod 2^22 (never 0)
//   uint64_t n_tiles;
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include "bmx_internal.h"

namespace bmx {

// Per-tile status word: [63:42] epoch tag (the call's sequence number mod 2^22, never 0), [41:40] kind, [39:0] value.
constexpr uint32_t ORDERED_TAG_SHIFT = 42;
constexpr uint64_t ORDERED_TAG_MASK = (1ull << 22) - 1;
constexpr uint64_t ORDERED_KIND_AGG = 1, ORDERED_KIND_PREFIX = 2;
constexpr uint64_t ORDERED_VALUE_MASK = (1ull << 40) - 1;

__device__ __forceinline__ uint64_t ordered_load_status(uint64_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ordered_store_status(uint64_t *p, uint64_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The look-back of one tile, called by one lane of the workgroup that holds tile t: publishes the tile's aggregate,
// finds the exclusive prefix over the status words of tiles t - 1 .. 0 and publishes the inclusive one.  Tiles
// t - 1 .. 0 were handed out before this one, so each is owned by a running workgroup and publishes.  The bound (~1 s)
// only keeps a wave from spinning for ever: a waiter that reaches it raises the give-up word (the host returns
// BMX_ERR_HIP, never this list) and goes on.  Returns the prefix; the caller follows with ordered_publish_total().
template <typename Args>
__device__ __forceinline__ uint64_t ordered_lookback(const Args &a, uint64_t t, uint64_t agg)
{
    const uint64_t tagbits = a.tag << ORDERED_TAG_SHIFT;
    uint64_t prefix = 0;
    if (t == 0) {
        ordered_store_status(&a.status[0], tagbits | (ORDERED_KIND_PREFIX << 40) | agg);
    } else {
        ordered_store_status(&a.status[t], tagbits | (ORDERED_KIND_AGG << 40) | agg);
        uint64_t i = t - 1;
        uint32_t spins = 0;
        for (;;) {
            const uint64_t w = ordered_load_status(&a.status[i]);
            const uint64_t kind = (w >> 40) & 3u;
            if ((w >> ORDERED_TAG_SHIFT) != a.tag || kind == 0) {
                if (++spins > (1u << 24)) {
                    __hip_atomic_store(&a.host_status[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
                continue;
            }
            prefix += w & ORDERED_VALUE_MASK;
            if (kind == ORDERED_KIND_PREFIX || i == 0) break;
            --i;
        }
        ordered_store_status(&a.status[t], tagbits | (ORDERED_KIND_PREFIX << 40) | ((prefix + agg) & ORDERED_VALUE_MASK));
    }
    return prefix;
}

// The last tile's inclusive prefix is the call's total: to pinned memory, then the sequence number behind it.
template <typename Args>
__device__ __forceinline__ void ordered_publish_total(const Args &a, uint64_t t, uint64_t inclusive)
{
    if (t == a.n_tiles - 1) {
        __hip_atomic_store(&a.host_status[0], inclusive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&a.host_status[2], a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// What a context keeps between calls.  A feature's state holds it as its FIRST member (ordered_set_seq() reaches it
// through the context's untyped pointer).
struct OrderedOut {
    uint64_t *d_status = nullptr; // per-tile look-back words, tagged with the call's epoch (cleared only when allocated
    uint64_t status_cap = 0;      // and when the 22-bit tag wraps)
    unsigned long long *d_ticket = nullptr; // monotonic: a call hands out n_tiles + grid tickets
    uint64_t ticket_base = 0;
    uint64_t *h_status = nullptr; // pinned, device-visible: {total, give-up, seq}
    uint64_t *h_status_dev = nullptr;
    uint64_t seq = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = -1.0f;
#ifdef BMX_EXPERIMENTS
    uint32_t force_piece_shift = 0; // libbmx_exp.so's knob "tile_piece_shift": 0, or log2 of the ends per lane of every call
    uint32_t force_max_grid = 0;    // ... "tile_max_grid": 0, or the most workgroups a call starts
    uint32_t last_piece_shift = 0;  // what the last launch ran with (bmx_exp_last_launch): log2 of the ends per lane,
    uint64_t last_grid = 0, last_tiles = 0; // its workgroups and its tiles
#endif

    void free()
    {
        if (d_status) (void)hipFree(d_status);
        if (d_ticket) (void)hipFree(d_ticket);
        if (h_status) (void)hipHostFree(h_status);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }

    // In front of the launch: allocates on first use, grows the status words, takes the call's sequence number, fills
    // the argument block's ordered-output fields (a.n_tiles is the caller's) and records the start event.  Everything
    // cleared here is cleared on `stream`, in front of the kernel that reads it.
    template <typename Args>
    int begin(const char *where, hipStream_t stream, Args &a, char *err, size_t errlen)
    {
        if (!d_ticket) {
            BMX_HIP(where, hipMalloc(&d_ticket, sizeof(unsigned long long)));
            BMX_HIP(where, hipMemsetAsync(d_ticket, 0, sizeof(unsigned long long), stream));
            ticket_base = 0;
        }
        if (!h_status) {
            BMX_HIP(where, hipHostMalloc(&h_status, 4 * sizeof(uint64_t), hipHostMallocMapped));
            std::memset(h_status, 0, 4 * sizeof(uint64_t));
            BMX_HIP(where, hipHostGetDevicePointer((void **)&h_status_dev, h_status, 0));
        }
        if (!ev0) BMX_HIP(where, hipEventCreate(&ev0));
        if (!ev1) BMX_HIP(where, hipEventCreate(&ev1));
        if (a.n_tiles > status_cap) {
            if (d_status) (void)hipFree(d_status);
            d_status = nullptr;
            status_cap = 0;
            const uint64_t cap = std::max<uint64_t>(a.n_tiles, 1024);
            BMX_HIP(where, hipMalloc(&d_status, cap * sizeof(uint64_t)));
            BMX_HIP(where, hipMemsetAsync(d_status, 0, cap * sizeof(uint64_t), stream)); // tag 0 is never a call's
            status_cap = cap;
        }
        ++seq;
        if ((seq & ORDERED_TAG_MASK) == 0) { // the tag wraps: old words could carry this call's tag
            BMX_HIP(where, hipMemsetAsync(d_status, 0, status_cap * sizeof(uint64_t), stream));
            ++seq;
        }
        a.status = d_status;
        a.ticket = d_ticket;
        a.ticket_base = ticket_base;
        a.host_status = h_status_dev;
        a.seq = seq;
        a.tag = seq & ORDERED_TAG_MASK;
        h_status[0] = h_status[1] = h_status[2] = 0;
        BMX_HIP(where, hipEventRecord(ev0, stream));
        return BMX_OK;
    }

    // Behind the launch of `grid` workgroups over n_tiles tiles: waits for the stream and reads the pinned words.
    int finish(const char *where, uint64_t grid, uint64_t n_tiles, hipStream_t stream, uint64_t capacity,
               uint64_t *n_matches, char *err, size_t errlen)
    {
        BMX_HIP(where, hipGetLastError());
        BMX_HIP(where, hipEventRecord(ev1, stream));
        BMX_HIP(where, hipStreamSynchronize(stream));
        ticket_base += n_tiles + grid; // every workgroup draws one ticket past the last tile
        (void)hipEventElapsedTime(&last_ms, ev0, ev1);

        volatile uint64_t *hs = h_status;
        if (hs[2] != seq) {
            snprintf(err, errlen, "%s: the kernel did not report its total (seq %llu, want %llu)", where,
                     (unsigned long long)hs[2], (unsigned long long)seq);
            return BMX_ERR_HIP;
        }
        if (hs[1] != 0) {
            snprintf(err, errlen, "%s: a tile waited longer than its bound for its predecessors' counts; result discarded",
                     where);
            return BMX_ERR_HIP;
        }
        const uint64_t total = hs[0];
        if (n_matches) *n_matches = total;
        return total > capacity ? BMX_ERR_CAPACITY : BMX_OK;
    }
};

// libbmx_exp.so's knob "ordered_seq": the next call of this session takes seq + 1 (tests reach the tag's wrap with it).
inline void ordered_set_seq(void *state, uint64_t seq)
{
    if (state) static_cast<OrderedOut *>(state)->seq = seq;
}

#ifdef BMX_EXPERIMENTS
constexpr uint32_t ORDERED_DICT_MAX_PIECE_SHIFT = 11; // the dictionary search: 6 + DICT_MAX_ROUNDS_SHIFT (bmx_dict.hip asserts it)

// ... "tile_piece_shift" and "tile_max_grid": the geometry of this session's calls from now on (0: the production rule's).
// A small grid cannot stall the look-back: tickets go out in ascending order and a workgroup holds one tile at a time, so
// every tile below a waiting one is held by a running workgroup or is published already.
inline void ordered_set_piece_shift(void *state, uint32_t ps)
{
    if (state) static_cast<OrderedOut *>(state)->force_piece_shift = ps;
}
inline void ordered_set_max_grid(void *state, uint32_t grid)
{
    if (state) static_cast<OrderedOut *>(state)->force_max_grid = grid;
}
// ... bmx_exp_last_launch: {piece shift, workgroups, tiles} of the session's last launch (zeros before the first)
inline void ordered_last_launch(const void *state, uint64_t out3[3])
{
    const OrderedOut *oo = static_cast<const OrderedOut *>(state);
    out3[0] = oo ? oo->last_piece_shift : 0;
    out3[1] = oo ? oo->last_grid : 0;
    out3[2] = oo ? oo->last_tiles : 0;
}
#endif

} // namespace bmx
