// bmx_gaps.hip -- host side of the gapped pattern search (bmx_search_gaps_device, bmx_gaps_starts_device,
// include/bmx.h): builds the Shift-And table and the four mask words of the extended recurrence from the classes and the
// optional positions, picks the word width and the lane piece and launches bmx_gaps_kernel.h's policy through the tile
// frame (bmx_tile_frame.h: state, geometry, the ordered-output call around the launch); for the starts it builds the same
// for the reversed positions and launches one lane per list entry.  The argument checks and the context are the shim's
// (bmx_shim.hip); everything here runs on a valid context with valid arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "bmx.h"
#include "bmx_gaps_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::MAX_GAPS_PATTERN == BMX_MAX_GAPS_PATTERN, "header and kernel disagree");
static_assert(sizeof(bmx::TileArgs) + sizeof(bmx::GapsMasks) <= 4096 && sizeof(bmx::GapsStartsArgs) <= 4096, "kernel arguments");

namespace {

constexpr const char *WHERE = "bmx_search_gaps_device";
constexpr const char *WHERE_STARTS = "bmx_gaps_starts_device";

struct GapsState {
    bmx::TileState tile; // (first: bmx_tile_frame.h)
    uint64_t *d_ws = nullptr; // the starts pass: its status word ...
    uint64_t *h_ws = nullptr; // ... and the pinned copy of it
};
static_assert(offsetof(GapsState, tile) == 0, "tile_state, ordered_set_seq");

// O, I, F, S for positions 0..m-1 with the optional ones in `optional`, shifted up by `up` bits.
bmx::GapsMasks gaps_masks(uint64_t optional, int32_t m, uint32_t up)
{
    const auto is_opt = [&](int32_t i) { return i >= 0 && i < m && ((optional >> i) & 1u); };
    bmx::GapsMasks k = {0, 0, 0, 0};
    for (int32_t i = 0; i < m; ++i) {
        if (!is_opt(i)) continue;
        k.opt |= 1ull << i;
        if (!is_opt(i - 1)) k.below |= 1ull << (i == 0 ? 0 : i - 1); // the block starts here
        if (!is_opt(i + 1)) k.last |= 1ull << i;                     // ... and ends here
    }
    int32_t b = 0; // the first mandatory position (the shim has checked that there is one)
    while (is_opt(b)) ++b;
    k.seed = b >= 63 ? ~0ull : (1ull << (b + 1)) - 1;
    k.opt <<= up, k.below <<= up, k.last <<= up, k.seed <<= up;
    return k;
}

} // namespace

void bmx_internal_gaps_free(void *state_v)
{
    GapsState *st = static_cast<GapsState *>(state_v);
    if (!st) return;
    st->tile.oo.free();
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    delete st;
}

float bmx_internal_gaps_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }

int bmx_internal_gaps(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                      const uint8_t *classes, int32_t m, uint64_t optional, uint64_t *d_ends, uint64_t capacity,
                      uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    GapsState *st = bmx::tile_state<GapsState>(state_v, n_matches);
    if (lead >= n) return BMX_OK; // no end is owned (before anything is put on `stream`)
    const bool wide = m > 32;
    void (*kernel)(const bmx::TileArgs, const bmx::GapsMasks) =
        wide ? bmx::tile_kernel<bmx::ShiftAndPolicy<true, bmx::GapsStep<true>>, bmx::GapsMasks>
             : bmx::tile_kernel<bmx::ShiftAndPolicy<false, bmx::GapsStep<false>>, bmx::GapsMasks>;
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.m = (uint32_t)m;
    a.warm = (uint32_t)m - 1;
    const uint32_t up = (wide ? 64u : 32u) - (uint32_t)m; // bit m - 1 is the top bit of the lane's word
    bmx::tile_class_table(classes, m, up, false, a.peq);
    const bmx::GapsMasks k = gaps_masks(optional, m, up);
    const auto piece = [&](uint64_t resident) { return bmx_internal_classes_piece_shift(n - lead, m, resident); };
    return bmx::tile_launch(&st->tile, WHERE, kernel, wide ? 1 : 0, num_cu, a, d_text, n, lead, base_offset, piece, d_ends, capacity, n_matches,
                            stream, err, errlen, k);
}

// count >= 1: d_starts[i] for d_ends[i].
int bmx_internal_gaps_starts(void **state_v, const void *d_text, uint64_t n, uint64_t base_offset, const uint8_t *classes,
                             int32_t m, uint64_t optional, const uint64_t *d_ends, uint64_t count, uint32_t flags,
                             uint64_t *d_starts, hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new GapsState();
    GapsState *st = static_cast<GapsState *>(*state_v);
    const uint64_t n_blocks = (count + bmx::GAPS_STARTS_BLOCK - 1) / bmx::GAPS_STARTS_BLOCK;
    if (n_blocks > 0x7fffffffull) {
        snprintf(err, errlen, "bmx_gaps_starts_device: more than 2^31 workgroups of list entries in one call");
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(WHERE_STARTS, hipMalloc(&st->d_ws, sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE_STARTS, hipHostMalloc(&st->h_ws, sizeof(uint64_t), hipHostMallocDefault));
    BMX_HIP(WHERE_STARTS, hipMemsetAsync(st->d_ws, 0, sizeof(uint64_t), stream)); // the status word starts clean in every call

    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::GapsStartsArgs a;
    std::memset(&a, 0, sizeof a);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.n = n;
    a.base = base_offset;
    a.ends = d_ends;
    a.count = count;
    a.starts = d_starts;
    a.ws = st->d_ws;
    a.m = (uint32_t)m;
    a.chunks = (uint32_t)(m + 7) / 8;
    a.longest = (flags & BMX_GAPS_LONGEST) ? 1u : 0u;
    // the REVERSED positions: bit i stands for position m - 1 - i, and so do the optional ones
    const bool wide = m > 32;
    const uint32_t up = (wide ? 64u : 32u) - (uint32_t)m;
    uint64_t reversed = 0;
    for (int32_t i = 0; i < m; ++i)
        if ((optional >> (m - 1 - i)) & 1u) reversed |= 1ull << i;
    bmx::tile_class_table(classes, m, up, true, a.peq);
    a.k = gaps_masks(reversed, m, up);
    void (*kernel)(const bmx::GapsStartsArgs) = wide ? bmx::gaps_starts_kernel<uint64_t> : bmx::gaps_starts_kernel<uint32_t>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(bmx::GAPS_STARTS_BLOCK), 0, stream, a);
    BMX_HIP(WHERE_STARTS, hipGetLastError());
    BMX_HIP(WHERE_STARTS, hipMemcpyAsync(st->h_ws, st->d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE_STARTS, hipStreamSynchronize(stream));

    const uint64_t bad = st->h_ws[0];
    if (bad != 0) {
        snprintf(err, errlen, "bmx_gaps_starts_device: %s%s", bad & bmx::GAPS_BAD_END ? "an end outside the view; " : "",
                 bad & bmx::GAPS_BAD_START ? "an end at which no match of this pattern ends; " : "");
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}
