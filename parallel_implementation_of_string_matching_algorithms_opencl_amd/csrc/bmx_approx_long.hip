// bmx_approx_long.hip -- host side of the approximate search for patterns of 65 to 512 bytes
// (bmx_search_approx_long_device, include/bmx.h): picks the word count and the lane piece, hands the pattern over as a
// kernel argument and launches bmx_approx_long_kernel.h's policy through the tile frame (bmx_tile_frame.h).  The argument
// checks, the context and the hand-over of m <= 64 to the one-word kernels are the shim's (bmx_shim.hip); everything here
// runs on a valid context with valid arguments and 64 < m <= 512.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "bmx.h"
#include "bmx_approx_long_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::MAX_APPROX_LONG_PATTERN == BMX_MAX_APPROX_LONG_PATTERN, "header and kernel disagree");
static_assert(sizeof(bmx::TileArgs) + sizeof(bmx::LongPattern) <= 4096, "kernel arguments");

// Ends per lane, the rule of bmx_internal_approx_piece_shift with its cap at 2^12: about n / (resident lanes), as a power of
// two in [64, 4096], and at least four warm-ups (m + k <= 767: 4096 ends).  A tile is 256 lanes of that many ends.
uint32_t bmx_internal_approx_long_piece_shift(uint64_t n, int32_t m, int32_t k, uint64_t resident_lanes)
{
    const uint64_t per = (n + resident_lanes - 1) / std::max<uint64_t>(resident_lanes, 1);
    uint32_t ps = std::min<uint32_t>(std::max<uint32_t>(bmx::ceil_log2(per), 6), 12);
    ps = std::max<uint32_t>(ps, std::min<uint32_t>(bmx::ceil_log2(4ull * (uint64_t)(m + k)), 12));
    return ps;
}

void bmx_internal_approx_long_free(void *state_v) { bmx::tile_free(static_cast<bmx::TileState *>(state_v)); }

float bmx_internal_approx_long_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }

int bmx_internal_approx_long(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                             const char *pat, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist, uint64_t capacity,
                             uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    bmx::TileState *st = bmx::tile_state(state_v, n_matches); // (its occupancy slots: W = 2, 4, 8)
    if (lead >= n) return BMX_OK; // no end to report (before anything is put on `stream`)
    const int W = bmx::words_for(m);
    void (*kernel)(const bmx::TileArgs, const bmx::LongPattern) =
        W == 2 ? bmx::tile_kernel<bmx::ApproxLongPolicy<2>, bmx::LongPattern>
               : W == 4 ? bmx::tile_kernel<bmx::ApproxLongPolicy<4>, bmx::LongPattern>
                        : bmx::tile_kernel<bmx::ApproxLongPolicy<8>, bmx::LongPattern>;
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.dist = capacity ? d_dist : nullptr;
    a.m = (uint32_t)m;
    a.k = (uint32_t)k;
    a.warm = (uint32_t)(m + k - 1);
    bmx::LongPattern p;
    std::memset(&p, 0, sizeof p);
    std::memcpy(p.w, pat, (size_t)m);
    const auto piece = [&](uint64_t resident) { return bmx_internal_approx_long_piece_shift(n, m, k, resident); };
    return bmx::tile_launch(st, "bmx_search_approx_long_device", kernel, W == 2 ? 0 : W == 4 ? 1 : 2, num_cu, a, d_text, n, lead,
                            base_offset, piece, d_ends, capacity, n_matches, stream, err, errlen, p);
}
