// bmx_approx.hip -- host side of the approximate search (bmx_search_approx_device, include/bmx.h): picks the word
// width and the lane piece, builds the Peq table and launches bmx_approx_kernel.h's policy through the tile frame
// (bmx_tile_frame.h: state, geometry, the ordered-output call around the launch).  The argument checks and the context are
// the shim's (bmx_shim.hip); everything here runs on a valid context with valid arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "bmx.h"
#include "bmx_approx_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::MAX_APPROX_PATTERN == BMX_MAX_APPROX_PATTERN, "header and kernel disagree");
static_assert(sizeof(bmx::TileArgs) <= 4096, "kernel arguments");

// Ends per lane: about n / (resident lanes), as a power of two in [64, 2048], and at least four warm-ups.  Small texts
// get short pieces (parallelism), large ones long pieces (the warm-up of m + k - 1 bytes per piece is overhead).
uint32_t bmx_internal_approx_piece_shift(uint64_t n, int32_t m, int32_t k, uint64_t resident_lanes)
{
    const uint64_t per = (n + resident_lanes - 1) / std::max<uint64_t>(resident_lanes, 1);
    uint32_t ps = std::min<uint32_t>(std::max<uint32_t>(bmx::ceil_log2(per), 6), 11);
    ps = std::max<uint32_t>(ps, std::min<uint32_t>(bmx::ceil_log2(4ull * (uint64_t)(m + k)), 11));
    return ps;
}

void bmx_internal_approx_free(void *state_v) { bmx::tile_free(static_cast<bmx::TileState *>(state_v)); }

float bmx_internal_approx_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }

int bmx_internal_approx(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                        const char *pat, const uint8_t *classes, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist,
                        uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    bmx::TileState *st = bmx::tile_state(state_v, n_matches);
    if (lead >= n) return BMX_OK; // no end to report (before anything is put on `stream`)
    const bool wide = m > 32;
    void (*kernel)(const bmx::TileArgs) =
        wide ? bmx::tile_kernel<bmx::ApproxPolicy<uint64_t>> : bmx::tile_kernel<bmx::ApproxPolicy<uint32_t>>;
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.dist = capacity ? d_dist : nullptr;
    a.m = (uint32_t)m;
    a.k = (uint32_t)k;
    a.warm = (uint32_t)(m + k - 1);
    if (pat) { // a string: position i holds one byte value
        for (int32_t i = 0; i < m; ++i) a.peq[(uint8_t)pat[i]] |= 1ull << i;
    } else { // classes (bmx_search_approx_classes_device): bit i = "the byte belongs to class i"
        bmx::tile_class_table(classes, m, 0, false, a.peq);
    }
    const auto piece = [&](uint64_t resident) { return bmx_internal_approx_piece_shift(n, m, k, resident); };
    return bmx::tile_launch(st, "bmx_search_approx_device", kernel, wide ? 1 : 0, num_cu, a, d_text, n, lead, base_offset, piece, d_ends,
                            capacity, n_matches, stream, err, errlen);
}
