// bmx_classes.hip -- host side of the class-pattern search (bmx_search_classes_device, include/bmx.h): builds the
// Shift-And table from the classes, picks the word width and the lane piece and launches bmx_classes_kernel.h's policy
// through the tile frame (bmx_tile_frame.h: state, geometry, the ordered-output call around the launch), in end
// coordinates.  The argument checks and the context are the shim's (bmx_shim.hip); everything here runs on a valid context
// with valid arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "bmx.h"
#include "bmx_classes_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::MAX_CLASS_PATTERN == BMX_MAX_CLASS_PATTERN, "header and kernel disagree");

// Ends per lane: about n / (resident lanes), as a power of two in [64, 2048], and at least four patterns (the warm-up of
// m - 1 bytes per piece is overhead).  From 128 on a piece is whole 128-byte lines of the text.
uint32_t bmx_internal_classes_piece_shift(uint64_t n, int32_t m, uint64_t resident_lanes)
{
    const uint64_t per = (n + resident_lanes - 1) / std::max<uint64_t>(resident_lanes, 1);
    uint32_t ps = std::min<uint32_t>(std::max<uint32_t>(bmx::ceil_log2(per), 6), 11);
    ps = std::max<uint32_t>(ps, bmx::ceil_log2(4ull * (uint64_t)m));
    return ps;
}

void bmx_internal_classes_free(void *state_v) { bmx::tile_free(static_cast<bmx::TileState *>(state_v)); }

float bmx_internal_classes_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }

int bmx_internal_classes(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                         const uint8_t *classes, int32_t m, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches,
                         hipStream_t stream, char *err, size_t errlen)
{
    bmx::TileState *st = bmx::tile_state(state_v, n_matches);
    // In end coordinates: start p is end p + m - 1, so the ends to report are [m - 1, min(n, n_own + m - 1)).
    const uint64_t lead = (uint64_t)m - 1;
    const uint64_t n_ends = n_own >= n ? n : std::min<uint64_t>(n, n_own + lead);
    if (lead >= n_ends) return BMX_OK; // no window fits or none is owned (before anything is put on `stream`)
    const bool wide = m > 32;
    void (*kernel)(const bmx::TileArgs) = wide ? bmx::tile_kernel<bmx::ShiftAndPolicy<true, bmx::ClassesStep<true>>>
                                               : bmx::tile_kernel<bmx::ShiftAndPolicy<false, bmx::ClassesStep<false>>>;
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.m = (uint32_t)m;
    a.warm = (uint32_t)lead;
    // B[c]: bit i set iff c is in class i, shifted up so that bit m - 1 is the top bit of the lane's word
    bmx::tile_class_table(classes, m, (wide ? 64u : 32u) - (uint32_t)m, false, a.peq);
    const auto piece = [&](uint64_t resident) { return bmx_internal_classes_piece_shift(n_ends, m, resident); };
    return bmx::tile_launch(st, "bmx_search_classes_device", kernel, wide ? 1 : 0, num_cu, a, d_text, n_ends, lead,
                            base_offset - lead /* reported: the start */, piece, d_starts, capacity, n_matches, stream, err, errlen);
}
