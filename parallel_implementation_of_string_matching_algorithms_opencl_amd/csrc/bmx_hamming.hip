// bmx_hamming.hip -- host side of the k-mismatch search (bmx_search_hamming_device, include/bmx.h): builds the mismatch
// table M from the string or the classes, picks the word width, the number of counter slices and the lane piece and
// launches bmx_hamming_kernel.h's policy through the tile frame (bmx_tile_frame.h: state, geometry, the ordered-output
// call around the launch), in end coordinates.  The argument checks and the context are the shim's (bmx_shim.hip);
// everything here runs on a valid context with valid arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "bmx.h"
#include "bmx_hamming_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::MAX_HAMMING_PATTERN == BMX_MAX_HAMMING_PATTERN && bmx::MAX_HAMMING_K == BMX_MAX_HAMMING_K,
              "header and kernel disagree");
static_assert(sizeof(bmx::TileArgs) + sizeof(bmx::HammingConsts) <= 4096, "kernel arguments");

void bmx_internal_hamming_free(void *state_v) { bmx::tile_free(static_cast<bmx::TileState *>(state_v)); }

float bmx_internal_hamming_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }

int bmx_internal_hamming(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                         const char *pat, const uint8_t *classes, int32_t m, int32_t k, uint64_t must, uint64_t *d_starts,
                         uint8_t *d_dist, uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    bmx::TileState *st = bmx::tile_state(state_v, n_matches);
    // In end coordinates: start p is end p + m - 1, so the ends to report are [m - 1, min(n, n_own + m - 1)).
    const uint64_t lead = (uint64_t)m - 1;
    const uint64_t n_ends = n_own >= n ? n : std::min<uint64_t>(n, n_own + lead);
    if (lead >= n_ends) return BMX_OK; // no window fits or none is owned (before anything is put on `stream`)
    const bool wide = m > 32;
    const bool four = k > 3; // two slices count to 3, four to 15
    typedef void (*Kernel)(const bmx::TileArgs, const bmx::HammingConsts);
    static const Kernel kernels[4] = {bmx::tile_kernel<bmx::HammingPolicy<false, 2>, bmx::HammingConsts>,
                                      bmx::tile_kernel<bmx::HammingPolicy<true, 2>, bmx::HammingConsts>,
                                      bmx::tile_kernel<bmx::HammingPolicy<false, 4>, bmx::HammingConsts>,
                                      bmx::tile_kernel<bmx::HammingPolicy<true, 4>, bmx::HammingConsts>};
    const int slot = (four ? 2 : 0) + (wide ? 1 : 0);
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.dist = capacity ? d_dist : nullptr;
    a.m = (uint32_t)m;
    a.k = (uint32_t)k;
    a.warm = (uint32_t)lead;
    // M[c]: bit i set iff c is NOT in class i, shifted up so that bit m - 1 is the top bit of the lane's word
    const uint32_t up = (wide ? 64u : 32u) - (uint32_t)m;
    if (pat) { // a string: position i holds one byte value
        for (int32_t i = 0; i < m; ++i) a.peq[(uint8_t)pat[i]] |= 1ull << (i + up);
    } else {
        bmx::tile_class_table(classes, m, up, false, a.peq);
    }
    const uint64_t positions = (m == 64 ? ~0ull : (1ull << m) - 1) << up;
    for (uint32_t c = 0; c < 256; ++c) a.peq[c] = ~a.peq[c] & positions;
    bmx::HammingConsts consts;
    consts.must = must << up;
    consts.bias = (four ? 15u : 3u) - (uint32_t)k;
    const auto piece = [&](uint64_t resident) { return bmx_internal_classes_piece_shift(n_ends, m, resident); };
    return bmx::tile_launch(st, "bmx_search_hamming_device", kernels[slot], slot, num_cu, a, d_text, n_ends, lead,
                            base_offset - lead /* reported: the start */, piece, d_starts, capacity, n_matches, stream, err, errlen,
                            consts);
}
