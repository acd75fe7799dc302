// bmx_classes.hip -- host side of the class-pattern search (bmx_search_classes_device, include/bmx.h): builds the
// Shift-And table from the classes, picks the word width and the lane piece and launches bmx_classes_kernel.h once inside
// an ordered-output call (bmx_ordered_out.h: status words, ticket, pinned result words, the wait for the stream).  The
// argument checks and the context are the shim's (bmx_shim.hip); everything here runs on a valid context with valid
// arguments.  The shape is bmx_approx.hip's: the kernel takes the same argument block, in end coordinates.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "bmx.h"
#include "bmx_classes_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::MAX_CLASS_PATTERN == BMX_MAX_CLASS_PATTERN, "header and kernel disagree");

namespace {

constexpr const char *WHERE = "bmx_search_classes_device";

struct ClassesState {
    bmx::OrderedOut oo; // (first: bmx_ordered_out.h)
    int blocks_per_cu[2] = {0, 0}; // resident workgroups per CU of the 32- and the 64-bit kernel
};
static_assert(offsetof(ClassesState, oo) == 0, "ordered_set_seq");

} // namespace

// Ends per lane: about n / (resident lanes), as a power of two in [64, 2048], and at least four patterns (the warm-up of
// m - 1 bytes per piece is overhead).  From 128 on a piece is whole 128-byte lines of the text.
uint32_t bmx_internal_classes_piece_shift(uint64_t n, int32_t m, uint64_t resident_lanes)
{
    const uint64_t per = (n + resident_lanes - 1) / std::max<uint64_t>(resident_lanes, 1);
    uint32_t ps = std::min<uint32_t>(std::max<uint32_t>(bmx::ceil_log2(per), 6), 11);
    ps = std::max<uint32_t>(ps, bmx::ceil_log2(4ull * (uint64_t)m));
    return ps;
}

void bmx_internal_classes_free(void *state_v)
{
    ClassesState *st = static_cast<ClassesState *>(state_v);
    if (!st) return;
    st->oo.free();
    delete st;
}

float bmx_internal_classes_ms(const void *state_v)
{
    const ClassesState *st = static_cast<const ClassesState *>(state_v);
    return st ? st->oo.last_ms : -1.0f;
}

int bmx_internal_classes(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                         const uint8_t *classes, int32_t m, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches,
                         hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new ClassesState();
    ClassesState *st = static_cast<ClassesState *>(*state_v);
    if (n_matches) *n_matches = 0;
    st->oo.last_ms = 0.0f;
    // In end coordinates: start p is end p + m - 1, so the ends to report are [m - 1, min(n, n_own + m - 1)).
    const uint64_t lead = (uint64_t)m - 1;
    const uint64_t n_ends = n_own >= n ? n : std::min<uint64_t>(n, n_own + lead);
    if (lead >= n_ends) return BMX_OK; // no window fits or none is owned (before anything is put on `stream`)
    const bool wide = m > 32;
    void (*kernel)(const bmx::ApproxArgs) = wide ? bmx::classes_kernel<true> : bmx::classes_kernel<false>;
    int &bpc = st->blocks_per_cu[wide ? 1 : 0];
    if (bpc == 0) {
        BMX_HIP(WHERE, hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kernel, bmx::CLASSES_BLOCK, 0));
        bpc = std::max(1, std::min(bpc, 8));
    }

    const uint64_t resident = (uint64_t)num_cu * (uint64_t)bpc * bmx::CLASSES_BLOCK;
    const uint32_t ps = bmx_internal_classes_piece_shift(n_ends, m, resident);
    const uint32_t tile_shift = ps + 8; // CLASSES_BLOCK lanes of 2^ps ends
    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::ApproxArgs a;
    std::memset(&a, 0, sizeof a);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.own_lo = lead + a.first;
    a.own_hi = n_ends + a.first;
    a.out_bias = base_offset - a.first - lead; // reported start = aligned end + out_bias
    a.tile_begin = a.own_lo >> tile_shift;
    a.n_tiles = ((a.own_hi + (1ull << tile_shift) - 1) >> tile_shift) - a.tile_begin;
    a.out = capacity ? d_starts : nullptr;
    a.cap = capacity;
    a.m = (uint32_t)m;
    a.warm = (uint32_t)lead;
    a.p_shift = ps;
    // B[c]: bit i set iff c is in class i, shifted up so that bit m - 1 is the top bit of the lane's word
    const uint32_t up = (wide ? 64u : 32u) - (uint32_t)m;
    for (int32_t i = 0; i < m; ++i)
        for (uint32_t c = 0; c < 256; ++c)
            if ((classes[(size_t)i * BMX_CLASS_BYTES + (c >> 3)] >> (c & 7)) & 1u) a.peq[c] |= 1ull << (i + up);

    int rc = st->oo.begin(WHERE, stream, a, err, errlen);
    if (rc != BMX_OK) return rc;
    const uint64_t grid = std::min<uint64_t>(a.n_tiles, resident / bmx::CLASSES_BLOCK);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(bmx::CLASSES_BLOCK), 0, stream, a);
    return st->oo.finish(WHERE, grid, a.n_tiles, stream, capacity, n_matches, err, errlen);
}
