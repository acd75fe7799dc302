// bmx_approx.hip -- host side of the approximate search (bmx_search_approx_device, include/bmx.h): picks the word
// width and the lane piece, builds the Peq table and launches bmx_approx_kernel.h once inside an ordered-output call
// (bmx_ordered_out.h: status words, ticket, pinned result words, the wait for the stream).  The argument checks and the
// context are the shim's (bmx_shim.hip); everything here runs on a valid context with valid arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "bmx.h"
#include "bmx_approx_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::MAX_APPROX_PATTERN == BMX_MAX_APPROX_PATTERN, "header and kernel disagree");
static_assert(sizeof(bmx::ApproxArgs) <= 4096, "kernel arguments");

namespace {

constexpr const char *WHERE = "bmx_search_approx_device";

struct ApproxState {
    bmx::OrderedOut oo; // (first: bmx_ordered_out.h)
    int blocks_per_cu[2] = {0, 0}; // resident workgroups per CU of the 32- and the 64-bit kernel
};
static_assert(offsetof(ApproxState, oo) == 0, "ordered_set_seq");

} // namespace

// Ends per lane: about n / (resident lanes), as a power of two in [64, 2048], and at least four warm-ups.  Small texts
// get short pieces (parallelism), large ones long pieces (the warm-up of m + k - 1 bytes per piece is overhead).
uint32_t bmx_internal_approx_piece_shift(uint64_t n, int32_t m, int32_t k, uint64_t resident_lanes)
{
    const uint64_t per = (n + resident_lanes - 1) / std::max<uint64_t>(resident_lanes, 1);
    uint32_t ps = std::min<uint32_t>(std::max<uint32_t>(bmx::ceil_log2(per), 6), 11);
    ps = std::max<uint32_t>(ps, std::min<uint32_t>(bmx::ceil_log2(4ull * (uint64_t)(m + k)), 11));
    return ps;
}

void bmx_internal_approx_free(void *state_v)
{
    ApproxState *st = static_cast<ApproxState *>(state_v);
    if (!st) return;
    st->oo.free();
    delete st;
}

float bmx_internal_approx_ms(const void *state_v)
{
    const ApproxState *st = static_cast<const ApproxState *>(state_v);
    return st ? st->oo.last_ms : -1.0f;
}

int bmx_internal_approx(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                        const char *pat, const uint8_t *classes, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist,
                        uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new ApproxState();
    ApproxState *st = static_cast<ApproxState *>(*state_v);
    if (n_matches) *n_matches = 0;
    st->oo.last_ms = 0.0f;
    if (lead >= n) return BMX_OK; // no end to report (before anything is put on `stream`)
    const bool wide = m > 32;
    void (*kernel)(const bmx::ApproxArgs) = wide ? bmx::approx_kernel<uint64_t> : bmx::approx_kernel<uint32_t>;
    int &bpc = st->blocks_per_cu[wide ? 1 : 0];
    if (bpc == 0) {
        BMX_HIP(WHERE, hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kernel, bmx::APPROX_BLOCK, 0));
        bpc = std::max(1, std::min(bpc, 8));
    }

    const uint64_t resident = (uint64_t)num_cu * (uint64_t)bpc * bmx::APPROX_BLOCK;
    const uint32_t ps = bmx_internal_approx_piece_shift(n, m, k, resident);
    const uint32_t tile_shift = ps + 8; // APPROX_BLOCK lanes of 2^ps ends
    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::ApproxArgs a;
    std::memset(&a, 0, sizeof a);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.own_lo = lead + a.first;
    a.own_hi = n + a.first;
    a.out_bias = base_offset - a.first;
    a.tile_begin = a.own_lo >> tile_shift;
    a.n_tiles = ((a.own_hi + (1ull << tile_shift) - 1) >> tile_shift) - a.tile_begin;
    a.out = capacity ? d_ends : nullptr;
    a.dist = capacity ? d_dist : nullptr;
    a.cap = capacity;
    a.m = (uint32_t)m;
    a.k = (uint32_t)k;
    a.warm = (uint32_t)(m + k - 1);
    a.p_shift = ps;
    if (pat) { // a string: position i holds one byte value
        for (int32_t i = 0; i < m; ++i) a.peq[(uint8_t)pat[i]] |= 1ull << i;
    } else { // classes (bmx_search_approx_classes_device): bit i = "the byte belongs to class i"
        for (int32_t i = 0; i < m; ++i)
            for (uint32_t c = 0; c < 256; ++c)
                if ((classes[(size_t)i * BMX_CLASS_BYTES + (c >> 3)] >> (c & 7)) & 1u) a.peq[c] |= 1ull << i;
    }

    int rc = st->oo.begin(WHERE, stream, a, err, errlen);
    if (rc != BMX_OK) return rc;
    const uint64_t grid = std::min<uint64_t>(a.n_tiles, resident / bmx::APPROX_BLOCK);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(bmx::APPROX_BLOCK), 0, stream, a);
    return st->oo.finish(WHERE, grid, a.n_tiles, stream, capacity, n_matches, err, errlen);
}
