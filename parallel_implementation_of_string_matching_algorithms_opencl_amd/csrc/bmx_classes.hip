// bmx_classes.hip -- host side of the class-pattern search (bmx_search_classes_device, include/bmx.h): builds the
// Shift-And table from the classes, picks the word width and the lane piece, keeps the per-tile status words, the ticket
// counter and the pinned result words between calls, launches bmx_classes_kernel.h once and waits for the stream.  The
// argument checks and the context are the shim's (bmx_shim.hip); everything here runs on a valid context with valid
// arguments.  The shape is bmx_approx.hip's: the kernel takes the same argument block, in end coordinates.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "bmx.h"
#include "bmx_classes_kernel.h"

static_assert(bmx::MAX_CLASS_PATTERN == BMX_MAX_CLASS_PATTERN, "header and kernel disagree");

namespace {

struct ClassesState {
    uint64_t *d_status = nullptr; // per-tile look-back words, tagged with the call's epoch (cleared only when allocated
    uint64_t status_cap = 0;      // and when the 22-bit tag wraps)
    unsigned long long *d_ticket = nullptr; // monotonic: a call hands out n_tiles + grid tickets
    uint64_t ticket_base = 0;
    uint64_t *h_status = nullptr; // pinned, device-visible: {total, give-up, seq}
    uint64_t *h_status_dev = nullptr;
    uint64_t seq = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = -1.0f;
    int blocks_per_cu[2] = {0, 0}; // resident workgroups per CU of the 32- and the 64-bit kernel
};

#define CHIP(expr)                                                                                              \
    do {                                                                                                        \
        hipError_t e__ = (expr);                                                                                \
        if (e__ != hipSuccess) {                                                                                \
            snprintf(err, errlen, "bmx_search_classes_device: %s failed: %s", #expr, hipGetErrorString(e__)); \
            return BMX_ERR_HIP;                                                                                 \
        }                                                                                                       \
    } while (0)

uint32_t ceil_log2(uint64_t x)
{
    uint32_t s = 0;
    while ((1ull << s) < x) ++s;
    return s;
}

} // namespace

// Ends per lane: about n / (resident lanes), as a power of two in [64, 2048], and at least four patterns (the warm-up of
// m - 1 bytes per piece is overhead).  From 128 on a piece is whole 128-byte lines of the text.
uint32_t bmx_internal_classes_piece_shift(uint64_t n, int32_t m, uint64_t resident_lanes)
{
    const uint64_t per = (n + resident_lanes - 1) / std::max<uint64_t>(resident_lanes, 1);
    uint32_t ps = std::min<uint32_t>(std::max<uint32_t>(ceil_log2(per), 6), 11);
    ps = std::max<uint32_t>(ps, ceil_log2(4ull * (uint64_t)m));
    return ps;
}

void bmx_internal_classes_free(void *state_v)
{
    ClassesState *st = static_cast<ClassesState *>(state_v);
    if (!st) return;
    if (st->d_status) (void)hipFree(st->d_status);
    if (st->d_ticket) (void)hipFree(st->d_ticket);
    if (st->h_status) (void)hipHostFree(st->h_status);
    if (st->ev0) (void)hipEventDestroy(st->ev0);
    if (st->ev1) (void)hipEventDestroy(st->ev1);
    delete st;
}

float bmx_internal_classes_ms(const void *state_v)
{
    const ClassesState *st = static_cast<const ClassesState *>(state_v);
    return st ? st->last_ms : -1.0f;
}

int bmx_internal_classes(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                         const uint8_t *classes, int32_t m, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches,
                         hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new ClassesState();
    ClassesState *st = static_cast<ClassesState *>(*state_v);
    if (n_matches) *n_matches = 0;
    st->last_ms = 0.0f;
    // In end coordinates: start p is end p + m - 1, so the ends to report are [m - 1, min(n, n_own + m - 1)).
    const uint64_t lead = (uint64_t)m - 1;
    const uint64_t n_ends = n_own >= n ? n : std::min<uint64_t>(n, n_own + lead);
    if (lead >= n_ends) return BMX_OK; // no window fits or none is owned (before anything is put on `stream`)
    if (!st->d_ticket) {
        CHIP(hipMalloc(&st->d_ticket, sizeof(unsigned long long)));
        CHIP(hipMemsetAsync(st->d_ticket, 0, sizeof(unsigned long long), stream));
        st->ticket_base = 0;
    }
    if (!st->h_status) {
        CHIP(hipHostMalloc(&st->h_status, 4 * sizeof(uint64_t), hipHostMallocMapped));
        std::memset(st->h_status, 0, 4 * sizeof(uint64_t));
        CHIP(hipHostGetDevicePointer((void **)&st->h_status_dev, st->h_status, 0));
    }
    if (!st->ev0) CHIP(hipEventCreate(&st->ev0));
    if (!st->ev1) CHIP(hipEventCreate(&st->ev1));
    const bool wide = m > 32;
    void (*kernel)(const bmx::ApproxArgs) = wide ? bmx::classes_kernel<true> : bmx::classes_kernel<false>;
    int &bpc = st->blocks_per_cu[wide ? 1 : 0];
    if (bpc == 0) {
        CHIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kernel, bmx::CLASSES_BLOCK, 0));
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

    if (a.n_tiles > st->status_cap) {
        if (st->d_status) (void)hipFree(st->d_status);
        st->d_status = nullptr;
        st->status_cap = 0;
        const uint64_t cap = std::max<uint64_t>(a.n_tiles, 1024);
        CHIP(hipMalloc(&st->d_status, cap * sizeof(uint64_t)));
        CHIP(hipMemsetAsync(st->d_status, 0, cap * sizeof(uint64_t), stream)); // tag 0 is never a call's
        st->status_cap = cap;
    }
    ++st->seq;
    if ((st->seq & bmx::APPROX_TAG_MASK) == 0) { // the tag wraps: old words could carry this call's tag
        CHIP(hipMemsetAsync(st->d_status, 0, st->status_cap * sizeof(uint64_t), stream));
        ++st->seq;
    }
    a.status = st->d_status;
    a.ticket = st->d_ticket;
    a.ticket_base = st->ticket_base;
    a.host_status = st->h_status_dev;
    a.seq = st->seq;
    a.tag = st->seq & bmx::APPROX_TAG_MASK;
    st->h_status[0] = st->h_status[1] = st->h_status[2] = 0;

    const uint64_t grid = std::min<uint64_t>(a.n_tiles, resident / bmx::CLASSES_BLOCK);
    CHIP(hipEventRecord(st->ev0, stream));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(bmx::CLASSES_BLOCK), 0, stream, a);
    CHIP(hipGetLastError());
    CHIP(hipEventRecord(st->ev1, stream));
    CHIP(hipStreamSynchronize(stream));
    st->ticket_base += a.n_tiles + grid; // every workgroup draws one ticket past the last tile
    (void)hipEventElapsedTime(&st->last_ms, st->ev0, st->ev1);

    volatile uint64_t *hs = st->h_status;
    if (hs[2] != st->seq) {
        snprintf(err, errlen, "bmx_search_classes_device: the kernel did not report its total (seq %llu, want %llu)",
                 (unsigned long long)hs[2], (unsigned long long)st->seq);
        return BMX_ERR_HIP;
    }
    if (hs[1] != 0) {
        snprintf(err, errlen, "bmx_search_classes_device: a tile waited longer than its bound for its predecessors' counts; "
                              "result discarded");
        return BMX_ERR_HIP;
    }
    const uint64_t total = hs[0];
    if (n_matches) *n_matches = total;
    return total > capacity ? BMX_ERR_CAPACITY : BMX_OK;
}
