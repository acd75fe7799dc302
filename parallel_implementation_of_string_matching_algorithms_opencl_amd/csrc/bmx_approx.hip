// bmx_approx.hip -- host side of the approximate search (bmx_search_approx_device, include/bmx.h): picks the word
// width and the lane piece, keeps the per-tile status words, the ticket counter and the pinned result words between
// calls, launches bmx_approx_kernel.h once and waits for the stream.  The argument checks and the context are the
// shim's (bmx_shim.hip); everything here runs on a valid context with valid arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "bmx.h"
#include "bmx_approx_kernel.h"

static_assert(bmx::MAX_APPROX_PATTERN == BMX_MAX_APPROX_PATTERN, "header and kernel disagree");
static_assert(sizeof(bmx::ApproxArgs) <= 4096, "kernel arguments");

namespace {

struct ApproxState {
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

#define AHIP(expr)                                                                                             \
    do {                                                                                                       \
        hipError_t e__ = (expr);                                                                               \
        if (e__ != hipSuccess) {                                                                               \
            snprintf(err, errlen, "bmx_search_approx_device: %s failed: %s", #expr, hipGetErrorString(e__)); \
            return BMX_ERR_HIP;                                                                                \
        }                                                                                                      \
    } while (0)

uint32_t ceil_log2(uint64_t x)
{
    uint32_t s = 0;
    while ((1ull << s) < x) ++s;
    return s;
}

} // namespace

// Ends per lane: about n / (resident lanes), as a power of two in [64, 2048], and at least four warm-ups.  Small texts
// get short pieces (parallelism), large ones long pieces (the warm-up of m + k - 1 bytes per piece is overhead).
uint32_t bmx_internal_approx_piece_shift(uint64_t n, int32_t m, int32_t k, uint64_t resident_lanes)
{
    const uint64_t per = (n + resident_lanes - 1) / std::max<uint64_t>(resident_lanes, 1);
    uint32_t ps = std::min<uint32_t>(std::max<uint32_t>(ceil_log2(per), 6), 11);
    ps = std::max<uint32_t>(ps, std::min<uint32_t>(ceil_log2(4ull * (uint64_t)(m + k)), 11));
    return ps;
}

void bmx_internal_approx_free(void *state_v)
{
    ApproxState *st = static_cast<ApproxState *>(state_v);
    if (!st) return;
    if (st->d_status) (void)hipFree(st->d_status);
    if (st->d_ticket) (void)hipFree(st->d_ticket);
    if (st->h_status) (void)hipHostFree(st->h_status);
    if (st->ev0) (void)hipEventDestroy(st->ev0);
    if (st->ev1) (void)hipEventDestroy(st->ev1);
    delete st;
}

float bmx_internal_approx_ms(const void *state_v)
{
    const ApproxState *st = static_cast<const ApproxState *>(state_v);
    return st ? st->last_ms : -1.0f;
}

int bmx_internal_approx(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                        const char *pat, const uint8_t *classes, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist,
                        uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new ApproxState();
    ApproxState *st = static_cast<ApproxState *>(*state_v);
    if (n_matches) *n_matches = 0;
    st->last_ms = 0.0f;
    if (lead >= n) return BMX_OK; // no end to report (before anything is put on `stream`: what is cleared below is cleared
                                  // in front of the kernel that reads it, on the same stream)
    if (!st->d_ticket) {
        AHIP(hipMalloc(&st->d_ticket, sizeof(unsigned long long)));
        AHIP(hipMemsetAsync(st->d_ticket, 0, sizeof(unsigned long long), stream));
        st->ticket_base = 0;
    }
    if (!st->h_status) {
        AHIP(hipHostMalloc(&st->h_status, 4 * sizeof(uint64_t), hipHostMallocMapped));
        std::memset(st->h_status, 0, 4 * sizeof(uint64_t));
        AHIP(hipHostGetDevicePointer((void **)&st->h_status_dev, st->h_status, 0));
    }
    if (!st->ev0) AHIP(hipEventCreate(&st->ev0));
    if (!st->ev1) AHIP(hipEventCreate(&st->ev1));
    const bool wide = m > 32;
    void (*kernel)(const bmx::ApproxArgs) = wide ? bmx::approx_kernel<uint64_t> : bmx::approx_kernel<uint32_t>;
    int &bpc = st->blocks_per_cu[wide ? 1 : 0];
    if (bpc == 0) {
        AHIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kernel, bmx::APPROX_BLOCK, 0));
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

    if (a.n_tiles > st->status_cap) {
        if (st->d_status) (void)hipFree(st->d_status);
        st->d_status = nullptr;
        st->status_cap = 0;
        const uint64_t cap = std::max<uint64_t>(a.n_tiles, 1024);
        AHIP(hipMalloc(&st->d_status, cap * sizeof(uint64_t)));
        AHIP(hipMemsetAsync(st->d_status, 0, cap * sizeof(uint64_t), stream)); // tag 0 is never a call's
        st->status_cap = cap;
    }
    ++st->seq;
    if ((st->seq & bmx::APPROX_TAG_MASK) == 0) { // the tag wraps: old words could carry this call's tag
        AHIP(hipMemsetAsync(st->d_status, 0, st->status_cap * sizeof(uint64_t), stream));
        ++st->seq;
    }
    a.status = st->d_status;
    a.ticket = st->d_ticket;
    a.ticket_base = st->ticket_base;
    a.host_status = st->h_status_dev;
    a.seq = st->seq;
    a.tag = st->seq & bmx::APPROX_TAG_MASK;
    st->h_status[0] = st->h_status[1] = st->h_status[2] = 0;

    const uint64_t grid = std::min<uint64_t>(a.n_tiles, resident / bmx::APPROX_BLOCK);
    AHIP(hipEventRecord(st->ev0, stream));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(bmx::APPROX_BLOCK), 0, stream, a);
    AHIP(hipGetLastError());
    AHIP(hipEventRecord(st->ev1, stream));
    AHIP(hipStreamSynchronize(stream));
    st->ticket_base += a.n_tiles + grid; // every workgroup draws one ticket past the last tile
    (void)hipEventElapsedTime(&st->last_ms, st->ev0, st->ev1);

    volatile uint64_t *hs = st->h_status;
    if (hs[2] != st->seq) {
        snprintf(err, errlen, "bmx_search_approx_device: the kernel did not report its total (seq %llu, want %llu)",
                 (unsigned long long)hs[2], (unsigned long long)st->seq);
        return BMX_ERR_HIP;
    }
    if (hs[1] != 0) {
        snprintf(err, errlen, "bmx_search_approx_device: a tile waited longer than its bound for its predecessors' counts; "
                              "result discarded");
        return BMX_ERR_HIP;
    }
    const uint64_t total = hs[0];
    if (n_matches) *n_matches = total;
    return total > capacity ? BMX_ERR_CAPACITY : BMX_OK;
}
