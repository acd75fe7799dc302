// bmx_spans.hip -- host side of the match spans (bmx_approx_spans_device, include/bmx.h): builds the reversed-pattern
// Peq table, keeps the status words, the tile counts of the selection and the events between calls, launches
// bmx_spans_kernel.h (selection: count, scan, fill; then the starts) and waits for the stream.  The argument checks and
// the context are the shim's (bmx_shim.hip), which also names the long entry (bmx_approx_long_spans_device: a string of more
// than 64 bytes, the starts by a column of several words); everything here runs on a valid context with valid arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "bmx.h"
#include "bmx_spans_kernel.h"
#include "bmx_internal.h"

static_assert(sizeof(bmx::SpansArgs) + sizeof(bmx::LongPattern) <= 4096, "kernel arguments");

namespace {

constexpr const char *WHERE = "bmx_approx_spans_device";

struct SpansHost {
    uint64_t *d_ws = nullptr;    // {status bits, kept entries}
    uint64_t *h_ws = nullptr;    // pinned copy of them
    uint64_t *d_tiles = nullptr; // selection: one word per tile
    uint64_t tiles_cap = 0;
    uint8_t *d_sel_dist = nullptr; // the kept distances when the caller wants none (the starts kernel checks them)
    uint64_t sel_dist_cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // around the selection's first two kernels, around the rest
    float last_ms = -1.0f;
};

} // namespace

void bmx_internal_spans_free(void *state_v)
{
    SpansHost *st = static_cast<SpansHost *>(state_v);
    if (!st) return;
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    if (st->d_tiles) (void)hipFree(st->d_tiles);
    if (st->d_sel_dist) (void)hipFree(st->d_sel_dist);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

float bmx_internal_spans_ms(const void *state_v)
{
    const SpansHost *st = static_cast<const SpansHost *>(state_v);
    return st ? st->last_ms : -1.0f;
}

// count >= 1.  flags == 0: d_starts[i] for d_ends[i].  BMX_SPANS_BEST: the kept entries to d_sel_ends / d_sel_dist (may be
// NULL) / d_starts, in list order.
int bmx_internal_spans(void **state_v, const void *d_text, uint64_t n, uint64_t base_offset, const char *pat,
                       const uint8_t *classes, int32_t m, int32_t k, const uint64_t *d_ends, const uint8_t *d_dist, uint64_t count,
                       uint32_t flags, uint64_t *d_starts, uint64_t *d_sel_ends, uint8_t *d_sel_dist, uint64_t *n_spans,
                       hipStream_t stream, char *err, size_t errlen)
{
    const char *where = m > BMX_MAX_APPROX_PATTERN ? "bmx_approx_long_spans_device" : WHERE; // the entry that runs this
    if (!*state_v) *state_v = new SpansHost();
    SpansHost *st = static_cast<SpansHost *>(*state_v);
    st->last_ms = -1.0f;
    if (n_spans) *n_spans = 0;
    const uint64_t n_tiles = (count + bmx::SPANS_TILE - 1) / bmx::SPANS_TILE;
    if ((count + bmx::SPANS_BLOCK - 1) / bmx::SPANS_BLOCK > 0x7fffffffull) {
        snprintf(err, errlen, "%s: more than 2^31 workgroups of list entries in one call", where);
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(where, hipMalloc(&st->d_ws, 2 * sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(where, hipHostMalloc(&st->h_ws, 2 * sizeof(uint64_t), hipHostMallocDefault));
    for (hipEvent_t &e : st->ev)
        if (!e) BMX_HIP(where, hipEventCreate(&e));
    BMX_HIP(where, hipMemsetAsync(st->d_ws, 0, 2 * sizeof(uint64_t), stream)); // the status word starts clean in every call

    const uint64_t *list_ends = d_ends;
    const uint8_t *list_dist = d_dist;
    uint64_t list_count = count;
    float ms_select = 0.0f;
    const bool best = (flags & BMX_SPANS_BEST) != 0;
    if (best) {
        if (n_tiles > st->tiles_cap) {
            if (st->d_tiles) (void)hipFree(st->d_tiles);
            st->d_tiles = nullptr;
            st->tiles_cap = 0;
            const uint64_t cap = std::max<uint64_t>(n_tiles, 1024);
            BMX_HIP(where, hipMalloc(&st->d_tiles, cap * sizeof(uint64_t)));
            st->tiles_cap = cap;
        }
        bmx::SpansSelectArgs s = {};
        s.ends = d_ends;
        s.dist = d_dist;
        s.count = count;
        s.k = (uint32_t)k;
        s.tiles = st->d_tiles;
        BMX_HIP(where, hipEventRecord(st->ev[0], stream));
        hipLaunchKernelGGL(bmx::spans_select_kernel<false>, dim3((uint32_t)n_tiles), dim3(bmx::SPANS_BLOCK), 0, stream, s);
        BMX_HIP(where, hipGetLastError());
        hipLaunchKernelGGL(bmx::spans_scan_kernel, dim3(1), dim3(bmx::SPANS_SCAN_BLOCK), 0, stream, st->d_tiles, n_tiles,
                           st->d_ws + 1);
        BMX_HIP(where, hipGetLastError());
        BMX_HIP(where, hipEventRecord(st->ev[1], stream));
        BMX_HIP(where, hipMemcpyAsync(st->h_ws, st->d_ws, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        BMX_HIP(where, hipStreamSynchronize(stream)); // the kept count sizes the rest
        if (hipEventElapsedTime(&ms_select, st->ev[0], st->ev[1]) != hipSuccess) ms_select = 0.0f;
        list_count = st->h_ws[1];
        if (list_count > count) {
            snprintf(err, errlen, "%s: the selection kept %llu of %llu entries", where,
                     (unsigned long long)list_count, (unsigned long long)count);
            return BMX_ERR_HIP;
        }
        if (list_count == 0) {
            st->last_ms = ms_select;
            return BMX_OK;
        }
        if (!d_sel_dist) {
            if (list_count > st->sel_dist_cap) {
                if (st->d_sel_dist) (void)hipFree(st->d_sel_dist);
                st->d_sel_dist = nullptr;
                st->sel_dist_cap = 0;
                const uint64_t cap = std::max<uint64_t>(list_count, 1 << 16);
                BMX_HIP(where, hipMalloc(&st->d_sel_dist, cap));
                st->sel_dist_cap = cap;
            }
            d_sel_dist = st->d_sel_dist;
        }
        s.sel_ends = d_sel_ends;
        s.sel_dist = d_sel_dist;
        BMX_HIP(where, hipEventRecord(st->ev[2], stream));
        hipLaunchKernelGGL(bmx::spans_select_kernel<true>, dim3((uint32_t)n_tiles), dim3(bmx::SPANS_BLOCK), 0, stream, s);
        BMX_HIP(where, hipGetLastError());
        list_ends = d_sel_ends;
        list_dist = d_sel_dist;
    } else {
        BMX_HIP(where, hipEventRecord(st->ev[2], stream));
    }

    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::SpansArgs a;
    std::memset(&a, 0, sizeof a);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.n = n;
    a.base = base_offset;
    a.ends = list_ends;
    a.dist = list_dist;
    a.count = list_count;
    a.starts = d_starts;
    a.ws = st->d_ws;
    a.m = (uint32_t)m;
    a.k = (uint32_t)k;
    a.chunks = (uint32_t)(m + k + 7) / 8;
    const uint64_t n_blocks = (list_count + bmx::SPANS_BLOCK - 1) / bmx::SPANS_BLOCK;
    if (m > BMX_MAX_APPROX_PATTERN) { // bmx_approx_long_spans_device (a string): the reversed pattern goes as an argument
        bmx::LongPattern rev;
        std::memset(&rev, 0, sizeof rev);
        uint8_t *r = reinterpret_cast<uint8_t *>(rev.w);
        for (int32_t i = 0; i < m; ++i) r[i] = (uint8_t)pat[m - 1 - i];
        const int W = bmx::words_for(m);
        void (*kernel)(const bmx::SpansArgs, const bmx::LongPattern) =
            W == 2 ? bmx::spans_starts_long_kernel<2> : W == 4 ? bmx::spans_starts_long_kernel<4> : bmx::spans_starts_long_kernel<8>;
        hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(bmx::SPANS_BLOCK), 0, stream, a, rev);
    } else {
        // the REVERSED pattern: bit i stands for position m - 1 - i (bmx_internal_approx builds the forward table the same way)
        if (pat) {
            for (int32_t i = 0; i < m; ++i) a.peq[(uint8_t)pat[m - 1 - i]] |= 1ull << i;
        } else {
            for (int32_t i = 0; i < m; ++i)
                for (uint32_t c = 0; c < 256; ++c)
                    if ((classes[(size_t)(m - 1 - i) * BMX_CLASS_BYTES + (c >> 3)] >> (c & 7)) & 1u) a.peq[c] |= 1ull << i;
        }
        void (*kernel)(const bmx::SpansArgs) = m > 32 ? bmx::spans_starts_kernel<uint64_t> : bmx::spans_starts_kernel<uint32_t>;
        hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(bmx::SPANS_BLOCK), 0, stream, a);
    }
    BMX_HIP(where, hipGetLastError());
    BMX_HIP(where, hipEventRecord(st->ev[3], stream));
    BMX_HIP(where, hipMemcpyAsync(st->h_ws, st->d_ws, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(where, hipStreamSynchronize(stream));
    float ms_rest = 0.0f;
    if (hipEventElapsedTime(&ms_rest, st->ev[2], st->ev[3]) == hipSuccess) st->last_ms = ms_select + ms_rest;

    const uint64_t bad = st->h_ws[0];
    if (bad != 0) {
        snprintf(err, errlen, "%s: %s%s%s", where, bad & bmx::SPANS_BAD_END ? "an end outside the view; " : "",
                 bad & bmx::SPANS_BAD_MIN ? "an end with no match within k edits; " : "",
                 bad & bmx::SPANS_BAD_DIST ? "a distance that is not this pattern's on this text; " : "");
        return BMX_ERR_ARG;
    }
    if (n_spans) *n_spans = list_count;
    return BMX_OK;
}
