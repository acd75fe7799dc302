// bmx_ed_batch.hip -- host side of the batched edit distance (bmx_edit_distance_batch_device, include/bmx.h): keeps the
// status words, the list of pairs for the pair-by-pair path and the events between calls, launches
// bmx_ed_batch_kernel.h once, runs the listed pairs through bmx_edit_distance_device on the same stream and waits for
// the stream.  The argument checks and the context are the shim's (bmx_shim.hip); everything here runs on a valid
// context with valid arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmx.h"
#include "bmx_ed_batch_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::ED_BATCH_WORD == BMX_ED_BATCH_WORD, "header and kernel disagree");
static_assert(bmx::ED_BATCH_LONG == BMX_ED_BATCH_LONG, "header and kernel disagree");
static_assert(bmx::ED_BATCH_NO_LIMIT == BMX_ED_NO_LIMIT, "header and kernel disagree");

namespace {

constexpr const char *WHERE = "bmx_edit_distance_batch_device";

struct EdBatchHost {
    uint64_t *d_ws = nullptr;   // {bad offsets seen, pairs listed}
    uint64_t *h_ws = nullptr;   // pinned copy of them
    uint64_t *d_list = nullptr; // list_cap entries of ED_BATCH_LIST_WORDS words, then list_cap answers (uint32)
    uint64_t list_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = -1.0f;
    int64_t last_fallbacks = -1;
};

} // namespace

void bmx_internal_ed_batch_free(void *state_v)
{
    EdBatchHost *st = static_cast<EdBatchHost *>(state_v);
    if (!st) return;
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    if (st->d_list) (void)hipFree(st->d_list);
    if (st->ev0) (void)hipEventDestroy(st->ev0);
    if (st->ev1) (void)hipEventDestroy(st->ev1);
    delete st;
}

float bmx_internal_ed_batch_ms(const void *state_v)
{
    const EdBatchHost *st = static_cast<const EdBatchHost *>(state_v);
    return st ? st->last_ms : -1.0f;
}

int64_t bmx_internal_ed_batch_fallbacks(const void *state_v)
{
    const EdBatchHost *st = static_cast<const EdBatchHost *>(state_v);
    return st ? st->last_fallbacks : -1;
}

int bmx_internal_ed_batch(void **state_v, bmx_ctx *ctx, const void *d_a, uint64_t a_bytes, const uint64_t *d_a_off,
                          uint64_t a_count, const void *d_b, uint64_t b_bytes, const uint64_t *d_b_off, uint64_t count,
                          uint32_t limit, uint32_t *d_dist, hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new EdBatchHost();
    EdBatchHost *st = static_cast<EdBatchHost *>(*state_v);
    st->last_ms = -1.0f;
    st->last_fallbacks = -1;
    const uint64_t n_blocks = (count + bmx::ED_BATCH_BLOCK - 1) / bmx::ED_BATCH_BLOCK;
    if (n_blocks > 0x7fffffffull) {
        snprintf(err, errlen, "bmx_edit_distance_batch_device: more than 2^31 workgroups of pairs in one call");
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(WHERE, hipMalloc(&st->d_ws, 2 * sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE, hipHostMalloc(&st->h_ws, 2 * sizeof(uint64_t), hipHostMallocDefault));
    if (!st->ev0) BMX_HIP(WHERE, hipEventCreate(&st->ev0));
    if (!st->ev1) BMX_HIP(WHERE, hipEventCreate(&st->ev1));
    if (!st->d_list) {
        const uint64_t cap = 4096;
        BMX_HIP(WHERE, hipMalloc(&st->d_list, cap * (bmx::ED_BATCH_LIST_WORDS * sizeof(uint64_t) + sizeof(uint32_t))));
        st->list_cap = cap;
    }

    bmx::EdBatchArgs a = {};
    a.a = static_cast<const uint8_t *>(d_a);
    a.b = static_cast<const uint8_t *>(d_b);
    a.a_off = d_a_off;
    a.b_off = d_b_off;
    a.a_bytes = a_bytes;
    a.b_bytes = b_bytes;
    a.count = count;
    a.one = a_count == 1 && count != 1 ? 1u : 0u; // (a single pair is the same either way)
    a.limit = limit;
    a.dist = d_dist;
    a.ws = st->d_ws;

    uint64_t n_fb = 0;
    for (int pass = 0; pass < 2; ++pass) { // a second pass only if the list was too short for the first
        a.list = st->d_list;
        a.list_cap = st->list_cap;
        BMX_HIP(WHERE, hipMemsetAsync(st->d_ws, 0, 2 * sizeof(uint64_t), stream));
        BMX_HIP(WHERE, hipEventRecord(st->ev0, stream));
        hipLaunchKernelGGL(bmx::ed_batch_kernel, dim3((uint32_t)n_blocks), dim3(bmx::ED_BATCH_BLOCK), 0, stream, a);
        BMX_HIP(WHERE, hipGetLastError());
        BMX_HIP(WHERE, hipEventRecord(st->ev1, stream));
        BMX_HIP(WHERE, hipMemcpyAsync(st->h_ws, st->d_ws, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        BMX_HIP(WHERE, hipStreamSynchronize(stream));
        if (hipEventElapsedTime(&st->last_ms, st->ev0, st->ev1) != hipSuccess) st->last_ms = -1.0f;
        if (st->h_ws[0] != 0) {
            snprintf(err, errlen, "bmx_edit_distance_batch_device: offsets that decrease, end past their blob or span 2^31 bytes");
            return BMX_ERR_ARG;
        }
        n_fb = st->h_ws[1];
        if (n_fb <= st->list_cap) break;
        (void)hipFree(st->d_list);
        st->d_list = nullptr;
        st->list_cap = 0;
        BMX_HIP(WHERE, hipMalloc(&st->d_list, n_fb * (bmx::ED_BATCH_LIST_WORDS * sizeof(uint64_t) + sizeof(uint32_t))));
        st->list_cap = n_fb;
    }
    st->last_fallbacks = (int64_t)n_fb;
    if (n_fb == 0) return BMX_OK;

    // Pairs the kernel does not cover: each through the single-pair path, on the same stream (same answer, no speed-up).
    // That path keeps its own time: bmx_last_edit_distance_ms reports the last of these pairs afterwards (bmx.h says so).
    std::vector<uint64_t> list(n_fb * bmx::ED_BATCH_LIST_WORDS);
    std::vector<uint32_t> vals(n_fb);
    BMX_HIP(WHERE, hipMemcpyAsync(list.data(), st->d_list, list.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE, hipStreamSynchronize(stream));
    for (uint64_t j = 0; j < n_fb; ++j) {
        const uint64_t *e = &list[j * bmx::ED_BATCH_LIST_WORDS];
        uint64_t d = 0;
        const int rc = bmx_edit_distance_device(ctx, a.a + e[1], e[2], a.b + e[3], e[4], &d, stream);
        if (rc != BMX_OK) return rc;
        vals[j] = (uint32_t)(limit != BMX_ED_NO_LIMIT ? std::min<uint64_t>(d, (uint64_t)limit + 1) : d);
    }
    uint32_t *d_vals = reinterpret_cast<uint32_t *>(st->d_list + st->list_cap * bmx::ED_BATCH_LIST_WORDS);
    BMX_HIP(WHERE, hipMemcpyAsync(d_vals, vals.data(), n_fb * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(bmx::ed_batch_scatter_kernel, dim3((uint32_t)((n_fb + 255) / 256)), dim3(256), 0, stream, st->d_list, d_vals,
                       n_fb, d_dist);
    BMX_HIP(WHERE, hipGetLastError());
    BMX_HIP(WHERE, hipStreamSynchronize(stream));
    return BMX_OK;
}
