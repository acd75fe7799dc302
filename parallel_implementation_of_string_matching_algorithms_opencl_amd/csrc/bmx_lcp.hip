// bmx_lcp.hip -- host side of the LCP array (bmx_lcp_*, include/bmx.h): per context the workspace (one int32 per text byte,
// the per-tile arrays and the list of long pairs), the status words with their pinned copy, the partials of the
// statistics and the events, kept between calls as bmx_sa.hip keeps the builder's.  The kernels and the algorithm are in
// bmx_lcp_kernel.h.  The argument checks and the context are the shim's (bmx_shim.hip); everything here runs on valid
// arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_lcp_kernel.h"

static_assert(bmx::LCP_LANE_BYTES == BMX_LCP_LANE_BYTES, "header and kernel disagree");
static_assert(bmx::LCP_LANE_BYTES % 8 == 0, "the lane compares whole words");

namespace {

constexpr size_t LCP_WS_KEEP = (size_t)1 << 30; // a workspace up to this size stays in the state between calls (as SA_WS_KEEP)

struct LcpHost {
    void *ws = nullptr;
    size_t ws_bytes = 0;
    uint32_t *d_words = nullptr; // LCP_WS_WORDS status / plan words
    uint32_t *h_words = nullptr; // pinned copy
    uint64_t *d_part = nullptr;  // statistics: 4 words per workgroup
    uint64_t *h_part = nullptr;  // pinned copy
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = -1.0f;
    int64_t last_long = -1;
};

int state_ready(void **state_v, LcpHost **out, const char *what, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new LcpHost();
    LcpHost *st = static_cast<LcpHost *>(*state_v);
    if (!st->d_words) BMX_HIP(what, hipMalloc(&st->d_words, bmx::LCP_WS_WORDS * sizeof(uint32_t)));
    if (!st->h_words) BMX_HIP(what, hipHostMalloc(&st->h_words, bmx::LCP_WS_WORDS * sizeof(uint32_t), hipHostMallocDefault));
    if (!st->d_part) BMX_HIP(what, hipMalloc(&st->d_part, 4 * bmx::LCP_STATS_GRID * sizeof(uint64_t)));
    if (!st->h_part) BMX_HIP(what, hipHostMalloc(&st->h_part, 4 * bmx::LCP_STATS_GRID * sizeof(uint64_t), hipHostMallocDefault));
    for (hipEvent_t &e : st->ev)
        if (!e) BMX_HIP(what, hipEventCreate(&e));
    *out = st;
    return BMX_OK;
}

uint32_t grid_for(uint64_t items) { return (uint32_t)std::min<uint64_t>((items + bmx::LCP_BLOCK - 1) / bmx::LCP_BLOCK, bmx::LCP_MAX_GRID); }

} // namespace

void bmx_internal_lcp_free(void *state_v)
{
    LcpHost *st = static_cast<LcpHost *>(state_v);
    if (!st) return;
    if (st->ws) (void)hipFree(st->ws);
    if (st->d_words) (void)hipFree(st->d_words);
    if (st->h_words) (void)hipHostFree(st->h_words);
    if (st->d_part) (void)hipFree(st->d_part);
    if (st->h_part) (void)hipHostFree(st->h_part);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

float bmx_internal_lcp_ms(const void *state_v) { return state_v ? static_cast<const LcpHost *>(state_v)->last_ms : -1.0f; }
int64_t bmx_internal_lcp_long_pairs(const void *state_v) { return state_v ? static_cast<const LcpHost *>(state_v)->last_long : -1; }

int bmx_internal_lcp(void **state_v, const uint8_t *d_text, uint32_t n, const int32_t *d_sa, int32_t *d_lcp, hipStream_t stream,
                     char *err, size_t errlen)
{
    const char *what = "bmx_lcp_array_device";
    LcpHost *st = nullptr;
    const int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    st->last_ms = -1.0f;
    st->last_long = -1;

    // plcp | tile_last | carry | list | seg_start
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const uint32_t tiles = (uint32_t)(((uint64_t)n + bmx::LCP_TILE - 1) / bmx::LCP_TILE);
    const uint32_t list_cap = std::max<uint32_t>(4096u, n / 64u);
    const size_t b_plcp = up((size_t)n * sizeof(int32_t)), b_tile = up((size_t)tiles * sizeof(int32_t));
    const size_t b_list = up((size_t)list_cap * sizeof(uint32_t));
    const size_t need = b_plcp + 2 * b_tile + 2 * b_list;
    if (st->ws_bytes < need) {
        if (st->ws) (void)hipFree(st->ws);
        st->ws = nullptr;
        st->ws_bytes = 0;
        BMX_HIP(what, hipMalloc(&st->ws, need));
        st->ws_bytes = need;
    }
    char *p = static_cast<char *>(st->ws);
    int32_t *plcp = reinterpret_cast<int32_t *>(p);
    int32_t *tile_last = reinterpret_cast<int32_t *>(p + b_plcp);
    int32_t *carry = reinterpret_cast<int32_t *>(p + b_plcp + b_tile);
    uint32_t *list = reinterpret_cast<uint32_t *>(p + b_plcp + 2 * b_tile);
    uint32_t *seg_start = reinterpret_cast<uint32_t *>(p + b_plcp + 2 * b_tile + b_list);
    int32_t *phi = d_lcp; // (the output is free until the gather)

    const uint32_t grid_n = grid_for(n), grid_t = std::min(tiles, bmx::LCP_MAX_GRID);
    const dim3 block(bmx::LCP_BLOCK), one(bmx::LCP_PLAN_BLOCK);
    BMX_HIP(what, hipMemsetAsync(st->d_words, 0, bmx::LCP_WS_WORDS * sizeof(uint32_t), stream));
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    BMX_HIP(what, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(phi), bmx::LCP_UNSET, n, stream));
    hipLaunchKernelGGL(bmx::lcp_phi_kernel, dim3(grid_n), block, 0, stream, d_sa, n, phi, st->d_words);
    hipLaunchKernelGGL(bmx::lcp_lane_kernel, dim3(grid_t), block, 0, stream, d_text, n, phi, plcp, tile_last, list, list_cap,
                       st->d_words);
    hipLaunchKernelGGL(bmx::lcp_plan_kernel, dim3(1), one, 0, stream, phi, n, list, list_cap, seg_start, st->d_words);
    hipLaunchKernelGGL(bmx::lcp_long_kernel, dim3(bmx::LCP_LONG_GRID), block, 0, stream, d_text, n, phi, plcp, list, seg_start,
                       st->d_words);
    hipLaunchKernelGGL(bmx::lcp_carry_kernel, dim3(1), one, 0, stream, tile_last, tiles, carry);
    hipLaunchKernelGGL(bmx::lcp_fill_kernel, dim3(grid_t), block, 0, stream, plcp, n, carry);
    hipLaunchKernelGGL(bmx::lcp_gather_kernel, dim3(grid_n), block, 0, stream, d_sa, n, plcp, d_lcp);
    BMX_HIP(what, hipGetLastError());
    BMX_HIP(what, hipEventRecord(st->ev[1], stream));
    BMX_HIP(what, hipMemcpyAsync(st->h_words, st->d_words, bmx::LCP_WS_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(what, hipStreamSynchronize(stream));
    if (hipEventElapsedTime(&st->last_ms, st->ev[0], st->ev[1]) != hipSuccess) st->last_ms = -1.0f;
    st->last_long = st->h_words[bmx::LCP_WS_LONG];
    if (st->ws_bytes > LCP_WS_KEEP) { // a large one is not kept
        (void)hipFree(st->ws);
        st->ws = nullptr;
        st->ws_bytes = 0;
    }
    if (st->h_words[bmx::LCP_WS_BAD]) {
        snprintf(err, errlen, "%s: d_sa is not a permutation of 0..n-1 (an entry outside [0, n), or one that occurs twice)", what);
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}

int bmx_internal_lcp_stats(void **state_v, const int32_t *d_lcp, uint32_t n, uint32_t min_len, uint64_t out[4], hipStream_t stream,
                           char *err, size_t errlen)
{
    const char *what = "bmx_lcp_stats_device";
    LcpHost *st = nullptr;
    const int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    const uint32_t grid = std::min(grid_for(n), bmx::LCP_STATS_GRID);
    hipLaunchKernelGGL(bmx::lcp_stats_kernel, dim3(grid), dim3(bmx::LCP_BLOCK), 0, stream, d_lcp, n, min_len, st->d_part);
    BMX_HIP(what, hipGetLastError());
    BMX_HIP(what, hipMemcpyAsync(st->h_part, st->d_part, 4 * (size_t)grid * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(what, hipStreamSynchronize(stream));
    uint64_t mx = 0, arg = ~0ull, sum = 0, cnt = 0;
    for (uint32_t g = 0; g < grid; ++g) { // in index order
        const uint64_t *q = st->h_part + 4 * (size_t)g;
        if (q[0] > mx || (q[0] == mx && q[1] < arg)) mx = q[0], arg = q[1];
        sum += q[2];
        cnt += q[3];
    }
    out[0] = mx, out[1] = arg, out[2] = sum, out[3] = cnt;
    return BMX_OK;
}
