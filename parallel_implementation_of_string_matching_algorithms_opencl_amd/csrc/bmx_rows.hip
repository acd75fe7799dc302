// bmx_rows.hip -- host side of the row-wise results (bmx_rows_*, include/bmx.h): per context the ordered
// output's words of the split, four status words with their pinned copy, the workspace of the matching rows (tile summaries,
// carries, heads) and the events, kept between calls as bmx_align.hip keeps the alignments'.  The kernels are
// in bmx_rows_kernel.h.  The argument checks and the context are the shim's (bmx_shim.hip); everything here runs on valid
// arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_rows_kernel.h"

static_assert(bmx::ROWS_NONE == BMX_ROW_NONE, "header and kernel disagree");
static_assert((bmx::ROWS_TILE & (bmx::ROWS_TILE - 1)) == 0, "bmx_exp_last_launch reports log2 of the tile");

namespace {

constexpr size_t ROWS_WS_KEEP = (size_t)1 << 30; // a workspace up to this size stays in the state between calls

struct RowsHost {
    bmx::OrderedOut oo; // the split's look-back words, ticket, pinned result words and events (first: ordered_set_seq)
    unsigned long long *d_words = nullptr; // ROWS_WORDS status words: [0] bad list, [1] longest row, [2] distinct rows of the list
    unsigned long long *h_words = nullptr; // pinned copy ([3]: the source of a lone off[0])
    void *d_work = nullptr;
    size_t work_bytes = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int blocks_per_cu = 0; // resident workgroups per CU of the split kernel
    uint64_t last_grid = 0, last_tiles = 0; // the last split's workgroups and tiles (bmx_exp_last_launch)
    float last_ms = -1.0f;
};

size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

int state_ready(void **state_v, RowsHost **out, const char *what, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new RowsHost();
    RowsHost *st = static_cast<RowsHost *>(*state_v);
    st->last_ms = -1.0f;
    if (!st->d_words) BMX_HIP(what, hipMalloc(&st->d_words, bmx::ROWS_WORDS * sizeof(uint64_t)));
    if (!st->h_words) BMX_HIP(what, hipHostMalloc(&st->h_words, bmx::ROWS_WORDS * sizeof(uint64_t), hipHostMallocDefault));
    for (hipEvent_t &e : st->ev)
        if (!e) BMX_HIP(what, hipEventCreate(&e));
    *out = st;
    return BMX_OK;
}

int work_ready(RowsHost *st, size_t need, const char *what, char *err, size_t errlen)
{
    if (st->work_bytes >= need) return BMX_OK;
    if (st->d_work) (void)hipFree(st->d_work);
    st->d_work = nullptr, st->work_bytes = 0;
    BMX_HIP(what, hipMalloc(&st->d_work, need));
    st->work_bytes = need;
    return BMX_OK;
}

void work_release(RowsHost *st)
{
    if (st->work_bytes <= ROWS_WS_KEEP) return; // a large one is not kept
    (void)hipFree(st->d_work);
    st->d_work = nullptr, st->work_bytes = 0;
}

uint32_t grid_for(uint64_t items) { return (uint32_t)((items + bmx::ROWS_BLOCK - 1) / bmx::ROWS_BLOCK); }

} // namespace

void bmx_internal_rows_free(void *state_v)
{
    RowsHost *st = static_cast<RowsHost *>(state_v);
    if (!st) return;
    st->oo.free();
    if (st->d_words) (void)hipFree(st->d_words);
    if (st->h_words) (void)hipHostFree(st->h_words);
    if (st->d_work) (void)hipFree(st->d_work);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

float bmx_internal_rows_ms(const void *state_v) { return state_v ? static_cast<const RowsHost *>(state_v)->last_ms : -1.0f; }

// libbmx_exp.so's bmx_exp_last_launch, session "rows": {log2 of the split's tile bytes, workgroups, tiles of the last split}
void bmx_internal_rows_last(const void *state_v, uint64_t out3[3])
{
    const RowsHost *st = static_cast<const RowsHost *>(state_v);
    out3[0] = bmx::ceil_log2(bmx::ROWS_TILE);
    out3[1] = st ? st->last_grid : 0;
    out3[2] = st ? st->last_tiles : 0;
}

int bmx_internal_rows_split(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t base_offset, uint8_t delim,
                            uint64_t *d_off, uint64_t capacity, uint64_t *n_rows, uint64_t *longest, hipStream_t stream, char *err,
                            size_t errlen)
{
    const char *what = "bmx_rows_split_device";
    RowsHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    if (n_rows) *n_rows = 0;
    if (longest) *longest = 0;
    if (n == 0) { // no row: the single entry off[0]
        if (capacity) {
            st->h_words[3] = base_offset;
            BMX_HIP(what, hipMemcpyAsync(d_off, &st->h_words[3], sizeof(uint64_t), hipMemcpyHostToDevice, stream));
            BMX_HIP(what, hipStreamSynchronize(stream));
        }
        st->last_ms = 0.0f;
        return BMX_OK;
    }
    if (st->blocks_per_cu == 0) {
        int bpc = 0;
        BMX_HIP(what, hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, bmx::rows_split_kernel, bmx::ROWS_BLOCK, 0));
        st->blocks_per_cu = std::max(1, std::min(bpc, 8));
    }
    bmx::RowsSplitArgs a{};
    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.own_lo = addr & 15ull;
    a.own_hi = n + a.own_lo;
    a.out_bias = base_offset - a.own_lo + 1;
    a.off = capacity ? d_off : nullptr;
    a.cap = capacity;
    a.base_offset = base_offset;
    a.splat = 0x01010101u * delim;
    a.n_tiles = (a.own_hi + bmx::ROWS_TILE - 1) / bmx::ROWS_TILE;
    const bool want_longest = longest != nullptr && capacity >= 2;
    if (want_longest) BMX_HIP(what, hipMemsetAsync(st->d_words, 0, bmx::ROWS_WORDS * sizeof(uint64_t), stream));
    rc = st->oo.begin(what, stream, a, err, errlen);
    if (rc != BMX_OK) return rc;
    const uint64_t grid = std::min<uint64_t>(a.n_tiles, (uint64_t)num_cu * (uint64_t)st->blocks_per_cu);
    st->last_grid = grid, st->last_tiles = a.n_tiles;
    hipLaunchKernelGGL(bmx::rows_split_kernel, dim3((uint32_t)grid), dim3(bmx::ROWS_BLOCK), 0, stream, a);
    if (want_longest) { // behind the split on the stream: the total is in pinned memory by then
        const uint32_t lgrid = std::min<uint32_t>(grid_for(std::min<uint64_t>(capacity - 1, n)), 1024u);
        hipLaunchKernelGGL(bmx::rows_longest_kernel, dim3(lgrid), dim3(bmx::ROWS_BLOCK), 0, stream, d_off, capacity,
                           st->oo.h_status_dev, st->d_words);
        BMX_HIP(what, hipMemcpyAsync(st->h_words, st->d_words, bmx::ROWS_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    }
    uint64_t rows = 0;
    rc = st->oo.finish(what, grid, a.n_tiles, stream, ~0ull, &rows, err, errlen);
    st->last_ms = st->oo.last_ms;
    if (rc != BMX_OK) return rc;
    if (n_rows) *n_rows = rows;
    const bool complete = capacity >= rows + 1;
    if (longest) {
        if (complete) {
            *longest = st->h_words[1];
        } else { // the offsets did not all go to the caller: once more into the workspace
            rc = work_ready(st, pad256((rows + 1) * sizeof(uint64_t)), what, err, errlen);
            if (rc != BMX_OK) return rc;
            const float ms = st->last_ms;
            rc = bmx_internal_rows_split(state_v, num_cu, d_text, n, base_offset, delim, static_cast<uint64_t *>(st->d_work), rows + 1,
                                         nullptr, longest, stream, err, errlen);
            st->last_ms = st->last_ms >= 0.0f ? st->last_ms + ms : ms;
            work_release(st);
            if (rc != BMX_OK) return rc;
        }
    }
    return complete || capacity == 0 ? BMX_OK : BMX_ERR_CAPACITY;
}

int bmx_internal_rows_of(void **state_v, const uint64_t *d_off, uint64_t rows, const uint64_t *d_starts, const uint64_t *d_ends,
                         uint64_t len, uint64_t count, uint64_t *d_row, hipStream_t stream, char *err, size_t errlen)
{
    const char *what = "bmx_rows_of_device";
    RowsHost *st = nullptr;
    const int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    hipLaunchKernelGGL(bmx::rows_of_kernel, dim3(grid_for(count)), dim3(bmx::ROWS_BLOCK), 0, stream, d_off, rows, d_starts, d_ends,
                       len, count, d_row);
    BMX_HIP(what, hipGetLastError());
    BMX_HIP(what, hipEventRecord(st->ev[1], stream));
    BMX_HIP(what, hipStreamSynchronize(stream));
    if (hipEventElapsedTime(&st->last_ms, st->ev[0], st->ev[1]) != hipSuccess) st->last_ms = -1.0f;
    return BMX_OK;
}

int bmx_internal_rows_matching(void **state_v, const uint64_t *d_row, uint64_t count, uint64_t rows, uint32_t flags,
                               uint64_t *d_rows_out, uint64_t *d_counts_out, uint64_t capacity, uint64_t *n_out, hipStream_t stream,
                               char *err, size_t errlen)
{
    const char *what = "bmx_rows_matching_device";
    RowsHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    if (n_out) *n_out = 0;
    const bool invert = (flags & BMX_ROWS_INVERT) != 0;
    const dim3 block(bmx::ROWS_BLOCK);

    // summaries (4 per tile) | carries (3 per tile) | total | first (count + 2) | hit (count + 1, the inverted call's heads)
    const uint64_t tiles = std::max<uint64_t>(grid_for(count), 1);
    const size_t b_sum = pad256(4 * tiles * sizeof(uint64_t)), b_carry = pad256(3 * tiles * sizeof(uint64_t)), b_total = 256;
    const bool want_counts = !invert && d_counts_out != nullptr && capacity > 0;
    const size_t b_first = want_counts ? pad256((count + 2) * sizeof(uint64_t)) : 0; // (only the counts read it)
    const size_t b_hit = invert ? pad256((count + 1) * sizeof(uint64_t)) : 0;
    rc = work_ready(st, b_sum + b_carry + b_total + b_first + b_hit, what, err, errlen);
    if (rc != BMX_OK) return rc;
    char *p = static_cast<char *>(st->d_work);
    uint64_t *summary = reinterpret_cast<uint64_t *>(p);
    uint64_t *carry = reinterpret_cast<uint64_t *>(p + b_sum);
    bmx::RowsPair *total = reinterpret_cast<bmx::RowsPair *>(p + b_sum + b_carry);
    uint64_t *first = reinterpret_cast<uint64_t *>(p + b_sum + b_carry + b_total);
    uint64_t *hit = reinterpret_cast<uint64_t *>(p + b_sum + b_carry + b_total + b_first);

    BMX_HIP(what, hipMemsetAsync(st->d_words, 0, bmx::ROWS_WORDS * sizeof(uint64_t), stream));
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    hipLaunchKernelGGL(bmx::rows_summary_kernel, dim3((uint32_t)tiles), block, 0, stream, d_row, count, summary);
    hipLaunchKernelGGL(bmx::rows_carry_kernel, dim3(1), block, 0, stream, summary, tiles, carry, total, want_counts ? first : nullptr,
                       st->d_words);
    if (!invert) {
        hipLaunchKernelGGL(bmx::rows_heads_kernel, dim3((uint32_t)tiles), block, 0, stream, d_row, count, rows, carry,
                           capacity ? d_rows_out : nullptr, want_counts ? first : nullptr, capacity, st->d_words);
        if (want_counts && count) // (an empty list has no row to count, and no launch has an empty grid)
            hipLaunchKernelGGL(bmx::rows_counts_kernel, dim3(grid_for(std::min(count, capacity))), block, 0, stream, first, total,
                               d_counts_out, capacity);
    } else {
        hipLaunchKernelGGL(bmx::rows_heads_kernel, dim3((uint32_t)tiles), block, 0, stream, d_row, count, rows, carry, hit,
                           (uint64_t *)nullptr, count, st->d_words);
        const uint64_t most = std::min(rows, capacity);
        if (most)
            hipLaunchKernelGGL(bmx::rows_absent_kernel, dim3(grid_for(most)), block, 0, stream, hit, total, rows, d_rows_out, capacity);
    }
    BMX_HIP(what, hipGetLastError());
    BMX_HIP(what, hipEventRecord(st->ev[1], stream));
    BMX_HIP(what, hipMemcpyAsync(st->h_words, st->d_words, bmx::ROWS_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(what, hipStreamSynchronize(stream));
    if (hipEventElapsedTime(&st->last_ms, st->ev[0], st->ev[1]) != hipSuccess) st->last_ms = -1.0f;
    work_release(st);
    if (st->h_words[0]) {
        snprintf(err, errlen, "%s: d_row decreases (NONE entries skipped) or holds an id at or past `rows` other than the no-row id", what);
        return BMX_ERR_ARG;
    }
    const uint64_t heads = st->h_words[2];
    const uint64_t out = invert ? rows - heads : heads;
    if (n_out) *n_out = out;
    return out > capacity ? BMX_ERR_CAPACITY : BMX_OK;
}
