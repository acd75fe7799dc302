// bmx_align.hip -- host side of the alignments (bmx_align_device, include/bmx.h): keeps the status words,
// the workspace and the events between calls, finds the longest pattern of the column (one wait), picks the instance and
// runs the entries in launches that fit the kept workspace: align_kernel, rocPRIM's exclusive scan of the launch's run
// counts (it starts at the running total, which stays in device memory), align_fill_kernel.  The argument checks and the
// context are the shim's (bmx_shim.hip); everything here runs on a valid context with valid arguments.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <rocprim/types/future_value.hpp>

#include <algorithm>
#include <cstdio>

#include "bmx.h"
#include "bmx_align_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::ALIGN_MAX_PATTERN == BMX_ALIGN_MAX_PATTERN && bmx::ALIGN_MAX_K == BMX_ALIGN_MAX_K, "header and kernel disagree");
static_assert(bmx::ALIGN_NONE == BMX_ALIGN_NONE && bmx::ALIGN_NONE == BMX_MAP_NO_HIT, "header and kernel disagree");
static_assert(bmx::ALIGN_NO_POS == BMX_MAP_NO_POS, "header and kernel disagree");
static_assert(bmx::CIGAR_INS == BMX_CIGAR_INS && bmx::CIGAR_DEL == BMX_CIGAR_DEL && bmx::CIGAR_EQ == BMX_CIGAR_EQ &&
                  bmx::CIGAR_X == BMX_CIGAR_X,
              "header and kernel disagree");

namespace {

constexpr const char *WHERE = "bmx_align_device";
constexpr size_t KEEP_BYTES = BMX_ALIGN_WORKSPACE_BYTES; // no launch takes more workspace, so all of it is kept
constexpr int WS_WORDS = 4;                              // {bad entry, bad walk, running total of runs, longest pattern}

struct AlignHost {
    uint64_t *d_ws = nullptr;
    uint64_t *h_ws = nullptr; // pinned copy
    void *d_work = nullptr;   // one launch's columns, slots, run counts and rocPRIM's temporary storage
    size_t work_bytes = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float last_ms = -1.0f;
    int64_t last_launches = -1;
};

size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

template <typename T, int W>
void launch_align(const bmx::AlignArgs &a, bool band, hipStream_t stream)
{
    const uint64_t lanes = a.e1 - a.e0;
    const dim3 grid((uint32_t)((lanes + bmx::ALIGN_BLOCK - 1) / bmx::ALIGN_BLOCK));
    if constexpr (sizeof(T) == 8) { // (the band is never stored for 32-bit words: align_use_band)
        if (band) {
            hipLaunchKernelGGL((bmx::align_kernel<T, W, true>), grid, dim3(bmx::ALIGN_BLOCK), 0, stream, a);
            return;
        }
    }
    hipLaunchKernelGGL((bmx::align_kernel<T, W, false>), grid, dim3(bmx::ALIGN_BLOCK), 0, stream, a);
}

} // namespace

void bmx_internal_align_free(void *state_v)
{
    AlignHost *st = static_cast<AlignHost *>(state_v);
    if (!st) return;
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    if (st->d_work) (void)hipFree(st->d_work);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

float bmx_internal_align_ms(const void *state_v)
{
    const AlignHost *st = static_cast<const AlignHost *>(state_v);
    return st ? st->last_ms : -1.0f;
}

int64_t bmx_internal_align_launches(const void *state_v)
{
    const AlignHost *st = static_cast<const AlignHost *>(state_v);
    return st ? st->last_launches : -1;
}

int bmx_internal_align(void **state_v, uint64_t ws_cap, const void *d_text, uint64_t n, uint64_t base_offset, const void *d_pat,
                       uint64_t pat_bytes, const uint64_t *d_pat_off, uint64_t pat_count, const uint32_t *d_pid,
                       const uint64_t *d_start, const uint64_t *d_end, uint64_t count, uint32_t k, uint8_t *d_dist,
                       uint64_t *d_op_off, uint32_t *d_ops, uint64_t capacity, uint64_t *n_ops, hipStream_t stream, char *err,
                       size_t errlen)
{
    if (!*state_v) *state_v = new AlignHost();
    AlignHost *st = static_cast<AlignHost *>(*state_v);
    st->last_ms = -1.0f;
    st->last_launches = -1;
    if (!st->d_ws) BMX_HIP(WHERE, hipMalloc(&st->d_ws, WS_WORDS * sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE, hipHostMalloc(&st->h_ws, WS_WORDS * sizeof(uint64_t), hipHostMallocDefault));
    for (hipEvent_t &e : st->ev)
        if (!e) BMX_HIP(WHERE, hipEventCreate(&e));
    const size_t keep = ws_cap ? std::min<size_t>(ws_cap, KEEP_BYTES) : KEEP_BYTES;

    // the longest pattern of the column: the instance and the chunk count (the one wait in between)
    auto lens = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), bmx::AlignPatLen{d_pat_off});
    size_t red_bytes = 0;
    BMX_HIP(WHERE, rocprim::reduce(nullptr, red_bytes, lens, (uint64_t *)nullptr, uint64_t(0), (size_t)pat_count, bmx::AlignMax(), stream));
    if (st->work_bytes < pad256(red_bytes)) {
        if (st->d_work) (void)hipFree(st->d_work);
        st->d_work = nullptr, st->work_bytes = 0;
        BMX_HIP(WHERE, hipMalloc(&st->d_work, pad256(red_bytes)));
        st->work_bytes = pad256(red_bytes);
    }
    BMX_HIP(WHERE, hipMemsetAsync(st->d_ws, 0, WS_WORDS * sizeof(uint64_t), stream));
    BMX_HIP(WHERE, hipEventRecord(st->ev[0], stream));
    BMX_HIP(WHERE, rocprim::reduce(st->d_work, red_bytes, lens, st->d_ws + 3, uint64_t(0), (size_t)pat_count, bmx::AlignMax(), stream));
    BMX_HIP(WHERE, hipEventRecord(st->ev[1], stream));
    BMX_HIP(WHERE, hipMemcpyAsync(st->h_ws, st->d_ws, WS_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE, hipStreamSynchronize(stream));
    // (a longer pattern is a bad entry if an entry takes it: the kernel says so)
    const uint32_t M = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(st->h_ws[3], 1), bmx::ALIGN_MAX_PATTERN);
    const int W = M <= 64 ? 1 : M <= 128 ? 2 : M <= 256 ? 4 : 8;
    const int word_bytes = M <= 32 ? 4 : 8;
    const uint32_t chunks = (M + k + 7) / 8;
    const uint32_t slot_words = 2 * k + 1;

    // entries per launch: whole waves, as many as the kept workspace holds (at least one wave)
    const bool band = bmx::align_use_band(k, word_bytes, W);
    const size_t wave_bytes = 64 * (bmx::align_entry_col_bytes(chunks, word_bytes, W, k) + (size_t)(slot_words + 1) * sizeof(uint32_t));
    size_t scan_bytes = 0;
    auto init = rocprim::future_value<uint64_t, const uint64_t *>(st->d_ws + 2);
    uint64_t per_launch = 0;
    {
        const uint64_t waves_all = (count + 63) / 64;
        const uint64_t waves_fit = std::max<uint64_t>((keep > (1u << 20) ? keep - (1u << 20) : 0) / wave_bytes, 1); // (1 MiB: the scan's storage)
        per_launch = std::min(waves_all, waves_fit) * 64;
        if (per_launch > 0x7fffffffull * bmx::ALIGN_BLOCK) per_launch = 0x7fffffffull * bmx::ALIGN_BLOCK;
    }
    BMX_HIP(WHERE, rocprim::exclusive_scan(nullptr, scan_bytes,
                                           rocprim::make_transform_iterator((const uint32_t *)nullptr, bmx::AlignToU64()),
                                           (uint64_t *)nullptr, init, (size_t)per_launch, rocprim::plus<uint64_t>(), stream));
    const size_t col_bytes = pad256((per_launch / 64) * 64 * bmx::align_entry_col_bytes(chunks, word_bytes, W, k));
    const size_t slot_bytes = pad256(per_launch * slot_words * sizeof(uint32_t));
    const size_t runs_bytes = pad256(per_launch * sizeof(uint32_t));
    const size_t need = col_bytes + slot_bytes + runs_bytes + pad256(scan_bytes);
    if (st->work_bytes < need) {
        if (st->d_work) (void)hipFree(st->d_work);
        st->d_work = nullptr, st->work_bytes = 0;
        BMX_HIP(WHERE, hipMalloc(&st->d_work, need));
        st->work_bytes = need;
    }
    char *work = static_cast<char *>(st->d_work);

    bmx::AlignArgs a = {};
    a.text = static_cast<const uint8_t *>(d_text);
    a.n = n, a.base_offset = base_offset;
    a.pat = static_cast<const uint8_t *>(d_pat);
    a.pat_bytes = pat_bytes, a.pat_off = d_pat_off, a.pat_count = pat_count;
    a.pid = d_pid, a.start = d_start, a.end = d_end;
    a.one = !d_pid && pat_count == 1 && count != 1 ? 1u : 0u; // (a single entry is the same either way)
    a.k = k, a.chunks = chunks;
    a.dist = d_dist;
    a.cols = work;
    a.slots = reinterpret_cast<uint32_t *>(work + col_bytes);
    a.nruns = reinterpret_cast<uint32_t *>(work + col_bytes + slot_bytes);
    a.status = st->d_ws;
    void *scan_tmp = work + col_bytes + slot_bytes + runs_bytes;
    auto runs64 = rocprim::make_transform_iterator(static_cast<const uint32_t *>(a.nruns), bmx::AlignToU64());

    BMX_HIP(WHERE, hipEventRecord(st->ev[2], stream));
    int64_t launches = 0;
    for (uint64_t e0 = 0; e0 < count; e0 += per_launch, ++launches) {
        a.e0 = e0, a.e1 = std::min(count, e0 + per_launch);
        if (word_bytes == 4) launch_align<uint32_t, 1>(a, false, stream);
        else if (W == 1) launch_align<uint64_t, 1>(a, band, stream);
        else if (W == 2) launch_align<uint64_t, 2>(a, band, stream);
        else if (W == 4) launch_align<uint64_t, 4>(a, band, stream);
        else launch_align<uint64_t, 8>(a, band, stream);
        BMX_HIP(WHERE, hipGetLastError());
        BMX_HIP(WHERE, rocprim::exclusive_scan(scan_tmp, scan_bytes, runs64, d_op_off + e0, init, (size_t)(a.e1 - a.e0),
                                               rocprim::plus<uint64_t>(), stream));
        hipLaunchKernelGGL(bmx::align_fill_kernel, dim3((uint32_t)((a.e1 - a.e0 + bmx::ALIGN_BLOCK - 1) / bmx::ALIGN_BLOCK)),
                           dim3(bmx::ALIGN_BLOCK), 0, stream, a.e0, a.e1, k, a.nruns, a.slots, d_op_off, d_ops, capacity,
                           st->d_ws + 2);
        BMX_HIP(WHERE, hipGetLastError());
    }
    BMX_HIP(WHERE, hipEventRecord(st->ev[3], stream));
    BMX_HIP(WHERE, hipMemcpyAsync(st->h_ws, st->d_ws, WS_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE, hipStreamSynchronize(stream));
    float ms0 = -1.0f, ms1 = -1.0f;
    if (hipEventElapsedTime(&ms0, st->ev[0], st->ev[1]) == hipSuccess && hipEventElapsedTime(&ms1, st->ev[2], st->ev[3]) == hipSuccess)
        st->last_ms = ms0 + ms1;
    st->last_launches = launches;
    if (st->work_bytes > KEEP_BYTES) { // (one wave of the largest shape stays far below it)
        (void)hipFree(st->d_work);
        st->d_work = nullptr, st->work_bytes = 0;
    }
    if (st->h_ws[0]) {
        snprintf(err, errlen,
                 "%s: an entry with a pattern id or offsets outside the column, a pattern of 0 or more than %d bytes, a position "
                 "outside the text, end < start or one position without the other",
                 WHERE, BMX_ALIGN_MAX_PATTERN);
        return BMX_ERR_ARG;
    }
    if (st->h_ws[1]) {
        snprintf(err, errlen, "%s: internal: a walk left its slot or its band, or its edits are not its distance", WHERE);
        return BMX_ERR_HIP;
    }
    if (n_ops) *n_ops = st->h_ws[2];
    return capacity > 0 && st->h_ws[2] > capacity ? BMX_ERR_CAPACITY : BMX_OK;
}
