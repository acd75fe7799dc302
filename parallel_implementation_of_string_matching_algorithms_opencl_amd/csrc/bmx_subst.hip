// bmx_subst.hip -- host side of the non-overlapping match selection, replace and extract (bmx_spans_select*, bmx_replace*,
// bmx_extract*, include/bmx.h) and of the copy with a template (bmx_expand_device): per context four status words with their pinned copy, the workspace (keys,
// prefix maxima, chain levels, flags, slots, pieces, rocPRIM's scratch), the device copy of the replacement and the events,
// kept between calls as bmx_rows.hip keeps the rows'.  The kernels are in bmx_subst_kernel.h.  The argument checks and
// the context are the shim's (bmx_shim.hip); everything here runs on valid arguments.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_subst_kernel.h"

static_assert(bmx::SUBST_NONE == BMX_ROW_NONE, "header and kernel disagree");
static_assert((1u << bmx::SUBST_TILE_SHIFT) <= (uint32_t)bmx::SUBST_BLOCK, "a workgroup's LDS round holds whole tiles");

namespace {

constexpr size_t SUBST_WS_KEEP = (size_t)1 << 30; // a workspace up to this size stays in the state between calls
constexpr size_t MAX_REPL = BMX_MAX_REPLACEMENT;   // (by this name inside BMX_HIP, which keeps its expression as text)
constexpr int MAX_LEVELS = 12;                    // 2^32 entries at the smallest tile (2^3): 11 levels

struct SubstHost {
    unsigned long long *d_words = nullptr; // SUBST_WORDS status words: [0] bad list
    unsigned long long *h_words = nullptr; // pinned: [0] bad list, [1] the total (entries taken, regions, span bytes)
    void *d_work = nullptr;
    size_t work_bytes = 0;
    uint8_t *d_repl = nullptr; // BMX_MAX_REPLACEMENT bytes
    uint8_t *h_repl = nullptr; // pinned
    hipEvent_t ev[2] = {nullptr, nullptr};
    uint64_t last_shift = bmx::SUBST_TILE_SHIFT, last_levels = 0, last_tiles = 0; // the last select (bmx_exp_last_launch)
    bool lds_attr = false; // the copy kernel may take BMX_MAX_REPLACEMENT bytes of dynamic LDS
    bool lds_attr_expand = false; // ... and the copy kernel of a template
    float last_ms = -1.0f;
};

size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

int state_ready(void **state_v, SubstHost **out, const char *what, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new SubstHost();
    SubstHost *st = static_cast<SubstHost *>(*state_v);
    st->last_ms = -1.0f;
    if (!st->d_words) BMX_HIP(what, hipMalloc(&st->d_words, bmx::SUBST_WORDS * sizeof(uint64_t)));
    if (!st->h_words) BMX_HIP(what, hipHostMalloc(&st->h_words, bmx::SUBST_WORDS * sizeof(uint64_t), hipHostMallocDefault));
    for (hipEvent_t &e : st->ev)
        if (!e) BMX_HIP(what, hipEventCreate(&e));
    *out = st;
    return BMX_OK;
}

int work_ready(SubstHost *st, size_t need, const char *what, char *err, size_t errlen)
{
    if (st->work_bytes >= need) return BMX_OK;
    if (st->d_work) (void)hipFree(st->d_work);
    st->d_work = nullptr, st->work_bytes = 0;
    BMX_HIP(what, hipMalloc(&st->d_work, need));
    st->work_bytes = need;
    return BMX_OK;
}

void work_release(SubstHost *st)
{
    if (st->work_bytes <= SUBST_WS_KEEP) return; // a large one is not kept
    (void)hipFree(st->d_work);
    st->d_work = nullptr, st->work_bytes = 0;
}

uint32_t grid_for(uint64_t items) { return (uint32_t)((items + bmx::SUBST_BLOCK - 1) / bmx::SUBST_BLOCK); }

// the workspace of a call, handed out front to back
struct Carver {
    char *p;
    size_t used = 0;
    template <typename T>
    T *take(size_t items)
    {
        T *r = p ? reinterpret_cast<T *>(p + used) : nullptr;
        used += pad256(items * sizeof(T));
        return r;
    }
};

// the words of the call to the host, behind everything on the stream; then the wait and the time between the events
int finish(SubstHost *st, const uint64_t *d_total, const char *what, hipStream_t stream, char *err, size_t errlen)
{
    BMX_HIP(what, hipGetLastError());
    BMX_HIP(what, hipEventRecord(st->ev[1], stream));
    BMX_HIP(what, hipMemcpyAsync(st->h_words, st->d_words, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    if (d_total) BMX_HIP(what, hipMemcpyAsync(st->h_words + 1, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(what, hipStreamSynchronize(stream));
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, st->ev[0], st->ev[1]) != hipSuccess) ms = -1.0f;
    st->last_ms = (ms >= 0.0f && st->last_ms >= 0.0f) ? st->last_ms + ms : ms;
    return BMX_OK;
}

} // namespace

void bmx_internal_subst_free(void *state_v)
{
    SubstHost *st = static_cast<SubstHost *>(state_v);
    if (!st) return;
    if (st->d_words) (void)hipFree(st->d_words);
    if (st->h_words) (void)hipHostFree(st->h_words);
    if (st->d_work) (void)hipFree(st->d_work);
    if (st->d_repl) (void)hipFree(st->d_repl);
    if (st->h_repl) (void)hipHostFree(st->h_repl);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

float bmx_internal_subst_ms(const void *state_v) { return state_v ? static_cast<const SubstHost *>(state_v)->last_ms : -1.0f; }

// libbmx_exp.so's bmx_exp_last_launch, session "select": {log2 T, levels of pointer jumping, tiles of T entries} of the last select
void bmx_internal_subst_last(const void *state_v, uint64_t out3[3])
{
    const SubstHost *st = static_cast<const SubstHost *>(state_v);
    out3[0] = st ? st->last_shift : bmx::SUBST_TILE_SHIFT;
    out3[1] = st ? st->last_levels : 0;
    out3[2] = st ? st->last_tiles : 0;
}

int bmx_internal_select(void **state_v, int tile_shift, const uint64_t *d_starts, const uint64_t *d_ends, uint64_t len, uint64_t count,
                        const uint64_t *d_row, uint32_t flags, uint64_t *d_starts_out, uint64_t *d_ends_out, uint64_t *d_index_out,
                        uint64_t capacity, uint64_t *n_out, hipStream_t stream, char *err, size_t errlen)
{
    const char *what = "bmx_spans_select_device";
    SubstHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    const uint32_t shift = tile_shift ? (uint32_t)tile_shift : bmx::SUBST_TILE_SHIFT;
    const bool merge = (flags & BMX_SELECT_MERGE) != 0;
    const bmx::SubstList l{d_starts, d_ends, d_row, len, count};
    const dim3 block(bmx::SUBST_BLOCK);
    const uint32_t grid = grid_for(count), grid1 = grid_for(count + 1);

    // L: the smallest level at which at most T blocks of T^L entries remain
    int levels = 0;
    while (!merge && ((count - 1) >> (shift * (uint32_t)(levels + 1))) != 0) ++levels; // (count < 2^32: the shift stays below 64)
    st->last_shift = shift, st->last_levels = merge ? 0 : (uint64_t)levels, st->last_tiles = (count + (1ull << shift) - 1) >> shift;

    size_t scan_bytes = 0, sum_bytes = 0;
    BMX_HIP(what, rocprim::inclusive_scan(nullptr, scan_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)count,
                                          rocprim::maximum<uint64_t>(), stream));
    BMX_HIP(what, rocprim::exclusive_scan(nullptr, sum_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, uint64_t(0),
                                          (size_t)count + 1, rocprim::plus<uint64_t>(), stream));
    scan_bytes = std::max(scan_bytes, sum_bytes);

    // q[0..3]: count + 1 words each | X_0 .. X_L and one more buffer for the rounds | E_1 .. E_L | rocPRIM's scratch
    uint64_t *q[4];
    uint32_t *x[MAX_LEVELS + 2], *entry[MAX_LEVELS + 1];
    void *scan_tmp = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Carver c{pass ? static_cast<char *>(st->d_work) : nullptr};
        for (uint64_t *&b : q) b = c.take<uint64_t>(count + 1);
        if (!merge) {
            for (int v = 0; v <= levels + 1; ++v) x[v] = c.take<uint32_t>(count);
            for (int v = 1; v <= levels; ++v) entry[v] = c.take<uint32_t>(((count - 1) >> (shift * (uint32_t)v)) + 1);
        }
        scan_tmp = c.take<char>(scan_bytes);
        if (pass == 0) {
            rc = work_ready(st, c.used, what, err, errlen);
            if (rc != BMX_OK) return rc;
        }
    }

    BMX_HIP(what, hipMemsetAsync(st->d_words, 0, bmx::SUBST_WORDS * sizeof(uint64_t), stream));
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    const uint64_t *slot = nullptr;
    if (!merge) {
        uint64_t *key = q[0], *pm = q[1], *taken = q[2], *slots = q[3];
        hipLaunchKernelGGL(bmx::select_key_kernel, dim3(grid), block, 0, stream, l, key);
        BMX_HIP(what, rocprim::inclusive_scan(scan_tmp, scan_bytes, (const uint64_t *)key, pm, (size_t)count,
                                              rocprim::maximum<uint64_t>(), stream));
        hipLaunchKernelGGL(bmx::select_next_kernel, dim3(grid), block, 0, stream, l, (const uint64_t *)pm, x[0], st->d_words);
        uint32_t *spare = x[levels + 1];
        for (int v = 1; v <= levels; ++v) {
            if (v == 1) {
                hipLaunchKernelGGL(bmx::select_level1_kernel, dim3(grid), block, 0, stream, (const uint32_t *)x[0], x[1], count, shift);
                continue;
            }
            // `shift` rounds from X_(v-1), which stays, between X_v and the spare buffer so that the last one ends in X_v
            const uint32_t *in = x[v - 1];
            for (uint32_t r = 0; r < shift; ++r) {
                uint32_t *out = ((shift - 1 - r) & 1u) ? spare : x[v];
                hipLaunchKernelGGL(bmx::select_jump_kernel, dim3(grid), block, 0, stream, in, out, count, shift * (uint32_t)v);
                in = out;
            }
        }
        BMX_HIP(what, hipMemsetAsync(taken, 0, (count + 1) * sizeof(uint64_t), stream));
        for (int v = 1; v <= levels; ++v)
            BMX_HIP(what, hipMemsetAsync(entry[v], 0xff, (((count - 1) >> (shift * (uint32_t)v)) + 1) * sizeof(uint32_t), stream));
        hipLaunchKernelGGL(bmx::select_top_kernel, dim3(1), dim3(64), 0, stream, (const uint64_t *)pm, (const uint32_t *)x[levels], count,
                           shift * (uint32_t)levels, levels ? entry[levels] : (uint32_t *)nullptr, taken);
        for (int v = levels; v >= 1; --v) {
            const uint64_t blocks = ((count - 1) >> (shift * (uint32_t)v)) + 1;
            hipLaunchKernelGGL(bmx::select_descend_kernel, dim3(grid_for(blocks)), block, 0, stream, (const uint32_t *)entry[v], blocks,
                               (const uint32_t *)x[v - 1], count, shift * (uint32_t)v, shift * (uint32_t)(v - 1),
                               v > 1 ? entry[v - 1] : (uint32_t *)nullptr, taken);
        }
        BMX_HIP(what, rocprim::exclusive_scan(scan_tmp, scan_bytes, (const uint64_t *)taken, slots, uint64_t(0), (size_t)count + 1,
                                              rocprim::plus<uint64_t>(), stream));
        if (capacity)
            hipLaunchKernelGGL(bmx::select_fill_kernel, dim3(grid), block, 0, stream, l, (const uint64_t *)slots, d_starts_out, d_ends_out,
                               d_index_out, capacity);
        slot = slots;
    } else {
        uint64_t *pe_key = q[0], *sm_key = q[1], *pe = q[2], *sm = q[3];
        hipLaunchKernelGGL(bmx::merge_key_kernel, dim3(grid), block, 0, stream, l, pe_key, sm_key);
        BMX_HIP(what, rocprim::inclusive_scan(scan_tmp, scan_bytes, (const uint64_t *)pe_key, pe, (size_t)count,
                                              rocprim::maximum<uint64_t>(), stream));
        BMX_HIP(what, rocprim::inclusive_scan(scan_tmp, scan_bytes, (const uint64_t *)sm_key, sm, (size_t)count,
                                              rocprim::maximum<uint64_t>(), stream));
        uint64_t *head = q[1], *slots = q[0]; // (the keys are spent)
        hipLaunchKernelGGL(bmx::merge_heads_kernel, dim3(grid1), block, 0, stream, l, (const uint64_t *)pe, (const uint64_t *)sm, head,
                           st->d_words);
        BMX_HIP(what, rocprim::exclusive_scan(scan_tmp, scan_bytes, (const uint64_t *)head, slots, uint64_t(0), (size_t)count + 1,
                                              rocprim::plus<uint64_t>(), stream));
        if (capacity)
            hipLaunchKernelGGL(bmx::merge_fill_kernel, dim3(grid), block, 0, stream, count, (const uint64_t *)slots, (const uint64_t *)pe,
                               (const uint64_t *)sm, d_starts_out, d_ends_out, d_index_out, capacity);
        slot = slots;
    }
    st->last_ms = 0.0f;
    rc = finish(st, slot + count, what, stream, err, errlen);
    work_release(st);
    if (rc != BMX_OK) return rc;
    if (st->h_words[0]) {
        snprintf(err, errlen, "%s: the list is out of order (%s)", what,
                 merge ? "merging needs non-decreasing ends" : "an entry starts behind the end of a later one");
        return BMX_ERR_ARG;
    }
    *n_out = st->h_words[1];
    return (capacity && st->h_words[1] > capacity) ? BMX_ERR_CAPACITY : BMX_OK;
}

// replace (d_off == NULL) and extract (d_off: count + 1 offsets); count >= 1
int bmx_internal_subst_copy(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_starts,
                            const uint64_t *d_ends, uint64_t len, uint64_t count, const void *repl, uint64_t repl_len, void *d_out,
                            uint64_t capacity, uint64_t *d_off, uint64_t *n_out, hipStream_t stream, char *err, size_t errlen)
{
    const bool extract = d_off != nullptr;
    const char *what = extract ? "bmx_extract_device" : "bmx_replace_device";
    SubstHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    if (!extract && repl_len) {
        if (!st->d_repl) BMX_HIP(what, hipMalloc(&st->d_repl, MAX_REPL));
        if (!st->h_repl) BMX_HIP(what, hipHostMalloc(&st->h_repl, MAX_REPL, hipHostMallocDefault));
    }
    const bmx::SubstList l{d_starts, d_ends, nullptr, len, count};
    const bmx::SubstView v{base_offset, n};
    const dim3 block(bmx::SUBST_BLOCK);
    const uint64_t pieces = extract ? count : count + 1;

    size_t scan_bytes = 0;
    auto lens = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), bmx::SubstSpanLen{l});
    BMX_HIP(what, rocprim::exclusive_scan(nullptr, scan_bytes, lens, (uint64_t *)nullptr, uint64_t(0), (size_t)count + 1,
                                          rocprim::plus<uint64_t>(), stream));
    uint64_t *d = nullptr, *a = nullptr, *delta = nullptr;
    void *scan_tmp = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Carver c{pass ? static_cast<char *>(st->d_work) : nullptr};
        d = c.take<uint64_t>(count + 1);
        a = c.take<uint64_t>(pieces);
        delta = c.take<uint64_t>(pieces);
        scan_tmp = c.take<char>(scan_bytes);
        if (pass == 0) {
            rc = work_ready(st, c.used, what, err, errlen);
            if (rc != BMX_OK) return rc;
        }
    }
    if (extract) d = d_off;

    BMX_HIP(what, hipMemsetAsync(st->d_words, 0, bmx::SUBST_WORDS * sizeof(uint64_t), stream));
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    hipLaunchKernelGGL(bmx::copy_check_kernel, dim3(grid_for(count)), block, 0, stream, l, v, st->d_words);
    BMX_HIP(what, rocprim::exclusive_scan(scan_tmp, scan_bytes, lens, d, uint64_t(0), (size_t)count + 1, rocprim::plus<uint64_t>(), stream));
    st->last_ms = 0.0f;
    rc = finish(st, d + count, what, stream, err, errlen);
    if (rc != BMX_OK) return rc;
    if (st->h_words[0]) {
        work_release(st);
        snprintf(err, errlen, "%s: the spans are not ascending and pairwise disjoint, or one reaches outside the view", what);
        return BMX_ERR_ARG;
    }
    const uint64_t span_bytes = st->h_words[1];
    const uint64_t total = extract ? span_bytes : n - span_bytes + count * repl_len;
    *n_out = total;
    const uint64_t bytes = std::min(total, capacity);
    if (bytes) {
        if (!extract && repl_len) { // through pinned memory: the caller's buffer is free when the call returns, whatever the stream does
            memcpy(st->h_repl, repl, repl_len);
            BMX_HIP(what, hipMemcpyAsync(st->d_repl, st->h_repl, repl_len, hipMemcpyHostToDevice, stream));
        }
        BMX_HIP(what, hipEventRecord(st->ev[0], stream));
        hipLaunchKernelGGL(bmx::copy_pieces_kernel, dim3(grid_for(pieces)), block, 0, stream, l, v, (const uint64_t *)d,
                           extract ? 0 : repl_len, extract ? 1 : 0, a, delta);
        bmx::SubstCopyArgs g{};
        const uint64_t addr = reinterpret_cast<uint64_t>(d_out);
        g.text = static_cast<const uint8_t *>(d_text);
        g.a = a, g.delta = delta, g.pieces = pieces;
        g.repl = st->d_repl;
        g.lead = extract ? 0u : (uint32_t)repl_len;
        g.out16 = reinterpret_cast<uint8_t *>(addr & ~15ull);
        g.own_lo = addr & 15ull;
        g.own_hi = bytes + g.own_lo;
        g.n_tiles = (g.own_hi + bmx::SUBST_TILE - 1) / bmx::SUBST_TILE;
        const size_t lds = (g.lead + 15u) & ~(size_t)15;
        if (lds && !st->lds_attr) {
            BMX_HIP(what, hipFuncSetAttribute(reinterpret_cast<const void *>(bmx::subst_copy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)MAX_REPL));
            st->lds_attr = true;
        }
        const uint64_t per_cu = lds > 16384 ? 2 : 8; // (the replacement in LDS bounds the resident workgroups)
        const uint64_t grid = std::min<uint64_t>(g.n_tiles, (uint64_t)num_cu * per_cu);
        hipLaunchKernelGGL(bmx::subst_copy_kernel, dim3((uint32_t)grid), block, lds, stream, g);
        rc = finish(st, nullptr, what, stream, err, errlen);
        if (rc != BMX_OK) return rc;
    }
    work_release(st);
    return (capacity && total > capacity) ? BMX_ERR_CAPACITY : BMX_OK;
}

// replace (d_off == NULL) and extract with a template; count >= 1, a template that bmx_compile_template accepted
int bmx_internal_expand(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_groups,
                        int32_t n_groups, uint64_t count, const bmx_template *t, const uint8_t *lits, void *d_out, uint64_t capacity,
                        uint64_t *d_off, uint64_t *n_out, hipStream_t stream, char *err, size_t errlen)
{
    const bool extract = d_off != nullptr;
    const char *what = "bmx_expand_device";
    SubstHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    if (t->lit_bytes) {
        if (!st->d_repl) BMX_HIP(what, hipMalloc(&st->d_repl, MAX_REPL));
        if (!st->h_repl) BMX_HIP(what, hipHostMalloc(&st->h_repl, MAX_REPL, hipHostMallocDefault));
    }
    bmx::ExpandList l{};
    l.groups = d_groups;
    l.count = count;
    l.pairs = (uint32_t)n_groups + 1;
    l.t1 = (uint32_t)t->n_refs + 1;
    l.first = extract ? 0u : 1u;
    bmx::SubstTemplate tp{};
    tp.t1 = l.t1, tp.first = l.first;
    for (int32_t r = 0; r < t->n_refs; ++r) l.ref[r] = t->ref[r];
    for (uint32_t r = 0; r < l.t1; ++r) l.lit_len[r] = tp.len[r] = t->lit_len[r], tp.off[r] = t->lit_off[r];
    const bmx::SubstView v{base_offset, n};
    const dim3 block(bmx::SUBST_BLOCK);
    const uint64_t pieces = count * l.t1 + l.first;

    size_t scan_bytes = 0;
    auto lens = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), bmx::ExpandPieceLen{l, v});
    BMX_HIP(what, rocprim::exclusive_scan(nullptr, scan_bytes, lens, (uint64_t *)nullptr, uint64_t(0), (size_t)pieces + 1,
                                          rocprim::plus<uint64_t>(), stream));
    uint64_t *a = nullptr, *delta = nullptr;
    void *scan_tmp = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Carver c{pass ? static_cast<char *>(st->d_work) : nullptr};
        a = c.take<uint64_t>(pieces + 1);
        delta = c.take<uint64_t>(pieces);
        scan_tmp = c.take<char>(scan_bytes);
        if (pass == 0) {
            rc = work_ready(st, c.used, what, err, errlen);
            if (rc != BMX_OK) return rc;
        }
    }

    BMX_HIP(what, hipMemsetAsync(st->d_words, 0, bmx::SUBST_WORDS * sizeof(uint64_t), stream));
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    hipLaunchKernelGGL(bmx::expand_check_kernel, dim3(grid_for(count)), block, 0, stream, l, v, st->d_words);
    BMX_HIP(what, rocprim::exclusive_scan(scan_tmp, scan_bytes, lens, a, uint64_t(0), (size_t)pieces + 1, rocprim::plus<uint64_t>(), stream));
    st->last_ms = 0.0f;
    rc = finish(st, a + pieces, what, stream, err, errlen);
    if (rc != BMX_OK) return rc;
    if (st->h_words[0]) {
        work_release(st);
        snprintf(err, errlen, "%s: the matches (group 0) are not ascending, pairwise disjoint, non-empty and inside the view, or a group "
                 "reaches outside its match", what);
        return BMX_ERR_ARG;
    }
    const uint64_t total = st->h_words[1];
    *n_out = total;
    const uint64_t bytes = std::min(total, capacity);
    if (bytes || extract) {
        BMX_HIP(what, hipEventRecord(st->ev[0], stream));
        hipLaunchKernelGGL(bmx::expand_delta_kernel, dim3(grid_for(pieces)), block, 0, stream, l, v, (const uint64_t *)a, pieces, delta, d_off);
    }
    if (bytes) {
        if (t->lit_bytes) { // through pinned memory: the caller's buffer is free when the call returns, whatever the stream does
            memcpy(st->h_repl, lits, t->lit_bytes);
            BMX_HIP(what, hipMemcpyAsync(st->d_repl, st->h_repl, t->lit_bytes, hipMemcpyHostToDevice, stream));
        }
        bmx::SubstCopyArgs g{};
        const uint64_t addr = reinterpret_cast<uint64_t>(d_out);
        g.text = static_cast<const uint8_t *>(d_text);
        g.a = a, g.delta = delta, g.pieces = pieces;
        g.repl = st->d_repl;
        g.lead = t->lit_bytes;
        g.out16 = reinterpret_cast<uint8_t *>(addr & ~15ull);
        g.own_lo = addr & 15ull;
        g.own_hi = bytes + g.own_lo;
        g.n_tiles = (g.own_hi + bmx::SUBST_TILE - 1) / bmx::SUBST_TILE;
        const size_t lds = (g.lead + 15u) & ~(size_t)15;
        if (lds && !st->lds_attr_expand) {
            BMX_HIP(what, hipFuncSetAttribute(reinterpret_cast<const void *>(bmx::expand_copy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)MAX_REPL));
            st->lds_attr_expand = true;
        }
        const uint64_t per_cu = lds > 16384 ? 2 : 8; // (the literals in LDS bound the resident workgroups)
        const uint64_t grid = std::min<uint64_t>(g.n_tiles, (uint64_t)num_cu * per_cu);
        hipLaunchKernelGGL(bmx::expand_copy_kernel, dim3((uint32_t)grid), block, lds, stream, g, tp);
    }
    if (bytes || extract) {
        rc = finish(st, nullptr, what, stream, err, errlen);
        if (rc != BMX_OK) return rc;
    }
    work_release(st);
    return (capacity && total > capacity) ? BMX_ERR_CAPACITY : BMX_OK;
}
