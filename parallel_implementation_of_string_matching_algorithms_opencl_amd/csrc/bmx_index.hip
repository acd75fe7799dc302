// bmx_index.hip -- host side of the text index (bmx_index_*, include/bmx.h): the index object (borrowed text, borrowed or
// owned suffix array, owned directory), and per context the status words, events and workspaces of the queries, kept
// between calls.  count = one launch of index_count_kernel; locate = that, rocPRIM's exclusive scan of the counts, the
// fill, rocPRIM's segmented radix sort of the 32-bit positions within their segments and the widening to base_offset + p.
// match = one launch of index_match_kernel (one lane per blob byte); seeds = that into workspace, rocPRIM's exclusive scan
// of the seed flags, the fill and the per-query offsets, with one wait at the end (bmx_index_match_kernel.h).
// map = the match kernel into workspace, rocPRIM's exclusive scan of the seeds' occurrence counts and its reduction to the
// longest seeded query, one wait for the candidate total, then the candidate fill, the verification, the start pass and
// the per-query best (bmx_index_map_kernel.h), and the wait at the end.
// Shared by the entries: make_query fills the kernels' query descriptor (IndexQuery, bmx_index_kernel.h), DevBuf is a
// workspace that grows with the calls (per query, per position or blob byte, per candidate), finish_phase is the tail in
// front of every wait that reads the status words, match_into_workspace is what seeds and map begin with, map_words
// picks map's instance.
// The argument checks and the context are the shim's (bmx_shim.hip); everything here runs on valid arguments.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmx.h"
#include "bmx_index_kernel.h"
#include "bmx_index_map_kernel.h"
#include "bmx_index_match_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::INDEX_MAX_PATTERN == BMX_MAX_PATTERN, "header and kernel disagree");
static_assert(bmx::MAP_NO_HIT == BMX_MAP_NO_HIT && bmx::INDEX_MAX_PATTERN <= 64 * 8, "header and kernel disagree");

struct bmx_index {
    const void *owner = nullptr; // the context it was created on
    int device = 0;
    const uint8_t *d_text = nullptr; // borrowed
    uint32_t n = 0;
    const int32_t *d_sa = nullptr; // borrowed, or own_sa
    int32_t *own_sa = nullptr;
    uint32_t *d_dir = nullptr; // INDEX_DIR_ENTRIES starts, then INDEX_DIR_ENTRIES counts
    float build_ms = 0.0f;
};

namespace {

constexpr int WS_WORDS = 5;
constexpr size_t KEEP_BYTES = 256ull << 20; // a larger per-position or per-candidate workspace is not kept between calls
constexpr uint64_t MIN_QUERIES = 1u << 16;  // the per-query workspace is never smaller

// A device buffer that a call grows to what it needs and that the next call finds again.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    char *at(size_t off) const { return static_cast<char *>(p) + off; }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr, bytes = 0;
    }
    int reserve(size_t need, const char *what, char *err, size_t errlen) // grows only; empty after a failure
    {
        if (need <= bytes) return BMX_OK;
        release();
        BMX_HIP(what, hipMalloc(&p, need));
        bytes = need;
        return BMX_OK;
    }
    void trim(size_t keep)
    {
        if (bytes > keep) release();
    }
};

struct IndexHost {
    uint64_t *d_ws = nullptr; // {bad offsets, bad byte, total, stored queries, stored positions}
    uint64_t *h_ws = nullptr; // pinned copy
    DevBuf d_q; // locate, per query: lo, cnt, 32-bit segment offsets
    DevBuf d_p; // locate, per stored position: two 32-bit key buffers; seeds and map, per blob byte: match_into_workspace;
                // behind either, rocPRIM's temporary storage
    DevBuf d_c; // per candidate of a map call: six 32-bit arrays
    int64_t map_candidates = -1; // of the last map call
    hipEvent_t mev[3] = {nullptr, nullptr, nullptr}; // ... behind its fill, its verification and its start pass
    float map_phase[5] = {-1.0f, -1.0f, -1.0f, -1.0f, 0.0f}; // ... ms of expansion, verification, starts, best; the instance's words
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float last_ms = -1.0f;
};

struct ToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

int state_ready(void **state_v, IndexHost **out, const char *what, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new IndexHost();
    IndexHost *st = static_cast<IndexHost *>(*state_v);
    st->last_ms = -1.0f;
    if (!st->d_ws) BMX_HIP(what, hipMalloc(&st->d_ws, WS_WORDS * sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(what, hipHostMalloc(&st->h_ws, WS_WORDS * sizeof(uint64_t), hipHostMallocDefault));
    for (hipEvent_t &e : st->ev)
        if (!e) BMX_HIP(what, hipEventCreate(&e));
    for (hipEvent_t &e : st->mev)
        if (!e) BMX_HIP(what, hipEventCreate(&e));
    *out = st;
    return BMX_OK;
}

bmx::IndexQuery make_query(const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off, uint64_t count,
                           bool use_dir, uint64_t *status)
{
    bmx::IndexQuery q = {};
    q.text = ix->d_text;
    q.n = ix->n;
    q.sa = ix->d_sa;
    q.pat = static_cast<const uint8_t *>(d_pat);
    q.pat_bytes = pat_bytes;
    q.pat_off = d_pat_off;
    q.count = count;
    q.dir_lo = use_dir ? ix->d_dir : nullptr;
    q.dir_cnt = use_dir ? ix->d_dir + bmx::INDEX_DIR_ENTRIES : nullptr;
    q.status = status;
    return q;
}

int status_rc(const uint64_t *h_ws, const char *what, char *err, size_t errlen)
{
    if (h_ws[0]) {
        snprintf(err, errlen, "%s: offsets that decrease or end past the blob, or a query of 0 or more than %d bytes", what,
                 BMX_MAX_PATTERN);
        return BMX_ERR_ARG;
    }
    if (h_ws[1]) {
        snprintf(err, errlen, "%s: a query byte >= 0x80", what);
        return BMX_ERR_DOMAIN;
    }
    return BMX_OK;
}

uint32_t blocks_for(uint64_t items) { return (uint32_t)((items + bmx::INDEX_BLOCK - 1) / bmx::INDEX_BLOCK); }

// The tail of a phase that began at `first`: the closing event, the status words to their pinned copy, the wait, and the
// phase's time in *ms, or -1.
int finish_phase(IndexHost *st, hipEvent_t first, hipEvent_t last, hipStream_t stream, const char *what, char *err, size_t errlen,
                 float *ms)
{
    BMX_HIP(what, hipEventRecord(last, stream));
    BMX_HIP(what, hipMemcpyAsync(st->h_ws, st->d_ws, WS_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(what, hipStreamSynchronize(stream));
    if (hipEventElapsedTime(ms, first, last) != hipSuccess) *ms = -1.0f;
    return BMX_OK;
}

void launch_match(const bmx::IndexMatchArgs &a, hipStream_t stream)
{
    const uint64_t lanes = std::max(a.q.pat_bytes, a.q.count);
    hipLaunchKernelGGL(bmx::index_match_kernel, dim3(blocks_for(lanes)), dim3(bmx::INDEX_BLOCK), 0, stream, a);
}

// an array of one 32-bit (or wider) entry per blob byte and one more, padded to 256 bytes
size_t per_byte_bytes(uint64_t pat_bytes, size_t entry = sizeof(uint32_t))
{
    return (((size_t)pat_bytes + 1) * entry + 255) & ~(size_t)255;
}

// What seeds and map begin with: the match kernel's answers for every blob byte in the per-position workspace, which
// holds qpos, len, lo, cnt (per_byte_bytes each) and then `extra_bytes` of the caller's, from `extra` on.  Zeroes the
// status words, marks every byte unanswered and opens the phase with ev[0].
struct MatchWork {
    uint32_t *qpos, *len, *lo, *cnt;
    char *extra;
};

int match_into_workspace(IndexHost *st, const bmx::IndexQuery &q, size_t extra_bytes, hipStream_t stream, MatchWork *w,
                         const char *what, char *err, size_t errlen)
{
    const size_t arr_bytes = per_byte_bytes(q.pat_bytes);
    const int rc = st->d_p.reserve(4 * arr_bytes + extra_bytes, what, err, errlen);
    if (rc != BMX_OK) return rc;
    w->qpos = reinterpret_cast<uint32_t *>(st->d_p.at(0)), w->len = reinterpret_cast<uint32_t *>(st->d_p.at(arr_bytes));
    w->lo = reinterpret_cast<uint32_t *>(st->d_p.at(2 * arr_bytes)), w->cnt = reinterpret_cast<uint32_t *>(st->d_p.at(3 * arr_bytes));
    w->extra = st->d_p.at(4 * arr_bytes);
    BMX_HIP(what, hipMemsetAsync(st->d_ws, 0, WS_WORDS * sizeof(uint64_t), stream));
    BMX_HIP(what, hipMemsetAsync(w->qpos, 0xff, arr_bytes, stream)); // INDEX_NO_QUERY: no lane has answered for this byte
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    launch_match({q, w->len, w->lo, w->cnt, w->qpos}, stream);
    BMX_HIP(what, hipGetLastError());
    return BMX_OK;
}

// the 64-bit words of the smallest map instance that covers a query of M bytes
int map_words(uint32_t M) { return M <= 64 ? 1 : M <= 128 ? 2 : M <= 256 ? 4 : 8; }

// one lane per blob byte, and one per query for its offsets
bool match_sizes_ok(uint64_t pat_bytes, uint64_t count) { return pat_bytes < 0x7fffffffull && count < 0x7fffffffull; }

} // namespace

void bmx_internal_index_state_free(void *state_v)
{
    IndexHost *st = static_cast<IndexHost *>(state_v);
    if (!st) return;
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    st->d_q.release();
    st->d_p.release();
    st->d_c.release();
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : st->mev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

float bmx_internal_index_ms(const void *state_v)
{
    const IndexHost *st = static_cast<const IndexHost *>(state_v);
    return st ? st->last_ms : -1.0f;
}

int64_t bmx_internal_index_map_candidates(const void *state_v)
{
    const IndexHost *st = static_cast<const IndexHost *>(state_v);
    return st ? st->map_candidates : -1;
}

int bmx_internal_index_map_phases(const void *state_v, float out[5])
{
    const IndexHost *st = static_cast<const IndexHost *>(state_v);
    if (!st || st->map_candidates < 0) return BMX_ERR_ARG;
    std::copy(st->map_phase, st->map_phase + 5, out);
    return BMX_OK;
}

const void *bmx_internal_index_owner(const bmx_index *ix) { return ix->owner; }
const int32_t *bmx_internal_index_sa(const bmx_index *ix) { return ix->d_sa; }
float bmx_internal_index_build_ms(const bmx_index *ix) { return ix->build_ms; }

void bmx_internal_index_destroy(bmx_index *ix)
{
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    if (ix->own_sa) (void)hipFree(ix->own_sa);
    if (ix->d_dir) (void)hipFree(ix->d_dir);
    delete ix;
}

int bmx_internal_index_create(void **state_v, bmx_ctx *ctx, int device, const void *d_text, uint64_t n, const int32_t *d_sa,
                              hipStream_t stream, bmx_index **out, char *err, size_t errlen)
{
    const char *what = "bmx_index_create_device";
    IndexHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    // A text that ends in two or more bytes 96 leaves suffixes tied in the builder's order: no interval to search.
    if (n >= 2) {
        uint8_t tail[2] = {0, 0};
        BMX_HIP(what, hipMemcpyAsync(tail, static_cast<const uint8_t *>(d_text) + (n - 2), 2, hipMemcpyDeviceToHost, stream));
        BMX_HIP(what, hipStreamSynchronize(stream));
        if (tail[0] == 96 && tail[1] == 96) {
            snprintf(err, errlen, "%s: the text ends in two or more bytes 96; the suffix array's order is unspecified there", what);
            return BMX_ERR_DOMAIN;
        }
    }
    bmx_index *ix = new bmx_index();
    ix->owner = ctx;
    ix->device = device;
    ix->d_text = static_cast<const uint8_t *>(d_text);
    ix->n = (uint32_t)n;
    ix->d_sa = d_sa;
    auto fail = [&](int code) {
        bmx_internal_index_destroy(ix);
        return code;
    };
    if (!d_sa) {
        hipError_t e = hipMalloc(&ix->own_sa, n * sizeof(int32_t));
        if (e != hipSuccess) {
            snprintf(err, errlen, "%s: %llu bytes for the suffix array: %s", what, (unsigned long long)(n * sizeof(int32_t)),
                     hipGetErrorString(e));
            return fail(BMX_ERR_HIP);
        }
        rc = bmx_suffix_array_device(ctx, d_text, n, ix->own_sa, stream);
        if (rc != BMX_OK) return fail(rc);
        ix->d_sa = ix->own_sa;
        ix->build_ms += std::max(0.0f, bmx_last_suffix_array_ms(ctx));
    }
    // The directory: the count kernel itself, without a directory, over all two-byte patterns.  Its boundary cases
    // then follow the comparator by construction.
    const uint32_t E = bmx::INDEX_DIR_ENTRIES;
    std::vector<uint8_t> blob(2 * E);
    std::vector<uint64_t> off(E + 1);
    for (uint32_t b = 0; b < E; ++b) blob[2 * b] = (uint8_t)(b / bmx::INDEX_DIR_SIDE), blob[2 * b + 1] = (uint8_t)(b % bmx::INDEX_DIR_SIDE);
    for (uint32_t b = 0; b <= E; ++b) off[b] = 2ull * b;
    uint8_t *d_tmp = nullptr;
    const size_t off_at = 2 * E; // (a multiple of 8)
    hipError_t e = hipMalloc(&d_tmp, off_at + (E + 1) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&ix->d_dir, 2 * E * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpyAsync(d_tmp, blob.data(), blob.size(), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tmp + off_at, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(st->d_ws, 0, WS_WORDS * sizeof(uint64_t), stream);
    if (e == hipSuccess) e = hipEventRecord(st->ev[0], stream);
    if (e == hipSuccess) {
        const bmx::IndexArgs a = {make_query(ix, d_tmp, 2 * E, reinterpret_cast<const uint64_t *>(d_tmp + off_at), E, false, st->d_ws),
                                  ix->d_dir, ix->d_dir + E};
        hipLaunchKernelGGL(bmx::index_count_kernel, dim3(blocks_for(E)), dim3(bmx::INDEX_BLOCK), 0, stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(st->ev[1], stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream); // (the host blobs above are read until here)
    if (d_tmp) (void)hipFree(d_tmp);
    if (e != hipSuccess) {
        snprintf(err, errlen, "%s: directory: %s", what, hipGetErrorString(e));
        return fail(BMX_ERR_HIP);
    }
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, st->ev[0], st->ev[1]) == hipSuccess) ix->build_ms += ms;
    *out = ix;
    return BMX_OK;
}

int bmx_internal_index_count(void **state_v, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                             uint64_t count, uint32_t *d_lo, uint32_t *d_cnt, int use_dir, hipStream_t stream, char *err,
                             size_t errlen)
{
    const char *what = "bmx_index_count_device";
    if (blocks_for(count) == 0 || count > 0x7fffffffull * bmx::INDEX_BLOCK) {
        snprintf(err, errlen, "%s: too many queries for one launch", what);
        return BMX_ERR_ARG;
    }
    IndexHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    BMX_HIP(what, hipMemsetAsync(st->d_ws, 0, WS_WORDS * sizeof(uint64_t), stream));
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    const bmx::IndexArgs a = {make_query(ix, d_pat, pat_bytes, d_pat_off, count, use_dir != 0, st->d_ws), d_lo, d_cnt};
    hipLaunchKernelGGL(bmx::index_count_kernel, dim3(blocks_for(count)), dim3(bmx::INDEX_BLOCK), 0, stream, a);
    BMX_HIP(what, hipGetLastError());
    rc = finish_phase(st, st->ev[0], st->ev[1], stream, what, err, errlen, &st->last_ms);
    return rc != BMX_OK ? rc : status_rc(st->h_ws, what, err, errlen);
}

int bmx_internal_index_locate(void **state_v, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes,
                              const uint64_t *d_pat_off, uint64_t count, uint64_t base_offset, uint64_t *d_out_off, uint64_t *d_pos,
                              uint64_t capacity, uint64_t *n_matches, int use_dir, hipStream_t stream, char *err, size_t errlen)
{
    const char *what = "bmx_index_locate_device";
    if (count >= 0x7fffffffull) { // the scan and the segmented sort take 32-bit sizes
        snprintf(err, errlen, "%s: 2^31 - 1 queries or more in one call", what);
        return BMX_ERR_ARG;
    }
    IndexHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    const uint64_t q_cap = std::max(count, MIN_QUERIES);
    rc = st->d_q.reserve(3 * (q_cap + 1) * sizeof(uint32_t), what, err, errlen);
    if (rc != BMX_OK) return rc;
    uint32_t *d_lo = static_cast<uint32_t *>(st->d_q.p), *d_cnt = d_lo + (q_cap + 1), *d_seg = d_cnt + (q_cap + 1);

    // counts, their exclusive scan (count + 1 entries: the last one is the total), the stored prefix of the queries
    BMX_HIP(what, hipMemsetAsync(st->d_ws, 0, WS_WORDS * sizeof(uint64_t), stream));
    // (entry `count` stays 0; so does a lane's that fails)
    BMX_HIP(what, hipMemsetAsync(d_cnt, 0, (count + 1) * sizeof(uint32_t), stream));
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    const bmx::IndexArgs a = {make_query(ix, d_pat, pat_bytes, d_pat_off, count, use_dir != 0, st->d_ws), d_lo, d_cnt};
    hipLaunchKernelGGL(bmx::index_count_kernel, dim3(blocks_for(count)), dim3(bmx::INDEX_BLOCK), 0, stream, a);
    BMX_HIP(what, hipGetLastError());
    auto counts64 = rocprim::make_transform_iterator(static_cast<const uint32_t *>(d_cnt), ToU64());
    size_t scan_bytes = 0;
    BMX_HIP(what, rocprim::exclusive_scan(nullptr, scan_bytes, counts64, d_out_off, uint64_t(0), (size_t)count + 1,
                                          rocprim::plus<uint64_t>(), stream));
    rc = st->d_p.reserve(scan_bytes, what, err, errlen);
    if (rc != BMX_OK) return rc;
    BMX_HIP(what, rocprim::exclusive_scan(st->d_p.p, scan_bytes, counts64, d_out_off, uint64_t(0), (size_t)count + 1,
                                          rocprim::plus<uint64_t>(), stream));
    hipLaunchKernelGGL(bmx::index_prefix_kernel, dim3(blocks_for(count + 1)), dim3(bmx::INDEX_BLOCK), 0, stream, d_out_off, count,
                       capacity, d_seg, st->d_ws + 2);
    BMX_HIP(what, hipGetLastError());
    rc = finish_phase(st, st->ev[0], st->ev[1], stream, what, err, errlen, &st->last_ms);
    if (rc == BMX_OK) rc = status_rc(st->h_ws, what, err, errlen);
    if (rc != BMX_OK) return rc;
    const uint64_t total = st->h_ws[2], stored_queries = st->h_ws[3], stored = st->h_ws[4];
    if (n_matches) *n_matches = total;
    const int rc_done = total > capacity ? BMX_ERR_CAPACITY : BMX_OK;
    if (stored == 0) return rc_done;
    if (stored >= 0x7fffffffull) {
        snprintf(err, errlen, "%s: 2^31 - 1 positions or more to store in one call (%llu); pass fewer queries at a time", what,
                 (unsigned long long)stored);
        return BMX_ERR_ARG;
    }

    // fill, ascending order within every segment, widen
    const size_t keys_bytes = ((stored * sizeof(uint32_t)) + 255) & ~(size_t)255;
    uint32_t end_bit = 1;
    while (end_bit < 32 && (ix->n - 1) >> end_bit) ++end_bit;
    size_t sort_bytes = 0;
    BMX_HIP(what, rocprim::segmented_radix_sort_keys(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                                     (unsigned)stored, (unsigned)stored_queries, d_seg, d_seg + 1, 0, end_bit,
                                                     stream));
    rc = st->d_p.reserve(2 * keys_bytes + sort_bytes, what, err, errlen);
    if (rc != BMX_OK) return rc;
    uint32_t *keys_in = reinterpret_cast<uint32_t *>(st->d_p.at(0));
    uint32_t *keys_out = reinterpret_cast<uint32_t *>(st->d_p.at(keys_bytes));
    void *sort_tmp = st->d_p.at(2 * keys_bytes);
    BMX_HIP(what, hipEventRecord(st->ev[2], stream));
    hipLaunchKernelGGL(bmx::index_fill_kernel, dim3(blocks_for(stored_queries)), dim3(bmx::INDEX_BLOCK), 0, stream, ix->d_sa, d_lo,
                       d_cnt, d_out_off, stored_queries, keys_in);
    BMX_HIP(what, hipGetLastError());
    BMX_HIP(what, rocprim::segmented_radix_sort_keys(sort_tmp, sort_bytes, keys_in, keys_out, (unsigned)stored,
                                                     (unsigned)stored_queries, d_seg, d_seg + 1, 0, end_bit, stream));
    hipLaunchKernelGGL(bmx::index_widen_kernel, dim3(blocks_for(stored)), dim3(bmx::INDEX_BLOCK), 0, stream, keys_out, stored,
                       base_offset, d_pos);
    BMX_HIP(what, hipGetLastError());
    BMX_HIP(what, hipEventRecord(st->ev[3], stream));
    BMX_HIP(what, hipStreamSynchronize(stream));
    float ms = 0.0f;
    if (st->last_ms >= 0.0f && hipEventElapsedTime(&ms, st->ev[2], st->ev[3]) == hipSuccess) st->last_ms += ms;
    st->d_p.trim(KEEP_BYTES);
    return rc_done;
}

int bmx_internal_index_match(void **state_v, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                             uint64_t count, uint32_t *d_len, uint32_t *d_lo, uint32_t *d_cnt, int use_dir, hipStream_t stream,
                             char *err, size_t errlen)
{
    const char *what = "bmx_index_match_device";
    if (!match_sizes_ok(pat_bytes, count)) {
        snprintf(err, errlen, "%s: 2^31 - 1 blob bytes or queries or more in one call", what);
        return BMX_ERR_ARG;
    }
    IndexHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    BMX_HIP(what, hipMemsetAsync(st->d_ws, 0, WS_WORDS * sizeof(uint64_t), stream));
    BMX_HIP(what, hipEventRecord(st->ev[0], stream));
    launch_match({make_query(ix, d_pat, pat_bytes, d_pat_off, count, use_dir != 0, st->d_ws), d_len, d_lo, d_cnt, nullptr}, stream);
    BMX_HIP(what, hipGetLastError());
    rc = finish_phase(st, st->ev[0], st->ev[1], stream, what, err, errlen, &st->last_ms);
    return rc != BMX_OK ? rc : status_rc(st->h_ws, what, err, errlen);
}

int bmx_internal_index_seeds(void **state_v, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                             uint64_t count, uint32_t min_len, uint32_t max_occ, uint64_t *d_seed_off, uint32_t *d_qpos,
                             uint32_t *d_len, uint32_t *d_lo, uint32_t *d_cnt, uint64_t capacity, uint64_t *n_seeds, int use_dir,
                             hipStream_t stream, char *err, size_t errlen)
{
    const char *what = "bmx_index_seeds_device";
    if (!match_sizes_ok(pat_bytes, count)) {
        snprintf(err, errlen, "%s: 2^31 - 1 blob bytes or queries or more in one call", what);
        return BMX_ERR_ARG;
    }
    IndexHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;

    // behind the match kernel's arrays: the scan's slots (pat_bytes + 1 entries), then rocPRIM's temporary storage
    const size_t arr_bytes = per_byte_bytes(pat_bytes);
    bmx::IndexSeedFlag flag = {nullptr, nullptr, nullptr, pat_bytes, min_len, max_occ};
    size_t scan_bytes = 0;
    BMX_HIP(what, rocprim::exclusive_scan(nullptr, scan_bytes,
                                          rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), flag),
                                          (uint32_t *)nullptr, uint32_t(0), (size_t)pat_bytes + 1, rocprim::plus<uint32_t>(), stream));
    MatchWork w;
    rc = match_into_workspace(st, make_query(ix, d_pat, pat_bytes, d_pat_off, count, use_dir != 0, st->d_ws), arr_bytes + scan_bytes,
                              stream, &w, what, err, errlen);
    if (rc != BMX_OK) return rc;
    uint32_t *w_slot = reinterpret_cast<uint32_t *>(w.extra);
    void *scan_tmp = w.extra + arr_bytes;
    flag.qpos = w.qpos, flag.len = w.len, flag.cnt = w.cnt;
    auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), flag);
    BMX_HIP(what, rocprim::exclusive_scan(scan_tmp, scan_bytes, flags, w_slot, uint32_t(0), (size_t)pat_bytes + 1,
                                          rocprim::plus<uint32_t>(), stream));
    if (capacity > 0 && pat_bytes > 0) {
        hipLaunchKernelGGL(bmx::index_seed_fill_kernel, dim3(blocks_for(pat_bytes)), dim3(bmx::INDEX_BLOCK), 0, stream, flag, w_slot,
                           w.lo, capacity, d_qpos, d_len, d_lo, d_cnt);
        BMX_HIP(what, hipGetLastError());
    }
    hipLaunchKernelGGL(bmx::index_seed_off_kernel, dim3(blocks_for(count + 1)), dim3(bmx::INDEX_BLOCK), 0, stream, d_pat_off, count,
                       pat_bytes, w_slot, d_seed_off, st->d_ws + 2);
    BMX_HIP(what, hipGetLastError());
    rc = finish_phase(st, st->ev[0], st->ev[1], stream, what, err, errlen, &st->last_ms);
    if (rc != BMX_OK) return rc;
    st->d_p.trim(KEEP_BYTES);
    rc = status_rc(st->h_ws, what, err, errlen);
    if (rc != BMX_OK) return rc;
    if (n_seeds) *n_seeds = st->h_ws[2];
    return st->h_ws[2] > capacity ? BMX_ERR_CAPACITY : BMX_OK;
}

namespace {

template <int W>
hipError_t map_launch(const bmx::IndexMapArgs &a, uint32_t longest, hipEvent_t between, hipStream_t stream)
{
    bmx::IndexMapArgs v = a;
    v.chunks = (longest + 2 * a.k + 7) / 8;
    hipLaunchKernelGGL(bmx::index_map_verify_kernel<W>, dim3(blocks_for(a.total)), dim3(bmx::INDEX_BLOCK), 0, stream, v);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(between, stream);
    if (e != hipSuccess) return e;
    v.chunks = (longest + a.k + 7) / 8;
    hipLaunchKernelGGL(bmx::index_map_start_kernel<W>, dim3(blocks_for(a.total)), dim3(bmx::INDEX_BLOCK), 0, stream, v);
    return hipGetLastError();
}

} // namespace

int bmx_internal_index_map(void **state_v, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                           uint64_t count, uint32_t min_len, uint32_t max_occ, uint32_t k, uint64_t base_offset,
                           uint64_t *d_best_start, uint64_t *d_best_end, uint8_t *d_best_dist, uint64_t *d_cand_off,
                           uint64_t *d_cand_start, uint64_t *d_cand_end, uint8_t *d_cand_dist, uint64_t capacity,
                           uint64_t *n_candidates, int use_dir, hipStream_t stream, char *err, size_t errlen)
{
    const char *what = "bmx_index_map_device";
    if (!match_sizes_ok(pat_bytes, count)) {
        snprintf(err, errlen, "%s: 2^31 - 1 blob bytes or queries or more in one call", what);
        return BMX_ERR_ARG;
    }
    IndexHost *st = nullptr;
    int rc = state_ready(state_v, &st, what, err, errlen);
    if (rc != BMX_OK) return rc;
    st->map_candidates = -1;

    // behind the match kernel's arrays: the scan of the candidates (64-bit, pat_bytes + 1 entries), then rocPRIM's
    // temporary storage of the scan and of the reduction
    const size_t scan_arr_bytes = per_byte_bytes(pat_bytes, sizeof(uint64_t));
    bmx::IndexMapCount cand = {{nullptr, nullptr, nullptr, pat_bytes, min_len, max_occ}};
    bmx::IndexMapSeededLen seeded = {d_pat_off, nullptr, pat_bytes};
    size_t scan_bytes = 0, red_bytes = 0;
    BMX_HIP(what, rocprim::exclusive_scan(nullptr, scan_bytes,
                                          rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), cand),
                                          (uint64_t *)nullptr, uint64_t(0), (size_t)pat_bytes + 1, rocprim::plus<uint64_t>(), stream));
    BMX_HIP(what, rocprim::reduce(nullptr, red_bytes,
                                  rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), seeded),
                                  (uint64_t *)nullptr, uint64_t(0), (size_t)count, bmx::IndexMapMax(), stream));
    const bmx::IndexQuery query = make_query(ix, d_pat, pat_bytes, d_pat_off, count, use_dir != 0, st->d_ws);
    MatchWork w;
    rc = match_into_workspace(st, query, scan_arr_bytes + std::max(scan_bytes, red_bytes), stream, &w, what, err, errlen);
    if (rc != BMX_OK) return rc;
    uint64_t *w_scan = reinterpret_cast<uint64_t *>(w.extra);
    void *tmp = w.extra + scan_arr_bytes;
    cand.flag.qpos = w.qpos, cand.flag.len = w.len, cand.flag.cnt = w.cnt;
    seeded.scan = w_scan;
    auto counts = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), cand);
    auto lens = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), seeded);
    BMX_HIP(what, rocprim::exclusive_scan(tmp, scan_bytes, counts, w_scan, uint64_t(0), (size_t)pat_bytes + 1,
                                          rocprim::plus<uint64_t>(), stream));
    hipLaunchKernelGGL(bmx::index_map_off_kernel, dim3(blocks_for(count + 1)), dim3(bmx::INDEX_BLOCK), 0, stream, d_pat_off, count,
                       pat_bytes, w_scan, d_cand_off, st->d_ws + 2);
    BMX_HIP(what, hipGetLastError());
    BMX_HIP(what, rocprim::reduce(tmp, red_bytes, lens, st->d_ws + 3, uint64_t(0), (size_t)count, bmx::IndexMapMax(), stream));
    rc = finish_phase(st, st->ev[0], st->ev[1], stream, what, err, errlen, &st->last_ms);
    if (rc != BMX_OK) return rc;
    auto trim = [&]() { st->d_p.trim(KEEP_BYTES), st->d_c.trim(KEEP_BYTES); };
    rc = status_rc(st->h_ws, what, err, errlen);
    if (rc != BMX_OK) {
        trim();
        return rc;
    }
    const uint64_t total = st->h_ws[2], longest = st->h_ws[3];
    if (n_candidates) *n_candidates = total;
    st->map_candidates = (int64_t)total;
    if (total > BMX_MAP_MAX_CANDIDATES) {
        trim();
        snprintf(err, errlen, "%s: %llu candidates, more than %llu; pass fewer queries at a time or a smaller max_occ", what,
                 (unsigned long long)total, (unsigned long long)BMX_MAP_MAX_CANDIDATES);
        return BMX_ERR_ARG;
    }

    bmx::IndexMapArgs a = {};
    a.q = query; // (both status words are 0: the match kernel has raised none)
    a.scan = w_scan, a.qpos = w.qpos, a.lo = w.lo;
    a.total = total, a.k = k;
    a.base_offset = base_offset;
    a.out_start = d_cand_start, a.out_end = d_cand_end, a.out_dist = d_cand_dist, a.capacity = capacity;
    a.best_start = d_best_start, a.best_end = d_best_end, a.best_dist = d_best_dist;
    BMX_HIP(what, hipEventRecord(st->ev[2], stream));
    int words = 0;
    if (total > 0) {
        const size_t col_bytes = ((size_t)total * sizeof(uint32_t) + 255) & ~(size_t)255;
        rc = st->d_c.reserve(6 * col_bytes, what, err, errlen);
        if (rc != BMX_OK) return rc;
        auto col = [&](size_t j) { return reinterpret_cast<uint32_t *>(st->d_c.at(j * col_bytes)); };
        a.cq = col(0), a.ci = col(1), a.cp = col(2), a.cend = col(3), a.cstart = col(4), a.cdist = col(5);
        hipLaunchKernelGGL(bmx::index_map_fill_kernel, dim3(blocks_for(total)), dim3(bmx::INDEX_BLOCK), 0, stream, a);
        BMX_HIP(what, hipGetLastError());
        BMX_HIP(what, hipEventRecord(st->mev[0], stream));
        // the smallest instance that covers the longest query with a seed
        const uint32_t M = (uint32_t)std::min<uint64_t>(longest, bmx::INDEX_MAX_PATTERN);
        words = map_words(M);
        BMX_HIP(what, words == 1   ? map_launch<1>(a, M, st->mev[1], stream)
                      : words == 2 ? map_launch<2>(a, M, st->mev[1], stream)
                      : words == 4 ? map_launch<4>(a, M, st->mev[1], stream)
                                   : map_launch<8>(a, M, st->mev[1], stream));
        BMX_HIP(what, hipEventRecord(st->mev[2], stream));
    }
    hipLaunchKernelGGL(bmx::index_map_best_kernel, dim3(blocks_for(count)), dim3(bmx::INDEX_BLOCK), 0, stream, a);
    BMX_HIP(what, hipGetLastError());
    float ms = 0.0f;
    rc = finish_phase(st, st->ev[2], st->ev[3], stream, what, err, errlen, &ms);
    if (rc != BMX_OK) return rc;
    // the phases, for tools/index_map_rate.py: expansion (seeds, scan, fill), verification, starts, best
    float *ph = st->map_phase;
    ph[0] = st->last_ms, ph[1] = ph[2] = 0.0f, ph[3] = -1.0f, ph[4] = (float)words;
    if (words) {
        float fill = 0.0f;
        if (hipEventElapsedTime(&fill, st->ev[2], st->mev[0]) == hipSuccess && ph[0] >= 0.0f) ph[0] += fill;
        if (hipEventElapsedTime(&ph[1], st->mev[0], st->mev[1]) != hipSuccess) ph[1] = -1.0f;
        if (hipEventElapsedTime(&ph[2], st->mev[1], st->mev[2]) != hipSuccess) ph[2] = -1.0f;
    }
    if (hipEventElapsedTime(&ph[3], words ? st->mev[2] : st->ev[2], st->ev[3]) != hipSuccess) ph[3] = -1.0f;
    if (st->last_ms >= 0.0f && ms >= 0.0f) st->last_ms += ms;
    trim();
    if (st->h_ws[0] || st->h_ws[1]) {
        snprintf(err, errlen, "%s: internal: %s", what,
                 st->h_ws[0] ? "a candidate failed its checks" : "a start pass disagrees with its verification");
        return BMX_ERR_HIP;
    }
    return capacity > 0 && total > capacity ? BMX_ERR_CAPACITY : BMX_OK;
}
