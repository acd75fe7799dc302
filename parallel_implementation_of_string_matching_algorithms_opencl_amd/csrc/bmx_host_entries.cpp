// bmx_host_entries.cpp -- the host-buffer entries of the C ABI (include/bmx.h): host buffers in, host buffers out, over
// the public device API.  Each checks its arguments (every BMX_ERR_ARG and BMX_ERR_DOMAIN before any HIP call: the CPU
// suite calls these with ctx = NULL on a machine without a GPU), uploads, runs the device entry and downloads.  HostCall
// holds one call's context and device buffers; IndexCall adds what the five index entries open with.  Plain host C++: no
// kernel, one object for both libraries.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmx.h"
#include "bmx_internal.h"

namespace {

// One host-buffer call: the context (the caller's, or one on device 0 that lives as long as the call), the device buffers
// the call hands out and the running return code.  upload() and alloc() do nothing once a step has failed; everything is
// freed when the call leaves scope.  A handle that must go before the context is the entry's to destroy, before this
// object (bmx_dict), or a derived class's (IndexCall).
class HostCall {
public:
    int rc = BMX_OK;

    HostCall(const char *entry, bmx_ctx *ctx_in) : entry_(entry), ctx_(ctx_in), own_ctx_(!ctx_in)
    {
        if (!ctx_) rc = bmx_ctx_create(0, &ctx_);
    }
    ~HostCall()
    {
        for (void *p : bufs_) (void)hipFree(p);
        if (own_ctx_ && ctx_) bmx_ctx_destroy(ctx_);
    }
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;

    bmx_ctx *ctx() const { return ctx_; }

    template <typename T = void>
    T *upload(const void *src, uint64_t bytes)
    {
        void *p = nullptr;
        if (rc == BMX_OK) rc = bmx_text_upload(ctx_, static_cast<const char *>(src), bytes, &p);
        return static_cast<T *>(keep(p));
    }
    template <typename T = void>
    T *alloc(uint64_t bytes)
    {
        void *p = nullptr;
        if (rc == BMX_OK) rc = bmx_device_alloc(ctx_, bytes, &p);
        return static_cast<T *>(keep(p));
    }
    void release(void *p)
    {
        const auto it = std::find(bufs_.begin(), bufs_.end(), p);
        if (it == bufs_.end()) return;
        (void)hipFree(p);
        bufs_.erase(it);
    }
    // (also behind BMX_ERR_CAPACITY: the stored prefix is still the caller's)
    void download(void *dst, const void *d_src, uint64_t bytes, const char *what)
    {
        if ((rc != BMX_OK && rc != BMX_ERR_CAPACITY) || bytes == 0) return;
        const hipError_t e = hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) return;
        char text[256];
        snprintf(text, sizeof text, "%s: download of %s: %s", entry_, what, hipGetErrorString(e));
        bmx_internal_set_error(text);
        rc = BMX_ERR_HIP;
    }

private:
    void *keep(void *p)
    {
        if (p) bufs_.push_back(p);
        return p;
    }
    const char *entry_;
    bmx_ctx *ctx_;
    bool own_ctx_;
    std::vector<void *> bufs_;
};

// What the five index entries open with, behind their argument checks: the text, the query blob and its offsets on the
// device and an index over the text (its own suffix array).  The index goes before the context does.
class IndexCall : public HostCall {
public:
    bmx_index *ix = nullptr;
    void *d_pat;
    const uint64_t *d_off;

    IndexCall(const char *entry, bmx_ctx *ctx_in, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes,
              const uint64_t *pat_off, uint64_t count)
        : HostCall(entry, ctx_in)
    {
        void *d_text = upload(text, n);
        d_pat = upload(pat, pat_bytes);
        d_off = upload<uint64_t>(pat_off, (count + 1) * sizeof(uint64_t));
        if (rc == BMX_OK) rc = bmx_index_create_device(ctx(), d_text, n, nullptr, nullptr, &ix);
    }
    ~IndexCall() { bmx_index_destroy(ix); }
};

// table errors (a pattern outside the ASCII domain) before any device work
int pattern_tables_ok(const char *pat, int32_t m)
{
    int32_t bad[BMX_BAD_TABLE_SIZE];
    std::vector<int32_t> good(m);
    return bmx_build_tables(pat, m, bad, good.data());
}

} // namespace

extern "C" {

int bmx_search(bmx_ctx *ctx_in, const char *text, uint64_t n, const char *pat, int32_t m, uint64_t *match_positions,
               uint64_t capacity, uint64_t *n_matches)
{
    if (!pat || m < 1 || m > BMX_MAX_PATTERN || (n > 0 && !text)) return BMX_ERR_ARG;
    if (capacity > 0 && !match_positions) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    const int trc = pattern_tables_ok(pat, m);
    if (trc != BMX_OK) return trc;
    if (n < (uint64_t)m) return BMX_OK;

    HostCall c("bmx_search", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n - (uint64_t)m + 1);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_out = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_device(c.ctx(), d_text, n, n, 0, pat, m, nullptr, nullptr, d_out, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(match_positions, d_out, std::min(total, dev_cap) * sizeof(uint64_t), "matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

// (bmx_search_multi and the resident multi-GPU search with its RCCL exchange: bmx_multi.hip)

int bmx_search_ranges(bmx_ctx *ctx_in, const char *text, uint64_t n, const char *pat, const int32_t *se, int32_t P,
                      int32_t *ans, const int32_t *good, const int32_t *bad, int32_t m)
{
    if (!text || !pat || !se || !ans || P < 0 || m < 1 || m > BMX_MAX_PATTERN) return BMX_ERR_ARG;
    if ((good == nullptr) != (bad == nullptr)) return BMX_ERR_ARG;
    for (int r = 0; r < P; ++r) {
        ans[r] = 0;
        const int64_t s = se[2 * r], e = se[2 * r + 1];
        if (s < 0 || (e >= s && (uint64_t)e >= n)) return BMX_ERR_ARG;
    }
    if (!good) {
        const int trc = pattern_tables_ok(pat, m);
        if (trc != BMX_OK) return trc;
    }
    HostCall c("bmx_search_ranges", ctx_in);
    const char *d_text = c.upload<char>(text, n);
    for (int r = 0; r < P && c.rc == BMX_OK; ++r) {
        const int64_t s = se[2 * r], e = se[2 * r + 1];
        if (e < s) continue;
        // inclusive range [s, e] as in kernel1.cl:14-19: windows wholly inside it
        const uint64_t len = (uint64_t)(e - s) + 1;
        uint64_t total = 0;
        c.rc = bmx_search_device(c.ctx(), d_text + s, len, len, (uint64_t)s, pat, m, good, bad, nullptr, 0, &total, nullptr);
        if (c.rc == BMX_ERR_CAPACITY) c.rc = BMX_OK; // (a count-only call: the total is all it asks for)
        ans[r] = (int32_t)total;
    }
    return c.rc;
}

int bmx_edit_distance(bmx_ctx *ctx_in, const char *a, uint64_t la, const char *b, uint64_t lb, uint64_t *distance)
{
    if (!distance || (la > 0 && !a) || (lb > 0 && !b)) return BMX_ERR_ARG;
    if (la == 0 || lb == 0) {
        *distance = la + lb;
        return BMX_OK;
    }
    HostCall c("bmx_edit_distance", ctx_in);
    void *d_a = c.upload(a, la);
    void *d_b = c.upload(b, lb);
    if (c.rc == BMX_OK) c.rc = bmx_edit_distance_device(c.ctx(), d_a, la, d_b, lb, distance, nullptr);
    return c.rc;
}

int bmx_edit_distance_batch(bmx_ctx *ctx_in, const void *a, uint64_t a_bytes, const uint64_t *a_off, uint64_t a_count,
                            const void *b, uint64_t b_bytes, const uint64_t *b_off, uint64_t count, uint32_t limit, uint32_t *dist)
{
    if (!bmx_ed_batch_args_ok(a, a_bytes, a_off, a_count, b, b_bytes, b_off, count, dist)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!bmx_ed_batch_offsets_ok(a_off, a_count, a_bytes) || !bmx_ed_batch_offsets_ok(b_off, count, b_bytes)) return BMX_ERR_ARG;
    HostCall c("bmx_edit_distance_batch", ctx_in);
    void *d_a = a_bytes ? c.upload(a, a_bytes) : nullptr;
    void *d_b = b_bytes ? c.upload(b, b_bytes) : nullptr;
    const uint64_t *d_a_off = c.upload<uint64_t>(a_off, (a_count + 1) * sizeof(uint64_t));
    const uint64_t *d_b_off = c.upload<uint64_t>(b_off, (count + 1) * sizeof(uint64_t));
    uint32_t *d_dist = c.alloc<uint32_t>(count * sizeof(uint32_t));
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_edit_distance_batch_device(c.ctx(), d_a, a_bytes, d_a_off, a_count, d_b, b_bytes, d_b_off, count, limit, d_dist,
                                          nullptr);
    if (c.rc == BMX_OK) c.download(dist, d_dist, count * sizeof(uint32_t), "the distances");
    return c.rc;
}

int bmx_suffix_array(bmx_ctx *ctx_in, const char *text, uint64_t n, int32_t *sa_out)
{
    if ((n > 0 && (!text || !sa_out)) || n >= (1ull << 31)) return BMX_ERR_ARG;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_suffix_array", ctx_in);
    void *d_text = c.upload(text, n);
    int32_t *d_sa = c.alloc<int32_t>(n * sizeof(int32_t));
    if (c.rc == BMX_OK) c.rc = bmx_suffix_array_device(c.ctx(), d_text, n, d_sa, nullptr);
    if (c.rc == BMX_OK) c.download(sa_out, d_sa, n * sizeof(int32_t), "the suffix array");
    return c.rc;
}

int bmx_rows_split(bmx_ctx *ctx_in, const char *text, uint64_t n, uint8_t delim, uint64_t *off, uint64_t capacity, uint64_t *n_rows,
                   uint64_t *longest)
{
    if (!bmx_rows_split_args_ok(text, n, off, capacity)) return BMX_ERR_ARG;
    if (n_rows) *n_rows = 0;
    if (longest) *longest = 0;
    if (n == 0) { // no row, the single entry off[0]: no device is touched
        if (capacity) off[0] = 0;
        return BMX_OK;
    }
    HostCall c("bmx_rows_split", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n + 1); // (no text has more than n rows)
    uint64_t rows = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_off = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_rows_split_device(c.ctx(), d_text, n, 0, delim, d_off, dev_cap, &rows, longest, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(off, d_off, std::min(rows + 1, dev_cap) * sizeof(uint64_t), "row offsets");
    if (n_rows) *n_rows = rows;
    return c.rc;
}

int bmx_rows_of(bmx_ctx *ctx_in, const uint64_t *off, uint64_t rows, const uint64_t *starts, const uint64_t *ends, uint64_t len,
                uint64_t count, uint64_t *row)
{
    if (!bmx_rows_of_args_ok(off, starts, ends, len, count, row)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    HostCall c("bmx_rows_of", ctx_in);
    const uint64_t *d_off = c.upload<uint64_t>(off, (rows + 1) * sizeof(uint64_t));
    const uint64_t *d_starts = starts ? c.upload<uint64_t>(starts, count * sizeof(uint64_t)) : nullptr;
    const uint64_t *d_ends = ends ? c.upload<uint64_t>(ends, count * sizeof(uint64_t)) : nullptr;
    uint64_t *d_row = c.alloc<uint64_t>(count * sizeof(uint64_t));
    if (c.rc == BMX_OK) c.rc = bmx_rows_of_device(c.ctx(), d_off, rows, d_starts, d_ends, len, count, d_row, nullptr);
    if (c.rc == BMX_OK) c.download(row, d_row, count * sizeof(uint64_t), "row ids");
    return c.rc;
}

int bmx_rows_matching(bmx_ctx *ctx_in, const uint64_t *row, uint64_t count, uint64_t rows, uint32_t flags, uint64_t *rows_out,
                      uint64_t *counts_out, uint64_t capacity, uint64_t *n_out)
{
    if (!bmx_rows_matching_args_ok(row, count, flags, rows_out, counts_out, capacity)) return BMX_ERR_ARG;
    if (n_out) *n_out = 0;
    HostCall c("bmx_rows_matching", ctx_in);
    // (no list has more distinct rows than entries, no text more absent rows than rows)
    const uint64_t dev_cap = std::min<uint64_t>(capacity, (flags & BMX_ROWS_INVERT) ? rows : std::min(count, rows));
    uint64_t total = 0;
    const uint64_t *d_row = count ? c.upload<uint64_t>(row, count * sizeof(uint64_t)) : nullptr;
    uint64_t *d_out = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_counts = dev_cap && counts_out ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_rows_matching_device(c.ctx(), d_row, count, rows, flags, d_out, d_counts, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(rows_out, d_out, std::min(total, dev_cap) * sizeof(uint64_t), "matching rows");
    if (d_counts) c.download(counts_out, d_counts, std::min(total, dev_cap) * sizeof(uint64_t), "their counts");
    if (n_out) *n_out = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_spans_select(bmx_ctx *ctx_in, const uint64_t *starts, const uint64_t *ends, uint64_t len, uint64_t count, const uint64_t *row,
                     uint32_t flags, uint64_t *starts_out, uint64_t *ends_out, uint64_t *index_out, uint64_t capacity, uint64_t *n_out)
{
    if (!bmx_select_args_ok(starts, ends, len, count, flags, starts_out, ends_out, capacity, n_out)) return BMX_ERR_ARG;
    *n_out = 0;
    if (count == 0) return BMX_OK;
    HostCall c("bmx_spans_select", ctx_in);
    const uint64_t dev_cap = std::min(capacity, count); // (no list has more entries taken than entries)
    const uint64_t *d_starts = starts ? c.upload<uint64_t>(starts, count * sizeof(uint64_t)) : nullptr;
    const uint64_t *d_ends = ends ? c.upload<uint64_t>(ends, count * sizeof(uint64_t)) : nullptr;
    const uint64_t *d_row = row ? c.upload<uint64_t>(row, count * sizeof(uint64_t)) : nullptr;
    uint64_t *d_so = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_eo = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_io = dev_cap && index_out ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    uint64_t total = 0;
    c.rc = bmx_spans_select_device(c.ctx(), d_starts, d_ends, len, count, d_row, flags, d_so, d_eo, d_io, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap) * sizeof(uint64_t);
    c.download(starts_out, d_so, stored, "the starts taken");
    c.download(ends_out, d_eo, stored, "the ends taken");
    if (d_io) c.download(index_out, d_io, stored, "their indices");
    *n_out = total;
    return c.rc;
}

namespace {
// replace (off == NULL) and extract over host buffers
int subst_copy_host(const char *entry, bmx_ctx *ctx_in, const char *text, uint64_t n, const uint64_t *starts, const uint64_t *ends,
                    uint64_t len, uint64_t count, const void *repl, uint64_t repl_len, void *out, uint64_t capacity, uint64_t *off,
                    uint64_t *n_out)
{
    const bool extract = off != nullptr;
    *n_out = 0;
    if (count == 0) { // no span: the text itself, or the single offset 0; no device is touched
        if (extract) {
            off[0] = 0;
            return BMX_OK;
        }
        *n_out = n;
        if (capacity) memcpy(out, text, std::min(n, capacity));
        return capacity && n > capacity ? BMX_ERR_CAPACITY : BMX_OK;
    }
    HostCall c(entry, ctx_in);
    const uint64_t most = extract ? n : n + count * repl_len; // (spans inside the text: no output is longer)
    const uint64_t dev_cap = std::min(capacity, most);
    void *d_text = n ? c.upload(text, n) : nullptr;
    const uint64_t *d_starts = starts ? c.upload<uint64_t>(starts, count * sizeof(uint64_t)) : nullptr;
    const uint64_t *d_ends = ends ? c.upload<uint64_t>(ends, count * sizeof(uint64_t)) : nullptr;
    void *d_out = dev_cap ? c.alloc(dev_cap) : nullptr;
    uint64_t *d_off = extract ? c.alloc<uint64_t>((count + 1) * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    uint64_t total = 0;
    if (extract) c.rc = bmx_extract_device(c.ctx(), d_text, n, 0, d_starts, d_ends, len, count, d_out, dev_cap, d_off, &total, nullptr);
    else c.rc = bmx_replace_device(c.ctx(), d_text, n, 0, d_starts, d_ends, len, count, repl, repl_len, d_out, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(out, d_out, std::min(total, dev_cap), "the output");
    if (extract) c.download(off, d_off, (count + 1) * sizeof(uint64_t), "the offsets");
    *n_out = total;
    return c.rc;
}
} // namespace

int bmx_replace(bmx_ctx *ctx_in, const char *text, uint64_t n, const uint64_t *starts, const uint64_t *ends, uint64_t len, uint64_t count,
                const void *repl, uint64_t repl_len, void *out, uint64_t capacity, uint64_t *n_out)
{
    if (!bmx_subst_copy_args_ok(text, n, starts, ends, len, count, repl, repl_len, out, capacity, false, nullptr, n_out)) return BMX_ERR_ARG;
    return subst_copy_host("bmx_replace", ctx_in, text, n, starts, ends, len, count, repl, repl_len, out, capacity, nullptr, n_out);
}

int bmx_extract(bmx_ctx *ctx_in, const char *text, uint64_t n, const uint64_t *starts, const uint64_t *ends, uint64_t len, uint64_t count,
                void *blob, uint64_t capacity, uint64_t *off, uint64_t *n_out)
{
    if (!bmx_subst_copy_args_ok(text, n, starts, ends, len, count, nullptr, 0, blob, capacity, true, off, n_out)) return BMX_ERR_ARG;
    return subst_copy_host("bmx_extract", ctx_in, text, n, starts, ends, len, count, nullptr, 0, blob, capacity, off, n_out);
}

// replace and extract with a template over host buffers: the device entry counts first, then fills what fits
int bmx_expand(bmx_ctx *ctx_in, const char *text, uint64_t n, const uint64_t *groups, int32_t n_groups, uint64_t count, const void *tmpl,
               uint64_t tmpl_len, uint32_t flags, void *out, uint64_t capacity, uint64_t *off, uint64_t *n_out)
{
    if (!bmx_expand_args_ok(text, n, groups, n_groups, count, flags, out, capacity, off, n_out)) return BMX_ERR_ARG;
    bmx_template t;
    std::vector<uint8_t> lits(tmpl_len <= BMX_MAX_REPLACEMENT ? (size_t)tmpl_len + 1 : 1);
    if (bmx_compile_template(tmpl, tmpl_len, n_groups, &t, lits.data()) != BMX_OK) return BMX_ERR_ARG;
    const bool extract = (flags & BMX_EXPAND_EXTRACT) != 0;
    *n_out = 0;
    if (count == 0) { // no match: the text itself, or the single offset 0; no device is touched
        if (extract) {
            off[0] = 0;
            return BMX_OK;
        }
        *n_out = n;
        if (capacity) memcpy(out, text, std::min(n, capacity));
        return capacity && n > capacity ? BMX_ERR_CAPACITY : BMX_OK;
    }
    HostCall c("bmx_expand", ctx_in);
    const uint64_t words = count * ((uint64_t)n_groups + 1) * 2;
    void *d_text = n ? c.upload(text, n) : nullptr;
    const uint64_t *d_groups = c.upload<uint64_t>(groups, words * sizeof(uint64_t));
    uint64_t *d_off = extract ? c.alloc<uint64_t>((count + 1) * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    uint64_t total = 0;
    c.rc = bmx_expand_device(c.ctx(), d_text, n, 0, d_groups, n_groups, count, tmpl, tmpl_len, flags, nullptr, 0, d_off, &total, nullptr);
    if (c.rc != BMX_OK) return c.rc;
    const uint64_t dev_cap = std::min(capacity, total);
    if (dev_cap) {
        void *d_out = c.alloc(dev_cap);
        if (c.rc != BMX_OK) return c.rc;
        c.rc = bmx_expand_device(c.ctx(), d_text, n, 0, d_groups, n_groups, count, tmpl, tmpl_len, flags, d_out, dev_cap, d_off, &total, nullptr);
        if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
        c.download(out, d_out, dev_cap, "the output");
    }
    if (extract) c.download(off, d_off, (count + 1) * sizeof(uint64_t), "the offsets");
    *n_out = total;
    if (c.rc == BMX_OK && capacity && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_lcp_array(bmx_ctx *ctx_in, const char *text, uint64_t n, int32_t *sa_out, int32_t *lcp_out)
{
    if (!bmx_lcp_args_ok(text, n, lcp_out)) return BMX_ERR_ARG;
    HostCall c("bmx_lcp_array", ctx_in);
    void *d_text = c.upload(text, n);
    int32_t *d_sa = c.alloc<int32_t>(n * sizeof(int32_t));
    int32_t *d_lcp = c.alloc<int32_t>(n * sizeof(int32_t));
    if (c.rc == BMX_OK) c.rc = bmx_suffix_array_device(c.ctx(), d_text, n, d_sa, nullptr);
    if (c.rc == BMX_OK) c.rc = bmx_lcp_array_device(c.ctx(), d_text, n, d_sa, d_lcp, nullptr);
    if (c.rc == BMX_OK) c.download(lcp_out, d_lcp, n * sizeof(int32_t), "the LCP array");
    if (c.rc == BMX_OK && sa_out) c.download(sa_out, d_sa, n * sizeof(int32_t), "the suffix array");
    return c.rc;
}

int bmx_align(bmx_ctx *ctx_in, const char *text, uint64_t n, uint64_t base_offset, const void *pat, uint64_t pat_bytes,
              const uint64_t *pat_off, uint64_t pat_count, const uint32_t *pid, const uint64_t *start, const uint64_t *end,
              uint64_t count, int32_t k, uint8_t *dist, uint64_t *op_off, uint32_t *ops, uint64_t capacity, uint64_t *n_ops)
{
    if (!bmx_align_args_ok(text, n, pat, pat_off, pat_count, pid, start, end, count, k, op_off, ops, capacity)) return BMX_ERR_ARG;
    if (n_ops) *n_ops = 0;
    if (count == 0) return BMX_OK;
    if (!bmx_align_entries_ok(n, base_offset, pat_bytes, pat_off, pat_count, pid, start, end, count)) return BMX_ERR_ARG;
    HostCall c("bmx_align", ctx_in);
    void *d_text = c.upload(text, n);
    void *d_pat = c.upload(pat, pat_bytes);
    const uint64_t *d_off = c.upload<uint64_t>(pat_off, (pat_count + 1) * sizeof(uint64_t));
    const uint32_t *d_pid = pid ? c.upload<uint32_t>(pid, count * sizeof(uint32_t)) : nullptr;
    const uint64_t *d_start = c.upload<uint64_t>(start, count * sizeof(uint64_t));
    const uint64_t *d_end = c.upload<uint64_t>(end, count * sizeof(uint64_t));
    // (no entry has more than 2k + 1 runs: a larger capacity needs no larger device list)
    const uint64_t dev_cap = std::min(capacity, count * (2 * (uint64_t)k + 1));
    uint64_t total = 0;
    uint64_t *d_op_off = c.alloc<uint64_t>((count + 1) * sizeof(uint64_t));
    uint32_t *d_ops = dev_cap ? c.alloc<uint32_t>(dev_cap * sizeof(uint32_t)) : nullptr;
    uint8_t *d_dist = dist ? c.alloc<uint8_t>(count) : nullptr;
    if (c.rc == BMX_OK)
        c.rc = bmx_align_device(c.ctx(), d_text, n, base_offset, d_pat, pat_bytes, d_off, pat_count, d_pid, d_start, d_end, count, k,
                                d_dist, d_op_off, d_ops, dev_cap, &total, nullptr);
    if (c.rc == BMX_OK || c.rc == BMX_ERR_CAPACITY) {
        if (dist) c.download(dist, d_dist, count, "the distances");
        c.download(op_off, d_op_off, (count + 1) * sizeof(uint64_t), "the script offsets");
        c.download(ops, d_ops, std::min(total, dev_cap) * sizeof(uint32_t), "the scripts");
        if (n_ops) *n_ops = total;
    }
    return c.rc;
}

} // extern "C"

namespace {

// the approximate search for a string (classes == NULL) or for classes (pat == NULL); lng: the string's long entry
int search_approx_host(const char *entry, bmx_ctx *ctx_in, const char *text, uint64_t n, const char *pat, const uint8_t *classes,
                       int32_t m, int32_t k, uint64_t *ends, uint8_t *dist, uint64_t capacity, uint64_t *n_matches, bool lng = false)
{
    const void *what = pat ? (const void *)pat : (const void *)classes;
    if (!(lng ? bmx_approx_long_args_ok(n, 0, what, m, k, ends, capacity) : bmx_approx_args_ok(n, 0, what, m, k, ends, capacity)) ||
        (n > 0 && !text))
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c(entry, ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint8_t *d_dist = dev_cap && dist ? c.alloc<uint8_t>(dev_cap) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = lng ? bmx_search_approx_long_device(c.ctx(), d_text, n, 0, 0, pat, m, k, d_ends, d_dist, dev_cap, &total, nullptr)
           : pat ? bmx_search_approx_device(c.ctx(), d_text, n, 0, 0, pat, m, k, d_ends, d_dist, dev_cap, &total, nullptr)
               : bmx_search_approx_classes_device(c.ctx(), d_text, n, 0, 0, classes, m, k, d_ends, d_dist, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    c.download(ends, d_ends, stored * sizeof(uint64_t), "approximate matches");
    if (dist) c.download(dist, d_dist, stored, "approximate matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

// ... and its match spans
int search_spans_host(const char *entry, bmx_ctx *ctx_in, const char *text, uint64_t n, const char *pat, const uint8_t *classes,
                      int32_t m, int32_t k, uint32_t flags, uint64_t *starts, uint64_t *ends, uint8_t *dist, uint64_t capacity,
                      uint64_t *n_spans, bool lng = false)
{
    const void *what = pat ? (const void *)pat : (const void *)classes;
    if (!(lng ? bmx_approx_long_args_ok(n, 0, what, m, k, ends, capacity) : bmx_approx_args_ok(n, 0, what, m, k, ends, capacity)) ||
        (flags & ~BMX_SPANS_BEST) || (capacity && !starts) || (n > 0 && !text))
        return BMX_ERR_ARG;
    if (n_spans) *n_spans = 0;
    if (n == 0) return BMX_OK;
    HostCall c(entry, ctx_in);
    uint64_t *d_ends = nullptr;
    uint8_t *d_dist = nullptr;
    uint64_t total = 0, spans = 0;
    void *d_text = c.upload(text, n);
    auto search = [&](uint64_t cap) {
        d_ends = cap ? c.alloc<uint64_t>(cap * sizeof(uint64_t)) : nullptr;
        d_dist = cap ? c.alloc<uint8_t>(cap) : nullptr;
        if (c.rc != BMX_OK) return;
        c.rc = lng ? bmx_search_approx_long_device(c.ctx(), d_text, n, 0, 0, pat, m, k, d_ends, d_dist, cap, &total, nullptr)
               : pat ? bmx_search_approx_device(c.ctx(), d_text, n, 0, 0, pat, m, k, d_ends, d_dist, cap, &total, nullptr)
                   : bmx_search_approx_classes_device(c.ctx(), d_text, n, 0, 0, classes, m, k, d_ends, d_dist, cap, &total, nullptr);
    };
    // counting only if `capacity` cannot hold a single end; else in one go if it holds them all
    search(std::min<uint64_t>(capacity, n));
    if (c.rc == BMX_ERR_CAPACITY) { // again, with room for all ends
        c.release(d_ends);
        c.release(d_dist);
        c.rc = BMX_OK;
        search(total);
    }
    uint64_t *d_starts = nullptr, *d_sel_ends = nullptr;
    uint8_t *d_sel_dist = nullptr;
    if (c.rc == BMX_OK && total) {
        d_starts = c.alloc<uint64_t>(total * sizeof(uint64_t));
        if (flags) d_sel_ends = c.alloc<uint64_t>(total * sizeof(uint64_t));
        if (flags) d_sel_dist = c.alloc<uint8_t>(total);
        if (c.rc == BMX_OK)
            c.rc = lng ? bmx_approx_long_spans_device(c.ctx(), d_text, n, 0, pat, m, k, d_ends, d_dist, total, flags, d_starts,
                                                      d_sel_ends, d_sel_dist, &spans, nullptr)
                   : pat ? bmx_approx_spans_device(c.ctx(), d_text, n, 0, pat, m, k, d_ends, d_dist, total, flags, d_starts, d_sel_ends,
                                                 d_sel_dist, &spans, nullptr)
                       : bmx_approx_spans_classes_device(c.ctx(), d_text, n, 0, classes, m, k, d_ends, d_dist, total, flags, d_starts,
                                                         d_sel_ends, d_sel_dist, &spans, nullptr);
    }
    if (c.rc != BMX_OK) return c.rc;
    const uint64_t stored = std::min(spans, capacity);
    c.download(starts, d_starts, stored * sizeof(uint64_t), "match spans");
    c.download(ends, flags ? d_sel_ends : d_ends, stored * sizeof(uint64_t), "match spans");
    if (dist) c.download(dist, flags ? d_sel_dist : d_dist, stored, "match spans");
    if (n_spans) *n_spans = spans;
    if (c.rc == BMX_OK && spans > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

} // namespace

extern "C" {

int bmx_search_approx(bmx_ctx *ctx, const char *text, uint64_t n, const char *pat, int32_t m, int32_t k, uint64_t *ends,
                      uint8_t *dist, uint64_t capacity, uint64_t *n_matches)
{
    if (!pat) return BMX_ERR_ARG;
    return search_approx_host("bmx_search_approx", ctx, text, n, pat, nullptr, m, k, ends, dist, capacity, n_matches);
}

int bmx_search_approx_long(bmx_ctx *ctx, const char *text, uint64_t n, const char *pat, int32_t m, int32_t k, uint64_t *ends,
                           uint8_t *dist, uint64_t capacity, uint64_t *n_matches)
{
    if (!pat) return BMX_ERR_ARG;
    return search_approx_host("bmx_search_approx_long", ctx, text, n, pat, nullptr, m, k, ends, dist, capacity, n_matches, true);
}

int bmx_search_approx_classes(bmx_ctx *ctx, const char *text, uint64_t n, const uint8_t *classes, int32_t m, int32_t k,
                              uint64_t *ends, uint8_t *dist, uint64_t capacity, uint64_t *n_matches)
{
    if (!classes) return BMX_ERR_ARG;
    return search_approx_host("bmx_search_approx_classes", ctx, text, n, nullptr, classes, m, k, ends, dist, capacity, n_matches);
}

int bmx_search_approx_spans(bmx_ctx *ctx, const char *text, uint64_t n, const char *pat, int32_t m, int32_t k, uint32_t flags,
                            uint64_t *starts, uint64_t *ends, uint8_t *dist, uint64_t capacity, uint64_t *n_spans)
{
    if (!pat) return BMX_ERR_ARG;
    return search_spans_host("bmx_search_approx_spans", ctx, text, n, pat, nullptr, m, k, flags, starts, ends, dist, capacity,
                             n_spans);
}

int bmx_search_approx_long_spans(bmx_ctx *ctx, const char *text, uint64_t n, const char *pat, int32_t m, int32_t k, uint32_t flags,
                                 uint64_t *starts, uint64_t *ends, uint8_t *dist, uint64_t capacity, uint64_t *n_spans)
{
    if (!pat) return BMX_ERR_ARG;
    return search_spans_host("bmx_search_approx_long_spans", ctx, text, n, pat, nullptr, m, k, flags, starts, ends, dist, capacity,
                             n_spans, true);
}

int bmx_search_approx_spans_classes(bmx_ctx *ctx, const char *text, uint64_t n, const uint8_t *classes, int32_t m, int32_t k,
                                    uint32_t flags, uint64_t *starts, uint64_t *ends, uint8_t *dist, uint64_t capacity,
                                    uint64_t *n_spans)
{
    if (!classes) return BMX_ERR_ARG;
    return search_spans_host("bmx_search_approx_spans_classes", ctx, text, n, nullptr, classes, m, k, flags, starts, ends, dist,
                             capacity, n_spans);
}

int bmx_search_classes(bmx_ctx *ctx_in, const char *text, uint64_t n, const uint8_t *classes, int32_t m,
                       uint64_t *match_positions, uint64_t capacity, uint64_t *n_matches)
{
    if (!bmx_classes_args_ok(n, classes, m, match_positions, capacity) || (n > 0 && !text)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n < (uint64_t)m) return BMX_OK;
    HostCall c("bmx_search_classes", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n - (uint64_t)m + 1);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_classes_device(c.ctx(), d_text, n, n, 0, classes, m, d_starts, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(match_positions, d_starts, std::min(total, dev_cap) * sizeof(uint64_t), "class matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

} // extern "C"

namespace {

// the k-mismatch search for a string (classes == NULL) or for classes (pat == NULL)
int search_hamming_host(const char *entry, bmx_ctx *ctx_in, const char *text, uint64_t n, const char *pat, const uint8_t *classes,
                        int32_t m, int32_t k, uint64_t must, uint64_t *starts, uint8_t *dist, uint64_t capacity, uint64_t *n_matches)
{
    const void *what = pat ? (const void *)pat : (const void *)classes;
    if (!bmx_hamming_args_ok(n, what, m, k, must, starts, capacity) || (n > 0 && !text)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n < (uint64_t)m) return BMX_OK;
    HostCall c(entry, ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n - (uint64_t)m + 1);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint8_t *d_dist = dev_cap && dist ? c.alloc<uint8_t>(dev_cap) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = pat ? bmx_search_hamming_device(c.ctx(), d_text, n, n, 0, pat, m, k, must, d_starts, d_dist, dev_cap, &total, nullptr)
               : bmx_search_hamming_classes_device(c.ctx(), d_text, n, n, 0, classes, m, k, must, d_starts, d_dist, dev_cap, &total,
                                                   nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    c.download(starts, d_starts, stored * sizeof(uint64_t), "k-mismatch matches");
    if (dist) c.download(dist, d_dist, stored, "k-mismatch matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

} // namespace

extern "C" {

int bmx_search_hamming(bmx_ctx *ctx, const char *text, uint64_t n, const char *pat, int32_t m, int32_t k, uint64_t must,
                       uint64_t *starts, uint8_t *dist, uint64_t capacity, uint64_t *n_matches)
{
    if (!pat) return BMX_ERR_ARG;
    return search_hamming_host("bmx_search_hamming", ctx, text, n, pat, nullptr, m, k, must, starts, dist, capacity, n_matches);
}

int bmx_search_hamming_classes(bmx_ctx *ctx, const char *text, uint64_t n, const uint8_t *classes, int32_t m, int32_t k,
                               uint64_t must, uint64_t *starts, uint8_t *dist, uint64_t capacity, uint64_t *n_matches)
{
    if (!classes) return BMX_ERR_ARG;
    return search_hamming_host("bmx_search_hamming_classes", ctx, text, n, nullptr, classes, m, k, must, starts, dist, capacity,
                               n_matches);
}

int bmx_search_gaps(bmx_ctx *ctx_in, const char *text, uint64_t n, const uint8_t *classes, int32_t m, uint64_t optional,
                    uint64_t *ends, uint64_t capacity, uint64_t *n_matches)
{
    if (!bmx_gaps_args_ok(n, 0, classes, m, optional, ends, capacity) || (n > 0 && !text)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_gaps", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_gaps_device(c.ctx(), d_text, n, 0, 0, classes, m, optional, d_ends, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(ends, d_ends, std::min(total, dev_cap) * sizeof(uint64_t), "gapped matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_gaps_spans(bmx_ctx *ctx_in, const char *text, uint64_t n, const uint8_t *classes, int32_t m, uint64_t optional,
                          uint32_t flags, uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_matches)
{
    if (!bmx_gaps_args_ok(n, 0, classes, m, optional, ends, capacity) || (capacity > 0 && !starts) || (n > 0 && !text) ||
        (flags & ~BMX_GAPS_LONGEST))
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_gaps_spans", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_gaps_device(c.ctx(), d_text, n, 0, 0, classes, m, optional, d_ends, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    const int src = bmx_gaps_starts_device(c.ctx(), d_text, n, 0, classes, m, optional, d_ends, stored, flags, d_starts, nullptr);
    if (src != BMX_OK) return src;
    c.download(ends, d_ends, stored * sizeof(uint64_t), "gapped matches");
    c.download(starts, d_starts, stored * sizeof(uint64_t), "gapped matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_regex(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re, uint64_t *ends, uint64_t capacity,
                     uint64_t *n_matches)
{
    if (!bmx_regex_args_ok(n, 0, re, ends, capacity) || (n > 0 && !text)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_device(c.ctx(), d_text, n, 0, 0, re, d_ends, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(ends, d_ends, std::min(total, dev_cap) * sizeof(uint64_t), "regex matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_regex_spans(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re, uint32_t flags, uint64_t *starts,
                           uint64_t *ends, uint64_t capacity, uint64_t *n_matches)
{
    if (!bmx_regex_args_ok(n, 0, re, ends, capacity) || (capacity > 0 && !starts) || (n > 0 && !text) ||
        (flags & ~BMX_REGEX_LONGEST))
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_spans", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_device(c.ctx(), d_text, n, 0, 0, re, d_ends, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    const int src = bmx_regex_starts_device(c.ctx(), d_text, n, 0, re, d_ends, stored, flags, d_starts, nullptr);
    if (src != BMX_OK) return src;
    c.download(ends, d_ends, stored * sizeof(uint64_t), "regex matches");
    c.download(starts, d_starts, stored * sizeof(uint64_t), "regex matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_regex_groups(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re, const bmx_regex_groups *gr, uint32_t flags,
                            uint64_t *starts, uint64_t *ends, uint64_t *groups, uint64_t capacity, uint64_t *n_matches)
{
    if (!bmx_regex_args_ok(n, 0, re, ends, capacity) || !bmx_regex_groups_valid(re, gr) || (capacity > 0 && (!starts || !groups)) ||
        (n > 0 && !text) || (flags & ~BMX_REGEX_LONGEST))
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_groups", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n), per_entry = ((uint64_t)gr->n_groups + 1) * 2 * sizeof(uint64_t);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_groups = dev_cap ? c.alloc<uint64_t>(dev_cap * per_entry) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_device(c.ctx(), d_text, n, 0, 0, re, d_ends, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    int src = bmx_regex_starts_device(c.ctx(), d_text, n, 0, re, d_ends, stored, flags, d_starts, nullptr);
    if (src == BMX_OK) src = bmx_regex_groups_device(c.ctx(), d_text, n, 0, re, gr, d_starts, d_ends, stored, d_groups, nullptr);
    if (src != BMX_OK) return src;
    c.download(ends, d_ends, stored * sizeof(uint64_t), "regex matches");
    c.download(starts, d_starts, stored * sizeof(uint64_t), "regex matches");
    c.download(groups, d_groups, stored * per_entry, "their groups");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_regex_long(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex_long *re, uint64_t *ends, uint64_t capacity,
                          uint64_t *n_matches)
{
    if (!bmx_regex_long_args_ok(n, 0, re, ends, capacity) || (n > 0 && !text)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_long", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_long_device(c.ctx(), d_text, n, 0, 0, re, d_ends, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(ends, d_ends, std::min(total, dev_cap) * sizeof(uint64_t), "regex matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_regex_long_spans(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex_long *re, uint32_t flags,
                                uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_matches)
{
    if (!bmx_regex_long_args_ok(n, 0, re, ends, capacity) || (capacity > 0 && !starts) || (n > 0 && !text) ||
        (flags & ~BMX_REGEX_LONGEST))
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_long_spans", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_long_device(c.ctx(), d_text, n, 0, 0, re, d_ends, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    const int src = bmx_regex_long_starts_device(c.ctx(), d_text, n, 0, re, d_ends, stored, flags, d_starts, nullptr);
    if (src != BMX_OK) return src;
    c.download(ends, d_ends, stored * sizeof(uint64_t), "regex matches");
    c.download(starts, d_starts, stored * sizeof(uint64_t), "regex matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

// The reversed automaton (pure host code; the starts pass and the begins search of bmx_regex.hip run it): bit i stands for
// position m - 1 - i, first and last swap, follow is transposed, the classes are mirrored.
int bmx_regex_reverse(const bmx_regex *re, bmx_regex *out)
{
    if (!bmx_regex_star_ok(re) || !out) return BMX_ERR_ARG;
    const int32_t m = re->m;
    const auto flip = [m](uint64_t set) {
        uint64_t r = 0;
        for (; set != 0; set &= set - 1) r |= 1ull << (m - 1 - __builtin_ctzll(set));
        return r;
    };
    bmx_regex r;
    std::memset(&r, 0, sizeof r);
    r.m = m;
    r.min_len = re->min_len;
    r.max_len = re->max_len;
    r.first = flip(re->last);
    r.last = flip(re->first);
    for (int32_t i = 0; i < m; ++i) {
        for (uint64_t f = re->follow[i]; f != 0; f &= f - 1) r.follow[m - 1 - __builtin_ctzll(f)] |= 1ull << (m - 1 - i);
        std::memcpy(r.classes + (size_t)(m - 1 - i) * BMX_CLASS_BYTES, re->classes + (size_t)i * BMX_CLASS_BYTES, BMX_CLASS_BYTES);
    }
    *out = r; // (out may be re)
    return BMX_OK;
}

int bmx_search_regex_begins(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re, uint64_t *starts, uint64_t capacity,
                            uint64_t *n_matches)
{
    if (!bmx_regex_begins_args_ok(n, 0, re, starts, capacity) || (n > 0 && !text)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_begins", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_begins_device(c.ctx(), d_text, n, 0, 0, re, d_starts, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(starts, d_starts, std::min(total, dev_cap) * sizeof(uint64_t), "regex match starts");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_regex_begins_spans(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re, uint32_t flags,
                                  uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_matches)
{
    if (!bmx_regex_begins_args_ok(n, 0, re, starts, capacity) || (capacity > 0 && !ends) || (n > 0 && !text) ||
        (flags & ~BMX_REGEX_LONGEST))
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_begins_spans", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_begins_device(c.ctx(), d_text, n, 0, 0, re, d_starts, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    const int erc = bmx_regex_ends_device(c.ctx(), d_text, n, 0, re, d_starts, stored, nullptr, flags, d_ends, nullptr);
    if (erc != BMX_OK) return erc;
    c.download(starts, d_starts, stored * sizeof(uint64_t), "regex match starts");
    c.download(ends, d_ends, stored * sizeof(uint64_t), "regex match ends");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

// The anchored forms: the whole text is there, so outside it counts as a line break on both sides.
namespace {
constexpr uint32_t OUTSIDE = 0x0A;

// ends (begins == false) or starts of the anchored matches, and where `other` is wanted the other side of each
int regex_anchored_host(const char *where, bool begins, bool spans, bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re,
                        const bmx_regex_anchors *an, uint32_t flags, uint64_t *list, uint64_t *other, uint64_t capacity,
                        uint64_t *n_matches)
{
    if (!bmx_regex_args_ok(n, 0, re, list, capacity) || !an || (spans && capacity > 0 && !other) || (n > 0 && !text) ||
        (flags & ~BMX_REGEX_LONGEST))
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c(where, ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_list = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_other = dev_cap && spans ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = begins ? bmx_search_regex_anchored_begins_device(c.ctx(), d_text, n, 0, 0, re, an, OUTSIDE, OUTSIDE, d_list, dev_cap, &total, nullptr)
                  : bmx_search_regex_anchored_device(c.ctx(), d_text, n, 0, 0, re, an, OUTSIDE, OUTSIDE, d_list, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    if (spans) {
        const int prc = begins ? bmx_regex_anchored_ends_device(c.ctx(), d_text, n, 0, re, an, OUTSIDE, OUTSIDE, d_list, stored, nullptr,
                                                                flags, d_other, nullptr)
                               : bmx_regex_anchored_starts_device(c.ctx(), d_text, n, 0, re, an, OUTSIDE, OUTSIDE, d_list, stored, flags,
                                                                  d_other, nullptr);
        if (prc != BMX_OK) return prc;
    }
    c.download(list, d_list, stored * sizeof(uint64_t), "anchored regex matches");
    if (spans) c.download(other, d_other, stored * sizeof(uint64_t), "anchored regex matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}
} // namespace

int bmx_search_regex_anchored(bmx_ctx *ctx, const char *text, uint64_t n, const bmx_regex *re, const bmx_regex_anchors *an,
                              uint64_t *ends, uint64_t capacity, uint64_t *n_matches)
{
    return regex_anchored_host("bmx_search_regex_anchored", false, false, ctx, text, n, re, an, 0, ends, nullptr, capacity, n_matches);
}

int bmx_search_regex_anchored_spans(bmx_ctx *ctx, const char *text, uint64_t n, const bmx_regex *re, const bmx_regex_anchors *an,
                                    uint32_t flags, uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_matches)
{
    return regex_anchored_host("bmx_search_regex_anchored_spans", false, true, ctx, text, n, re, an, flags, ends, starts, capacity,
                               n_matches);
}

int bmx_search_regex_anchored_begins(bmx_ctx *ctx, const char *text, uint64_t n, const bmx_regex *re, const bmx_regex_anchors *an,
                                     uint64_t *starts, uint64_t capacity, uint64_t *n_matches)
{
    return regex_anchored_host("bmx_search_regex_anchored_begins", true, false, ctx, text, n, re, an, 0, starts, nullptr, capacity,
                               n_matches);
}

int bmx_search_regex_anchored_begins_spans(bmx_ctx *ctx, const char *text, uint64_t n, const bmx_regex *re,
                                           const bmx_regex_anchors *an, uint32_t flags, uint64_t *starts, uint64_t *ends,
                                           uint64_t capacity, uint64_t *n_matches)
{
    return regex_anchored_host("bmx_search_regex_anchored_begins_spans", true, true, ctx, text, n, re, an, flags, starts, ends, capacity,
                               n_matches);
}

int bmx_search_regex_star(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re, uint64_t *ends, uint64_t capacity,
                          uint64_t *n_matches)
{
    if (!bmx_regex_star_args_ok(n, 0, re, ends, capacity) || (n > 0 && !text)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_star", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_star_device(c.ctx(), d_text, n, 0, 0, re, d_ends, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(ends, d_ends, std::min(total, dev_cap) * sizeof(uint64_t), "regex matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_regex_star_spans(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re, uint32_t window, uint32_t flags,
                                uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_matches)
{
    if (!bmx_regex_star_args_ok(n, 0, re, ends, capacity) || (capacity > 0 && !starts) || (n > 0 && !text) ||
        (flags & ~BMX_REGEX_LONGEST) || window < 1 || window > BMX_MAX_REGEX_STAR_WINDOW)
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_star_spans", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_star_device(c.ctx(), d_text, n, 0, 0, re, d_ends, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    const int src = bmx_regex_star_starts_device(c.ctx(), d_text, n, 0, re, d_ends, stored, window, flags, d_starts, nullptr);
    if (src != BMX_OK) return src;
    c.download(ends, d_ends, stored * sizeof(uint64_t), "regex matches");
    c.download(starts, d_starts, stored * sizeof(uint64_t), "regex matches");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_regex_star_begins(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re, uint64_t *starts,
                                 uint64_t capacity, uint64_t *n_matches)
{
    if (!bmx_regex_star_begins_args_ok(n, 0, re, starts, capacity) || (n > 0 && !text)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_star_begins", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_star_begins_device(c.ctx(), d_text, n, 0, 0, re, d_starts, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    c.download(starts, d_starts, std::min(total, dev_cap) * sizeof(uint64_t), "regex match starts");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_search_regex_star_begins_spans(bmx_ctx *ctx_in, const char *text, uint64_t n, const bmx_regex *re, uint32_t window,
                                       uint32_t flags, uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_matches,
                                       uint64_t *n_clipped)
{
    if (!bmx_regex_star_begins_args_ok(n, 0, re, starts, capacity) || (capacity > 0 && !ends) || (n > 0 && !text) ||
        (flags & ~BMX_REGEX_LONGEST) || window < 1 || window > BMX_MAX_REGEX_STAR_WINDOW)
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (n_clipped) *n_clipped = 0;
    if (n == 0) return BMX_OK;
    HostCall c("bmx_search_regex_star_begins_spans", ctx_in);
    const uint64_t dev_cap = std::min<uint64_t>(capacity, n);
    uint64_t total = 0;
    void *d_text = c.upload(text, n);
    uint64_t *d_starts = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    uint64_t *d_ends = dev_cap ? c.alloc<uint64_t>(dev_cap * sizeof(uint64_t)) : nullptr;
    if (c.rc != BMX_OK) return c.rc;
    c.rc = bmx_search_regex_star_begins_device(c.ctx(), d_text, n, 0, 0, re, d_starts, dev_cap, &total, nullptr);
    if (c.rc != BMX_OK && c.rc != BMX_ERR_CAPACITY) return c.rc;
    const uint64_t stored = std::min(total, dev_cap);
    const int erc = bmx_regex_star_ends_device(c.ctx(), d_text, n, 0, re, d_starts, stored, nullptr, window, flags, d_ends, n_clipped, nullptr);
    if (erc != BMX_OK) return erc;
    c.download(starts, d_starts, stored * sizeof(uint64_t), "regex match starts");
    c.download(ends, d_ends, stored * sizeof(uint64_t), "regex match ends");
    if (n_matches) *n_matches = total;
    if (c.rc == BMX_OK && total > capacity) c.rc = BMX_ERR_CAPACITY;
    return c.rc;
}

int bmx_dict_search(bmx_ctx *ctx_in, const char *text, uint64_t n, const char *const *pats, const int32_t *ms, int32_t K,
                    uint64_t *pos, uint32_t *pid, uint64_t capacity, uint64_t *n_matches)
{
    const int prc = bmx_dict_patterns_ok(pats, ms, K);
    if (prc != BMX_OK) return prc;
    if ((n > 0 && !text) || n >= (1ull << 40) || (capacity > 0 && !pos)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    HostCall c("bmx_dict_search", ctx_in);
    bmx_dict *d = nullptr;
    uint64_t total = 0;
    if (c.rc == BMX_OK) c.rc = bmx_dict_create(c.ctx(), pats, ms, K, &d);
    void *d_text = n ? c.upload(text, n) : nullptr;
    uint64_t *d_pos = capacity ? c.alloc<uint64_t>(capacity * sizeof(uint64_t)) : nullptr;
    uint32_t *d_pid = capacity && pid ? c.alloc<uint32_t>(capacity * sizeof(uint32_t)) : nullptr;
    if (c.rc == BMX_OK) c.rc = bmx_dict_search_device(c.ctx(), d, d_text, n, n, 0, d_pos, d_pid, capacity, &total, nullptr);
    if (c.rc == BMX_OK || c.rc == BMX_ERR_CAPACITY) {
        const uint64_t stored = std::min(total, capacity);
        c.download(pos, d_pos, stored * sizeof(uint64_t), "dictionary matches");
        if (pid) c.download(pid, d_pid, stored * sizeof(uint32_t), "dictionary matches");
        if (n_matches) *n_matches = total;
    }
    bmx_dict_destroy(d); // before the context
    return c.rc;
}

int bmx_index_count(bmx_ctx *ctx_in, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes, const uint64_t *pat_off,
                    uint64_t count, uint32_t *cnt)
{
    if (!text || n == 0 || n >= (1ull << 31) || !bmx_index_query_args_ok(pat, pat_off, count, cnt)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    const int qrc = bmx_index_queries_ok(pat, pat_bytes, pat_off, count);
    if (qrc != BMX_OK) return qrc;
    IndexCall c("bmx_index_count", ctx_in, text, n, pat, pat_bytes, pat_off, count);
    uint32_t *d_cnt = c.alloc<uint32_t>(count * sizeof(uint32_t));
    if (c.rc == BMX_OK) c.rc = bmx_index_count_device(c.ctx(), c.ix, c.d_pat, pat_bytes, c.d_off, count, nullptr, d_cnt, nullptr);
    if (c.rc == BMX_OK) c.download(cnt, d_cnt, count * sizeof(uint32_t), "the counts");
    return c.rc;
}

int bmx_index_locate(bmx_ctx *ctx_in, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes, const uint64_t *pat_off,
                     uint64_t count, uint64_t *out_off, uint64_t *pos, uint64_t capacity, uint64_t *n_matches)
{
    if (!text || n == 0 || n >= (1ull << 31) || !bmx_index_query_args_ok(pat, pat_off, count, out_off) ||
        (count > 0 && capacity > 0 && !pos))
        return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (count == 0) return BMX_OK;
    const int qrc = bmx_index_queries_ok(pat, pat_bytes, pat_off, count);
    if (qrc != BMX_OK) return qrc;
    IndexCall c("bmx_index_locate", ctx_in, text, n, pat, pat_bytes, pat_off, count);
    uint64_t total = 0;
    uint64_t *d_out_off = c.alloc<uint64_t>((count + 1) * sizeof(uint64_t));
    uint64_t *d_pos = capacity ? c.alloc<uint64_t>(capacity * sizeof(uint64_t)) : nullptr;
    if (c.rc == BMX_OK)
        c.rc = bmx_index_locate_device(c.ctx(), c.ix, c.d_pat, pat_bytes, c.d_off, count, 0, d_out_off, d_pos, capacity, &total,
                                       nullptr);
    if (c.rc == BMX_OK || c.rc == BMX_ERR_CAPACITY) {
        c.download(out_off, d_out_off, (count + 1) * sizeof(uint64_t), "the positions");
        // (behind the stored segments: unspecified, as in the device entry)
        c.download(pos, d_pos, std::min(total, capacity) * sizeof(uint64_t), "the positions");
        if (n_matches) *n_matches = total;
    }
    return c.rc;
}

int bmx_index_match(bmx_ctx *ctx_in, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes, const uint64_t *pat_off,
                    uint64_t count, uint32_t *len, uint32_t *lo, uint32_t *cnt)
{
    if (!text || n == 0 || n >= (1ull << 31) || !bmx_index_query_args_ok(pat, pat_off, count, len)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    const int qrc = bmx_index_queries_ok(pat, pat_bytes, pat_off, count);
    if (qrc != BMX_OK) return qrc;
    IndexCall c("bmx_index_match", ctx_in, text, n, pat, pat_bytes, pat_off, count);
    // (only the bytes inside the queries come back: the caller's entries outside them stay as they are)
    const uint64_t at = pat_off[0], used = pat_off[count] - at;
    uint32_t *d_len = c.alloc<uint32_t>(pat_bytes * sizeof(uint32_t));
    uint32_t *d_lo = lo ? c.alloc<uint32_t>(pat_bytes * sizeof(uint32_t)) : nullptr;
    uint32_t *d_cnt = cnt ? c.alloc<uint32_t>(pat_bytes * sizeof(uint32_t)) : nullptr;
    if (c.rc == BMX_OK)
        c.rc = bmx_index_match_device(c.ctx(), c.ix, c.d_pat, pat_bytes, c.d_off, count, d_len, d_lo, d_cnt, nullptr);
    if (c.rc == BMX_OK) {
        c.download(len + at, d_len + at, used * sizeof(uint32_t), "the match lengths");
        if (lo) c.download(lo + at, d_lo + at, used * sizeof(uint32_t), "the interval starts");
        if (cnt) c.download(cnt + at, d_cnt + at, used * sizeof(uint32_t), "the interval sizes");
    }
    return c.rc;
}

int bmx_index_seeds(bmx_ctx *ctx_in, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes, const uint64_t *pat_off,
                    uint64_t count, uint32_t min_len, uint32_t max_occ, uint64_t *seed_off, uint32_t *qpos, uint32_t *len,
                    uint32_t *lo, uint32_t *cnt, uint64_t capacity, uint64_t *n_seeds)
{
    if (!text || n == 0 || n >= (1ull << 31) ||
        !bmx_index_seeds_args_ok(pat, pat_off, count, min_len, seed_off, qpos, len, lo, cnt, capacity))
        return BMX_ERR_ARG;
    if (n_seeds) *n_seeds = 0;
    if (count == 0) return BMX_OK;
    const int qrc = bmx_index_queries_ok(pat, pat_bytes, pat_off, count);
    if (qrc != BMX_OK) return qrc;
    IndexCall c("bmx_index_seeds", ctx_in, text, n, pat, pat_bytes, pat_off, count);
    uint64_t total = 0;
    // (no more seeds than blob bytes: a larger capacity needs no larger device lists)
    const uint64_t dev_cap = std::min(capacity, pat_bytes);
    uint64_t *d_seed_off = c.alloc<uint64_t>((count + 1) * sizeof(uint64_t));
    uint32_t *d_out = dev_cap ? c.alloc<uint32_t>(4 * dev_cap * sizeof(uint32_t)) : nullptr;
    if (c.rc == BMX_OK)
        c.rc = bmx_index_seeds_device(c.ctx(), c.ix, c.d_pat, pat_bytes, c.d_off, count, min_len, max_occ, d_seed_off, d_out,
                                      d_out ? d_out + dev_cap : nullptr, d_out ? d_out + 2 * dev_cap : nullptr,
                                      d_out ? d_out + 3 * dev_cap : nullptr, dev_cap, &total, nullptr);
    if (c.rc == BMX_OK || c.rc == BMX_ERR_CAPACITY) {
        const uint64_t stored = std::min(total, dev_cap) * sizeof(uint32_t);
        c.download(seed_off, d_seed_off, (count + 1) * sizeof(uint64_t), "the seed offsets");
        c.download(qpos, d_out, stored, "the seeds");
        c.download(len, d_out + dev_cap, stored, "the seeds");
        c.download(lo, d_out + 2 * dev_cap, stored, "the seeds");
        c.download(cnt, d_out + 3 * dev_cap, stored, "the seeds");
        if (n_seeds) *n_seeds = total;
    }
    return c.rc;
}

int bmx_index_map(bmx_ctx *ctx_in, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes, const uint64_t *pat_off,
                  uint64_t count, uint32_t min_len, uint32_t max_occ, int32_t k, uint64_t *best_start, uint64_t *best_end,
                  uint8_t *best_dist, uint64_t *cand_off, uint64_t *cand_start, uint64_t *cand_end, uint8_t *cand_dist,
                  uint64_t capacity, uint64_t *n_candidates)
{
    if (!text || n == 0 || n >= (1ull << 31) ||
        !bmx_index_map_args_ok(pat, pat_off, count, min_len, max_occ, k, best_start, best_end, best_dist, cand_start, cand_end,
                               cand_dist, capacity))
        return BMX_ERR_ARG;
    if (n_candidates) *n_candidates = 0;
    if (count == 0) return BMX_OK;
    const int qrc = bmx_index_queries_ok(pat, pat_bytes, pat_off, count);
    if (qrc != BMX_OK) return qrc;
    IndexCall c("bmx_index_map", ctx_in, text, n, pat, pat_bytes, pat_off, count);
    uint64_t total = 0;
    // (a blob byte is at most one seed of at most max_occ occurrences, and no call has more than BMX_MAP_MAX_CANDIDATES:
    // a larger capacity needs no larger device lists, and one pass fills them)
    const uint64_t most = pat_bytes > BMX_MAP_MAX_CANDIDATES / max_occ ? BMX_MAP_MAX_CANDIDATES : pat_bytes * max_occ;
    const uint64_t dev_cap = std::min(capacity, most);
    uint64_t *d_best = c.alloc<uint64_t>(2 * count * sizeof(uint64_t) + count);
    uint64_t *d_cand_off = cand_off ? c.alloc<uint64_t>((count + 1) * sizeof(uint64_t)) : nullptr;
    uint64_t *d_cand = dev_cap ? c.alloc<uint64_t>(2 * dev_cap * sizeof(uint64_t) + dev_cap) : nullptr;
    if (c.rc == BMX_OK)
        c.rc = bmx_index_map_device(c.ctx(), c.ix, c.d_pat, pat_bytes, c.d_off, count, min_len, max_occ, k, 0, d_best, d_best + count,
                                    reinterpret_cast<uint8_t *>(d_best + 2 * count), d_cand_off, d_cand,
                                    d_cand ? d_cand + dev_cap : nullptr,
                                    d_cand ? reinterpret_cast<uint8_t *>(d_cand + 2 * dev_cap) : nullptr, dev_cap, &total, nullptr);
    const uint64_t lists = std::min(total, dev_cap);
    if (c.rc == BMX_OK || c.rc == BMX_ERR_CAPACITY) {
        c.download(best_start, d_best, count * sizeof(uint64_t), "the mappings");
        c.download(best_end, d_best + count, count * sizeof(uint64_t), "the mappings");
        c.download(best_dist, d_best + 2 * count, count, "the mappings");
        if (cand_off) c.download(cand_off, d_cand_off, (count + 1) * sizeof(uint64_t), "the candidate offsets");
        c.download(cand_start, d_cand, lists * sizeof(uint64_t), "the candidates");
        c.download(cand_end, d_cand + dev_cap, lists * sizeof(uint64_t), "the candidates");
        c.download(cand_dist, d_cand + 2 * dev_cap, lists, "the candidates");
        if (n_candidates) *n_candidates = total;
    }
    return c.rc;
}

} // extern "C"
