// bmx_shim.hip -- the C ABI of libbmx.so (include/bmx.h): a thin HIP shim that
// stands where the reference's OpenCL host plumbing stood
// (BoyreMoore/BoyreMoore/BoyreMoore.cpp:213-312: context, six buffers, five
// blocking writes, runtime JIT, seven kernel arguments, NDRange, blocking read).
// No JIT (the kernel is compiled for gfx950 ahead of time), no per-call context,
// the text can stay resident, and match positions come back as an ordered list
// instead of device printf lines.
// This file holds the context, the error text and the thin dispatch into the
// per-feature files (the exact search: bmx_scan.hip, whose entry points are
// defined there), plus the device helpers of the corpus and the multi-GPU merge.
#include "bmx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "bmx_internal.h"
#include "bmx_aux_kernels.h"
#ifdef BMX_EXPERIMENTS
#include "bmx_exp.h"
#include "bmx_ordered_out.h"
#include "bmx_probe_kernel.h"
#endif

namespace {

thread_local char g_err[512] = "";

void set_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return BMX_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

} // namespace

// for the library's other translation units (bmx_multi.hip, bmx_host_entries.cpp): the text bmx_last_error() returns on
// this thread
void bmx_internal_set_error(const char *text) { snprintf(g_err, sizeof g_err, "%s", text ? text : ""); }
// ... and the buffer itself, for the files that format their messages in place (bmx_scan.hip)
char *bmx_internal_error_buffer(size_t *len)
{
    *len = sizeof g_err;
    return g_err;
}

extern "C" {

const char *bmx_last_error(void) { return g_err; }
const char *bmx_version(void) { return "bmx 0.1 (gfx950)"; }

int bmx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bmx_ctx_create(int device, bmx_ctx **out)
{
    if (!out) return BMX_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
        set_err("no HIP device %d (count %d)", device, n);
        return BMX_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(device));
    bmx_ctx *ctx = new bmx_ctx();
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        ctx->num_cu = prop.multiProcessorCount;
    const hipError_t e = bmx_internal_scan_create(&ctx->scan); // eager: a first search allocates nothing of the context's
    if (e != hipSuccess) {
        set_err("bmx_ctx_create: %s", hipGetErrorString(e));
        bmx_ctx_destroy(ctx);
        return BMX_ERR_HIP;
    }
    *out = ctx;
    return BMX_OK;
}

void bmx_ctx_destroy(bmx_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    bmx_internal_scan_free(ctx->scan);
    bmx_internal_ed_free(ctx->ed);
    bmx_internal_sa_free(ctx->sa);
    bmx_internal_lcp_free(ctx->lcp);
    bmx_internal_approx_free(ctx->approx);
    bmx_internal_approx_long_free(ctx->approx_long);
    bmx_internal_classes_free(ctx->classes);
    bmx_internal_hamming_free(ctx->hamming);
    bmx_internal_gaps_free(ctx->gaps);
    bmx_internal_regex_free(ctx->regex);
    bmx_internal_regex_long_free(ctx->regex_long);
    bmx_internal_regex_groups_free(ctx->regex_groups);
    bmx_internal_regex_begins_free(ctx->regex_begins);
    bmx_internal_regex_anchored_free(ctx->regex_anchored);
    bmx_internal_regex_anchored_begins_free(ctx->regex_anchored_begins);
    bmx_internal_regex_star_free(ctx->regex_star);
    bmx_internal_regex_star_begins_free(ctx->regex_star_begins);
    bmx_internal_ed_batch_free(ctx->ed_batch);
    bmx_internal_spans_free(ctx->spans);
    bmx_internal_dict_state_free(ctx->dict);
    bmx_internal_index_state_free(ctx->index);
    bmx_internal_align_free(ctx->align);
    bmx_internal_rows_free(ctx->rows);
    bmx_internal_subst_free(ctx->subst);
    delete ctx;
}

int bmx_merge_gathered_device(bmx_ctx *ctx, const uint64_t *d_gathered, int32_t world, uint64_t slot_stride,
                              uint64_t *d_merged, uint64_t merged_capacity, uint64_t *d_total, uint64_t seq,
                              void *stream_v)
{
    if (!ctx || !d_gathered || !d_total || world < 1 || slot_stride < 1) return BMX_ERR_ARG;
    if (merged_capacity > 0 && !d_merged) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bmx::merge_gathered_kernel, dim3(world), dim3(256), 0, (hipStream_t)stream_v, d_gathered,
                       (int)world, slot_stride, d_merged, merged_capacity, d_total, seq);
    HIPCHK(hipGetLastError());
    return BMX_OK;
}

// ---- edit distance (bmx_ed.hip) -------------------------------------------
int bmx_set_ed_variant(bmx_ctx *ctx, int variant)
{
    if (!ctx) return BMX_ERR_ARG;
    if (!bmx_internal_ed_variant_ok(variant)) { // a schedule of libbmx_exp.so only, or none at all
        set_err("bmx_set_ed_variant: schedule %d is not part of this library (experiments: libbmx_exp.so)", variant);
        return BMX_ERR_ARG;
    }
    ctx->ed_knobs.variant = variant;
    return BMX_OK;
}

float bmx_last_edit_distance_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_ed_ms(ctx->ed) : -1.0f; }

int bmx_edit_distance_device(bmx_ctx *ctx, const void *d_a, uint64_t la, const void *d_b, uint64_t lb,
                             uint64_t *distance, void *stream_v)
{
    if (!ctx || !distance || (la > 0 && !d_a) || (lb > 0 && !d_b)) return BMX_ERR_ARG;
    if (la >= (1ull << 31) || lb >= (1ull << 31)) return BMX_ERR_ARG;
    if (la == 0 || lb == 0) { // D[0][c] = c, D[r][0] = r (sequential.c:28-32)
        bmx_internal_ed_no_kernel(ctx->ed);
        *distance = la + lb;
        return BMX_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_ed(&ctx->ed, &ctx->ed_knobs, d_a, la, d_b, lb, distance, (hipStream_t)stream_v, g_err, sizeof g_err);
}

// ---- batched edit distance (bmx_ed_batch.hip) --------------------------------------------------
int bmx_edit_distance_batch_device(bmx_ctx *ctx, const void *d_a, uint64_t a_bytes, const uint64_t *d_a_off, uint64_t a_count,
                                   const void *d_b, uint64_t b_bytes, const uint64_t *d_b_off, uint64_t count, uint32_t limit,
                                   uint32_t *d_dist, void *stream_v)
{
    if (!bmx_ed_batch_args_ok(d_a, a_bytes, d_a_off, a_count, d_b, b_bytes, d_b_off, count, d_dist)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_ed_batch(&ctx->ed_batch, ctx, d_a, a_bytes, d_a_off, a_count, d_b, b_bytes, d_b_off, count, limit, d_dist,
                                 (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_ed_batch_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_ed_batch_ms(ctx->ed_batch) : -1.0f; }

int64_t bmx_last_ed_batch_fallbacks(bmx_ctx *ctx) { return ctx ? bmx_internal_ed_batch_fallbacks(ctx->ed_batch) : -1; }

// ---- suffix array (bmx_sa.hip) ---------------------------------------------
int bmx_suffix_array_device(bmx_ctx *ctx, const void *d_text, uint64_t n, int32_t *d_sa, void *stream_v)
{
    if (!ctx || (n > 0 && (!d_text || !d_sa)) || n >= (1ull << 31)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_suffix_array(&ctx->sa, (const uint8_t *)d_text, (uint32_t)n, d_sa, (hipStream_t)stream_v, ctx->sa_flags, g_err,
                                     sizeof g_err);
}

float bmx_last_suffix_array_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_sa_ms(ctx->sa) : -1.0f; }
int bmx_last_suffix_array_rounds(bmx_ctx *ctx) { return ctx ? bmx_internal_sa_rounds(ctx->sa) : 0; }
int bmx_last_suffix_array_lds_rounds(bmx_ctx *ctx) { return ctx ? bmx_internal_sa_lds_rounds(ctx->sa) : 0; }

// ---- LCP array over the suffix array (bmx_lcp.hip) ---------------------------------------------
int bmx_lcp_array_device(bmx_ctx *ctx, const void *d_text, uint64_t n, const int32_t *d_sa, int32_t *d_lcp, void *stream_v)
{
    if (!bmx_lcp_args_ok(d_text, n, d_lcp) || !d_sa || !ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_lcp(&ctx->lcp, (const uint8_t *)d_text, (uint32_t)n, d_sa, d_lcp, (hipStream_t)stream_v, g_err, sizeof g_err);
}

int bmx_lcp_stats_device(bmx_ctx *ctx, const int32_t *d_lcp, uint64_t n, uint32_t min_len, uint64_t out[4], void *stream_v)
{
    if (!d_lcp || !out || n == 0 || n >= (1ull << 31) || !ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_lcp_stats(&ctx->lcp, d_lcp, (uint32_t)n, min_len, out, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_lcp_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_lcp_ms(ctx->lcp) : -1.0f; }
int64_t bmx_last_lcp_long_pairs(bmx_ctx *ctx) { return ctx ? bmx_internal_lcp_long_pairs(ctx->lcp) : -1; }

// ---- row-wise results (bmx_rows.hip) -------------------------------------------------------------
int bmx_rows_split_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, uint8_t delim, uint64_t *d_off,
                          uint64_t capacity, uint64_t *n_rows, uint64_t *longest, void *stream_v)
{
    if (!bmx_rows_split_args_ok(d_text, n, d_off, capacity) || !ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_rows_split(&ctx->rows, ctx->num_cu, d_text, n, base_offset, delim, d_off, capacity, n_rows, longest,
                                   (hipStream_t)stream_v, g_err, sizeof g_err);
}

int bmx_rows_of_device(bmx_ctx *ctx, const uint64_t *d_off, uint64_t rows, const uint64_t *d_starts, const uint64_t *d_ends,
                       uint64_t len, uint64_t count, uint64_t *d_row, void *stream_v)
{
    if (!bmx_rows_of_args_ok(d_off, d_starts, d_ends, len, count, d_row)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_rows_of(&ctx->rows, d_off, rows, d_starts, d_ends, len, count, d_row, (hipStream_t)stream_v, g_err, sizeof g_err);
}

int bmx_rows_matching_device(bmx_ctx *ctx, const uint64_t *d_row, uint64_t count, uint64_t rows, uint32_t flags, uint64_t *d_rows_out,
                             uint64_t *d_counts_out, uint64_t capacity, uint64_t *n_out, void *stream_v)
{
    if (!bmx_rows_matching_args_ok(d_row, count, flags, d_rows_out, d_counts_out, capacity) || !ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_rows_matching(&ctx->rows, d_row, count, rows, flags, d_rows_out, d_counts_out, capacity, n_out,
                                      (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_rows_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_rows_ms(ctx->rows) : -1.0f; }

// ---- non-overlapping match selection, replace and extract (bmx_subst.hip) ------------------------
int bmx_spans_select_device(bmx_ctx *ctx, const uint64_t *d_starts, const uint64_t *d_ends, uint64_t len, uint64_t count,
                            const uint64_t *d_row, uint32_t flags, uint64_t *d_starts_out, uint64_t *d_ends_out, uint64_t *d_index_out,
                            uint64_t capacity, uint64_t *n_out, void *stream_v)
{
    if (!bmx_select_args_ok(d_starts, d_ends, len, count, flags, d_starts_out, d_ends_out, capacity, n_out)) return BMX_ERR_ARG;
    if (count == 0) {
        *n_out = 0;
        return BMX_OK;
    }
    if (!ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_select(&ctx->subst, ctx->select_tile_shift, d_starts, d_ends, len, count, d_row, flags, d_starts_out, d_ends_out,
                               d_index_out, capacity, n_out, (hipStream_t)stream_v, g_err, sizeof g_err);
}

int bmx_replace_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_starts,
                       const uint64_t *d_ends, uint64_t len, uint64_t count, const void *repl, uint64_t repl_len, void *d_out,
                       uint64_t capacity, uint64_t *n_out, void *stream_v)
{
    if (!bmx_subst_copy_args_ok(d_text, n, d_starts, d_ends, len, count, repl, repl_len, d_out, capacity, false, nullptr, n_out))
        return BMX_ERR_ARG;
    if (count == 0 && (n == 0 || capacity == 0)) {
        *n_out = n;
        return BMX_OK;
    }
    if (!ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    if (count == 0) { // no span: the text itself
        *n_out = n;
        HIPCHK(hipMemcpyAsync(d_out, d_text, std::min(n, capacity), hipMemcpyDeviceToDevice, (hipStream_t)stream_v));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream_v));
        return n > capacity ? BMX_ERR_CAPACITY : BMX_OK;
    }
    return bmx_internal_subst_copy(&ctx->subst, ctx->num_cu, d_text, n, base_offset, d_starts, d_ends, len, count, repl, repl_len, d_out,
                                   capacity, nullptr, n_out, (hipStream_t)stream_v, g_err, sizeof g_err);
}

int bmx_extract_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_starts,
                       const uint64_t *d_ends, uint64_t len, uint64_t count, void *d_blob, uint64_t capacity, uint64_t *d_off,
                       uint64_t *n_out, void *stream_v)
{
    if (!bmx_subst_copy_args_ok(d_text, n, d_starts, d_ends, len, count, nullptr, 0, d_blob, capacity, true, d_off, n_out))
        return BMX_ERR_ARG;
    if (!ctx) return BMX_ERR_ARG;
    *n_out = 0;
    HIPCHK(hipSetDevice(ctx->device));
    if (count == 0) { // no span: the single offset 0
        HIPCHK(hipMemsetAsync(d_off, 0, sizeof(uint64_t), (hipStream_t)stream_v));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream_v));
        return BMX_OK;
    }
    return bmx_internal_subst_copy(&ctx->subst, ctx->num_cu, d_text, n, base_offset, d_starts, d_ends, len, count, nullptr, 0, d_blob,
                                   capacity, d_off, n_out, (hipStream_t)stream_v, g_err, sizeof g_err);
}

// ... with a template (bmx_compile_template is bmx_regex_compile.cpp); the template's errors come before any HIP call
int bmx_expand_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_groups, int32_t n_groups,
                      uint64_t count, const void *tmpl, uint64_t tmpl_len, uint32_t flags, void *d_out, uint64_t capacity,
                      uint64_t *d_off, uint64_t *n_out, void *stream_v)
{
    if (!bmx_expand_args_ok(d_text, n, d_groups, n_groups, count, flags, d_out, capacity, d_off, n_out)) return BMX_ERR_ARG;
    bmx_template t;
    std::vector<uint8_t> lits(tmpl_len <= BMX_MAX_REPLACEMENT ? (size_t)tmpl_len + 1 : 1);
    if (bmx_compile_template(tmpl, tmpl_len, n_groups, &t, lits.data()) != BMX_OK) return BMX_ERR_ARG;
    const bool extract = (flags & BMX_EXPAND_EXTRACT) != 0;
    if (!extract && count == 0 && (n == 0 || capacity == 0)) {
        *n_out = n;
        return BMX_OK;
    }
    if (!ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    if (count == 0) { // no match: the text itself, or the single offset 0
        *n_out = extract ? 0 : n;
        if (extract) HIPCHK(hipMemsetAsync(d_off, 0, sizeof(uint64_t), (hipStream_t)stream_v));
        else HIPCHK(hipMemcpyAsync(d_out, d_text, std::min(n, capacity), hipMemcpyDeviceToDevice, (hipStream_t)stream_v));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream_v));
        return !extract && n > capacity ? BMX_ERR_CAPACITY : BMX_OK;
    }
    return bmx_internal_expand(&ctx->subst, ctx->num_cu, d_text, n, base_offset, d_groups, n_groups, count, &t, lits.data(), d_out,
                               capacity, extract ? d_off : nullptr, n_out, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_subst_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_subst_ms(ctx->subst) : -1.0f; }

// ---- approximate search (bmx_approx.hip) -------------------------------------------------------
int bmx_search_approx_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                             const char *pat, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist, uint64_t capacity,
                             uint64_t *n_matches, void *stream_v)
{
    if (!bmx_approx_args_ok(n, lead, pat, m, k, d_ends, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->approx_last_long = false;
    return bmx_internal_approx(&ctx->approx, ctx->num_cu, d_text, n, lead, base_offset, pat, nullptr, m, k, d_ends, d_dist,
                               capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

// the same with a class per pattern position: only the kernel's Peq table is built differently
int bmx_search_approx_classes_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                     const uint8_t *classes, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist,
                                     uint64_t capacity, uint64_t *n_matches, void *stream_v)
{
    if (!bmx_approx_args_ok(n, lead, classes, m, k, d_ends, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->approx_last_long = false;
    return bmx_internal_approx(&ctx->approx, ctx->num_cu, d_text, n, lead, base_offset, nullptr, classes, m, k, d_ends, d_dist,
                               capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

// patterns of up to BMX_MAX_APPROX_LONG_PATTERN bytes: more than 64 take a column of several words (bmx_approx_long.hip),
// the others the kernels above
int bmx_search_approx_long_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                  const char *pat, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist, uint64_t capacity,
                                  uint64_t *n_matches, void *stream_v)
{
    if (!bmx_approx_long_args_ok(n, lead, pat, m, k, d_ends, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    if (m <= BMX_MAX_APPROX_PATTERN)
        return bmx_search_approx_device(ctx, d_text, n, lead, base_offset, pat, m, k, d_ends, d_dist, capacity, n_matches, stream_v);
    HIPCHK(hipSetDevice(ctx->device));
    ctx->approx_last_long = true;
    return bmx_internal_approx_long(&ctx->approx_long, ctx->num_cu, d_text, n, lead, base_offset, pat, m, k, d_ends, d_dist,
                                    capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_approx_ms(bmx_ctx *ctx)
{
    if (!ctx) return -1.0f;
    return ctx->approx_last_long ? bmx_internal_approx_long_ms(ctx->approx_long) : bmx_internal_approx_ms(ctx->approx);
}

// ---- class-pattern search (bmx_classes.hip; bmx_compile_classes is bmx_classes_compile.cpp) -----
int bmx_search_classes_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                              const uint8_t *classes, int32_t m, uint64_t *d_match_positions, uint64_t capacity,
                              uint64_t *n_matches, void *stream_v)
{
    if (!bmx_classes_args_ok(n, classes, m, d_match_positions, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_classes(&ctx->classes, ctx->num_cu, d_text, n, n_own, base_offset, classes, m, d_match_positions,
                                capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_classes_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_classes_ms(ctx->classes) : -1.0f; }

// ---- k-mismatch search (bmx_hamming.hip) --------------------------------------------------------
int bmx_search_hamming_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset, const char *pat,
                              int32_t m, int32_t k, uint64_t must, uint64_t *d_starts, uint8_t *d_dist, uint64_t capacity,
                              uint64_t *n_matches, void *stream_v)
{
    if (!bmx_hamming_args_ok(n, pat, m, k, must, d_starts, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_hamming(&ctx->hamming, ctx->num_cu, d_text, n, n_own, base_offset, pat, nullptr, m, k, must, d_starts, d_dist,
                                capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

// the same with a class per pattern position: only the kernel's table is built differently
int bmx_search_hamming_classes_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                                      const uint8_t *classes, int32_t m, int32_t k, uint64_t must, uint64_t *d_starts,
                                      uint8_t *d_dist, uint64_t capacity, uint64_t *n_matches, void *stream_v)
{
    if (!bmx_hamming_args_ok(n, classes, m, k, must, d_starts, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_hamming(&ctx->hamming, ctx->num_cu, d_text, n, n_own, base_offset, nullptr, classes, m, k, must, d_starts,
                                d_dist, capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_hamming_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_hamming_ms(ctx->hamming) : -1.0f; }

// ---- gapped pattern search (bmx_gaps.hip; bmx_compile_gaps is bmx_gaps_compile.cpp) -------------
int bmx_search_gaps_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                           const uint8_t *classes, int32_t m, uint64_t optional, uint64_t *d_ends, uint64_t capacity,
                           uint64_t *n_matches, void *stream_v)
{
    if (!bmx_gaps_args_ok(n, lead, classes, m, optional, d_ends, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_gaps(&ctx->gaps, ctx->num_cu, d_text, n, lead, base_offset, classes, m, optional, d_ends, capacity,
                             n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_gaps_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_gaps_ms(ctx->gaps) : -1.0f; }

int bmx_gaps_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const uint8_t *classes, int32_t m,
                           uint64_t optional, const uint64_t *d_ends, uint64_t count, uint32_t flags, uint64_t *d_starts,
                           void *stream_v)
{
    if (!bmx_gaps_starts_args_ok(n, classes, m, optional, d_ends, count, flags, d_starts)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (an end needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_gaps_starts(&ctx->gaps, d_text, n, base_offset, classes, m, optional, d_ends, count, flags, d_starts,
                                    (hipStream_t)stream_v, g_err, sizeof g_err);
}

// ---- regular-expression search (bmx_regex.hip; bmx_compile_regex is bmx_regex_compile.cpp) ------
int bmx_search_regex_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset, const bmx_regex *re,
                            uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, void *stream_v)
{
    if (!bmx_regex_args_ok(n, lead, re, d_ends, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex(&ctx->regex, ctx->num_cu, d_text, n, lead, base_offset, re, d_ends, capacity, n_matches,
                              (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_regex_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_regex_ms(ctx->regex) : -1.0f; }

int bmx_regex_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                            const uint64_t *d_ends, uint64_t count, uint32_t flags, uint64_t *d_starts, void *stream_v)
{
    if (!bmx_regex_starts_args_ok(n, re, d_ends, count, flags, d_starts)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (an end needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_starts(&ctx->regex, d_text, n, base_offset, re, d_ends, count, 0, flags, d_starts, nullptr,
                                     (hipStream_t)stream_v, g_err, sizeof g_err);
}

// ... the capture groups of every span of a list (bmx_regex_groups.hip; bmx_compile_regex_groups is bmx_regex_compile.cpp)
int bmx_regex_groups_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                            const bmx_regex_groups *gr, const uint64_t *d_starts, const uint64_t *d_ends, uint64_t count,
                            uint64_t *d_groups, void *stream_v)
{
    if (!bmx_regex_groups_args_ok(n, re, gr, d_starts, d_ends, count, d_groups)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (a span needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_groups(&ctx->regex_groups, d_text, n, base_offset, re, gr, d_starts, d_ends, count, d_groups,
                                     (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_regex_groups_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_regex_groups_ms(ctx->regex_groups) : -1.0f; }

// ... for automata of up to 128 positions (bmx_regex_long.hip; bmx_compile_regex_long is bmx_regex_compile.cpp)
int bmx_search_regex_long_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                 const bmx_regex_long *re, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, void *stream_v)
{
    if (!bmx_regex_long_args_ok(n, lead, re, d_ends, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_long(&ctx->regex_long, ctx->num_cu, d_text, n, lead, base_offset, re, d_ends, capacity, n_matches,
                                   (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_regex_long_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_regex_long_ms(ctx->regex_long) : -1.0f; }

int bmx_regex_long_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex_long *re,
                                 const uint64_t *d_ends, uint64_t count, uint32_t flags, uint64_t *d_starts, void *stream_v)
{
    if (!bmx_regex_long_starts_args_ok(n, re, d_ends, count, flags, d_starts)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (an end needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_long_starts(&ctx->regex_long, d_text, n, base_offset, re, d_ends, count, flags, d_starts,
                                          (hipStream_t)stream_v, g_err, sizeof g_err);
}

// ... the mirror image: every start, and the end of every start of a list
int bmx_search_regex_begins_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t tail, uint64_t base_offset,
                                   const bmx_regex *re, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches, void *stream_v)
{
    if (!bmx_regex_begins_args_ok(n, tail, re, d_starts, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_begins(&ctx->regex_begins, ctx->num_cu, ctx->regex_begins_piece_shift, d_text, n, tail, base_offset, re,
                                     d_starts, capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_regex_begins_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_regex_begins_ms(ctx->regex_begins) : -1.0f; }

int bmx_regex_ends_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                          const uint64_t *d_starts, uint64_t count, const uint64_t *d_limit, uint32_t flags, uint64_t *d_ends,
                          void *stream_v)
{
    if (!bmx_regex_ends_args_ok(n, re, d_starts, count, flags, d_ends)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (a start needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_ends(&ctx->regex_begins, d_text, n, base_offset, re, d_starts, count, d_limit, flags, d_ends,
                                   (hipStream_t)stream_v, g_err, sizeof g_err);
}

// ---- anchored regular-expression search (bmx_regex_anchored.hip; bmx_compile_regex_anchored is bmx_regex_compile.cpp) ------
int bmx_search_regex_anchored_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                     const bmx_regex *re, const bmx_regex_anchors *an, uint32_t left, uint32_t right, uint64_t *d_ends,
                                     uint64_t capacity, uint64_t *n_matches, void *stream_v)
{
    if (!bmx_regex_args_ok(n, lead, re, d_ends, capacity) || !bmx_regex_anchors_ok(an, left, right) || !ctx || (n > 0 && !d_text))
        return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_anchored(&ctx->regex_anchored, ctx->num_cu, d_text, n, lead, base_offset, re, an, left, right, d_ends,
                                       capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_regex_anchored_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_regex_anchored_ms(ctx->regex_anchored) : -1.0f; }

int bmx_regex_anchored_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                     const bmx_regex_anchors *an, uint32_t left, uint32_t right, const uint64_t *d_ends,
                                     uint64_t count, uint32_t flags, uint64_t *d_starts, void *stream_v)
{
    if (!bmx_regex_starts_args_ok(n, re, d_ends, count, flags, d_starts) || !bmx_regex_anchors_ok(an, left, right)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (an end needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_anchored_starts(&ctx->regex_anchored, d_text, n, base_offset, re, an, left, right, d_ends, count, flags,
                                              d_starts, (hipStream_t)stream_v, g_err, sizeof g_err);
}

int bmx_search_regex_anchored_begins_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t tail, uint64_t base_offset,
                                            const bmx_regex *re, const bmx_regex_anchors *an, uint32_t left, uint32_t right,
                                            uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches, void *stream_v)
{
    if (!bmx_regex_begins_args_ok(n, tail, re, d_starts, capacity) || !bmx_regex_anchors_ok(an, left, right) || !ctx ||
        (n > 0 && !d_text))
        return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_anchored_begins(&ctx->regex_anchored_begins, ctx->num_cu, ctx->regex_begins_piece_shift, d_text, n, tail,
                                              base_offset, re, an, left, right, d_starts, capacity, n_matches, (hipStream_t)stream_v,
                                              g_err, sizeof g_err);
}

float bmx_last_regex_anchored_begins_ms(bmx_ctx *ctx)
{
    return ctx ? bmx_internal_regex_anchored_begins_ms(ctx->regex_anchored_begins) : -1.0f;
}

int bmx_regex_anchored_ends_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                   const bmx_regex_anchors *an, uint32_t left, uint32_t right, const uint64_t *d_starts,
                                   uint64_t count, const uint64_t *d_limit, uint32_t flags, uint64_t *d_ends, void *stream_v)
{
    if (!bmx_regex_ends_args_ok(n, re, d_starts, count, flags, d_ends) || !bmx_regex_anchors_ok(an, left, right)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (a start needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_anchored_ends(&ctx->regex_anchored_begins, d_text, n, base_offset, re, an, left, right, d_starts, count,
                                            d_limit, flags, d_ends, (hipStream_t)stream_v, g_err, sizeof g_err);
}

// ---- regular-expression search with unbounded repetition (bmx_regex_star.hip; bmx_compile_regex_star is
// bmx_regex_compile.cpp) ------
int bmx_search_regex_star_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                 const bmx_regex *re, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, void *stream_v)
{
    if (!bmx_regex_star_args_ok(n, lead, re, d_ends, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_star(&ctx->regex_star, ctx->num_cu, &ctx->regex_star_knobs, d_text, n, lead, base_offset, re, d_ends,
                                   capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_regex_star_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_regex_star_ms(ctx->regex_star) : -1.0f; }

int bmx_regex_star_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                 const uint64_t *d_ends, uint64_t count, uint32_t window, uint32_t flags, uint64_t *d_starts,
                                 void *stream_v)
{
    if (!bmx_regex_star_starts_args_ok(n, re, d_ends, count, window, flags, d_starts)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (an end needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t bad = 0;
    const int rc = bmx_internal_regex_starts(&ctx->regex, d_text, n, base_offset, re, d_ends, count, window, flags, d_starts, &bad,
                                             (hipStream_t)stream_v, g_err, sizeof g_err);
    if (rc != BMX_OK || !(bad & BMX_REGEX_STARTS_NO_MATCH)) return rc;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_star_lengths(re->m, re->first, re->last, re->follow, &min_len, &max_len, nullptr);
    if (max_len != BMX_REGEX_UNBOUNDED && (max_len <= 0 || (uint32_t)max_len <= window)) { // no longer match can exist
        set_err("bmx_regex_star_starts_device: an end at which no match of this expression ends");
        return BMX_ERR_ARG;
    }
    return bmx_internal_regex_star_starts_fix(d_text, base_offset, re, d_ends, count, d_starts, (hipStream_t)stream_v, g_err,
                                              sizeof g_err);
}

// ... the mirror image: every start, and the end of every start of a list within a window (bmx_regex_star_begins.hip)
int bmx_search_regex_star_begins_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t tail, uint64_t base_offset,
                                        const bmx_regex *re, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches,
                                        void *stream_v)
{
    if (!bmx_regex_star_begins_args_ok(n, tail, re, d_starts, capacity) || !ctx || (n > 0 && !d_text)) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_regex_star_begins(&ctx->regex_star_begins, ctx->num_cu, &ctx->regex_star_begins_knobs, d_text, n, tail,
                                          base_offset, re, d_starts, capacity, n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_regex_star_begins_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_regex_star_begins_ms(ctx->regex_star_begins) : -1.0f; }

int bmx_regex_star_ends_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                               const uint64_t *d_starts, uint64_t count, const uint64_t *d_limit, uint32_t window, uint32_t flags,
                               uint64_t *d_ends, uint64_t *n_clipped, void *stream_v)
{
    if (!bmx_regex_star_ends_args_ok(n, re, d_starts, count, window, flags, d_ends)) return BMX_ERR_ARG;
    if (n_clipped) *n_clipped = 0;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (a start needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t bad = 0, clipped = 0;
    const int rc = bmx_internal_regex_star_ends(&ctx->regex_star_begins, d_text, n, base_offset, re, d_starts, count, d_limit, window,
                                                flags, !ctx->regex_star_ends_no_early_exit, d_ends, &bad, &clipped,
                                                (hipStream_t)stream_v, g_err, sizeof g_err);
    if (rc != BMX_OK) return rc;
    if (n_clipped) *n_clipped = clipped;
    if (!(bad & BMX_REGEX_STAR_ENDS_NO_MATCH)) return BMX_OK;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_star_lengths(re->m, re->first, re->last, re->follow, &min_len, &max_len, nullptr);
    if (max_len != BMX_REGEX_UNBOUNDED && (max_len <= 0 || (uint32_t)max_len <= window)) { // no longer match can exist
        set_err("bmx_regex_star_ends_device: a start at which no match of this expression begins");
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}

// ---- match spans of the approximate search (bmx_spans.hip) --------------------------------------
namespace {
int spans_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const char *pat, const uint8_t *classes,
                 int32_t m, int32_t k, const uint64_t *d_ends, const uint8_t *d_dist, uint64_t count, uint32_t flags,
                 uint64_t *d_starts, uint64_t *d_sel_ends, uint8_t *d_sel_dist, uint64_t *n_spans, void *stream_v)
{
    if (!bmx_spans_args_ok(n, pat ? (const void *)pat : (const void *)classes, m, k, d_ends, d_dist, count, flags, d_starts, d_sel_ends))
        return BMX_ERR_ARG;
    if (n_spans) *n_spans = 0;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (an end needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_spans(&ctx->spans, d_text, n, base_offset, pat, classes, m, k, d_ends, d_dist, count, flags, d_starts,
                              d_sel_ends, d_sel_dist, n_spans, (hipStream_t)stream_v, g_err, sizeof g_err);
}
} // namespace

int bmx_approx_spans_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const char *pat, int32_t m,
                            int32_t k, const uint64_t *d_ends, const uint8_t *d_dist, uint64_t count, uint32_t flags,
                            uint64_t *d_starts, uint64_t *d_sel_ends, uint8_t *d_sel_dist, uint64_t *n_spans, void *stream_v)
{
    if (!pat) return BMX_ERR_ARG;
    return spans_device(ctx, d_text, n, base_offset, pat, nullptr, m, k, d_ends, d_dist, count, flags, d_starts, d_sel_ends,
                        d_sel_dist, n_spans, stream_v);
}

int bmx_approx_spans_classes_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const uint8_t *classes,
                                    int32_t m, int32_t k, const uint64_t *d_ends, const uint8_t *d_dist, uint64_t count,
                                    uint32_t flags, uint64_t *d_starts, uint64_t *d_sel_ends, uint8_t *d_sel_dist,
                                    uint64_t *n_spans, void *stream_v)
{
    if (!classes) return BMX_ERR_ARG;
    return spans_device(ctx, d_text, n, base_offset, nullptr, classes, m, k, d_ends, d_dist, count, flags, d_starts, d_sel_ends,
                        d_sel_dist, n_spans, stream_v);
}

// a string of up to BMX_MAX_APPROX_LONG_PATTERN bytes (the list of bmx_search_approx_long_device): the same state, the same
// selection, the starts by a column of several words where m > 64
int bmx_approx_long_spans_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const char *pat, int32_t m,
                                 int32_t k, const uint64_t *d_ends, const uint8_t *d_dist, uint64_t count, uint32_t flags,
                                 uint64_t *d_starts, uint64_t *d_sel_ends, uint8_t *d_sel_dist, uint64_t *n_spans, void *stream_v)
{
    if (!bmx_spans_long_args_ok(n, pat, m, k, d_ends, d_dist, count, flags, d_starts, d_sel_ends)) return BMX_ERR_ARG;
    if (m <= BMX_MAX_APPROX_PATTERN)
        return bmx_approx_spans_device(ctx, d_text, n, base_offset, pat, m, k, d_ends, d_dist, count, flags, d_starts, d_sel_ends,
                                       d_sel_dist, n_spans, stream_v);
    if (n_spans) *n_spans = 0;
    if (count == 0) return BMX_OK;
    if (!ctx || !d_text) return BMX_ERR_ARG; // (an end needs a byte: n == 0 cannot have one)
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_spans(&ctx->spans, d_text, n, base_offset, pat, nullptr, m, k, d_ends, d_dist, count, flags, d_starts,
                              d_sel_ends, d_sel_dist, n_spans, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_spans_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_spans_ms(ctx->spans) : -1.0f; }

// ---- dictionary search (bmx_dict.hip) ----------------------------------------------------------
int bmx_dict_create(bmx_ctx *ctx, const char *const *pats, const int32_t *ms, int32_t K, bmx_dict **out)
{
    const int rc = bmx_dict_patterns_ok(pats, ms, K);
    if (rc != BMX_OK) return rc;
    if (!ctx || !out) return BMX_ERR_ARG;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_dict_create(ctx, ctx->device, pats, ms, K, out, g_err, sizeof g_err);
}

void bmx_dict_destroy(bmx_dict *d) { bmx_internal_dict_destroy(d); }

int bmx_dict_search_device(bmx_ctx *ctx, const bmx_dict *d, const void *d_text, uint64_t n, uint64_t n_own,
                           uint64_t base_offset, uint64_t *d_pos, uint32_t *d_pid, uint64_t capacity, uint64_t *n_matches,
                           void *stream_v)
{
    if (!ctx || !d || bmx_internal_dict_owner(d) != ctx || (n > 0 && !d_text) || n >= (1ull << 40) ||
        (capacity > 0 && !d_pos))
        return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_dict_search(&ctx->dict, ctx->num_cu, d, d_text, n, n_own, base_offset, d_pos, d_pid, capacity,
                                    n_matches, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_dict_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_dict_ms(ctx->dict) : -1.0f; }

int64_t bmx_last_dict_candidates(bmx_ctx *ctx) { return ctx ? bmx_internal_dict_candidates(ctx->dict) : -1; }

// ---- text index (bmx_index.hip) ------------------------------------------------------------------
int bmx_index_create_device(bmx_ctx *ctx, const void *d_text, uint64_t n, const int32_t *d_sa, void *stream_v, bmx_index **out)
{
    if (!ctx || !d_text || !out || n == 0 || n >= (1ull << 31)) return BMX_ERR_ARG;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_index_create(&ctx->index, ctx, ctx->device, d_text, n, d_sa, (hipStream_t)stream_v, out, g_err,
                                     sizeof g_err);
}

void bmx_index_destroy(bmx_index *ix) { bmx_internal_index_destroy(ix); }

int bmx_index_sa(const bmx_index *ix, const int32_t **d_sa_out)
{
    if (!ix || !d_sa_out) return BMX_ERR_ARG;
    *d_sa_out = bmx_internal_index_sa(ix);
    return BMX_OK;
}

float bmx_index_build_ms(const bmx_index *ix) { return ix ? bmx_internal_index_build_ms(ix) : -1.0f; }

int bmx_index_count_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                           uint64_t count, uint32_t *d_lo, uint32_t *d_cnt, void *stream_v)
{
    if (!bmx_index_query_args_ok(d_pat, d_pat_off, count, d_cnt)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !ix || bmx_internal_index_owner(ix) != ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_index_count(&ctx->index, ix, d_pat, pat_bytes, d_pat_off, count, d_lo, d_cnt, !ctx->index_no_dir,
                                    (hipStream_t)stream_v, g_err, sizeof g_err);
}

int bmx_index_locate_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                            uint64_t count, uint64_t base_offset, uint64_t *d_out_off, uint64_t *d_pos, uint64_t capacity,
                            uint64_t *n_matches, void *stream_v)
{
    if (!bmx_index_query_args_ok(d_pat, d_pat_off, count, d_out_off) || (count > 0 && capacity > 0 && !d_pos)) return BMX_ERR_ARG;
    if (n_matches) *n_matches = 0;
    if (count == 0) return BMX_OK;
    if (!ctx || !ix || bmx_internal_index_owner(ix) != ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_index_locate(&ctx->index, ix, d_pat, pat_bytes, d_pat_off, count, base_offset, d_out_off, d_pos, capacity,
                                     n_matches, !ctx->index_no_dir, (hipStream_t)stream_v, g_err, sizeof g_err);
}

int bmx_index_match_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                           uint64_t count, uint32_t *d_len, uint32_t *d_lo, uint32_t *d_cnt, void *stream_v)
{
    if (!bmx_index_query_args_ok(d_pat, d_pat_off, count, d_len)) return BMX_ERR_ARG;
    if (count == 0) return BMX_OK;
    if (!ctx || !ix || bmx_internal_index_owner(ix) != ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_index_match(&ctx->index, ix, d_pat, pat_bytes, d_pat_off, count, d_len, d_lo, d_cnt, !ctx->index_no_dir,
                                    (hipStream_t)stream_v, g_err, sizeof g_err);
}

int bmx_index_seeds_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                           uint64_t count, uint32_t min_len, uint32_t max_occ, uint64_t *d_seed_off, uint32_t *d_qpos,
                           uint32_t *d_len, uint32_t *d_lo, uint32_t *d_cnt, uint64_t capacity, uint64_t *n_seeds, void *stream_v)
{
    if (!bmx_index_seeds_args_ok(d_pat, d_pat_off, count, min_len, d_seed_off, d_qpos, d_len, d_lo, d_cnt, capacity))
        return BMX_ERR_ARG;
    if (n_seeds) *n_seeds = 0;
    if (count == 0) return BMX_OK;
    if (!ctx || !ix || bmx_internal_index_owner(ix) != ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_index_seeds(&ctx->index, ix, d_pat, pat_bytes, d_pat_off, count, min_len, max_occ, d_seed_off, d_qpos,
                                    d_len, d_lo, d_cnt, capacity, n_seeds, !ctx->index_no_dir, (hipStream_t)stream_v, g_err,
                                    sizeof g_err);
}

int bmx_index_map_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                         uint64_t count, uint32_t min_len, uint32_t max_occ, int32_t k, uint64_t base_offset,
                         uint64_t *d_best_start, uint64_t *d_best_end, uint8_t *d_best_dist, uint64_t *d_cand_off,
                         uint64_t *d_cand_start, uint64_t *d_cand_end, uint8_t *d_cand_dist, uint64_t capacity,
                         uint64_t *n_candidates, void *stream_v)
{
    if (!bmx_index_map_args_ok(d_pat, d_pat_off, count, min_len, max_occ, k, d_best_start, d_best_end, d_best_dist, d_cand_start,
                               d_cand_end, d_cand_dist, capacity))
        return BMX_ERR_ARG;
    if (n_candidates) *n_candidates = 0;
    if (count == 0) return BMX_OK;
    if (!ctx || !ix || bmx_internal_index_owner(ix) != ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_index_map(&ctx->index, ix, d_pat, pat_bytes, d_pat_off, count, min_len, max_occ, (uint32_t)k, base_offset,
                                  d_best_start, d_best_end, d_best_dist, d_cand_off, d_cand_start, d_cand_end, d_cand_dist,
                                  capacity, n_candidates, !ctx->index_no_dir, (hipStream_t)stream_v, g_err, sizeof g_err);
}

int64_t bmx_last_index_map_candidates(bmx_ctx *ctx) { return ctx ? bmx_internal_index_map_candidates(ctx->index) : -1; }

int bmx_last_index_map_phases(bmx_ctx *ctx, float out[5])
{
    return ctx && out ? bmx_internal_index_map_phases(ctx->index, out) : BMX_ERR_ARG;
}

float bmx_last_index_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_index_ms(ctx->index) : -1.0f; }

// ---- alignments (bmx_align.hip) ------------------------------------------------------------------
int bmx_align_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const void *d_pat, uint64_t pat_bytes,
                     const uint64_t *d_pat_off, uint64_t pat_count, const uint32_t *d_pid, const uint64_t *d_start,
                     const uint64_t *d_end, uint64_t count, int32_t k, uint8_t *d_dist, uint64_t *d_op_off, uint32_t *d_ops,
                     uint64_t capacity, uint64_t *n_ops, void *stream_v)
{
    if (!bmx_align_args_ok(d_text, n, d_pat, d_pat_off, pat_count, d_pid, d_start, d_end, count, k, d_op_off, d_ops, capacity))
        return BMX_ERR_ARG;
    if (n_ops) *n_ops = 0;
    if (count == 0) return BMX_OK;
    if (!ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return bmx_internal_align(&ctx->align, (uint64_t)(ctx->align_ws_kib > 0 ? ctx->align_ws_kib : 0) << 10, d_text, n, base_offset,
                              d_pat, pat_bytes, d_pat_off, pat_count, d_pid, d_start, d_end, count, (uint32_t)k, d_dist, d_op_off,
                              d_ops, capacity, n_ops, (hipStream_t)stream_v, g_err, sizeof g_err);
}

float bmx_last_align_ms(bmx_ctx *ctx) { return ctx ? bmx_internal_align_ms(ctx->align) : -1.0f; }

int64_t bmx_last_align_launches(bmx_ctx *ctx) { return ctx ? bmx_internal_align_launches(ctx->align) : -1; }

int bmx_device_alloc(bmx_ctx *ctx, uint64_t bytes, void **d_ptr_out)
{
    if (!ctx || !d_ptr_out) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMalloc(d_ptr_out, bytes ? bytes : 1));
    return BMX_OK;
}

int bmx_device_free(bmx_ctx *ctx, void *d_ptr)
{
    if (!ctx) return BMX_ERR_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    if (d_ptr) HIPCHK(hipFree(d_ptr));
    return BMX_OK;
}

int bmx_text_upload(bmx_ctx *ctx, const char *text, uint64_t n, void **d_text_out)
{
    if (!ctx || !d_text_out || (n > 0 && !text)) return BMX_ERR_ARG;
    int rc = bmx_device_alloc(ctx, n, d_text_out);
    if (rc != BMX_OK) return rc;
    if (n) {
        const hipError_t e = hipMemcpy(*d_text_out, text, n, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_err("bmx_text_upload: %s", hipGetErrorString(e));
            (void)hipFree(*d_text_out);
            *d_text_out = nullptr;
            return BMX_ERR_HIP;
        }
    }
    return BMX_OK;
}

int bmx_device_download(bmx_ctx *ctx, void *dst, const void *d_src, uint64_t bytes)
{
    if (!ctx || (bytes > 0 && (!dst || !d_src))) return BMX_ERR_ARG;
    if (bytes == 0) return BMX_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return BMX_OK;
}

#ifdef BMX_EXPERIMENTS
// libbmx_exp.so only: the measurement / test switches of a context (round 2 read them from the environment on every call,
// in the product library too).  Returns BMX_ERR_ARG for an unknown name.
int bmx_exp_ed_stamps(bmx_ctx *ctx, uint64_t *out280)
{
    if (!ctx || !out280) return BMX_ERR_ARG;
    return bmx_internal_ed_stamps(ctx->ed, out280);
}

int bmx_exp_set_knob(bmx_ctx *ctx, const char *name, int value)
{
    if (!ctx || !name) return BMX_ERR_ARG;
    const std::string k(name);
    if (k == "max_grid") ctx->scan_knobs.max_grid = value;
    else if (k == "no_dense") ctx->scan_knobs.no_dense = value != 0;
    else if (k == "no_text_sample") ctx->scan_knobs.text_sample = value == 0;
    else if (k == "multi_no_qgram") ctx->scan_knobs.multi_no_qgram = value != 0;
    else if (k == "ed_lag") ctx->ed_knobs.lag = value;
    else if (k == "ed_group") ctx->ed_knobs.group = value;
    else if (k == "ed_step_x") ctx->ed_knobs.step_x = value;
    else if (k == "ed_stamp_block") ctx->ed_knobs.stamp_block = value;
    else if (k == "sa_flags") ctx->sa_flags = value;
    else if (k == "index_no_dir") ctx->index_no_dir = value != 0;
    else if (k == "align_ws_kib") ctx->align_ws_kib = value;
    else if (k == "select_tile_shift" && (value == 0 || (value >= 3 && value <= 8))) ctx->select_tile_shift = value;
    else if (k == "regex_star_force_slow") ctx->regex_star_knobs.force_slow = value != 0;
    else if (k == "regex_star_piece_shift" && (value == 0 || (value >= 4 && value <= 12))) ctx->regex_star_knobs.piece_shift = value;
    else if (k == "regex_begins_piece_shift" && (value == 0 || (value >= 4 && value <= 12))) ctx->regex_begins_piece_shift = value;
    else if (k == "regex_star_warm" && value >= 0 && value <= 65536 && value % 16 == 0) ctx->regex_star_knobs.warm = value;
    else if (k == "regex_star_begins_force_slow") ctx->regex_star_begins_knobs.force_slow = value != 0;
    else if (k == "regex_star_begins_piece_shift" && (value == 0 || (value >= 4 && value <= 12))) ctx->regex_star_begins_knobs.piece_shift = value;
    else if (k == "regex_star_begins_warm" && value >= 0 && value <= 65536 && value % 16 == 0) ctx->regex_star_begins_knobs.warm = value;
    else if (k == "regex_star_ends_no_early_exit") ctx->regex_star_ends_no_early_exit = value != 0;
    else if (k == "ordered_seq" && value >= 0) {
        for (void *session : {ctx->approx, ctx->approx_long, ctx->classes, ctx->hamming, ctx->gaps, ctx->regex, ctx->regex_long, ctx->regex_begins, ctx->regex_anchored, ctx->regex_anchored_begins, ctx->regex_star, ctx->regex_star_begins, ctx->dict}) bmx::ordered_set_seq(session, (uint64_t)value);
    } else if (k == "tile_piece_shift" && (value == 0 || (value >= 6 && value <= 12))) {
        // the dictionary's tile is 2^(value - 6) rounds of 8 KiB and at most 256 KiB: a context with a dictionary session
        // takes no 12
        if ((uint32_t)value > bmx::ORDERED_DICT_MAX_PIECE_SHIFT && ctx->dict) return BMX_ERR_ARG;
        for (void *session : {ctx->approx, ctx->approx_long, ctx->classes, ctx->hamming, ctx->gaps, ctx->regex, ctx->regex_long, ctx->regex_begins, ctx->regex_anchored, ctx->regex_anchored_begins, ctx->regex_star, ctx->regex_star_begins, ctx->dict}) bmx::ordered_set_piece_shift(session, (uint32_t)value);
    } else if (k == "tile_max_grid" && value >= 0) {
        for (void *session : {ctx->approx, ctx->approx_long, ctx->classes, ctx->hamming, ctx->gaps, ctx->regex, ctx->regex_long, ctx->regex_begins, ctx->regex_anchored, ctx->regex_anchored_begins, ctx->regex_star, ctx->regex_star_begins, ctx->dict}) bmx::ordered_set_max_grid(session, (uint32_t)value);
    } else return BMX_ERR_ARG;
    return BMX_OK;
}

// libbmx_exp.so only: what the last launch of one ordered-output session ran with (tests assert the geometry they forced)
int bmx_exp_last_launch(bmx_ctx *ctx, const char *session, uint64_t *out3)
{
    if (!ctx || !session || !out3) return BMX_ERR_ARG;
    const std::string k(session);
    const void *state = nullptr;
    if (k == "approx") state = ctx->approx;
    else if (k == "approx_long") state = ctx->approx_long;
    else if (k == "classes") state = ctx->classes;
    else if (k == "hamming") state = ctx->hamming;
    else if (k == "gaps") state = ctx->gaps;
    else if (k == "regex") state = ctx->regex;
    else if (k == "regex_long") state = ctx->regex_long;
    else if (k == "regex_begins") state = ctx->regex_begins;
    else if (k == "regex_anchored") state = ctx->regex_anchored;
    else if (k == "regex_anchored_begins") state = ctx->regex_anchored_begins;
    else if (k == "regex_star") state = ctx->regex_star;
    else if (k == "regex_star_begins") state = ctx->regex_star_begins;
    else if (k == "dict") state = ctx->dict;
    else if (k == "rows") { // (its own state: the tile is fixed, so out3[0] is log2 of its bytes)
        bmx_internal_rows_last(ctx->rows, out3);
        return BMX_OK;
    } else if (k == "select") { // (its own state too: log2 T, levels, tiles of the last selection)
        bmx_internal_subst_last(ctx->subst, out3);
        return BMX_OK;
    } else return BMX_ERR_ARG;
    bmx::ordered_last_launch(state, out3);
    return BMX_OK;
}

// libbmx_exp.so only: what the last bmx_search_regex_star_device of the context did (include/bmx_exp.h)
int bmx_exp_regex_star_last(bmx_ctx *ctx, uint64_t *out10)
{
    if (!ctx || !out10) return BMX_ERR_ARG;
    bmx_internal_regex_star_last(ctx->regex_star, out10);
    return BMX_OK;
}

// ... and the last bmx_search_regex_star_begins_device
int bmx_exp_regex_star_begins_last(bmx_ctx *ctx, uint64_t *out10)
{
    if (!ctx || !out10) return BMX_ERR_ARG;
    bmx_internal_regex_star_begins_last(ctx->regex_star_begins, out10);
    return BMX_OK;
}

// libbmx_exp.so only (tools/hbm_read_probe.py): read-only sweep of n bytes at d_text with plain global loads into
// registers -- no LDS, no barrier, no tiles (bmx_probe_kernel.h).  `unroll` loads in flight per lane (4, 8, 16), `nt`
// cache policy, `block` threads per workgroup, `blocks_per_cu` of them per CU.  ms_out[i] = duration of launch i (HIP
// events on `stream`).
int bmx_probe_read(bmx_ctx *ctx, const void *d_text, uint64_t n, int block, int blocks_per_cu, int unroll, int nt,
                   int launches, float *ms_out, void *stream_v)
{
    if (!ctx || !d_text || !ms_out || launches < 1 || block < 64 || block > 1024 || block % 64 || blocks_per_cu < 1) return BMX_ERR_ARG;
    if (((uintptr_t)d_text & 15u) != 0) return BMX_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_v;
    HIPCHK(hipSetDevice(ctx->device));
    void (*k)(const uint8_t *, uint64_t, uint32_t *) = nullptr;
    switch (unroll * 2 + (nt ? 1 : 0)) {
    case 2: k = bmx::probe_read_kernel<1, 0>; break;
    case 3: k = bmx::probe_read_kernel<1, 1>; break;
    case 4: k = bmx::probe_read_kernel<2, 0>; break;
    case 5: k = bmx::probe_read_kernel<2, 1>; break;
    case 8: k = bmx::probe_read_kernel<4, 0>; break;
    case 9: k = bmx::probe_read_kernel<4, 1>; break;
    case 16: k = bmx::probe_read_kernel<8, 0>; break;
    case 17: k = bmx::probe_read_kernel<8, 1>; break;
    case 32: k = bmx::probe_read_kernel<16, 0>; break;
    case 33: k = bmx::probe_read_kernel<16, 1>; break;
    default: return BMX_ERR_ARG;
    }
    uint32_t *d_sink = nullptr;
    HIPCHK(hipMalloc(&d_sink, sizeof(uint32_t)));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    hipError_t e = hipMemsetAsync(d_sink, 0, sizeof(uint32_t), stream);
    const uint32_t grid = (uint32_t)(ctx->num_cu * blocks_per_cu);
    for (int i = 0; i < launches && e == hipSuccess; ++i) {
        e = hipEventRecord(e0, stream);
        hipLaunchKernelGGL(k, dim3(grid), dim3(block), 0, stream, (const uint8_t *)d_text, n >> 4, d_sink);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(e1, stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_out[i], e0, e1);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(d_sink);
    if (e != hipSuccess) {
        set_err("bmx_probe_read: %s", hipGetErrorString(e));
        return BMX_ERR_HIP;
    }
    return BMX_OK;
}
#endif

int bmx_gen_text_device(bmx_ctx *ctx, void *d_dst, uint64_t start, uint64_t len, uint64_t seed, int kind,
                        void *stream_v)
{
    if (!ctx || (len > 0 && !d_dst) || (kind != 0 && kind != 1)) return BMX_ERR_ARG;
    if (len == 0) return BMX_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t nwords = ((start + len + 7) >> 3) - (start >> 3);
    const uint32_t block = 256;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nwords + block - 1) / block, (uint64_t)ctx->num_cu * 32);
    hipLaunchKernelGGL(bmx::gen_text_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream_v, (uint8_t *)d_dst,
                       start, len, seed, kind);
    HIPCHK(hipGetLastError());
    return BMX_OK;
}

int bmx_plant_device(bmx_ctx *ctx, void *d_dst, uint64_t start, uint64_t len, const char *pat, int32_t m,
                     const uint64_t *offsets, uint64_t count, void *stream_v)
{
    if (!ctx || !pat || m < 1 || m > BMX_MAX_PATTERN || (count > 0 && !offsets) || (len > 0 && !d_dst))
        return BMX_ERR_ARG;
    if (count == 0 || len == 0) return BMX_OK;
    hipStream_t stream = (hipStream_t)stream_v;
    HIPCHK(hipSetDevice(ctx->device));
    uint64_t *d_off = nullptr;
    uint8_t *d_pat = nullptr;
    HIPCHK(hipMalloc(&d_off, count * sizeof(uint64_t)));
    hipError_t e = hipMalloc(&d_pat, (size_t)m);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, offsets, count * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pat, pat, (size_t)m, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        const uint64_t total = count * (uint64_t)m;
        const uint32_t block = 256;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((total + block - 1) / block, (uint64_t)ctx->num_cu * 8);
        hipLaunchKernelGGL(bmx::plant_kernel, dim3(grid), dim3(block), 0, stream, (uint8_t *)d_dst, start, len,
                           d_pat, (uint32_t)m, d_off, count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_off);
    if (d_pat) (void)hipFree(d_pat);
    if (e != hipSuccess) {
        set_err("bmx_plant_device: %s", hipGetErrorString(e));
        return BMX_ERR_HIP;
    }
    return BMX_OK;
}

} // extern "C"
