// bmx_internal.h -- what the library's translation units share and the C ABI (include/bmx.h) does not show: the context
// (struct bmx_ctx), the bmx_internal_* functions the shim calls (included by the shim and by every file that defines one, so a changed
// signature fails to compile), the HIP-check macro of the per-feature files, and the argument checks that the device
// entries (bmx_shim.hip, bmx_scan.hip) and the host-buffer entries (bmx_host_entries.cpp) both make before any HIP call.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <cstddef>
#include <cstdio>

#include "bmx.h"
#include "bmx_regex_sets.h"

// In a function with `char *err, size_t errlen` that returns a BMX_* code: `where` names the entry point.
#define BMX_HIP(where, expr)                                                                      \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            snprintf(err, errlen, "%s: %s failed: %s", (where), #expr, hipGetErrorString(e__)); \
            return BMX_ERR_HIP;                                                                   \
        }                                                                                         \
    } while (0)

namespace bmx {
inline uint32_t ceil_log2(uint64_t x)
{
    uint32_t s = 0;
    while ((1ull << s) < x) ++s;
    return s;
}
} // namespace bmx

// bmx_shim.hip: the text bmx_last_error() returns on this thread
void bmx_internal_set_error(const char *text);
char *bmx_internal_error_buffer(size_t *len); // ... and its buffer (thread-local), for a file that formats its own messages
// bmx_scan.hip: the exact search's state, made eagerly with the context (the first HIP error, or hipSuccess; *state is
// set either way).  Its entry points of the C ABI are defined in that file.  What (libbmx_exp.so) bmx_exp_set_knob sets:
struct bmx_scan_knobs {
    bool text_sample = true;     // false: the walker goes by the pattern's symbols, not the text's
    int max_grid = 0;            // > 0: at most this many workgroups per scan (small texts then reach the stolen tail)
    bool no_dense = false;       // true: no fill pass (a full parking buffer appends the direct way)
    bool multi_no_qgram = false; // true: the multi-pattern pass walks byte-wise only
};
hipError_t bmx_internal_scan_create(void **state);
void bmx_internal_scan_free(void *state);
// bmx_sort.hip
int bmx_internal_radix_sort(uint64_t *d_keys, uint64_t n, unsigned end_bit, void **scratch, size_t *scratch_bytes, hipStream_t stream,
                            char *err, size_t errlen);
// bmx_sa.hip (flags: 1 = library rounds only, 2 = a host wait per round, 4 = per-round trace on stderr)
int bmx_internal_suffix_array(void **state, const uint8_t *d_text, uint32_t n, int32_t *d_sa, hipStream_t stream, int flags, char *err,
                              size_t errlen);
void bmx_internal_sa_free(void *state);
float bmx_internal_sa_ms(const void *state);
int bmx_internal_sa_rounds(const void *state);
int bmx_internal_sa_lds_rounds(const void *state);
// bmx_ed.hip: the single-pair edit distance.  What bmx_set_ed_variant and (libbmx_exp.so) bmx_exp_set_knob set:
struct bmx_ed_knobs {
    int variant = 0;      // schedule (include/bmx.h, bmx_set_ed_variant)
    int lag = -1;         // rows a band is assumed to trail its predecessor by (< 0: the schedule's measured one)
    int group = 32;       // hand-over group of the band pipeline (16 or 32 rows)
    int stamp_block = -1; // the band whose cycle counts bmx_exp_ed_stamps returns (< 0: the middle forward band)
    int step_x = 0;       // timing experiment on the helper-wave band's step (index into g_ed_step_experiments)
};
int bmx_internal_ed(void **state, const bmx_ed_knobs *knobs, const void *d_a, uint64_t la, const void *d_b, uint64_t lb,
                    uint64_t *distance, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_ed_free(void *state);
float bmx_internal_ed_ms(const void *state);
void bmx_internal_ed_no_kernel(void *state); // a call the shim answered itself (an empty string): the last ms is -1 again
bool bmx_internal_ed_variant_ok(int variant); // what bmx_set_ed_variant accepts in THIS library
int bmx_internal_ed_stamps(const void *state, uint64_t *out280); // libbmx_exp.so only
// bmx_approx.hip
int bmx_internal_approx(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                        const char *pat, const uint8_t *classes, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist,
                        uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_approx_free(void *state);
float bmx_internal_approx_ms(const void *state);
// bmx_approx_long.hip (64 < m <= BMX_MAX_APPROX_LONG_PATTERN)
int bmx_internal_approx_long(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                             const char *pat, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist, uint64_t capacity,
                             uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_approx_long_free(void *state);
float bmx_internal_approx_long_ms(const void *state);
uint32_t bmx_internal_approx_long_piece_shift(uint64_t n, int32_t m, int32_t k, uint64_t resident_lanes); // log2 of the ends per lane
// bmx_classes.hip
int bmx_internal_classes(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                         const uint8_t *classes, int32_t m, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches,
                         hipStream_t stream, char *err, size_t errlen);
void bmx_internal_classes_free(void *state);
float bmx_internal_classes_ms(const void *state);
uint32_t bmx_internal_classes_piece_shift(uint64_t n, int32_t m, uint64_t resident_lanes); // log2 of the ends per lane
// bmx_hamming.hip (pat: the string, or NULL and the classes)
int bmx_internal_hamming(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                         const char *pat, const uint8_t *classes, int32_t m, int32_t k, uint64_t must, uint64_t *d_starts,
                         uint8_t *d_dist, uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_hamming_free(void *state);
float bmx_internal_hamming_ms(const void *state);
// bmx_gaps.hip
int bmx_internal_gaps(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                      const uint8_t *classes, int32_t m, uint64_t optional, uint64_t *d_ends, uint64_t capacity,
                      uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen);
int bmx_internal_gaps_starts(void **state, const void *d_text, uint64_t n, uint64_t base_offset, const uint8_t *classes,
                             int32_t m, uint64_t optional, const uint64_t *d_ends, uint64_t count, uint32_t flags,
                             uint64_t *d_starts, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_gaps_free(void *state);
float bmx_internal_gaps_ms(const void *state);
// bmx_regex.hip
int bmx_internal_regex(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                       const bmx_regex *re, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, hipStream_t stream,
                       char *err, size_t errlen);
int bmx_internal_regex_starts(void **state, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                              const uint64_t *d_ends, uint64_t count, uint32_t window, uint32_t flags, uint64_t *d_starts,
                              uint64_t *bad_out, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_regex_free(void *state);
float bmx_internal_regex_ms(const void *state);
// bmx_regex_long.hip: the same two passes for automata of up to 128 positions (struct bmx_regex_long)
int bmx_internal_regex_long(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                            const bmx_regex_long *re, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, hipStream_t stream,
                            char *err, size_t errlen);
int bmx_internal_regex_long_starts(void **state, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex_long *re,
                                   const uint64_t *d_ends, uint64_t count, uint32_t flags, uint64_t *d_starts, hipStream_t stream,
                                   char *err, size_t errlen);
void bmx_internal_regex_long_free(void *state);
float bmx_internal_regex_long_ms(const void *state);
constexpr uint64_t BMX_REGEX_STARTS_NO_MATCH = 2; // *bad_out: some end had no match (csrc/bmx_regex_kernel.h, REGEX_BAD_START)
// bmx_regex_groups.hip: the capture groups of every span of a list (a state of its own: status word, the tables' block)
int bmx_internal_regex_groups(void **state, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                              const bmx_regex_groups *gr, const uint64_t *d_starts, const uint64_t *d_ends, uint64_t count,
                              uint64_t *d_groups, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_regex_groups_free(void *state);
float bmx_internal_regex_groups_ms(const void *state);
// ... its mirror image: every start (a state of its own; piece_shift: 0, or log2 of the starts per lane -- libbmx_exp.so's
// knob) and the end of every start of a list (d_limit: NULL, or the last byte each entry may use)
int bmx_internal_regex_begins(void **state, int num_cu, int piece_shift, const void *d_text, uint64_t n, uint64_t tail,
                              uint64_t base_offset, const bmx_regex *re, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches,
                              hipStream_t stream, char *err, size_t errlen);
int bmx_internal_regex_ends(void **state, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                            const uint64_t *d_starts, uint64_t count, const uint64_t *d_limit, uint32_t flags, uint64_t *d_ends,
                            hipStream_t stream, char *err, size_t errlen);
void bmx_internal_regex_begins_free(void *state);
float bmx_internal_regex_begins_ms(const void *state);
// bmx_regex_anchored.hip: the four of them with a condition on the byte before and after a match (left, right: the bytes
// next to the view); a state for the forward pair and one for the begins pair
int bmx_internal_regex_anchored(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                const bmx_regex *re, const bmx_regex_anchors *an, uint32_t left, uint32_t right, uint64_t *d_ends,
                                uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen);
int bmx_internal_regex_anchored_starts(void **state, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                       const bmx_regex_anchors *an, uint32_t left, uint32_t right, const uint64_t *d_ends,
                                       uint64_t count, uint32_t flags, uint64_t *d_starts, hipStream_t stream, char *err, size_t errlen);
int bmx_internal_regex_anchored_begins(void **state, int num_cu, int piece_shift, const void *d_text, uint64_t n, uint64_t tail,
                                       uint64_t base_offset, const bmx_regex *re, const bmx_regex_anchors *an, uint32_t left,
                                       uint32_t right, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches, hipStream_t stream,
                                       char *err, size_t errlen);
int bmx_internal_regex_anchored_ends(void **state, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                     const bmx_regex_anchors *an, uint32_t left, uint32_t right, const uint64_t *d_starts,
                                     uint64_t count, const uint64_t *d_limit, uint32_t flags, uint64_t *d_ends, hipStream_t stream,
                                     char *err, size_t errlen);
void bmx_internal_regex_anchored_free(void *state);
void bmx_internal_regex_anchored_begins_free(void *state);
float bmx_internal_regex_anchored_ms(const void *state);
float bmx_internal_regex_anchored_begins_ms(const void *state);
// bmx_regex_star.hip.  What (libbmx_exp.so) bmx_exp_set_knob sets:
struct bmx_regex_star_knobs {
    int piece_shift = 0;     // 0, or log2 of the ends per lane (4..12; the shared "tile_piece_shift" begins at 6)
    int warm = 0;            // 0, or the bytes of the pair warm-up (a multiple of 16)
    bool force_slow = false; // the exact slow path runs behind the first launch even when nothing is tainted
};
int bmx_internal_regex_star(void **state, int num_cu, const bmx_regex_star_knobs *knobs, const void *d_text, uint64_t n,
                            uint64_t lead, uint64_t base_offset, const bmx_regex *re, uint64_t *d_ends, uint64_t capacity,
                            uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen);
int bmx_internal_regex_star_starts_fix(const void *d_text, uint64_t base_offset, const bmx_regex *re, const uint64_t *d_ends,
                                       uint64_t count, uint64_t *d_starts, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_regex_star_free(void *state);
float bmx_internal_regex_star_ms(const void *state);
void bmx_internal_regex_star_last(const void *state, uint64_t out10[10]); // libbmx_exp.so only
uint32_t bmx_internal_regex_star_piece_shift(uint64_t n, uint64_t resident_lanes); // log2 of the ends per lane
uint32_t bmx_internal_regex_star_warm(uint32_t piece_shift);                       // bytes of the pair warm-up
// ... what its slow path runs between its kernels, also for the begins search: the column offsets by a scan, and the sweep
int bmx_internal_regex_star_offsets(const char *where, void **d_scan, size_t *scan_cap, const uint64_t *d_u, uint64_t n_pieces,
                                    uint64_t *d_off, uint64_t *h_total, hipStream_t stream, char *err, size_t errlen);
int bmx_internal_regex_star_sweep(const char *where, uint64_t n_pieces, const uint64_t *d_e, const uint64_t *d_u, const uint64_t *d_off,
                                  const uint64_t *d_base, const uint64_t *d_cols, uint64_t *d_entry, hipStream_t stream, char *err,
                                  size_t errlen);
// bmx_regex_star_begins.hip: its mirror image, every start (a state and knobs of its own, the piece and warm-up rules
// above), and the end of every start of a list within a window (*bad_out: the status bits, of which only a start outside
// the view is an error there; *clipped_out: the entries whose state outlived the window)
int bmx_internal_regex_star_begins(void **state, int num_cu, const bmx_regex_star_knobs *knobs, const void *d_text, uint64_t n,
                                   uint64_t tail, uint64_t base_offset, const bmx_regex *re, uint64_t *d_starts, uint64_t capacity,
                                   uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen);
int bmx_internal_regex_star_ends(void **state, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                 const uint64_t *d_starts, uint64_t count, const uint64_t *d_limit, uint32_t window, uint32_t flags,
                                 bool early_exit, uint64_t *d_ends, uint64_t *bad_out, uint64_t *clipped_out, hipStream_t stream,
                                 char *err, size_t errlen);
void bmx_internal_regex_star_begins_free(void *state);
float bmx_internal_regex_star_begins_ms(const void *state);
void bmx_internal_regex_star_begins_last(const void *state, uint64_t out10[10]); // libbmx_exp.so only
constexpr uint64_t BMX_REGEX_STAR_ENDS_NO_MATCH = 2; // *bad_out: some start had no match (csrc/bmx_regex_star_begins_kernel.h)
// bmx_ed_batch.hip
int bmx_internal_ed_batch(void **state, bmx_ctx *ctx, const void *d_a, uint64_t a_bytes, const uint64_t *d_a_off, uint64_t a_count,
                          const void *d_b, uint64_t b_bytes, const uint64_t *d_b_off, uint64_t count, uint32_t limit,
                          uint32_t *d_dist, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_ed_batch_free(void *state);
float bmx_internal_ed_batch_ms(const void *state);
int64_t bmx_internal_ed_batch_fallbacks(const void *state);
// bmx_spans.hip
int bmx_internal_spans(void **state, const void *d_text, uint64_t n, uint64_t base_offset, const char *pat, const uint8_t *classes,
                       int32_t m, int32_t k, const uint64_t *d_ends, const uint8_t *d_dist, uint64_t count, uint32_t flags,
                       uint64_t *d_starts, uint64_t *d_sel_ends, uint8_t *d_sel_dist, uint64_t *n_spans, hipStream_t stream,
                       char *err, size_t errlen);
void bmx_internal_spans_free(void *state);
float bmx_internal_spans_ms(const void *state);
// bmx_dict.hip
int bmx_internal_dict_create(const void *owner, int device, const char *const *pats, const int32_t *ms, int32_t K,
                             bmx_dict **out, char *err, size_t errlen);
void bmx_internal_dict_destroy(bmx_dict *d);
const void *bmx_internal_dict_owner(const bmx_dict *d);
int bmx_internal_dict_search(void **state, int num_cu, const bmx_dict *d, const void *d_text, uint64_t n, uint64_t n_own,
                             uint64_t base_offset, uint64_t *d_pos, uint32_t *d_pid, uint64_t capacity,
                             uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_dict_state_free(void *state);
float bmx_internal_dict_ms(const void *state);
int64_t bmx_internal_dict_candidates(const void *state);
// bmx_index.hip
int bmx_internal_index_create(void **state, bmx_ctx *ctx, int device, const void *d_text, uint64_t n, const int32_t *d_sa,
                              hipStream_t stream, bmx_index **out, char *err, size_t errlen);
void bmx_internal_index_destroy(bmx_index *ix);
const void *bmx_internal_index_owner(const bmx_index *ix);
const int32_t *bmx_internal_index_sa(const bmx_index *ix);
float bmx_internal_index_build_ms(const bmx_index *ix);
int bmx_internal_index_count(void **state, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                             uint64_t count, uint32_t *d_lo, uint32_t *d_cnt, int use_dir, hipStream_t stream, char *err,
                             size_t errlen);
int bmx_internal_index_locate(void **state, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                              uint64_t count, uint64_t base_offset, uint64_t *d_out_off, uint64_t *d_pos, uint64_t capacity,
                              uint64_t *n_matches, int use_dir, hipStream_t stream, char *err, size_t errlen);
int bmx_internal_index_match(void **state, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                             uint64_t count, uint32_t *d_len, uint32_t *d_lo, uint32_t *d_cnt, int use_dir, hipStream_t stream,
                             char *err, size_t errlen);
int bmx_internal_index_seeds(void **state, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                             uint64_t count, uint32_t min_len, uint32_t max_occ, uint64_t *d_seed_off, uint32_t *d_qpos,
                             uint32_t *d_len, uint32_t *d_lo, uint32_t *d_cnt, uint64_t capacity, uint64_t *n_seeds, int use_dir,
                             hipStream_t stream, char *err, size_t errlen);
int bmx_internal_index_map(void **state, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                           uint64_t count, uint32_t min_len, uint32_t max_occ, uint32_t k, uint64_t base_offset,
                           uint64_t *d_best_start, uint64_t *d_best_end, uint8_t *d_best_dist, uint64_t *d_cand_off,
                           uint64_t *d_cand_start, uint64_t *d_cand_end, uint8_t *d_cand_dist, uint64_t capacity,
                           uint64_t *n_candidates, int use_dir, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_index_state_free(void *state);
float bmx_internal_index_ms(const void *state);
int64_t bmx_internal_index_map_candidates(const void *state);
int bmx_internal_index_map_phases(const void *state, float out[5]);
// bmx_align.hip (ws_cap: 0, or the workspace one launch may take -- libbmx_exp.so's knob)
int bmx_internal_align(void **state, uint64_t ws_cap, const void *d_text, uint64_t n, uint64_t base_offset, const void *d_pat,
                       uint64_t pat_bytes, const uint64_t *d_pat_off, uint64_t pat_count, const uint32_t *d_pid,
                       const uint64_t *d_start, const uint64_t *d_end, uint64_t count, uint32_t k, uint8_t *d_dist,
                       uint64_t *d_op_off, uint32_t *d_ops, uint64_t capacity, uint64_t *n_ops, hipStream_t stream, char *err,
                       size_t errlen);
void bmx_internal_align_free(void *state);
float bmx_internal_align_ms(const void *state);
int64_t bmx_internal_align_launches(const void *state);
// bmx_lcp.hip
int bmx_internal_lcp(void **state, const uint8_t *d_text, uint32_t n, const int32_t *d_sa, int32_t *d_lcp, hipStream_t stream,
                     char *err, size_t errlen);
int bmx_internal_lcp_stats(void **state, const int32_t *d_lcp, uint32_t n, uint32_t min_len, uint64_t out[4], hipStream_t stream,
                           char *err, size_t errlen);
void bmx_internal_lcp_free(void *state);
float bmx_internal_lcp_ms(const void *state);
int64_t bmx_internal_lcp_long_pairs(const void *state);
// bmx_rows.hip
int bmx_internal_rows_split(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t base_offset, uint8_t delim,
                            uint64_t *d_off, uint64_t capacity, uint64_t *n_rows, uint64_t *longest, hipStream_t stream, char *err,
                            size_t errlen);
int bmx_internal_rows_of(void **state, const uint64_t *d_off, uint64_t rows, const uint64_t *d_starts, const uint64_t *d_ends,
                         uint64_t len, uint64_t count, uint64_t *d_row, hipStream_t stream, char *err, size_t errlen);
int bmx_internal_rows_matching(void **state, const uint64_t *d_row, uint64_t count, uint64_t rows, uint32_t flags,
                               uint64_t *d_rows_out, uint64_t *d_counts_out, uint64_t capacity, uint64_t *n_out, hipStream_t stream,
                               char *err, size_t errlen);
void bmx_internal_rows_free(void *state);
float bmx_internal_rows_ms(const void *state);
void bmx_internal_rows_last(const void *state, uint64_t out3[3]); // libbmx_exp.so only
// bmx_subst.hip (tile_shift: 0, or log2 of the selection's tile -- libbmx_exp.so's knob; the copy: d_off NULL = replace)
int bmx_internal_select(void **state, int tile_shift, const uint64_t *d_starts, const uint64_t *d_ends, uint64_t len, uint64_t count,
                        const uint64_t *d_row, uint32_t flags, uint64_t *d_starts_out, uint64_t *d_ends_out, uint64_t *d_index_out,
                        uint64_t capacity, uint64_t *n_out, hipStream_t stream, char *err, size_t errlen);
int bmx_internal_subst_copy(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_starts,
                            const uint64_t *d_ends, uint64_t len, uint64_t count, const void *repl, uint64_t repl_len, void *d_out,
                            uint64_t capacity, uint64_t *d_off, uint64_t *n_out, hipStream_t stream, char *err, size_t errlen);
// ... the copy with a template (t, lits: bmx_compile_template's; d_off NULL = replace, else the offsets of the column)
int bmx_internal_expand(void **state, int num_cu, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_groups,
                        int32_t n_groups, uint64_t count, const bmx_template *t, const uint8_t *lits, void *d_out, uint64_t capacity,
                        uint64_t *d_off, uint64_t *n_out, hipStream_t stream, char *err, size_t errlen);
void bmx_internal_subst_free(void *state);
float bmx_internal_subst_ms(const void *state);
void bmx_internal_subst_last(const void *state, uint64_t out3[3]); // libbmx_exp.so only

// ---- the context: the device, the switches and one opaque state per feature (made on first use and owned by the
// feature's file; the exact search's eagerly) ----
struct bmx_ctx {
    int device = 0;
    int num_cu = 256;
    // Measurement / test switches.  Only libbmx_exp.so can change them (bmx_exp_set_knob); in the product library they keep
    // these values and nothing reads the environment.
    bmx_scan_knobs scan_knobs;
    bmx_ed_knobs ed_knobs;     // edit distance: the schedule (bmx_set_ed_variant) and the band pipeline's switches
    int sa_flags = 0;          // suffix array: 1 = library rounds only, 2 = a host wait per round, 4 = per-round trace on stderr
    bool index_no_dir = false; // libbmx_exp.so: queries search the whole array, not their directory bucket
    void *scan = nullptr; // exact search: variant choice, counters, buckets, status words, event ring, last launch (bmx_scan.hip)
    void *ed = nullptr; // edit distance: the band pipeline's workspace, last ms, stamps, events (bmx_ed.hip)
    void *sa = nullptr; // suffix array: workspace, pinned round counters, last ms and round counts (bmx_sa.hip)
    void *lcp = nullptr; // LCP array: workspace, status words, statistics partials, events, last ms and long pairs (bmx_lcp.hip)
    void *classes = nullptr; // class-pattern search: the same kind of state, its own (bmx_classes.hip)
    void *hamming = nullptr; // k-mismatch search: the same again (bmx_hamming.hip)
    void *gaps = nullptr; // gapped pattern search: the same again, and the status word of its starts pass (bmx_gaps.hip)
    void *regex = nullptr; // regular-expression search: the same as the gapped search's, its own (bmx_regex.hip)
    void *regex_long = nullptr; // ... for up to 128 positions: the same and the block of its tables (bmx_regex_long.hip)
    void *regex_groups = nullptr; // ... its capture groups pass: status word, the block of its tables, events (bmx_regex_groups.hip)
    void *regex_begins = nullptr; // ... its begins search and ends pass: the same again, their own (bmx_regex.hip)
    int regex_begins_piece_shift = 0; // libbmx_exp.so: 0, or log2 of the starts per lane of the begins search (4..12)
    void *regex_anchored = nullptr; // ... anchored: the same and the gate tables (bmx_regex_anchored.hip)
    void *regex_anchored_begins = nullptr; // ... and its begins search and ends pass (regex_begins_piece_shift applies)
    void *regex_star = nullptr; // ... with unbounded repetition: the same, the taint words and the slow path's workspace (bmx_regex_star.hip)
    bmx_regex_star_knobs regex_star_knobs;
    void *regex_star_begins = nullptr; // ... and its begins search and ends pass: the same again, their own (bmx_regex_star_begins.hip)
    bmx_regex_star_knobs regex_star_begins_knobs;
    bool regex_star_ends_no_early_exit = false; // libbmx_exp.so: the ends pass walks its whole window (to time the early exit)
    void *approx = nullptr; // approximate search: look-back words, ticket, pinned result words, events (bmx_approx.hip)
    void *approx_long = nullptr; // ... for patterns of more than 64 bytes: the same kind of state, its own (bmx_approx_long.hip)
    bool approx_last_long = false; // which of the two the last approximate search on this context used (bmx_last_approx_ms)
    void *ed_batch = nullptr; // batched edit distance: status words, fallback list, events (bmx_ed_batch.hip)
    void *spans = nullptr; // match spans: status words, tile counts of the selection, events (bmx_spans.hip)
    void *dict = nullptr;   // dictionary search: the same for its kernel (bmx_dict.hip)
    void *index = nullptr;  // text index: status words, events, workspace of count / locate (bmx_index.hip)
    void *align = nullptr;  // alignments: status words, events, the launches' workspace (bmx_align.hip)
    int align_ws_kib = 0;   // libbmx_exp.so: > 0: one launch of the alignments takes at most this much workspace (KiB)
    void *rows = nullptr;   // row-wise results: the split's ordered output, status words, events, workspace (bmx_rows.hip)
    void *subst = nullptr;  // selection, replace, extract: status words, events, workspace, the replacement (bmx_subst.hip)
    int select_tile_shift = 0; // libbmx_exp.so: 0, or log2 of the selection's tile (3..8) in place of the production one
};

// ---- argument checks: every argument error, before any HIP call (the CPU suite calls the entries with ctx = NULL) ----

// batched edit distance
inline bool bmx_ed_batch_args_ok(const void *a, uint64_t a_bytes, const uint64_t *a_off, uint64_t a_count, const void *b,
                                 uint64_t b_bytes, const uint64_t *b_off, uint64_t count, const uint32_t *dist)
{
    if (count == 0) return true;
    return (a_count == 1 || a_count == count) && a_off && b_off && dist && (a || a_bytes == 0) && (b || b_bytes == 0);
}
// ... the host entry's offsets: monotone, the last one inside the blob, every string below 2^31 bytes
inline bool bmx_ed_batch_offsets_ok(const uint64_t *off, uint64_t strings, uint64_t bytes)
{
    for (uint64_t i = 0; i < strings; ++i)
        if (off[i + 1] < off[i] || off[i + 1] - off[i] >= (1ull << 31)) return false;
    return off[strings] <= bytes;
}

// approximate search (pat: the string or the classes)
inline bool bmx_approx_args_ok(uint64_t n, uint64_t lead, const void *pat, int32_t m, int32_t k, const void *ends, uint64_t capacity)
{
    return pat && m >= 1 && m <= BMX_MAX_APPROX_PATTERN && k >= 0 && k < m && lead <= n && n < (1ull << 40) &&
           (capacity == 0 || ends);
}

// ... for patterns of up to BMX_MAX_APPROX_LONG_PATTERN bytes (a string)
inline bool bmx_approx_long_args_ok(uint64_t n, uint64_t lead, const void *pat, int32_t m, int32_t k, const void *ends,
                                    uint64_t capacity)
{
    return pat && m >= 1 && m <= BMX_MAX_APPROX_LONG_PATTERN && k >= 0 && k < m && k <= BMX_MAX_APPROX_LONG_K && lead <= n &&
           n < (1ull << 40) && (capacity == 0 || ends);
}

// class-pattern search
inline bool bmx_classes_args_ok(uint64_t n, const uint8_t *classes, int32_t m, const void *starts, uint64_t capacity)
{
    return classes && m >= 1 && m <= BMX_MAX_CLASS_PATTERN && n < (1ull << 40) && (capacity == 0 || starts);
}

// k-mismatch search (pat: the string or the classes): k below m and at most BMX_MAX_HAMMING_K, `must` inside the pattern
inline bool bmx_hamming_args_ok(uint64_t n, const void *pat, int32_t m, int32_t k, uint64_t must, const void *starts, uint64_t capacity)
{
    if (!pat || m < 1 || m > BMX_MAX_HAMMING_PATTERN || k < 0 || k >= m || k > BMX_MAX_HAMMING_K) return false;
    if (m < 64 && (must >> m) != 0) return false;
    return n < (1ull << 40) && (capacity == 0 || starts);
}

// gapped pattern search: the classes, and optional positions that lie inside the pattern and leave one mandatory
inline bool bmx_gaps_pattern_ok(const uint8_t *classes, int32_t m, uint64_t optional)
{
    if (!classes || m < 1 || m > BMX_MAX_GAPS_PATTERN) return false;
    const uint64_t all = m == 64 ? ~0ull : (1ull << m) - 1;
    return (optional & ~all) == 0 && optional != all;
}
inline bool bmx_gaps_args_ok(uint64_t n, uint64_t lead, const uint8_t *classes, int32_t m, uint64_t optional, const void *ends,
                             uint64_t capacity)
{
    return bmx_gaps_pattern_ok(classes, m, optional) && lead <= n && n < (1ull << 40) && (capacity == 0 || ends);
}
// ... and the starts of its matches
inline bool bmx_gaps_starts_args_ok(uint64_t n, const uint8_t *classes, int32_t m, uint64_t optional, const uint64_t *ends,
                                    uint64_t count, uint32_t flags, const uint64_t *starts)
{
    if (!bmx_gaps_pattern_ok(classes, m, optional) || n >= (1ull << 40) || (flags & ~BMX_GAPS_LONGEST)) return false;
    return count == 0 || (ends && starts);
}

// regular-expression search: a valid automaton (bmx_regex_sets.h)
inline bool bmx_regex_ok(const bmx_regex *re) { return re && bmx_regex_sets_ok(re->m, re->first, re->last, re->follow); }
inline bool bmx_regex_args_ok(uint64_t n, uint64_t lead, const bmx_regex *re, const void *ends, uint64_t capacity)
{
    return bmx_regex_ok(re) && lead <= n && n < (1ull << 40) && (capacity == 0 || ends);
}
// ... and the starts of its matches
inline bool bmx_regex_starts_args_ok(uint64_t n, const bmx_regex *re, const uint64_t *ends, uint64_t count, uint32_t flags,
                                     const uint64_t *starts)
{
    if (!bmx_regex_ok(re) || n >= (1ull << 40) || (flags & ~BMX_REGEX_LONGEST)) return false;
    return count == 0 || (ends && starts);
}

// ... and their capture groups: a valid pair, the two lists and the output where there is an entry
inline bool bmx_regex_groups_args_ok(uint64_t n, const bmx_regex *re, const bmx_regex_groups *gr, const uint64_t *starts,
                                     const uint64_t *ends, uint64_t count, const uint64_t *groups)
{
    if (!bmx_regex_groups_valid(re, gr) || n >= (1ull << 40)) return false;
    return count == 0 || (starts && ends && groups);
}
// ... the copy with a template (text and out: host or device; off: the offsets of the column with BMX_EXPAND_EXTRACT)
inline bool bmx_expand_args_ok(const void *text, uint64_t n, const uint64_t *groups, int32_t n_groups, uint64_t count, uint32_t flags,
                               const void *out, uint64_t capacity, const uint64_t *off, const uint64_t *n_out)
{
    if ((n > 0 && !text) || n >= (1ull << 40) || !n_out || (capacity > 0 && !out) || (flags & ~BMX_EXPAND_EXTRACT)) return false;
    if (((flags & BMX_EXPAND_EXTRACT) && !off) || n_groups < 0 || n_groups > BMX_MAX_REGEX_GROUPS) return false;
    if (count >= (1ull << 32) || (count > 0 && !groups)) return false;
    if (n > 0 && capacity > 0) {
        const uintptr_t t = reinterpret_cast<uintptr_t>(text), o = reinterpret_cast<uintptr_t>(out);
        if (t < o + capacity && o < t + n) return false;
    }
    return true;
}

// ... for up to 128 positions: the same rules on struct bmx_regex_long
inline bool bmx_regex_long_args_ok(uint64_t n, uint64_t lead, const bmx_regex_long *re, const void *ends, uint64_t capacity)
{
    return bmx_regex_long_sets_ok(re) && lead <= n && n < (1ull << 40) && (capacity == 0 || ends);
}

inline bool bmx_regex_long_starts_args_ok(uint64_t n, const bmx_regex_long *re, const uint64_t *ends, uint64_t count, uint32_t flags,
                                          const uint64_t *starts)
{
    if (!bmx_regex_long_sets_ok(re) || n >= (1ull << 40) || (flags & ~BMX_REGEX_LONGEST)) return false;
    return count == 0 || (ends && starts);
}

// ... every start: the view runs `tail` bytes past the last owned start
inline bool bmx_regex_begins_args_ok(uint64_t n, uint64_t tail, const bmx_regex *re, const void *starts, uint64_t capacity)
{
    return bmx_regex_ok(re) && tail <= n && n < (1ull << 40) && (capacity == 0 || starts);
}
// ... and the ends of the matches that begin there
inline bool bmx_regex_ends_args_ok(uint64_t n, const bmx_regex *re, const uint64_t *starts, uint64_t count, uint32_t flags,
                                   const uint64_t *ends)
{
    if (!bmx_regex_ok(re) || n >= (1ull << 40) || (flags & ~BMX_REGEX_LONGEST)) return false;
    return count == 0 || (starts && ends);
}

// ... anchored: every struct of classes goes with a valid automaton; the two neighbour bytes are byte values
inline bool bmx_regex_anchors_ok(const bmx_regex_anchors *an, uint32_t left, uint32_t right) { return an && left <= 255 && right <= 255; }

// ... with unbounded repetition: follow[] may hold any bit below m
inline bool bmx_regex_star_ok(const bmx_regex *re) { return re && bmx_regex_star_sets_ok(re->m, re->first, re->last, re->follow); }
inline bool bmx_regex_star_args_ok(uint64_t n, uint64_t lead, const bmx_regex *re, const void *ends, uint64_t capacity)
{
    return bmx_regex_star_ok(re) && lead <= n && n < (1ull << 40) && (capacity == 0 || ends);
}
inline bool bmx_regex_star_starts_args_ok(uint64_t n, const bmx_regex *re, const uint64_t *ends, uint64_t count, uint32_t window,
                                          uint32_t flags, const uint64_t *starts)
{
    if (!bmx_regex_star_ok(re) || n >= (1ull << 40) || (flags & ~BMX_REGEX_LONGEST)) return false;
    if (window < 1 || window > BMX_MAX_REGEX_STAR_WINDOW) return false;
    return count == 0 || (ends && starts);
}

// ... every start of such an automaton, and the ends of the matches that begin there, within a window
inline bool bmx_regex_star_begins_args_ok(uint64_t n, uint64_t tail, const bmx_regex *re, const void *starts, uint64_t capacity)
{
    return bmx_regex_star_ok(re) && tail <= n && n < (1ull << 40) && (capacity == 0 || starts);
}
inline bool bmx_regex_star_ends_args_ok(uint64_t n, const bmx_regex *re, const uint64_t *starts, uint64_t count, uint32_t window,
                                        uint32_t flags, const uint64_t *ends)
{
    if (!bmx_regex_star_ok(re) || n >= (1ull << 40) || (flags & ~BMX_REGEX_LONGEST)) return false;
    if (window < 1 || window > BMX_MAX_REGEX_STAR_WINDOW) return false;
    return count == 0 || (starts && ends);
}

// match spans (pat: the string or the classes)
inline bool bmx_spans_args_ok(uint64_t n, const void *pat, int32_t m, int32_t k, const uint64_t *ends, const uint8_t *dist,
                              uint64_t count, uint32_t flags, const uint64_t *starts, const uint64_t *sel_ends)
{
    if (!pat || m < 1 || m > BMX_MAX_APPROX_PATTERN || k < 0 || k >= m || n >= (1ull << 40) || (flags & ~BMX_SPANS_BEST)) return false;
    if (count == 0) return true;
    return ends && starts && (flags == 0 || (dist && sel_ends));
}

// ... for patterns of up to BMX_MAX_APPROX_LONG_PATTERN bytes (a string)
inline bool bmx_spans_long_args_ok(uint64_t n, const void *pat, int32_t m, int32_t k, const uint64_t *ends, const uint8_t *dist,
                                   uint64_t count, uint32_t flags, const uint64_t *starts, const uint64_t *sel_ends)
{
    if (!pat || m < 1 || m > BMX_MAX_APPROX_LONG_PATTERN || k < 0 || k >= m || k > BMX_MAX_APPROX_LONG_K || n >= (1ull << 40) ||
        (flags & ~BMX_SPANS_BEST))
        return false;
    if (count == 0) return true;
    return ends && starts && (flags == 0 || (dist && sel_ends));
}

// alignments: the column, the lists and the outputs where there is an entry, k, and which pattern an entry takes
inline bool bmx_align_args_ok(const void *text, uint64_t n, const void *pat, const uint64_t *pat_off, uint64_t pat_count,
                              const uint32_t *pid, const uint64_t *start, const uint64_t *end, uint64_t count, int32_t k,
                              const uint64_t *op_off, const uint32_t *ops, uint64_t capacity)
{
    if (k < 0 || k > BMX_ALIGN_MAX_K || n >= (1ull << 40)) return false;
    if (count == 0) return true;
    if (!pid && pat_count != 1 && pat_count != count) return false;
    return text && pat && pat_off && start && end && op_off && (capacity == 0 || ops);
}
// ... the host entry's entries: what the kernel calls a bad entry (csrc/bmx_align_kernel.h)
inline bool bmx_align_entries_ok(uint64_t n, uint64_t base_offset, uint64_t pat_bytes, const uint64_t *pat_off, uint64_t pat_count,
                                 const uint32_t *pid, const uint64_t *start, const uint64_t *end, uint64_t count)
{
    for (uint64_t p = 0; p < pat_count; ++p)
        if (pat_off[p + 1] < pat_off[p] || pat_off[p + 1] > pat_bytes) return false;
    for (uint64_t e = 0; e < count; ++e) {
        const uint64_t s = start[e], j = end[e];
        if (s == BMX_MAP_NO_POS && j == BMX_MAP_NO_POS) continue;
        if (s == BMX_MAP_NO_POS || j == BMX_MAP_NO_POS || s < base_offset || j < s || j - base_offset >= n) return false;
        const uint64_t p = pid ? pid[e] : pat_count == 1 ? 0 : e;
        if (p >= pat_count) return false;
        const uint64_t m = pat_off[p + 1] - pat_off[p];
        if (m == 0 || m > BMX_ALIGN_MAX_PATTERN) return false;
    }
    return true;
}

// row-wise results: the split (text: host or device) ...
inline bool bmx_rows_split_args_ok(const void *text, uint64_t n, const uint64_t *off, uint64_t capacity)
{
    return (n == 0 || text) && n < (1ull << 40) && (capacity == 0 || off);
}
// ... the row of every match: exactly one of {both lists, len == 0}, {starts, len >= 1}, {ends, len >= 1}
inline bool bmx_rows_of_args_ok(const uint64_t *off, const uint64_t *starts, const uint64_t *ends, uint64_t len, uint64_t count,
                                const uint64_t *row)
{
    if (count == 0) return true;
    if (!off || !row || (!starts && !ends)) return false;
    return (starts && ends) ? len == 0 : len >= 1;
}
// ... and the matching rows: no counts of rows that have none
inline bool bmx_rows_matching_args_ok(const uint64_t *row, uint64_t count, uint32_t flags, const uint64_t *rows_out,
                                      const uint64_t *counts_out, uint64_t capacity)
{
    if ((flags & ~BMX_ROWS_INVERT) || ((flags & BMX_ROWS_INVERT) && counts_out)) return false;
    return (count == 0 || row) && (capacity == 0 || rows_out);
}

// selection, replace and extract: a list in one of the three forms of bmx_rows_of_device
inline bool bmx_span_list_ok(const uint64_t *starts, const uint64_t *ends, uint64_t len, uint64_t count)
{
    if (count >= (1ull << 32)) return false;
    if (count == 0) return true;
    if (!starts && !ends) return false;
    return (starts && ends) ? len == 0 : len >= 1;
}
inline bool bmx_select_args_ok(const uint64_t *starts, const uint64_t *ends, uint64_t len, uint64_t count, uint32_t flags,
                               const uint64_t *starts_out, const uint64_t *ends_out, uint64_t capacity, const uint64_t *n_out)
{
    if ((flags & ~BMX_SELECT_MERGE) || !n_out) return false;
    return bmx_span_list_ok(starts, ends, len, count) && (capacity == 0 || (starts_out && ends_out));
}
// ... the copy (text and out: host or device; off: the offsets of an extract, NULL for a replace).  A device output must
// not overlap the text.
inline bool bmx_subst_copy_args_ok(const void *text, uint64_t n, const uint64_t *starts, const uint64_t *ends, uint64_t len,
                                   uint64_t count, const void *repl, uint64_t repl_len, const void *out, uint64_t capacity,
                                   bool extract, const uint64_t *off, const uint64_t *n_out)
{
    if ((n > 0 && !text) || n >= (1ull << 40) || !n_out || (capacity > 0 && !out) || (extract && !off)) return false;
    if (repl_len > BMX_MAX_REPLACEMENT || (repl_len > 0 && !repl)) return false;
    if (!bmx_span_list_ok(starts, ends, len, count)) return false;
    if (n > 0 && capacity > 0) {
        const uintptr_t t = reinterpret_cast<uintptr_t>(text), o = reinterpret_cast<uintptr_t>(out);
        if (t < o + capacity && o < t + n) return false;
    }
    return true;
}

// a dictionary's patterns: BMX_ERR_ARG for NULL arrays or a count or length out of range, BMX_ERR_DOMAIN for a byte >= 0x80
// (as bmx_build_tables)
inline int bmx_dict_patterns_ok(const char *const *pats, const int32_t *ms, int32_t K)
{
    if (!pats || !ms || K < 1 || K > BMX_MAX_DICT) return BMX_ERR_ARG;
    for (int32_t i = 0; i < K; ++i)
        if (!pats[i] || ms[i] < 1 || ms[i] > BMX_MAX_PATTERN) return BMX_ERR_ARG;
    for (int32_t i = 0; i < K; ++i)
        for (int32_t j = 0; j < ms[i]; ++j)
            if ((uint8_t)pats[i][j] >= 0x80) return BMX_ERR_DOMAIN;
    return BMX_OK;
}

// the LCP array: the text (host or device), its length, the output
inline bool bmx_lcp_args_ok(const void *text, uint64_t n, const void *lcp) { return text && lcp && n >= 1 && n < (1ull << 31); }

// a query call of the text index
inline bool bmx_index_query_args_ok(const void *pat, const uint64_t *pat_off, uint64_t count, const void *out)
{
    return count == 0 || (pat && pat_off && out);
}
// ... of its seeds: the offsets out, the four lists where there is room for any, and a smallest length
inline bool bmx_index_seeds_args_ok(const void *pat, const uint64_t *pat_off, uint64_t count, uint32_t min_len, const void *seed_off,
                                    const void *qpos, const void *len, const void *lo, const void *cnt, uint64_t capacity)
{
    if (min_len == 0) return false;
    return count == 0 || (pat && pat_off && seed_off && (capacity == 0 || (qpos && len && lo && cnt)));
}
// ... of its read mapping: the three per-query outputs, the three lists where there is room for any, min_len and max_occ
// of at least 1 and at most BMX_MAP_MAX_K edits
inline bool bmx_index_map_args_ok(const void *pat, const uint64_t *pat_off, uint64_t count, uint32_t min_len, uint32_t max_occ,
                                  int32_t k, const void *best_start, const void *best_end, const void *best_dist,
                                  const void *cand_start, const void *cand_end, const void *cand_dist, uint64_t capacity)
{
    if (min_len == 0 || max_occ == 0 || k < 0 || k > BMX_MAP_MAX_K) return false;
    return count == 0 || (pat && pat_off && best_start && best_end && best_dist &&
                          (capacity == 0 || (cand_start && cand_end && cand_dist)));
}
// ... the host entry's queries: BMX_ERR_ARG for offsets that decrease or end past the blob and for a length of 0 or above
// BMX_MAX_PATTERN, BMX_ERR_DOMAIN for a byte >= 0x80
inline int bmx_index_queries_ok(const void *pat, uint64_t pat_bytes, const uint64_t *off, uint64_t count)
{
    for (uint64_t i = 0; i < count; ++i)
        if (off[i + 1] < off[i] || off[i + 1] > pat_bytes || off[i + 1] == off[i] || off[i + 1] - off[i] > BMX_MAX_PATTERN)
            return BMX_ERR_ARG;
    const uint8_t *p = static_cast<const uint8_t *>(pat);
    for (uint64_t j = off[0]; j < off[count]; ++j)
        if (p[j] >= 0x80) return BMX_ERR_DOMAIN;
    return BMX_OK;
}
