/*
 * bmx.h -- C ABI of libbmx.so: Boyer-Moore exact string matching on AMD
 * Instinct MI355X (gfx950).  Plain pointers and sizes only; no C++ or torch
 * types cross this boundary.
 *
 * What each entry point replaces in the reference (paths relative to the
 * reference checkout; the reference has no function API, its contract is the
 * OpenCL kernel signature plus the host call sequence around it):
 *
 *   bmx_build_tables      BoyreMoore/BoyreMoore/BoyreMoore.cpp:150-190 (+ helpers :13-60)
 *   bmx_ctx_create        BoyreMoore.cpp:217-231   clGetPlatformIDs .. clCreateCommandQueue
 *   bmx_ctx_destroy       BoyreMoore.cpp:299-312   clRelease*
 *   bmx_search            BoyreMoore.cpp:233-286   6x clCreateBuffer, 5x clEnqueueWriteBuffer,
 *                                                  7x clSetKernelArg, clEnqueueNDRangeKernel,
 *                                                  clEnqueueReadBuffer -- as ONE call that returns
 *                                                  the match positions the kernel only printf()s
 *                                                  (BoyreMoore/x64/Debug/kernel1.cl:24)
 *   bmx_search_multi      the same, with the text cut over several GPUs (stands where the
 *                         reference cuts it over two work-items, BoyreMoore.cpp:94-141, :273)
 *   bmx_multi_*           the same host shape kept across searches: devices, communicators and the
 *                         text stay (the reference sets all of it up per iteration, :217-256)
 *   bmx_search_ranges     kernel1.cl:1 `search(A,B,se,ans,gstable,bstable,sublength)` with the
 *                         launch of BoyreMoore.cpp:264-286: same seven arguments, same per-range
 *                         counts in ans[]
 *   bmx_edit_distance     EditDistance-1/EditDistance-1/EditDistance-1.cpp:278-345 + kernal.cl:5-56 (second program)
 *   bmx_edit_distance_batch  EditDistance-1.cpp:278-345 looped by the caller: a column of string pairs in one call
 *   bmx_suffix_array      SuffixArrays/SuffixArrays/SuffixArrays.cpp:101-154, :417-470 + kernel.cl (third program)
 *   bmx_search_device     the same scan on a text already resident in HBM (the reference re-uploads
 *                         per iteration, BoyreMoore.cpp:246; its timer also starts after the upload, :258)
 *   bmx_search_approx     no counterpart: matches within k edits, the recurrence of kernal.cl:5-56 in Myers'
 *                         bit-parallel form with kernel1.cl:24's one report per hit (section below)
 *   bmx_search_classes    no counterpart in the reference: a pattern position is a set of byte values (wildcards,
 *                         sets, case folding, IUPAC codes), matched by Shift-And (section below)
 *   bmx_index_*           no counterpart: pattern count and locate by binary search over the array bmx_suffix_array
 *                         builds, in the order it builds it; the longest match at every query position and the
 *                         seeds among them; reads mapped by extending the seeds to alignments within k edits
 *                         (section below)
 *
 * Semantics (bit-exact with the reference kernel run as one work-item over
 * [0, n-1]): match_positions receives, in ascending order, every
 * start offset p with text[p .. p+m) == pattern, overlapping occurrences
 * included (after a hit the reference advances by one, kernel1.cl:24).
 *
 * Domain: the reference is defined for 7-bit ASCII, 1 <= m <= 99, n < 2^31.
 * libbmx accepts any byte values, 1 <= m <= BMX_MAX_PATTERN and 64-bit n; bytes
 * >= 0x80 in the TEXT get the full shift m (they cannot occur in an ASCII
 * pattern).  Patterns with bytes >= 0x80 are rejected by bmx_build_tables
 * (BMX_ERR_DOMAIN) exactly where the reference would index bad[] out of range.
 */
#ifndef BMX_H
#define BMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMX_MAX_PATTERN 512
#define BMX_BAD_TABLE_SIZE 128 /* int badSymTab[128], BoyreMoore.cpp:151 */

/* return codes */
#define BMX_OK 0
#define BMX_ERR_ARG (-1)      /* NULL pointer, m < 1, m > BMX_MAX_PATTERN, bad range          */
#define BMX_ERR_DOMAIN (-2)   /* pattern byte >= 0x80                                          */
#define BMX_ERR_TABLE (-3)    /* reserved (shift tables cannot stall the scan: shifts are clamped
                                 to >= 1 exactly as kernel1.cl:28 clamps d1)                   */
#define BMX_ERR_CAPACITY (-4) /* more matches than capacity: `capacity` of them are returned
                                 (which ones is unspecified), ascending; *n_matches holds the
                                 TRUE total so the caller can retry with room for all        */
#define BMX_ERR_HIP (-5)      /* a HIP runtime call failed; see bmx_last_error()               */
#define BMX_ERR_NO_DEVICE (-6)

typedef struct bmx_ctx bmx_ctx; /* one GPU: stream, device workspace, tables */

/* ---- host-side table builder (pure C++, no GPU needed) ------------------- */

/* bad[128]: m for every symbol, then m-1-i for pat[i], i = 0..m-2 (last write wins).
 * good[m]: strong good-suffix shift indexed by the number of matched characters
 * k = 1..m-1; good[0] is unused by the scan and set to 1. */
int bmx_build_tables(const char *pat, int32_t m, int32_t bad[BMX_BAD_TABLE_SIZE], int32_t *good);

/* ---- context -------------------------------------------------------------- */

int bmx_device_count(void);
int bmx_ctx_create(int device, bmx_ctx **out);
void bmx_ctx_destroy(bmx_ctx *ctx);
const char *bmx_last_error(void);
const char *bmx_version(void);

/* ---- the (text, pattern, match_positions) entry point --------------------- */

/* Host buffers in, host buffers out.  Uploads the text, scans, sorts, downloads.
 * ctx may be NULL (a context on device 0 is created and destroyed inside). */
int bmx_search(bmx_ctx *ctx, const char *text, uint64_t n, const char *pat, int32_t m,
               uint64_t *match_positions, uint64_t capacity, uint64_t *n_matches);

/* One process driving several GPUs: the text is cut into n_devices contiguous
 * shards (boundaries on multiples of 16 B, each shard followed by its (m-1)-byte
 * halo; a hit belongs to the shard holding its first byte), uploaded, searched by
 * bmx_multi_search below and the global ascending list -- identical to
 * bmx_search's -- is returned.  devices == NULL means 0 .. n_devices-1; a device
 * may be listed more than once (its shards then share it and the exchange is
 * staged through host memory).  The device set of the previous call -- contexts,
 * streams, the RCCL communicators -- is kept inside the library; the text is
 * uploaded per call (host buffers in, host buffers out: PCIe-bound by contract).
 * Replaces the reference's 2-way split of the text at spaces over two work-items
 * (BoyreMoore.cpp:94-141 + global size 2 at :273), which loses the hits that
 * straddle the cut. */
int bmx_search_multi(const char *text, uint64_t n, const char *pat, int32_t m,
                     const int32_t *devices, int32_t n_devices, uint64_t *match_positions,
                     uint64_t capacity, uint64_t *n_matches);

/* ---- one host process, several GPUs, text RESIDENT, one RCCL exchange per search ------- */

/* The reference drives all of its work-items from one C++ main (BoyreMoore.cpp:213-312) and sets
 * everything up again for every iteration (:217-256).  bmx_multi is that host shape over D devices
 * with everything kept: per device a context, a stream and the exchange buffers, and ONE RCCL
 * communicator clique over the listed devices (ncclCommInitAll; librccl is bound at run time).
 * The text is cut like bmx_search_multi cuts it and stays in HBM; every search is, per device on its
 * own stream, scan + ordering into a fixed slot [count | 8192 offsets], then ONE ncclAllGather of
 * the slots inside ncclGroupStart/End (the all-gatherv of match offsets: RCCL has no v-variant),
 * then a merge kernel that leaves the global ascending list on every device; the host polls device
 * 0's pinned totals and downloads that list.  A result with more than 8192 matches on some device
 * is produced exactly (second search into buffers of the counted size, lists concatenated through
 * the host).  A clique cannot list a device twice: such a set (tests on a 1-GPU box) stages the
 * slots through host memory instead, everything else being the same code.
 * The one-process-per-GPU form of the same exchange is shard.py / bench.py. */
typedef struct bmx_multi bmx_multi;
int bmx_multi_create(const int32_t *devices, int32_t n_devices, bmx_multi **out);
void bmx_multi_destroy(bmx_multi *mg);
int bmx_multi_device_count(const bmx_multi *mg);
int bmx_multi_uses_rccl(const bmx_multi *mg); /* 1: a real clique; 0: slots staged through host memory */
/* Make text[0..n) resident, cut over the devices; every shard carries a halo of m_max - 1 bytes, so patterns
 * of up to m_max bytes can be searched.  Replaces a text made resident before. */
int bmx_multi_text_upload(bmx_multi *mg, const char *text, uint64_t n, int32_t m_max);
/* The same with the synthetic corpus of bmx_gen_text_device generated in place, shard by shard, from the
 * global byte index; bmx_multi_plant copies `pat` over the given GLOBAL offsets (as bmx_plant_device). */
int bmx_multi_gen_text(bmx_multi *mg, uint64_t n, uint64_t seed, int kind, int32_t m_max);
int bmx_multi_plant(bmx_multi *mg, const char *pat, int32_t m, const uint64_t *offsets, uint64_t count);
/* Shard i: out = {first byte, resident bytes, window starts owned}; *d_text_out its device pointer. */
int bmx_multi_shard(const bmx_multi *mg, int32_t i, uint64_t out[3], void **d_text_out);
/* (pattern) -> match_positions over the resident text: host array of `capacity` offsets, ascending,
 * *n_matches the true total (BMX_ERR_CAPACITY if larger). */
int bmx_multi_search(bmx_multi *mg, const char *pat, int32_t m, uint64_t *match_positions, uint64_t capacity,
                     uint64_t *n_matches);
/* Of the most recent bmx_multi_search: the slowest device's scan-kernel time (ms, HIP events), and how the
 * lists were exchanged: 1 = RCCL all-gather of slots, 2 = slots staged through host memory, 3 = exact path. */
float bmx_multi_last_scan_ms(bmx_multi *mg);
int bmx_multi_last_exchange(const bmx_multi *mg);

/* Reference kernel contract: P inclusive ranges se[2P] (int, as the reference),
 * ans[P] = hits whose whole window lies inside the range.  Tables are the
 * caller's (as the reference passes its own); NULL tables are built inside. */
int bmx_search_ranges(bmx_ctx *ctx, const char *text, uint64_t n, const char *pat,
                      const int32_t *se, int32_t P, int32_t *ans, const int32_t *good,
                      const int32_t *bad, int32_t m);

/* ---- device-resident text -------------------------------------------------- */

/* d_text: device pointer to n text bytes (any alignment).  d_match_positions:
 * device buffer of `capacity` uint64.  Every reported offset is
 * base_offset + (index into d_text): a shard of a larger corpus passes its
 * global start.  Only windows that START in [0, n_own) are reported, while
 * bytes up to n may be read: a shard passes n = n_own + (m-1) halo bytes
 * (n_own == n - m + 1 or more means "all of it").
 * `stream` is a hipStream_t used as is (NULL = the null stream).  On return the
 * offsets are sorted ascending in d_match_positions and *n_matches is valid.
 * capacity 0 counts only; like any capacity below the total it returns
 * BMX_ERR_CAPACITY when there are matches.
 * The host waits by polling a pinned status word that the ordering kernel writes
 * after the list is complete (system-scope release), not by synchronising the
 * stream: work the caller enqueues on `stream` afterwards is ordered as usual. */
int bmx_search_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own,
                      uint64_t base_offset, const char *pat, int32_t m, const int32_t *good,
                      const int32_t *bad, uint64_t *d_match_positions, uint64_t capacity,
                      uint64_t *n_matches, void *stream);

/* Same, split in two so a caller can time / overlap / graph-capture the device
 * work: _enqueue launches scan + ordering on `stream` and returns without
 * synchronising; _finish synchronises, reads the count and orders the rare
 * large result (> BMX_SMALL_SORT matches) with a radix sort.
 * Which walker runs depends on the alphabet of the TEXT: the ordering kernel of every search samples 4 x 256 bytes of
 * the text it has just scanned and _finish remembers the number of distinct byte values per (d_text, n) pair (the 16
 * most recent).  The FIRST search on a text therefore goes by the pattern's own symbols and later ones by the text's:
 * _enqueue never waits for the device.  The match list does not depend on any of it. */
/* Repeated searches through several contexts on ONE stream (search i of context A, search i + 1 of context B, ...): with on != 0
 * a context's ordering kernel runs on a stream of the context's own behind its scan's stop event, so that `stream` holds nothing
 * but scans and the next context's scan starts right behind this one (it used to start behind this one's ordering kernel: ~13 us
 * per search on config 2); one CU is left out of the scan's grid for the ordering kernels (the scan is HBM-bound).  _finish is
 * where the list is valid, as before; work enqueued on `stream` after _enqueue is ordered behind the SCAN only; a second _enqueue
 * on the same context without _finish waits for the first one's ordering kernel.  Off (the state of a new context): scan and
 * ordering on `stream`.  Inside a graph capture the ordering stays on `stream` either way. */
int bmx_set_order_overlap(bmx_ctx *ctx, int on);
int bmx_search_device_enqueue(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own,
                              uint64_t base_offset, const char *pat, int32_t m,
                              const int32_t *good, const int32_t *bad,
                              uint64_t *d_match_positions, uint64_t capacity, void *stream);
int bmx_search_device_finish(bmx_ctx *ctx, uint64_t *d_match_positions, uint64_t capacity,
                             uint64_t *n_matches, void *stream);

/* 1 if the most recent bmx_search_device_finish on ctx had to SORT the list (dense or clustered
 * matches: the ordering kernel that runs right behind the scan could not do it from its position
 * buckets).  Whoever consumed d_match_positions on the stream BEFORE _finish -- the multi-GPU
 * exchange below does -- has then seen the unordered list and must take it again. */
int bmx_last_search_sorted(bmx_ctx *ctx);

/* Make `stream` wait until the SCAN kernel of the most recent enqueue on ctx has finished (not its
 * ordering kernel, not whatever the caller put behind it): a second context can then start its own
 * scan on `stream` back to back with this one while this context's ordering and exchange still run
 * on their own stream.  bench.py keeps two searches in flight this way. */
int bmx_stream_wait_last_scan(bmx_ctx *ctx, void *stream);

/* ---- multi-GPU exchange helpers (the collective itself is RCCL, outside) ------ */

/* Copy the match count of the most recent enqueue on ctx to d_dst[0], on-stream
 * (no host round trip): lets a rank publish [count | offsets...] as one fixed-size
 * slot of an all-gather.  If the list is not ordered yet at that point (dense or
 * clustered matches: _finish will sort it) the published count has bit 62 set, i.e.
 * it is larger than any slot, and every rank falls back to the exact exchange.
 * With bmx_set_order_overlap on, `stream` is first made to wait for the context's ordering kernel (the count and the list
 * are that kernel's): the copy and whatever the caller enqueues on `stream` behind it see both. */
int bmx_count_to_device(bmx_ctx *ctx, uint64_t *d_dst, void *stream);

/* After an all-gather of `world` slots of `slot_stride` uint64 each, laid out
 * [count, offset_0, offset_1, ...]: write the rank-order concatenation of the
 * valid offsets to d_merged (ascending globally, because shards are contiguous and
 * each list is ascending), the total to d_total[0] and the largest per-rank count
 * as published to d_total[1].  Counts larger than slot_stride-1 are clamped: a
 * caller that sees d_total[1] > slot_stride-1 falls back to an exact exchange.
 * d_total has THREE words; `seq` is stored to d_total[2] last with a system-scope
 * release, so d_total may be pinned host memory that the host polls for `seq`
 * instead of synchronising the stream. */
int bmx_merge_gathered_device(bmx_ctx *ctx, const uint64_t *d_gathered, int32_t world,
                              uint64_t slot_stride, uint64_t *d_merged, uint64_t merged_capacity,
                              uint64_t *d_total, uint64_t seq, void *stream);

/* Text upload kept apart from the scan (repeated queries on a resident text). */
int bmx_text_upload(bmx_ctx *ctx, const char *text, uint64_t n, void **d_text_out);
int bmx_device_free(bmx_ctx *ctx, void *d_ptr);
int bmx_device_alloc(bmx_ctx *ctx, uint64_t bytes, void **d_ptr_out);

/* Several patterns in ONE pass over a text resident in HBM (SURVEY.md s8 f3 in full: the reference re-uploads
 * the text and re-JITs its kernel for every query, BoyreMoore.cpp:213-256; here the text is fetched once per
 * tile and walked once per pattern, each with its own shift tables -- BoyreMoore.cpp:150-190 -- in LDS; every
 * pattern is walked the way a single search of it would be: the quad-SAD skip loop on texts over large alphabets,
 * the 8-gram form of the bad-symbol rule for nine and more characters over at most eight distinct symbols,
 * byte-wise otherwise).  The call does not synchronise the stream: it ends with the wait for the search's pinned
 * status word, like bmx_search_device.
 * K = 1..BMX_MAX_MULTI patterns of ms[k] bytes.  On return d_match_positions holds pattern 0's matches in
 * ascending order, then pattern 1's, ...: pattern k's are the n_matches[k] entries from index first[k]
 * (n_matches and first: host arrays of K entries).  d_text, n, n_own, base_offset as in bmx_search_device.
 * The match lists are exactly those of K calls of bmx_search_device; results too dense or too clustered for the
 * one-pass bookkeeping are produced by exactly that, pattern by pattern (same answer, no speed-up).
 * More matches in all than `capacity`: BMX_ERR_CAPACITY, n_matches[] still the true counts. */
#define BMX_MAX_MULTI 8
int bmx_search_device_multi(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                            const char *const *pats, const int32_t *ms, int32_t K, uint64_t *d_match_positions,
                            uint64_t capacity, uint64_t *n_matches, uint64_t *first, void *stream);

/* ---- measurement ----------------------------------------------------------- */

/* Duration of the most recent scan kernel launched through ctx, from HIP events
 * recorded on the launch stream around that kernel alone (ms); < 0 if none. */
float bmx_last_scan_ms(bmx_ctx *ctx);
/* Durations (ms) of the most recent scan kernels, newest first, from the context's
 * ring of 64 event pairs: lets a benchmark time K searches without synchronising
 * on an event inside its timed region.  Returns the number written (<= max_n). */
int bmx_scan_ms_history(bmx_ctx *ctx, float *ms_out, int32_t max_n);
/* Scan-kernel launch geometry for pattern length m (of the explicitly chosen variant, else
 * of the variant the most recent search picked): out[0]=grid (workgroups),
 * out[1]=threads per workgroup, out[2]=window starts per synchronisation unit
 * (workgroup tile or wave piece), out[3]=LDS bytes per workgroup, out[4]=window
 * starts per lane, out[5]=kernel kind (0 workgroup tiles, 1 wave streams, 2 three-buffer ring). */
int bmx_scan_geometry(bmx_ctx *ctx, int32_t m, uint64_t out[6]);
/* Diagnostic kernel builds only (variant 15): per-wave s_memtime sums of the last
 * launch, 8 words per wave {issue, walk, dma_wait, barrier_wait, tiles, 0, 0, 0}.
 * Returns the number of words copied. */
int bmx_scan_stamps(bmx_ctx *ctx, uint64_t *out, uint64_t max_words);
/* Kernel choice: -1 = automatic (the state of a new context: by pattern length and alphabet),
 * >= 0 = that slot of the kernel table.  libbmx.so contains only kernels whose match lists are
 * valid and parity-tested; every other slot (schedules that lost, timing-only builds) exists in
 * libbmx_exp.so alone (same sources, -DBMX_EXPERIMENTS, used by tools/) and is refused here
 * with BMX_ERR_ARG.  bmx_variant_count() = number of slots (built or not). */
int bmx_set_variant(bmx_ctx *ctx, int variant, int blocks_per_cu);
int bmx_variant_count(void);
/* The slot of the kernel table that the most recent search on ctx ran (what the automatic choice picked). */
int bmx_last_variant(bmx_ctx *ctx);

/* ---- edit distance: the reference's second algorithm ------------ */

/* Levenshtein distance between a[0..la) and b[0..lb): replaces the host loop of
 * EditDistance-1/EditDistance-1/EditDistance-1.cpp:278-345 (one launch of kernal.cl:5-56
 * per anti-diagonal over a full (la+1) x (lb+1) table) and its CPU twin
 * sequential.c:18-46 (editDistDP).  Only the distance is returned -- the value the
 * reference prints (EditDistance-1.cpp:369); the table is never materialised.
 * Any lengths < 2^31 (the reference is only correct for equal lengths). */
int bmx_edit_distance(bmx_ctx *ctx, const char *a, uint64_t la, const char *b, uint64_t lb,
                      uint64_t *distance);
int bmx_edit_distance_device(bmx_ctx *ctx, const void *d_a, uint64_t la, const void *d_b, uint64_t lb,
                             uint64_t *distance, void *stream);
/* Device time (ms, HIP events around the kernels) of the last call; -1 if it ran none. */
float bmx_last_edit_distance_ms(bmx_ctx *ctx);
/* Schedule, for experiments: 0 = the library's choice (one launch: a pipeline of bit-parallel
 * column bands of 2,048 columns from both corners of the table, a band = a workgroup of four waves,
 * csrc/bmx_ed_bits3_kernel.h = schedule 13); 1..7 = value bands of 64 C columns and their tile
 * shapes; 8..10 = the first bit-parallel band, 1 / 2 / 4 rows per step; 11, 12 = one wave per
 * band with everything but the recurrence out of the step; +32 = one launch per pair of tile
 * diagonals from both corners; +16 = one launch per tile diagonal from the top-left corner only.
 * Every schedule returns the same distance.  The slot numbers are stable, and bmx_set_variant's rule
 * holds: libbmx.so builds 0 and 13 (the same schedule) with their +16 / +32 tiles and refuses
 * every other value with BMX_ERR_ARG; the schedules that lost exist in libbmx_exp.so alone. */
int bmx_set_ed_variant(bmx_ctx *ctx, int variant);

/* ---- batched edit distance: many string pairs in one call ------------------------------------ */

/* A column of pairs instead of one pair per call: a fuzzy join of two string columns, a query word against a word list,
 * reads against candidate loci, the hits of bmx_search_approx or bmx_dict_search post-filtered.  The reference sets
 * everything up again for each run (EditDistance-1/EditDistance-1/EditDistance-1.cpp:278-345); here one launch takes
 * every pair, one pair per lane, with Myers' bit-parallel recurrence in its global form (csrc/bmx_ed_batch_kernel.h).
 *
 * Layout: two string columns in the Arrow layout.  Each side is a byte blob plus count + 1 non-decreasing uint64
 * offsets; string i of side b is d_b[d_b_off[i] .. d_b_off[i+1]), side a the same.  a_count is count (pairwise: a[i]
 * against b[i]) or 1 (the single query a[0] against every b[i]; d_a_off then has two entries).  Any byte values, any
 * alignment, empty strings allowed (the distance is then the other string's length; the blob of an all-empty side may be
 * NULL with 0 bytes); every string has fewer than 2^31 bytes, the blobs are 64-bit sized.
 * Result: d_dist[i] = the unit-cost Levenshtein distance of pair i, the value bmx_edit_distance returns.  With limit !=
 * BMX_ED_NO_LIMIT it is min(distance, limit + 1) ("within limit or not"), and a pair whose lengths differ by more than
 * limit is answered without touching its bytes.
 * Which path a pair takes: a pair whose SHORTER string has at most BMX_ED_BATCH_WORD bytes and whose longer one has at
 * most BMX_ED_BATCH_LONG runs in the batch kernel, and so does every pair of a one-against-many call whose query has 1 ..
 * BMX_ED_BATCH_WORD bytes, whatever the candidate's length.  Every other pair is listed by the kernel and answered by
 * bmx_edit_distance_device, pair by pair on the same stream: the same answer with no speed-up (one launch and one host
 * wait per such pair).  bmx_last_ed_batch_fallbacks says how many there were.
 * Such a pair is a bmx_edit_distance_device call on ctx like any other: after a batch call that had some,
 * bmx_last_edit_distance_ms reports the last of them.  A batch call without any leaves that value alone.
 * Errors: NULL pointers where count > 0 and a_count not in {1, count} return BMX_ERR_ARG before any HIP call, with ctx =
 * NULL too; count == 0 returns BMX_OK and launches nothing.  The host entry checks the offsets on the host (monotone, the
 * last one at most the blob size, strings below 2^31 bytes), also before any HIP call.  The device entry checks them in
 * the kernel: a lane that finds off[i+1] < off[i], an end past a_bytes / b_bytes or a length of 2^31 or more reads no
 * string byte and raises a status word; the call then returns BMX_ERR_ARG and d_dist is unspecified.
 * All device work goes on `stream` (NULL = the null stream); the call returns after synchronising that stream. */
#define BMX_ED_BATCH_WORD 64            /* a pair whose SHORTER string has at most this many bytes runs in the batch kernel */
#define BMX_ED_BATCH_LONG 65536         /* ... unless its longer string has more bytes than this (one lane walks it) */
#define BMX_ED_NO_LIMIT 0xFFFFFFFFu
int bmx_edit_distance_batch_device(bmx_ctx *ctx, const void *d_a, uint64_t a_bytes, const uint64_t *d_a_off, uint64_t a_count,
                                   const void *d_b, uint64_t b_bytes, const uint64_t *d_b_off, uint64_t count, uint32_t limit,
                                   uint32_t *d_dist, void *stream);
/* Host buffers in, host buffers out (upload, bmx_edit_distance_batch_device on the null stream, download).  ctx may be
 * NULL (a context on device 0 is created and destroyed inside). */
int bmx_edit_distance_batch(bmx_ctx *ctx /* NULL: device 0 */, const void *a, uint64_t a_bytes, const uint64_t *a_off,
                            uint64_t a_count, const void *b, uint64_t b_bytes, const uint64_t *b_off, uint64_t count,
                            uint32_t limit, uint32_t *dist);
/* Device time (ms, HIP events around the batch kernel) of the last batch call on ctx; < 0 if none. */
float bmx_last_ed_batch_ms(bmx_ctx *ctx);
/* Pairs of the last batch call on ctx that took the pair-by-pair path; < 0 if none. */
int64_t bmx_last_ed_batch_fallbacks(bmx_ctx *ctx);

/* ---- approximate search: matches within k edits (Sellers' k-differences problem) ---------- */

/* The question that joins the scan and the edit distance above: where does pat occur in the text with at most k
 * substitutions, insertions or deletions?  The reference has no such program; its closest relatives are the
 * edit-distance recurrence of EditDistance-1/EditDistance-1/kernal.cl:5-56 (here Myers' bit-parallel form of it, one
 * 32- or 64-bit word per lane) and the one report per hit of BoyreMoore/x64/Debug/kernel1.cl:24.  A caller that
 * would otherwise run bmx_edit_distance over every substring of the text, or an agrep-style filter on the host, calls
 * this instead.
 *
 * Semantics: for the view d_text[0..n) and pat[0..m), every END index j with min over s of ED(pat, text[s..j]) <= k
 * (Levenshtein distance, unit costs; 0 <= s <= j + 1), ascending, each with that minimum (0..k) in d_dist.  Every
 * qualifying j is reported, so one match with k errors usually shows as a short run of adjacent ends.  With k = 0 the
 * ends are exactly bmx_search_device's starts + m - 1.  Any byte values; 1 <= m <= BMX_MAX_APPROX_PATTERN,
 * 0 <= k < m, n < 2^40, any alignment of d_text.
 * Shards: only ends j in [lead, n) are reported, each as base_offset + j; alignments may start anywhere in the view,
 * before lead included.  An alignment of cost <= k spans at most m + k bytes, so a shard passes a view that begins
 * m + k - 1 bytes (clipped at 0) before its first end, with lead = that amount: the shards' lists then concatenate to
 * the whole text's list.
 * Capacity: d_ends (and d_dist, which may be NULL) have room for `capacity` entries; the stored entries are the LOWEST
 * `capacity` ends, ascending; *n_matches is the true total, and a total above capacity returns BMX_ERR_CAPACITY
 * (capacity 0 counts only).  Argument errors (m or k out of range, lead > n, NULL pointers where a capacity needs
 * them) return BMX_ERR_ARG before any HIP call.  A workgroup that waits longer than its bound (~1 s) for its
 * predecessors' counts makes the call return BMX_ERR_HIP: a list is never returned partly ordered.
 * One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising that stream. */
#define BMX_MAX_APPROX_PATTERN 64
int bmx_search_approx_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                             const char *pat, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist /* may be NULL */,
                             uint64_t capacity, uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out (upload, bmx_search_approx_device, download).  ctx may be NULL (a context on
 * device 0 is created and destroyed inside); ends / dist as above (dist may be NULL). */
int bmx_search_approx(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const char *pat, int32_t m,
                      int32_t k, uint64_t *ends, uint8_t *dist, uint64_t capacity, uint64_t *n_matches);
/* Device time (ms, HIP events around the approximate-search kernel) of the last call on ctx, whichever of the entries of
 * this section or of bmx_search_approx_classes* made it; < 0 if none. */
float bmx_last_approx_ms(bmx_ctx *ctx);

/* Patterns of up to 512 bytes: a sequencing read or a long motif, placed without an index.  The semantics are word for
 * word those of bmx_search_approx_device -- every end j in [lead, n) with min over s of ED(pat, text[s..j]) <= k,
 * ascending, that minimum in d_dist; the lead / base_offset contract with a view that begins m + k - 1 bytes early; the
 * lowest `capacity` ends stored, the true total returned, BMX_ERR_CAPACITY above it; any byte values, any alignment of
 * d_text, n < 2^40.  Domain: 1 <= m <= BMX_MAX_APPROX_LONG_PATTERN, 0 <= k < m and k <= BMX_MAX_APPROX_LONG_K (a
 * distance stays one byte).  m <= BMX_MAX_APPROX_PATTERN is handed to bmx_search_approx_device and returns its lists;
 * above it a lane carries Myers' column in ceil(m / 64) 64-bit words, run by a kernel of 2, 4 or 8 words
 * (csrc/bmx_approx_long_kernel.h), so a call costs about that many times a one-word call.
 * Argument errors return BMX_ERR_ARG before any HIP call.  One kernel launch on `stream`; the call returns after
 * synchronising that stream; bmx_last_approx_ms times it. */
#define BMX_MAX_APPROX_LONG_PATTERN 512
#define BMX_MAX_APPROX_LONG_K 255
int bmx_search_approx_long_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                  const char *pat, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist /* may be NULL */,
                                  uint64_t capacity, uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out, as bmx_search_approx (ctx may be NULL; dist may be NULL). */
int bmx_search_approx_long(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const char *pat, int32_t m,
                           int32_t k, uint64_t *ends, uint8_t *dist, uint64_t capacity, uint64_t *n_matches);

/* ---- class-pattern search: wildcards, sets, case folding, IUPAC codes ---------------------- */

/* A fixed-length pattern whose every position is a SET of byte values: what `grep -i`, a `.` or `[0-9]` position and a
 * degenerate primer such as GTGYCAGCMGCCGCGGTAA ask for.  The reference has no such program.  The matcher is Shift-And
 * (Baeza-Yates and Gonnet), one 32- or 64-bit word per lane, with the approximate search's ordered output
 * (csrc/bmx_classes_kernel.h).
 *
 * A pattern is m classes of BMX_CLASS_BYTES bytes each: byte value b belongs to class i iff bit (b & 7) of
 * classes[i * BMX_CLASS_BYTES + (b >> 3)] is set.  An empty class is legal and matches nothing.
 * Semantics: every start p with p < n_own, p + m <= n and text[p + i] in class i for all i in [0, m), ascending, each
 * reported as base_offset + p; overlapping matches count; n_own >= n means all of the view.  These are
 * bmx_search_device's conventions: a shard passes m - 1 halo bytes and the shards' lists concatenate to the whole text's
 * list, and with every class a singleton the list is exactly bmx_search_device's for that string.  Any byte values in
 * text and classes; 1 <= m <= BMX_MAX_CLASS_PATTERN, n < 2^40, any alignment of d_text.
 * Capacity: the stored entries are the LOWEST `capacity` starts; *n_matches is the true total, and a larger total returns
 * BMX_ERR_CAPACITY (capacity 0 counts only).  Argument errors (NULL pointers where needed, m out of range, n too large)
 * return BMX_ERR_ARG before any HIP call, with ctx = NULL too.  A workgroup that waits longer than its bound (~1 s) for
 * its predecessors' counts makes the call return BMX_ERR_HIP: a list is never returned partly ordered.
 * One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising that stream. */
#define BMX_MAX_CLASS_PATTERN 64
#define BMX_CLASS_BYTES 32 /* one class: a 256-bit set; byte value b belongs iff bit (b & 7) of byte (b >> 3) is set */
#define BMX_CLASS_ICASE 1u
#define BMX_CLASS_IUPAC 2u
/* Pure host code, no GPU (like bmx_build_tables): one element of expr is one class, *m the number of elements.
 *   .        every byte value
 *   [...]    a set: x-y is an inclusive range (x <= y), a leading ^ negates, ] directly after [ or [^ is a literal
 *            (so is a - that does not stand between two items)
 *   \xHH     the byte with that two-digit hexadecimal value; \ before any other byte: that byte as a literal (both
 *            inside sets too)
 *   any byte other than . [ \ is itself.  No repetition, alternation or anchors.
 * BMX_CLASS_ICASE: every ASCII letter in a class brings its other case (applied before a set's negation).
 * BMX_CLASS_IUPAC: outside brackets and escapes the upper-case letters R Y S W K M B D H V N stand for their nucleotide
 * sets over ACGT (N = ACGT, R = AG, Y = CT, ...); A C G T stay literal; with both flags the lower-case bases belong too.
 * BMX_ERR_ARG: NULL arguments, an unterminated set, a reversed range, a dangling \, bad hex, zero elements or more than
 * BMX_MAX_CLASS_PATTERN; *m and classes are then untouched.  classes has room for BMX_MAX_CLASS_PATTERN classes. */
int bmx_compile_classes(const char *expr, uint64_t expr_len, uint32_t flags,
                        uint8_t *classes /* BMX_MAX_CLASS_PATTERN * BMX_CLASS_BYTES */, int32_t *m);
int bmx_search_classes_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                              const uint8_t *classes, int32_t m, uint64_t *d_match_positions, uint64_t capacity,
                              uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out (upload, bmx_search_classes_device, download). */
int bmx_search_classes(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const uint8_t *classes, int32_t m,
                       uint64_t *match_positions, uint64_t capacity, uint64_t *n_matches);
/* Device time (ms, HIP events around the class-search kernel) of the last call on ctx; < 0 if none. */
float bmx_last_classes_ms(bmx_ctx *ctx);
/* bmx_search_approx_device with "text[j] == pat[i]" replaced by "text[j] in class i": the same ends, distances, lead
 * contract, domain (m <= BMX_MAX_APPROX_PATTERN, 0 <= k < m), errors and kernel; bmx_last_approx_ms times it. */
int bmx_search_approx_classes_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                     const uint8_t *classes, int32_t m, int32_t k, uint64_t *d_ends, uint8_t *d_dist,
                                     uint64_t capacity, uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out, as bmx_search_approx (ctx may be NULL; dist may be NULL). */
int bmx_search_approx_classes(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const uint8_t *classes, int32_t m,
                              int32_t k, uint64_t *ends, uint8_t *dist, uint64_t capacity, uint64_t *n_matches);

/* ---- k-mismatch (Hamming) search: at most k substitutions, no insertions or deletions -------- */

/* Where does a fixed-length pattern occur with at most k positions wrong: a barcode, an adapter or a primer site with a few
 * mismatches, a peptide motif, a CRISPR guide of 20 bases with up to k mismatches next to a PAM such as NGG that must match
 * exactly.  The approximate search answers a wider question (edits, every end of a run of ends); this one counts
 * substitutions only and reports each window once, by its start.  The reference has no such program.  The matcher is
 * Shift-Add (Baeza-Yates and Gonnet) with bit-sliced counters, two slices for k <= 3 and four for k <= 15, in one 32- or
 * 64-bit word per slice and lane, over the class search's walk and ordered output (csrc/bmx_hamming_kernel.h).
 *
 * A pattern is m classes as in bmx_search_classes_device; the string form is m singleton classes.
 * Semantics: every start p with p < n_own and p + m <= n at which d(p), the number of positions i in [0, m) with
 * text[p + i] NOT in class i, is at most k and no position i with bit i of `must` set mismatches; ascending, each reported
 * as base_offset + p, with d(p) in d_dist (one byte per entry, 0..k; d_dist may be NULL).  A class of every byte value
 * never counts; an empty class always mismatches (it counts 1, or rules the window out if it is in `must`).  With k = 0
 * the list is bmx_search_classes_device's, every distance is 0 and `must` has no effect.  Every hit's end p + m - 1 is
 * among bmx_search_approx_classes_device's ends at the same k, with an edit distance <= d(p).
 * Overlapping matches count; n_own >= n means all of the view.  These are bmx_search_device's conventions: a shard passes
 * m - 1 halo bytes and the shards' lists concatenate to the whole text's list.  Any byte values in text and classes;
 * 1 <= m <= BMX_MAX_HAMMING_PATTERN, 0 <= k < m, k <= BMX_MAX_HAMMING_K, no bit of `must` at or above m, n < 2^40, any
 * alignment of d_text.
 * Capacity: the stored entries are the LOWEST `capacity` starts; *n_matches is the true total, and a larger total returns
 * BMX_ERR_CAPACITY (capacity 0 counts only).  Argument errors (NULL pointers where needed, m, k or `must` out of range, n
 * too large) return BMX_ERR_ARG before any HIP call, with ctx = NULL too.  A workgroup that waits longer than its bound
 * (~1 s) for its predecessors' counts makes the call return BMX_ERR_HIP: a list is never returned partly ordered.
 * One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising that stream. */
#define BMX_MAX_HAMMING_PATTERN 64
#define BMX_MAX_HAMMING_K 15
int bmx_search_hamming_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                              const char *pat, int32_t m, int32_t k, uint64_t must, uint64_t *d_starts,
                              uint8_t *d_dist /* may be NULL */, uint64_t capacity, uint64_t *n_matches, void *stream);
int bmx_search_hamming_classes_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                                      const uint8_t *classes, int32_t m, int32_t k, uint64_t must, uint64_t *d_starts,
                                      uint8_t *d_dist /* may be NULL */, uint64_t capacity, uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out (upload, the device entry, download; dist may be NULL). */
int bmx_search_hamming(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const char *pat, int32_t m, int32_t k,
                       uint64_t must, uint64_t *starts, uint8_t *dist, uint64_t capacity, uint64_t *n_matches);
int bmx_search_hamming_classes(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const uint8_t *classes, int32_t m,
                               int32_t k, uint64_t must, uint64_t *starts, uint8_t *dist, uint64_t capacity, uint64_t *n_matches);
/* Device time (ms, HIP events around the k-mismatch kernel) of the last call on ctx; < 0 if none. */
float bmx_last_hamming_ms(bmx_ctx *ctx);

/* ---- gapped pattern search: optional and counted classes, PROSITE --------------------------- */

/* A class pattern whose parts sit at a variable distance: C-x(2,4)-C-x(3)-[LIVMFYWC]-x(8)-H-x(3,5)-H (the PROSITE
 * zinc-finger signature), a primer pair with 10 to 20 bases between its halves, colou?r.  One pass over the text answers
 * what otherwise takes one bmx_search_classes_device pass per combination of gap lengths.  The reference has no such
 * program.  The matcher is Navarro and Raffinot's extended Shift-And restricted to BOUNDED repetition, one 32- or 64-bit
 * word per lane, with the class search's geometry and ordered output (csrc/bmx_gaps_kernel.h).
 *
 * A gapped pattern is M positions, 1 <= M <= BMX_MAX_GAPS_PATTERN.  Position i has a class (BMX_CLASS_BYTES bytes, encoded
 * exactly as for bmx_search_classes; an empty class is legal) and is OPTIONAL iff bit i of `optional` is set.  At least one
 * position must be mandatory (a pattern that matches the empty string is BMX_ERR_ARG) and no bit at or above M may be set.
 * A substring text[s..j] of length L >= 1 MATCHES iff there are positions i_0 < i_1 < ... < i_{L-1} that contain every
 * mandatory position, with text[s + t] in class i_t for every t.
 * Semantics: every END j in [lead, n) for which some s with 0 <= s <= j matches, each end once, ascending, reported as
 * base_offset + j.  Ends, not starts, because several starts can share one end (the approximate search's convention).
 * A match spans at most M bytes, so a shard passes a view that begins M - 1 bytes (clipped at 0) before its first end,
 * with lead = that amount: the shards' lists then concatenate to the whole text's list.
 * Two identities: with optional == 0 the list is bmx_search_classes_device's starts + M - 1; for any pattern it is the
 * union of "starts + length - 1" over the fixed-length class patterns that the choices of optional positions give.
 * Any byte values in text and classes; n < 2^40, any alignment of d_text.
 * Capacity: the stored entries are the LOWEST `capacity` ends; *n_matches is the true total, and a larger total returns
 * BMX_ERR_CAPACITY (capacity 0 counts only).  Argument errors (NULL pointers where needed, M or `optional` out of range,
 * lead > n, n too large) return BMX_ERR_ARG before any HIP call, with ctx = NULL too.  A workgroup that waits longer
 * than its bound (~1 s) for its predecessors' counts makes the call return BMX_ERR_HIP: a list is never returned partly
 * ordered.  One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising that stream.
 * Out of scope: unbounded repetition (* and +), anchors, M > 64; alternation and groups are not part of this search but of
 * the regular-expression search below (bmx_compile_regex, bmx_search_regex_device). */
#define BMX_MAX_GAPS_PATTERN 64
#define BMX_GAPS_PROSITE 4u /* (beside BMX_CLASS_ICASE and BMX_CLASS_IUPAC in the flags of bmx_compile_gaps) */
/* Pure host code, no GPU.  *m is the number of positions after expansion, bit i of *optional says that position i is
 * optional; classes has room for BMX_MAX_GAPS_PATTERN classes.
 * Default syntax: the elements of bmx_compile_classes (. [...] [^...] \xHH \c, any other byte; BMX_CLASS_ICASE and
 * BMX_CLASS_IUPAC as there), each optionally followed by ONE quantifier: ? or {a} or {a,b}, decimal, 0 <= a <= b, b >= 1.
 * An element with {a,b} expands to a mandatory copies followed by b - a optional ones; ? is {0,1}.  \? \{ \* \+ are
 * literals, and inside a set these four bytes are literals anyway.
 * BMX_GAPS_PROSITE: elements separated by -; x is any byte, [ABC] a set, {ABC} a negated set (one or more bytes, taken
 * literally: no ranges, no escapes), any other byte than - ] } ( ) < > . , is itself; (n) or (a,b) behind an element is
 * its repetition, with the same bounds; one trailing . is ignored.  The anchors < and > are out of scope and return
 * BMX_ERR_ARG, inside a set too.  BMX_CLASS_ICASE combines normally; BMX_CLASS_IUPAC with this flag is BMX_ERR_ARG.
 * BMX_ERR_ARG: NULL arguments; a flag bit other than the three above; an unescaped * or +; {a,}; a quantifier with no element in front of it or right after
 * another quantifier; b == 0, a > b, a malformed or unterminated {...} or (...); more than BMX_MAX_GAPS_PATTERN positions
 * after expansion; no mandatory position; zero elements; an empty PROSITE element or set; every error of
 * bmx_compile_classes (an unterminated set, a reversed range, a dangling \, bad hex).  The outputs are then untouched. */
int bmx_compile_gaps(const char *expr, uint64_t expr_len, uint32_t flags,
                     uint8_t *classes /* BMX_MAX_GAPS_PATTERN * BMX_CLASS_BYTES */, uint64_t *optional, int32_t *m);
int bmx_search_gaps_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                           const uint8_t *classes, int32_t m, uint64_t optional, uint64_t *d_ends, uint64_t capacity,
                           uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out (upload, bmx_search_gaps_device with lead = 0, download). */
int bmx_search_gaps(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const uint8_t *classes, int32_t m,
                    uint64_t optional, uint64_t *ends, uint64_t capacity, uint64_t *n_matches);
/* Device time (ms, HIP events around the gapped-search kernel) of the last bmx_search_gaps_device on ctx; < 0 if none. */
float bmx_last_gaps_ms(bmx_ctx *ctx);
/* The START of a match for every end of a device-resident list, as bmx_search_gaps_device returns it for the same view,
 * pattern and base_offset: d_starts[i] = base_offset + s with text[s..j_i] a match, d_ends[i] = base_offset + j_i.  By
 * default s is the LARGEST such start (the shortest match), with BMX_GAPS_LONGEST the smallest s >= 0 of the view (the
 * longest; a shard's halo of M - 1 bytes holds it).  One list entry per lane; the lane walks at most M bytes backwards
 * from j.  Every end of the search is a true end of a match, so there is no selection of entries.
 * Errors: NULL pointers where needed, a pattern or n out of range and unknown flag bits return BMX_ERR_ARG before any HIP
 * call, with ctx = NULL too; count == 0 returns BMX_OK and launches nothing.  An entry outside
 * [base_offset, base_offset + n) reads no byte and raises a status word, and so does an entry at which no match ends (a
 * list of another pattern or text): the call then returns BMX_ERR_ARG and the outputs are unspecified.
 * No byte outside the aligned 16-byte lines that hold text[0..n) is read, none below text[0]'s line.
 * One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising it. */
#define BMX_GAPS_LONGEST 1u
int bmx_gaps_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const uint8_t *classes, int32_t m,
                           uint64_t optional, const uint64_t *d_ends, uint64_t count, uint32_t flags, uint64_t *d_starts,
                           void *stream);
/* Host buffers in, host buffers out: upload, bmx_search_gaps_device, bmx_gaps_starts_device (flags: BMX_GAPS_LONGEST or
 * 0), download.  starts[i] belongs to ends[i]; capacity and *n_matches as for bmx_search_gaps.  ctx may be NULL. */
int bmx_search_gaps_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const uint8_t *classes, int32_t m,
                          uint64_t optional, uint32_t flags, uint64_t *starts, uint64_t *ends, uint64_t capacity,
                          uint64_t *n_matches);

/* ---- regular-expression search: groups, alternation, counted repeats (star-free) ------------- */

/* ATG([ACGT]{3}){2,4}(TAA|TAG|TGA), (ERROR|FATAL|PANIC): [0-9]{2,4}, ([0-9]{1,3}\.){3}[0-9]{1,3}: one pass over the text
 * answers what otherwise takes one class or gapped pass per fixed-length variant and a merge of their lists.  The
 * expressions are the STAR-FREE ones: a star-free expression has a longest match, so a lane's warm-up of a fixed number
 * of bytes is exact and the geometry, the shard contract and the ordered output are the gapped search's.  The reference
 * has no such program.  The matcher runs the Glushkov (position) automaton bit-parallel, one 32- or 64-bit word per
 * lane: positions whose only successor is the next one move by a shift, the others through small tables in LDS
 * (csrc/bmx_regex_kernel.h).
 *
 * The automaton is plain data.  Positions are numbered left to right; position i has a class (BMX_CLASS_BYTES bytes,
 * encoded exactly as for bmx_search_classes; an empty class is legal, and so are positions that no match can use).
 * A substring text[s..j] of length L >= 1 MATCHES iff there are positions i_0, .., i_{L-1} with i_0 in `first`,
 * i_{t+1} in follow[i_t], i_{L-1} in `last` and text[s + t] in class i_t for every t.
 * Valid: 1 <= m <= BMX_MAX_REGEX_POSITIONS; first and last non-zero; no bit at or above m in first, last or any
 * follow[i]; follow[i] holds only bits j > i.  The automaton is then acyclic, a match visits a position at most once and
 * max_len <= m.  The search entries recompute min_len and max_len from the sets and do not read the two fields;
 * bmx_compile_regex fills them so that the caller knows its halo. */
#define BMX_MAX_REGEX_POSITIONS 64
typedef struct bmx_regex {
    int32_t  m;                 /* positions, 1..64, numbered left to right after expansion */
    int32_t  min_len, max_len;  /* shortest / longest match in bytes; filled by bmx_compile_regex */
    uint64_t first;             /* bit i: a match may begin with position i */
    uint64_t last;              /* bit i: a match may end with position i */
    uint64_t follow[BMX_MAX_REGEX_POSITIONS];  /* bit j of follow[i]: position j may come right after i */
    uint8_t  classes[BMX_MAX_REGEX_POSITIONS * BMX_CLASS_BYTES];  /* as for bmx_search_classes */
} bmx_regex;
/* Pure host code, no GPU.
 *   alt    := concat ('|' concat)*        an empty alternative is allowed: (a|) is a?
 *   concat := repeat*
 *   repeat := atom quant?                 quant := '?' | '{a}' | '{a,b}'   decimal, 0 <= a <= b, b >= 1
 *   atom   := element | '(' alt ')'
 * An element is exactly one element of bmx_compile_classes (. [...] [^...] \xHH \c, any other byte; BMX_CLASS_ICASE and
 * BMX_CLASS_IUPAC as there, and no other flag), so \( \) \| \? \{ \* \+ are literals and inside a set these bytes are
 * literals anyway.  X{a,b} expands to a copies of X followed by b - a optional copies, for a group as for an element;
 * first, last, follow and nullability come from the standard Glushkov recursion.  Groups do not capture here; bmx_compile_regex_groups at the end of this file makes
 * the same automaton and the capture model beside it.
 * BMX_ERR_ARG, with *out untouched and a text in bmx_last_error: NULL arguments; an unknown flag bit; an unescaped * or +,
 * or {a,} (unbounded repetition is out of scope); unbalanced ( or ); a quantifier with nothing in front of it or right
 * after another quantifier (so (?: is an error); b == 0, a > b, a malformed or unterminated {...}; nesting deeper than 32;
 * more than BMX_MAX_REGEX_POSITIONS positions after expansion, or zero; an expression that matches the empty string;
 * every error of bmx_compile_classes. */
int bmx_compile_regex(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *out);
/* Semantics: every END j in [lead, n) at which some match ends, each end once, ascending, reported as base_offset + j
 * (ends, as in the gapped search: several starts can share one end).  A match spans at most max_len bytes, so a shard
 * passes a view that begins max_len - 1 bytes (clipped at 0) before its first end, with lead = that amount: the shards'
 * lists then concatenate to the whole text's list.
 * Two identities: an expression without groups gives bmx_search_gaps_device's list; any expression gives the union of
 * "starts + length - 1" over the fixed-length class patterns that its paths from `first` to `last` spell.
 * Any byte values in text and classes; n < 2^40, any alignment of d_text.
 * Capacity: the stored entries are the LOWEST `capacity` ends; *n_matches is the true total, and a larger total returns
 * BMX_ERR_CAPACITY (capacity 0 counts only).  Argument errors (NULL pointers where needed, an automaton that is not valid,
 * lead > n, n too large) return BMX_ERR_ARG before any HIP call, with ctx = NULL too.  A workgroup that waits longer
 * than its bound (~1 s) for its predecessors' counts makes the call return BMX_ERR_HIP: a list is never returned partly
 * ordered.  One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising that stream.
 * Out of scope: unbounded repetition (* + {a,}; bmx_search_regex_star_device below), back-references inside the
 * expression (capture groups: bmx_regex_groups_device at the end of this file), more than 64 positions (up to 128: bmx_compile_regex_long and bmx_search_regex_long_device at the end of this file).  Anchors
 * and word boundaries: bmx_compile_regex_anchored and bmx_search_regex_anchored_device below. */
int bmx_search_regex_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                            const bmx_regex *re, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out (upload, bmx_search_regex_device with lead = 0, download). */
int bmx_search_regex(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                     uint64_t *ends, uint64_t capacity, uint64_t *n_matches);
/* Device time (ms, HIP events around the regex-search kernel) of the last bmx_search_regex_device on ctx; < 0 if none. */
float bmx_last_regex_ms(bmx_ctx *ctx);
/* The START of a match for every end of a device-resident list, as bmx_search_regex_device returns it for the same view,
 * automaton and base_offset: d_starts[i] = base_offset + s with text[s..j_i] a match, d_ends[i] = base_offset + j_i.  By
 * default s is the LARGEST such start (the shortest match), with BMX_REGEX_LONGEST the smallest s >= 0 of the view (the
 * longest; a shard's halo of max_len - 1 bytes holds it).  One list entry per lane; the lane runs the reversed automaton
 * over at most max_len bytes backwards from j.
 * Errors: NULL pointers where needed, an automaton that is not valid, n out of range and unknown flag bits return
 * BMX_ERR_ARG before any HIP call, with ctx = NULL too; count == 0 returns BMX_OK and launches nothing.  An entry outside
 * [base_offset, base_offset + n) reads no byte and raises a status word, and so does an entry at which no match ends (a
 * list of another expression or text): the call then returns BMX_ERR_ARG and the outputs are unspecified.
 * No byte outside the aligned 16-byte lines that hold text[0..n) is read, none below text[0]'s line.
 * One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising it. */
#define BMX_REGEX_LONGEST 1u
int bmx_regex_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                            const uint64_t *d_ends, uint64_t count, uint32_t flags, uint64_t *d_starts, void *stream);
/* Host buffers in, host buffers out: upload, bmx_search_regex_device, bmx_regex_starts_device (flags: BMX_REGEX_LONGEST or
 * 0), download.  starts[i] belongs to ends[i]; capacity and *n_matches as for bmx_search_regex.  ctx may be NULL. */
int bmx_search_regex_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re, uint32_t flags,
                           uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_matches);

/* ---- regular-expression search with unbounded repetition: * + {a,} ------------------------- */

/* ERROR.*timeout, [0-9]+\.[0-9]+, ATG([ACGT]{3})+(TAA|TAG|TGA), [A-Za-z_][A-Za-z0-9_]*\(: the same automaton struct and
 * the same per-byte step as above, with a cycle in follow[].  A cycle means there is no longest match, so no fixed
 * warm-up makes a lane exact; the entries below are exact all the same, for every valid automaton and every text
 * (csrc/bmx_regex_star_kernel.h).  The star-free entries above are unchanged and still refuse a cycle.
 *
 * max_len of an automaton with a cycle among the positions a match can use. */
#define BMX_REGEX_UNBOUNDED (-1)
/* bmx_compile_regex's grammar with  quant := '?' | '*' | '+' | '{a}' | '{a,}' | '{a,b}'.  X+ adds follow[l] |= first(X)
 * for every l in last(X) (the Glushkov rule, for a group as for an element); X* is (X+)?; X{a,} is a - 1 copies of X
 * followed by X+ (a == 0: X*).  Every other rule and every other error of bmx_compile_regex holds: an expression that
 * matches the empty string (a*, (ab)*) is an error, so are more than 64 positions, nesting deeper than 32 and a
 * quantifier right after another one; *out is untouched on error; the text in bmx_last_error begins with
 * "bmx_compile_regex_star: ".  For an expression without * + {a,} the output equals bmx_compile_regex's byte for byte.
 * min_len is the shortest match; max_len the longest, or BMX_REGEX_UNBOUNDED.  Pure host code, no GPU. */
int bmx_compile_regex_star(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *out);
/* Valid for the entries below: 1 <= m <= BMX_MAX_REGEX_POSITIONS; first and last non-zero; no bit at or above m in first,
 * last or any follow[i].  follow[i] may hold ANY bit below m, i itself included.  min_len and max_len are not read.
 *
 * Semantics: every END j in [lead, n) at which some text[s..j] with 0 <= s OF THE VIEW matches, each end once, ascending,
 * reported as base_offset + j.  The list is exact: there is no approximation and no "unresolved" error.  An automaton
 * without a cycle gives bmx_search_regex_device's list.
 * Sharding: a match may begin anywhere, so there is no halo that makes shards' lists concatenate to the whole text's.
 * What a caller CAN conclude from a shard whose view begins at text byte v: every reported end is an end of the whole
 * text's list, and the ends it misses are those whose every match begins before v.  With a view that begins at text
 * byte 0 and lead = the shard's first end, the shard's list is that slice of the whole text's list (at the price of
 * reading the text in front).  A state carried from one shard into the next is not offered.
 * Capacity, *n_matches, the argument errors before any HIP call (with ctx = NULL too), n < 2^40, any alignment and
 * BMX_ERR_HIP in place of a partly ordered list: as for bmx_search_regex_device.
 * One kernel launch in the common case: a lane warms up in front of its first end from the empty and from the full set
 * of positions at once and is exact if the two meet.  If some lane's do not, the call repeats the search exactly with
 * three more passes over the text (the state at every piece boundary as a linear map, a sweep over those, the search
 * from the swept states); its workspace, 40 bytes per piece plus 8 per stored column, is allocated on the first such
 * call and kept with the context.  The call returns after synchronising `stream`. */
int bmx_search_regex_star_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                 const bmx_regex *re, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out (upload, bmx_search_regex_star_device with lead = 0, download). */
int bmx_search_regex_star(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                          uint64_t *ends, uint64_t capacity, uint64_t *n_matches);
/* Device time (ms) of the last bmx_search_regex_star_device on ctx: the one launch, or, where the call repeated the
 * search, from the first launch to the end of the last; < 0 if none. */
float bmx_last_regex_star_ms(bmx_ctx *ctx);
/* The START of a match of at most `window` bytes for every end of a device-resident list: the largest such start (the
 * shortest match), with BMX_REGEX_LONGEST the smallest one that is still within `window` bytes of the end and within the
 * view.  1 <= window <= BMX_MAX_REGEX_STAR_WINDOW.  An end at which no match that short ends gets UINT64_MAX and is not
 * an error: a longer one may exist.  The bound is explicit because with .* the longest start is the text's first byte.
 * Errors as for bmx_regex_starts_device, with the validity rule above and window out of range among the argument
 * errors; an end outside the view raises the status word, and so does an end without a match within `window` if the
 * automaton has no cycle and its longest match fits the window, so that no longer one can exist (BMX_ERR_ARG, outputs
 * unspecified).  Where some end has no match a second small kernel writes the sentinels. */
#define BMX_MAX_REGEX_STAR_WINDOW 65536u
int bmx_regex_star_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                 const uint64_t *d_ends, uint64_t count, uint32_t window, uint32_t flags, uint64_t *d_starts,
                                 void *stream);
/* Host buffers in, host buffers out: upload, bmx_search_regex_star_device, bmx_regex_star_starts_device, download. */
int bmx_search_regex_star_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                                uint32_t window, uint32_t flags, uint64_t *starts, uint64_t *ends, uint64_t capacity,
                                uint64_t *n_matches);

/* ---- match spans of the approximate search: (start, end, distance) ------------------------- */

/* The approximate search reports ENDS, and every qualifying end, so one occurrence shows as a run of adjacent ends.
 * This post-pass over a device-resident list of ends gives what a caller slices at: the START of every match and, with
 * BMX_SPANS_BEST, one entry per occurrence.  It changes nothing in the search and in what the search returns.
 *
 * The list: d_ends[i] = base_offset + j_i with d_dist[i] = min over s of ED(pat, text[s..j_i]) <= k, as
 * bmx_search_approx[_classes]_device returns it for the same view, pattern, k and base_offset (the lists of shards
 * concatenate by contract; select on the whole).
 * Start: for an end j with distance d, the LARGEST s with ED(pat, text[s..j]) == d, the shortest span that attains the
 * minimum, reported as base_offset + s.  Its length L = j - s + 1 satisfies m - d <= L <= m + d, so start <= end.
 * BMX_SPANS_BEST: entry i is kept iff dist[i] <= dprev and dist[i] < dnext, where dprev = dist[i-1] if i > 0 and
 * ends[i-1] == ends[i] - 1, else k + 1, and dnext = dist[i+1] if i + 1 < count and ends[i+1] == ends[i] + 1, else k + 1:
 * the last end of every local minimum of the distance along a run of adjacent ends (an end that is not in the list
 * counts as k + 1).  The rule takes LIST neighbours literally, so it is defined for any list.  Adjacent ends differ by
 * at most 1 in distance, so a rising plateau (1,2,2,3) also keeps its last 2: the price of a rule without look-back.
 * Example: text xxabcdxxabxdxxacdxx, pattern abcd, k = 1; the search returns ends [4,5,6,11,16], dist [1,0,1,1,1].
 *   flags 0           (2,4,1) (2,5,0) (2,6,1) (8,11,1) (14,16,1)      as (start, end, dist)
 *   BMX_SPANS_BEST    (2,5,0) (8,11,1) (14,16,1)
 *
 * Outputs: buffers with room for `count` entries that do not overlap the inputs; *n_spans is the number written.  With
 * flags == 0 that is `count` and d_starts[i] belongs to d_ends[i], in whatever order the list has (d_sel_ends and
 * d_sel_dist are not written).  With BMX_SPANS_BEST the kept entries go to d_sel_ends / d_sel_dist / d_starts in list
 * order: ascending in, ascending out.
 * Domain: that of the search (1 <= m <= BMX_MAX_APPROX_PATTERN, 0 <= k < m, n < 2^40, any alignment of d_text, any byte
 * values); count is 64-bit.
 * Errors: NULL pointers where needed, m / k / n out of range and unknown flag bits return BMX_ERR_ARG before any HIP
 * call, with ctx = NULL too; count == 0 returns BMX_OK and launches nothing.  An entry whose end is not in
 * [base_offset, base_offset + n) reads no byte and raises a status word, and so does an entry whose minimum over its
 * window is above k or (where a distance is at hand) differs from it: a list of another pattern or text.  The call then
 * returns BMX_ERR_ARG and the outputs are unspecified.
 * No byte outside the aligned 16-byte lines that hold text[0..n) is read, none below text[0]'s line.
 * All device work goes on `stream` (NULL = the null stream); the call returns after synchronising it (with
 * BMX_SPANS_BEST also once in between, to read the kept count). */
#define BMX_SPANS_BEST 1u
int bmx_approx_spans_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const char *pat, int32_t m,
                            int32_t k, const uint64_t *d_ends, const uint8_t *d_dist /* may be NULL iff flags == 0 */,
                            uint64_t count, uint32_t flags, uint64_t *d_starts,
                            uint64_t *d_sel_ends /* may be NULL iff flags == 0 */, uint8_t *d_sel_dist /* may be NULL */,
                            uint64_t *n_spans, void *stream);
/* The same with a class per pattern position (the list of bmx_search_approx_classes_device). */
int bmx_approx_spans_classes_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset,
                                    const uint8_t *classes, int32_t m, int32_t k, const uint64_t *d_ends,
                                    const uint8_t *d_dist, uint64_t count, uint32_t flags, uint64_t *d_starts,
                                    uint64_t *d_sel_ends, uint8_t *d_sel_dist, uint64_t *n_spans, void *stream);
/* Host buffers in, host buffers out: upload, bmx_search_approx[_classes]_device (counting first where `capacity` cannot
 * hold every end), the spans, download.  ctx may be NULL; dist may be NULL.  *n_spans is the true number of spans; more
 * than `capacity` returns BMX_ERR_CAPACITY with the lowest `capacity` spans stored (capacity 0 counts only). */
int bmx_search_approx_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const char *pat, int32_t m,
                            int32_t k, uint32_t flags, uint64_t *starts, uint64_t *ends, uint8_t *dist, uint64_t capacity,
                            uint64_t *n_spans);
int bmx_search_approx_spans_classes(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const uint8_t *classes,
                                    int32_t m, int32_t k, uint32_t flags, uint64_t *starts, uint64_t *ends, uint8_t *dist,
                                    uint64_t capacity, uint64_t *n_spans);
/* The same for the lists of bmx_search_approx_long_device: a string of up to BMX_MAX_APPROX_LONG_PATTERN bytes with
 * k <= BMX_MAX_APPROX_LONG_K.  Definitions, outputs, BMX_SPANS_BEST, the three list checks and the synchronisation are
 * those of bmx_approx_spans_device; above 64 bytes the starts kernel carries the reversed pattern's column in several
 * words and walks at most m + k bytes back from every end. */
int bmx_approx_long_spans_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const char *pat, int32_t m,
                                 int32_t k, const uint64_t *d_ends, const uint8_t *d_dist /* may be NULL if flags == 0 */,
                                 uint64_t count, uint32_t flags, uint64_t *d_starts, uint64_t *d_sel_ends, uint8_t *d_sel_dist,
                                 uint64_t *n_spans, void *stream);
int bmx_search_approx_long_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const char *pat, int32_t m,
                                 int32_t k, uint32_t flags, uint64_t *starts, uint64_t *ends, uint8_t *dist, uint64_t capacity,
                                 uint64_t *n_spans);
/* Device time (ms, HIP events around the spans kernels) of the last call on ctx (the long entries included); < 0 if none. */
float bmx_last_spans_ms(bmx_ctx *ctx);

/* ---- dictionary search: many patterns in one pass ------------------------------------------ */

/* What `grep -F -f words.txt` asks: every occurrence of every pattern of a word list, a block list or a set of primers,
 * in ONE pass over a resident text (bmx_search_device_multi takes at most BMX_MAX_MULTI patterns and walks each with its
 * own tables).  The reference has no such program; its one report per hit is BoyreMoore/x64/Debug/kernel1.cl:24.
 *
 * A dictionary is built once on the host (LDS filter bitmaps, an exact-prefix table, the patterns packed in one blob),
 * uploaded to ctx's device and reused across searches and texts.  1 <= K <= BMX_MAX_DICT patterns, 1 <= ms[i] <=
 * BMX_MAX_PATTERN; a pattern byte >= 0x80 returns BMX_ERR_DOMAIN (as bmx_build_tables does).
 * Semantics: every pair (p, i) with text[p .. p + ms[i]) == pats[i], ordered by p, then by i, positions in d_pos and
 * pattern indices in d_pid (which may be NULL).  Overlapping matches count, every pattern matching at one p counts, and
 * identical patterns under different indices are each reported.  Restricted to one i the positions are those of
 * bmx_search_device(pats[i]).  Text bytes may have any value; n < 2^40, any alignment of d_text.
 * Shards: only windows that start in [0, n_own) and fit in n are reported, each as base_offset + p (n_own >= n: all);
 * a shard passes a halo of max(ms) - 1 bytes and the shards' lists concatenate to the whole text's list.
 * Capacity: the stored pairs are the LOWEST `capacity` pairs in the order above; *n_matches is the true total, and a
 * larger total returns BMX_ERR_CAPACITY (capacity 0 counts only).  Argument errors (NULL pointers, K or m out of
 * range, a dictionary of another context) return BMX_ERR_ARG / BMX_ERR_DOMAIN before any HIP call, with ctx = NULL
 * too.  A workgroup that waits longer than its bound (~1 s) for its predecessors' counts makes the call return
 * BMX_ERR_HIP: a list is never returned partly ordered.
 * One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising that stream. */
#define BMX_MAX_DICT 65536
typedef struct bmx_dict bmx_dict;
int bmx_dict_create(bmx_ctx *ctx, const char *const *pats, const int32_t *ms, int32_t K, bmx_dict **out);
void bmx_dict_destroy(bmx_dict *d);
int bmx_dict_search_device(bmx_ctx *ctx, const bmx_dict *d, const void *d_text, uint64_t n, uint64_t n_own,
                           uint64_t base_offset, uint64_t *d_pos, uint32_t *d_pid /* may be NULL */, uint64_t capacity,
                           uint64_t *n_matches, void *stream);
/* Host buffers in and out (upload, bmx_dict_create, bmx_dict_search_device, download, bmx_dict_destroy).  ctx may be
 * NULL (a context on device 0 is created and destroyed inside); pid may be NULL. */
int bmx_dict_search(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const char *const *pats,
                    const int32_t *ms, int32_t K, uint64_t *pos, uint32_t *pid, uint64_t capacity, uint64_t *n_matches);
/* Device time (ms, HIP events around the dictionary kernel) of the last dictionary search on ctx; < 0 if none. */
float bmx_last_dict_ms(bmx_ctx *ctx);
/* Text positions of the last dictionary search on ctx that passed the LDS filters and were looked up in the
 * exact-prefix table (the filters' false positives plus the matching positions); < 0 if none. */
int64_t bmx_last_dict_candidates(bmx_ctx *ctx);

/* ---- suffix array: the reference's third program -------------------- */

/* sa[j] = start of the j-th suffix of text[0..n), n < 2^31, in the order the reference's
 * buildSuffixArray produces (SuffixArrays/SuffixArrays/SuffixArrays.cpp:101-154; its GPU path is
 * :417-470 with kernel.cl).  That is the ordinary suffix array for the reference's domain
 * (lower-case text); outside it one quirk of the reference is kept: in the first round "past the
 * end" ranks like character 96, so the one-character suffix text[n-1] sorts after suffixes whose
 * second character is below 'a'.  (A text ending in two or more characters 96 leaves suffixes
 * tied in the reference itself; their mutual order is then unspecified.) */
int bmx_suffix_array(bmx_ctx *ctx, const char *text, uint64_t n, int32_t *sa);
int bmx_suffix_array_device(bmx_ctx *ctx, const void *d_text, uint64_t n, int32_t *d_sa, void *stream);
/* Device time (ms) and number of doubling rounds of the last call. */
float bmx_last_suffix_array_ms(bmx_ctx *ctx);
int bmx_last_suffix_array_rounds(bmx_ctx *ctx);
/* ... of which done by the one-kernel LDS path (every group of tied suffixes fitted a workgroup's window). */
int bmx_last_suffix_array_lds_rounds(bmx_ctx *ctx);

/* ---- LCP array over the suffix array, with repeat statistics -------------------------------- */

/* What answers questions about the text itself (the longest repeat, the number of distinct substrings, the intervals of
 * the array that share L bytes), and what every next step over the array starts from.  The reference has no such
 * program.
 *
 * bmx_lcp_array_device: d_lcp[0] = 0 and, for j >= 1, d_lcp[j] = the largest h with sa[j-1] + h <= n, sa[j] + h <= n and
 * text[sa[j-1] .. +h) == text[sa[j] .. +h).  Bytes compare as plain bytes: no virtual symbol, nothing past n.  This is
 * defined for ANY permutation d_sa of 0..n-1, not only for the order bmx_suffix_array_device builds, and that is what is
 * computed.  Domain: 1 <= n < 2^31, any byte values, any alignment of d_text.  d_lcp holds n entries; d_text and d_sa
 * are only read.
 * The method is the Phi / irreducible-LCP algorithm (Karkkainen, Manzini, Puglisi 2009; csrc/bmx_lcp_kernel.h): a pair
 * of suffixes whose common prefix follows from the pair one position to the left is not compared.  A pair that is
 * compared is taken by one lane for its first BMX_LCP_LANE_BYTES bytes (and a look at the next one); a longer common
 * prefix leaves the one-lane path and is compared by whole waves, a pair far longer than the others by many of them.
 * Errors: NULL pointers, n == 0 and n >= 2^31 return BMX_ERR_ARG before any HIP call, with ctx == NULL too.  A d_sa that
 * is not a permutation of 0..n-1 (an entry outside [0, n), or an entry that occurs twice) raises a status word and the
 * call returns BMX_ERR_ARG; the outputs are then unspecified, no text byte has been read at an offset taken from a bad
 * entry and no store has gone outside the buffers.
 * All device work goes on `stream`; the calls return after synchronising it.  Workspace: one int32 per text byte, two
 * int32 per 1,024 text bytes and two per 64 (the list of long pairs).  It lives in the context beside the builder's
 * (per-feature state behind bmx_ctx, freed by bmx_ctx_destroy), is reused by later calls and grown on demand; one above
 * 1 GiB is freed when the call returns, as the builder's is.
 *
 * bmx_lcp_array: host buffers.  Uploads the text, calls bmx_suffix_array_device and bmx_lcp_array_device, downloads lcp
 * (n entries) and, if sa is not NULL, the array.  Its domain is the builder's.
 *
 * bmx_lcp_stats_device: out (host memory) = {max of lcp, the smallest j that attains it, sum of lcp, number of j with
 * lcp[j] >= min_len} over d_lcp[0..n).  Integer arithmetic, partial results combined in a fixed order: the same in every
 * run.  For the array bmx_suffix_array_device builds of a text that does not end in two or more bytes 96 (the text
 * index's domain): out[0] is the length of the longest substring that occurs twice, at sa[out[1]-1] and sa[out[1]], and
 * the text has n(n+1)/2 - out[2] distinct substrings.
 *
 * Measured on one MI355X (HIP events around the LCP kernels; the suffix-array build beside it on the same text): 2^25
 * bytes of random lower-case text 2.04 ms (build 6.92 ms); a 61-letter paragraph repeated to 2^24 + 4,097 bytes 0.66 ms
 * (36.7 ms); 2^25 - 1 bytes of one letter 0.46 ms (60.6 ms). */
#define BMX_LCP_LANE_BYTES 64 /* a pair with a longer common prefix leaves the one-lane path */
int bmx_lcp_array_device(bmx_ctx *ctx, const void *d_text, uint64_t n, const int32_t *d_sa, int32_t *d_lcp, void *stream);
int bmx_lcp_array(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, int32_t *sa /* out, may be NULL */,
                  int32_t *lcp);
int bmx_lcp_stats_device(bmx_ctx *ctx, const int32_t *d_lcp, uint64_t n, uint32_t min_len, uint64_t out[4], void *stream);
/* HIP events around the LCP kernels of the last bmx_lcp_array_device (ms); < 0 if none. */
float bmx_last_lcp_ms(bmx_ctx *ctx);
/* Pairs of the last bmx_lcp_array_device whose common prefix exceeded BMX_LCP_LANE_BYTES; < 0 if none.  (A pair that
 * finds the list of long pairs full is counted and finished by its lane.) */
int64_t bmx_last_lcp_long_pairs(bmx_ctx *ctx);

/* ---- text index: batched pattern count and locate over the suffix array ------------------- */

/* What consumes bmx_suffix_array_device: a column of 10^5 .. 10^7 queries against ONE resident text (k-mer counts, read
 * seeding, log-key lookups), each answered in O(m + log n) reads with no pass over the text.  Every other search of the
 * library reads the whole text per call.  The reference has no such program; its array is SuffixArrays.cpp:101-154.
 *
 * The order that is searched is the builder's, not memcmp's: outside lower-case text the array keeps the reference's
 * "past the end ranks as character 96" rule (above).  For a text that does not end in two or more bytes 96 it is the
 * sorted order of, per suffix i: text[i..n) as signed char; then, if n - 1 - i is even, ONE virtual symbol strictly
 * between byte 95 and byte 96; then "nothing", below everything.  A suffix that runs out before the query is never a
 * match.  The suffixes that begin with a query are one interval [lo, lo + cnt) of the array and exactly its true
 * occurrences: those p with p + m <= n and text[p..p+m) == query (csrc/bmx_index_kernel.h has the comparator).
 *
 * Text and ownership: 1 <= n < 2^31, any byte values, any alignment.  The index BORROWS d_text and a caller's d_sa (the
 * array bmx_suffix_array_device gives for this text): both stay alive and unchanged until bmx_index_destroy.  With d_sa
 * == NULL the array is built here (bmx_suffix_array_device on `stream`) and owned.  The index owns its directory: for
 * each of the 128 x 128 two-byte prefixes the (start, count) of its interval, 128 KiB in device memory, made at creation
 * by the count kernel itself.  A text that ends in two or more bytes 96 returns BMX_ERR_DOMAIN (the reference leaves
 * such suffixes tied).  Several indexes may live on one context.
 * Queries: one string column in the Arrow layout of bmx_edit_distance_batch_device, a byte blob plus count + 1
 * non-decreasing uint64 offsets.  Every query has 1 .. BMX_MAX_PATTERN bytes, all < 0x80; duplicates and queries longer
 * than the text are fine.
 * count: d_cnt[i] = occurrences of query i (overlapping ones count); d_lo[i] (d_lo may be NULL) = its first index in the
 * array, so sa[d_lo[i] .. d_lo[i] + d_cnt[i]) are its occurrences in array order.  With d_cnt[i] == 0, d_lo[i] is the
 * query's insertion point.
 * locate: d_out_off (count + 1 entries) = the exclusive prefix sum of the counts, always written in full, so
 * d_out_off[count] == *n_matches == the true total.  d_pos[d_out_off[i] .. d_out_off[i+1]) = base_offset + p for every
 * occurrence of query i, ASCENDING: for one query the list of bmx_search_device.  A total above `capacity` returns
 * BMX_ERR_CAPACITY; every query whose segment ends at or below capacity is then stored complete and ascending and the
 * rest of d_pos is unspecified.  capacity 0 counts only (d_pos may be NULL).  One call stores fewer than 2^31 - 1
 * positions and takes fewer than 2^31 - 1 queries (BMX_ERR_ARG beyond; pass fewer queries at a time).
 * Errors: NULL pointers where count > 0, n == 0 or n >= 2^31 and an index of another context return BMX_ERR_ARG before
 * any HIP call, with ctx = NULL too; count == 0 returns BMX_OK and launches nothing (*n_matches = 0,
 * d_out_off untouched).  The host entry checks offsets, lengths and bytes on the host.  The device entries check them in
 * the kernel: a lane that finds a decreasing offset, an end past pat_bytes, a length of 0 or above BMX_MAX_PATTERN, or
 * a byte >= 0x80 reads no text and raises a status word; the call then returns BMX_ERR_ARG (BMX_ERR_DOMAIN for the
 * byte) and the outputs are unspecified.
 * No text or query byte is read except as part of the aligned 8-byte word that holds it.
 * All device work goes on `stream` (NULL = the null stream); the calls return after synchronising it (locate also once
 * in between, to read the total). */
typedef struct bmx_index bmx_index;
int bmx_index_create_device(bmx_ctx *ctx, const void *d_text, uint64_t n, const int32_t *d_sa /* NULL: built here and owned */,
                            void *stream, bmx_index **out);
void bmx_index_destroy(bmx_index *ix);
/* The array the index searches (the caller's, or the one built here): n int32 in device memory. */
int bmx_index_sa(const bmx_index *ix, const int32_t **d_sa_out);
int bmx_index_count_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                           uint64_t count, uint32_t *d_lo /* may be NULL */, uint32_t *d_cnt, void *stream);
int bmx_index_locate_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                            uint64_t count, uint64_t base_offset, uint64_t *d_out_off /* count + 1 */, uint64_t *d_pos,
                            uint64_t capacity, uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out (upload, bmx_index_create_device, bmx_index_count_device, download, destroy). */
int bmx_index_count(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes,
                    const uint64_t *pat_off, uint64_t count, uint32_t *cnt);
/* The same for bmx_index_locate_device with base_offset 0 (what bmx_cli --index-count prints comes through it). */
int bmx_index_locate(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes,
                     const uint64_t *pat_off, uint64_t count, uint64_t *out_off /* count + 1 */, uint64_t *pos, uint64_t capacity,
                     uint64_t *n_matches);
/* Matching statistics and seeds: what read seeding needs when the whole query does not occur (a 150-byte read with one
 * substitution has a count of 0).  Index, text and query column are those of bmx_index_count_device.
 * match: entry b of each output belongs to blob byte b.  For byte b of query q, at position i = b - off[q] with
 * m = off[q+1] - off[q]: d_len[b] = the largest l <= m - i such that query[i .. i+l) occurs in the text (p + l <= n, plain
 * byte equality; the match never runs into the next query); 0 if query[i] occurs nowhere.  d_lo[b], d_cnt[b] (either may
 * be NULL) = the interval of the array whose suffixes begin with query[i .. i+len): cnt occurrences, sa[lo .. lo+cnt)
 * their starts; both 0 with len 0.  Within a query len[b+1] >= len[b] - 1.  Entries of blob bytes outside every query
 * (b < off[0] or b >= off[count]) are left untouched.
 * seeds: position i of query q is a seed for (min_len, max_occ) iff len >= min_len, and i == 0 or len[i-1] <= len[i] (the
 * match is not contained in the match of the position before it, hence in none of that query: the query's super-maximal
 * exact matches, each maximal in the text in both directions), and max_occ == 0 or cnt <= max_occ (a dropped seed is
 * not replaced by anything).  d_seed_off (count + 1 entries) = the exclusive prefix sum of the seeds per query, always
 * written in full, so d_seed_off[count] == *n_seeds == the true total.  The seeds are listed in order of (query,
 * position) as four parallel arrays of `capacity` entries: position in the query, len, lo, cnt.  capacity 0 counts only
 * (the four pointers may be NULL).  A total above `capacity` returns BMX_ERR_CAPACITY with the first `capacity` seeds of
 * that order stored.  The list is the same in every run (no atomics).  The text positions of a seed are
 * sa[lo .. lo+cnt) of bmx_index_sa, in array order.
 * One call takes fewer than 2^31 - 1 blob bytes and fewer than 2^31 - 1 queries (BMX_ERR_ARG beyond).
 * Errors: NULL pointers where count > 0, min_len == 0 and an index of another context return BMX_ERR_ARG before any HIP
 * call, with ctx = NULL too (the host entries: n == 0 or n >= 2^31 as well); count == 0 returns BMX_OK and launches
 * nothing (*n_seeds = 0).  Offsets, lengths and bytes are checked as by count: on the host by the host entries, in the
 * kernel by the device entries (a bad lane reads neither text nor array; BMX_ERR_ARG, or BMX_ERR_DOMAIN for a byte >=
 * 0x80; outputs unspecified).  All device work goes on `stream`; the calls return after synchronising it, once. */
int bmx_index_match_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes,
                           const uint64_t *d_pat_off, uint64_t count, uint32_t *d_len /* pat_bytes entries */,
                           uint32_t *d_lo /* may be NULL */, uint32_t *d_cnt /* may be NULL */, void *stream);
int bmx_index_seeds_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes,
                           const uint64_t *d_pat_off, uint64_t count, uint32_t min_len, uint32_t max_occ /* 0: no limit */,
                           uint64_t *d_seed_off /* count + 1 */, uint32_t *d_qpos, uint32_t *d_len, uint32_t *d_lo,
                           uint32_t *d_cnt, uint64_t capacity, uint64_t *n_seeds, void *stream);
/* Host buffers in, host buffers out, an index built for the call (len, lo, cnt: pat_bytes entries; lo, cnt may be NULL). */
int bmx_index_match(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes,
                    const uint64_t *pat_off, uint64_t count, uint32_t *len, uint32_t *lo, uint32_t *cnt);
/* The same for bmx_index_seeds_device (what bmx_cli --index-seeds prints comes through it). */
int bmx_index_seeds(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes,
                    const uint64_t *pat_off, uint64_t count, uint32_t min_len, uint32_t max_occ, uint64_t *seed_off,
                    uint32_t *qpos, uint32_t *len, uint32_t *lo, uint32_t *cnt, uint64_t capacity, uint64_t *n_seeds);
/* Read mapping: seeds extended to alignments within k edits, one (start, end, distance) per read.
 * Index, text and query column are those of bmx_index_seeds_device; min_len >= 1, 1 <= max_occ (0 is BMX_ERR_ARG here: an
 * unbounded seed is never extended), 0 <= k <= BMX_MAP_MAX_K.
 * Candidates: the seeds of (min_len, max_occ) are exactly those of bmx_index_seeds_device, in its order.  For every seed
 * (q, i, len, lo, cnt) and every t in [0, cnt) there is one candidate: its occurrence is p = sa[lo + t], its diagonal
 * d = p - i (signed).  Candidates are listed in order of (query, seed, t) and are NOT de-duplicated: two seeds of a read
 * on one diagonal give two candidates, so that the list is literal and the same in every run (no atomics).  d_cand_off
 * (count + 1 entries, may be NULL) = the exclusive prefix sum of the candidates per query, always written in full.
 * Window of a candidate, with m the query's length: [w0, w1) = [max(0, d - k), min(n, d + m + k)).  Every alignment of the
 * whole query with at most k edits that contains the seed's exact match lies inside it.
 * Hit of a candidate: with D(j) = min over s >= w0 of ED(query, text[s..j]) for every j of the window (what
 * bmx_search_approx defines on the view text[w0..w1)), dist = the minimum of D, end = the LARGEST j that attains it,
 * start = the LARGEST s >= w0 with ED(query, text[s..end]) == dist (the rule of bmx_approx_spans_device on that view).
 * The candidate is a hit iff dist <= k; otherwise dist = BMX_MAP_NO_HIT and both positions are BMX_MAP_NO_POS.  Positions
 * go out as base_offset + position, into three parallel lists of `capacity` entries.
 * Per query: among its hits the one with the smallest (dist, end) goes to d_best_start[q], d_best_end[q], d_best_dist[q]
 * (count entries each); a query without a seed or without a hit gets NO_POS, NO_POS, NO_HIT.
 * *n_candidates is the true total.  A total above a non-zero `capacity` returns BMX_ERR_CAPACITY with the first
 * `capacity` candidates of the order stored; the per-query results are complete either way.  capacity == 0 (the three
 * list pointers may be NULL) never returns BMX_ERR_CAPACITY: the per-query answer is the product.  A total above
 * BMX_MAP_MAX_CANDIDATES returns BMX_ERR_ARG: pass fewer queries at a time or a smaller max_occ.
 * Errors: NULL pointers where count > 0, min_len == 0, max_occ == 0, k outside [0, BMX_MAP_MAX_K] and an index of another
 * context return BMX_ERR_ARG before any HIP call, with ctx = NULL too (the host entry: n == 0 or n >= 2^31 as well);
 * count == 0 returns BMX_OK and launches nothing (*n_candidates = 0).  Offsets, lengths and bytes are checked as by
 * seeds.  All device work goes on `stream`; the call waits for it once in between, to read the candidate total and the
 * longest query that has a seed, and once at the end.  No text byte is read except as part of the aligned 8-byte word
 * that holds it, and none outside the candidate's window's words. */
#define BMX_MAP_MAX_K 64
#define BMX_MAP_NO_HIT 255u
#define BMX_MAP_NO_POS UINT64_MAX
#define BMX_MAP_MAX_CANDIDATES (1ull << 27)
int bmx_index_map_device(bmx_ctx *ctx, const bmx_index *ix, const void *d_pat, uint64_t pat_bytes, const uint64_t *d_pat_off,
                         uint64_t count, uint32_t min_len, uint32_t max_occ, int32_t k, uint64_t base_offset,
                         uint64_t *d_best_start, uint64_t *d_best_end, uint8_t *d_best_dist /* count entries each */,
                         uint64_t *d_cand_off /* count + 1, may be NULL */, uint64_t *d_cand_start, uint64_t *d_cand_end,
                         uint8_t *d_cand_dist /* `capacity` entries each, may be NULL iff capacity == 0 */, uint64_t capacity,
                         uint64_t *n_candidates, void *stream);
/* Host buffers in, host buffers out, an index built for the call, base_offset 0 (what bmx_cli --index-map prints comes
 * through it). */
int bmx_index_map(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const void *pat, uint64_t pat_bytes,
                  const uint64_t *pat_off, uint64_t count, uint32_t min_len, uint32_t max_occ, int32_t k, uint64_t *best_start,
                  uint64_t *best_end, uint8_t *best_dist, uint64_t *cand_off /* may be NULL */, uint64_t *cand_start,
                  uint64_t *cand_end, uint8_t *cand_dist, uint64_t capacity, uint64_t *n_candidates);
/* Candidates of the last bmx_index_map_device on ctx (the true total); < 0 if none. */
int64_t bmx_last_index_map_candidates(bmx_ctx *ctx);
/* Where the last bmx_index_map_device on ctx spent its device time (ms, HIP events): out[0] candidate expansion (match
 * kernel, scan, fill), out[1] verification, out[2] start pass, out[3] per-query best; out[4] = the 64-bit words of the
 * instance that ran (0: no candidate).  BMX_ERR_ARG if there was no such call.  For tools/index_map_rate.py. */
int bmx_last_index_map_phases(bmx_ctx *ctx, float out[5]);
/* Device time (ms, HIP events around the query kernels) of the last count / locate / match / seeds / map call on ctx; < 0
 * if none. */
float bmx_last_index_ms(bmx_ctx *ctx);
/* Device time (ms) of the index's creation: the suffix array if it was built here, plus the directory. */
float bmx_index_build_ms(const bmx_index *ix);

/* ---- alignments: a CIGAR for every approximate match and mapped read ------- */

/* What says HOW a pattern lies in a span that bmx_approx_spans_device or bmx_index_map_device reported: which bytes are
 * equal, substituted, inserted or deleted.  The reference has no such program.
 *
 * Inputs.  The text is resident: d_text holds n bytes, text byte 0 is global position base_offset.  The patterns are one
 * string column in the Arrow layout of bmx_edit_distance_batch_device (a byte blob plus pat_count + 1 non-decreasing
 * uint64 offsets); bytes may have any value, each pattern has 1 .. BMX_ALIGN_MAX_PATTERN bytes.  Entry e aligns pattern
 * pid[e] against the span text[s..j] with d_start[e] = base_offset + s and d_end[e] = base_offset + j, the end INCLUSIVE,
 * as the spans and map entries report it.  With d_pid == NULL, pat_count is `count` (entry e takes pattern e) or 1 (every
 * entry takes pattern 0), the a_count convention of the batched edit distance.  So best_start / best_end of
 * bmx_index_map_device go in unchanged with pat_count == count, and the lists of bmx_approx_spans_device with
 * pat_count == 1.
 * Result.  D[i][t] = ED(pat[0..i), span[0..t)) is the plain unit-cost table, m the pattern's length, L the span's.
 * d_dist[e] (d_dist may be NULL) = D[m][L], the GLOBAL distance of the whole pattern against the whole span.  The script
 * is the walk from (m, L) back to (0, 0) that takes at each cell the first of these steps that keeps the value:
 * diagonal ('=' if the two bytes are equal, else 'X'), up ('I': a pattern byte with no text byte), left ('D': a text byte
 * with no pattern byte).  It is written from the start of the span to its end with equal neighbouring ops merged into
 * runs, one op word per run: run length << 4 | code, the BAM encoding.  That puts gaps as far left as they can go, and it
 * makes ONE script per span, so results compare bit for bit.  A script with d edits has at most 2d + 1 runs.
 * abcd / abxd: 2=1X1=.  abcd / acd: 1=1I2=.  abcd / abccd: 2=1D2=.  AAA / AA: 1I2=.  GATTACA / GCATGCA: 1=2X1=1X2=.
 * No alignment.  An entry with start == end == BMX_MAP_NO_POS (a read without a hit), with |L - m| > k (answered without
 * reading a byte) or with D[m][L] > k gets dist = BMX_ALIGN_NONE and an empty script.  These are not errors.
 * Output.  d_op_off (count + 1 entries) = the exclusive prefix sum of the runs per entry, always written in full, so
 * d_op_off[count] == *n_ops == the true total; d_ops[d_op_off[e] .. d_op_off[e+1]) is entry e's script.  A total above a
 * non-zero `capacity` returns BMX_ERR_CAPACITY; every entry whose segment ends at or below capacity is then stored
 * complete and the rest of d_ops is unspecified (the rule of bmx_index_locate_device).  capacity 0 counts only (d_ops may
 * be NULL).  The output is the same in every run: no atomics decide anything.
 * Domain and errors.  0 <= k <= BMX_ALIGN_MAX_K, n < 2^40, any alignment of d_text.  NULL pointers where count > 0, k out
 * of range and, with d_pid == NULL, a pat_count that is neither 1 nor count return BMX_ERR_ARG before any HIP call, with
 * ctx == NULL too; count == 0 returns BMX_OK and launches nothing (*n_ops = 0).  The host entry checks offsets, lengths,
 * pids and positions on the host.  The device entry checks them in the kernel: an entry with pid >= pat_count, offsets
 * that decrease or end past pat_bytes, a pattern of 0 or more than BMX_ALIGN_MAX_PATTERN bytes, a position outside
 * [base_offset, base_offset + n), end < start, or exactly one of the two positions equal to BMX_MAP_NO_POS reads neither
 * pattern nor text and raises a status word; the call then returns BMX_ERR_ARG and the outputs are unspecified.
 * No text byte is read except inside the aligned 8-byte words that hold the span.
 * Method (csrc/bmx_align_kernel.h): one entry per lane; Myers' bit-parallel column in its global form over the span;
 * every column leaves two bits per row in workspace (the diagonal step keeps the value; the bytes are equal, or else the
 * up step keeps it); the same lane walks back from (m, L) on those bits alone, several columns per load; runs collected
 * per entry, rocPRIM's exclusive scan, a fill pass.  The longest pattern M of the column picks the instance: a 32-bit
 * word, or 1, 2, 4 or 8 64-bit words, w = 4, 8, 16, 32 or 64 bytes per column and plane.  A walk of at most k edits stays
 * on rows |i - t| <= k; where that band is narrower than the words (M > 32, k <= 63 and b = 4 ceil((2k + 1) / 32) < w)
 * only the band is stored, b bytes per column and plane.
 * Workspace: per entry 8 ceil((M + k) / 8) columns x 2 min(w, b) bytes, plus 2k + 2 32-bit words.  It lives behind bmx_ctx
 * like the other features', is grown on demand and kept.  A call that would need more than BMX_ALIGN_WORKSPACE_BYTES runs
 * its entries in launches of as many whole waves as fit; the lists still come out as one.
 * All device work goes on `stream`; the call waits for it once in between, to read the longest pattern, and once at the
 * end.
 *
 * bmx_align: host buffers, base_offset as given.  Uploads text, column and lists, calls bmx_align_device with room for
 * every possible run and downloads; `capacity` is the room in ops.
 *
 * Measured on one MI355X: DESIGN.md s24. */
#define BMX_ALIGN_MAX_PATTERN 512
#define BMX_ALIGN_MAX_K 254
#define BMX_ALIGN_NONE 255u /* no alignment within k (== BMX_MAP_NO_HIT) */
#define BMX_CIGAR_INS 1u    /* pattern byte with no text byte   (SAM I) */
#define BMX_CIGAR_DEL 2u    /* text byte with no pattern byte   (SAM D) */
#define BMX_CIGAR_EQ 7u     /* bytes equal                      (SAM =) */
#define BMX_CIGAR_X 8u      /* bytes differ                     (SAM X) */
#define BMX_ALIGN_WORKSPACE_BYTES (1ull << 30)
int bmx_align_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const void *d_pat, uint64_t pat_bytes,
                     const uint64_t *d_pat_off, uint64_t pat_count, const uint32_t *d_pid /* may be NULL */,
                     const uint64_t *d_start, const uint64_t *d_end, uint64_t count, int32_t k, uint8_t *d_dist /* may be NULL */,
                     uint64_t *d_op_off /* count + 1 */, uint32_t *d_ops, uint64_t capacity, uint64_t *n_ops, void *stream);
int bmx_align(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, uint64_t base_offset, const void *pat,
              uint64_t pat_bytes, const uint64_t *pat_off, uint64_t pat_count, const uint32_t *pid /* may be NULL */,
              const uint64_t *start, const uint64_t *end, uint64_t count, int32_t k, uint8_t *dist /* may be NULL */,
              uint64_t *op_off /* count + 1 */, uint32_t *ops, uint64_t capacity, uint64_t *n_ops);
/* Device time (ms, HIP events around the reduction and around the launches) of the last bmx_align_device on ctx; < 0 if
 * none. */
float bmx_last_align_ms(bmx_ctx *ctx);
/* Launches of the alignment kernel in the last bmx_align_device on ctx (more than 1: the entries did not fit the
 * workspace at once); < 0 if none. */
int64_t bmx_last_align_launches(bmx_ctx *ctx);

/* ---- row-wise results: lines of a text, the row of each match, the matching rows ---- */

/* Every search returns byte offsets into one text.  These three post-passes turn such lists into rows -- the lines of a
 * log (grep -n, -c, -v) or the strings of a column (str.contains, str.count) -- on device-resident lists, with no atomics
 * on the output and no sort.  The reference has no such program.
 *
 * Rows.  rows + 1 ascending uint64_t offsets off[0..rows], in the coordinates of the match lists (base_offset included).
 * Row r is the byte range [off[r], off[r+1]).  Empty rows are legal where the caller supplies the offsets.  Bytes below
 * off[0] or at or above off[rows] belong to no row.
 * Split at a delimiter byte d.  off[0] = base_offset, off[i] = base_offset + (position of the i-th d) + 1, off[rows] =
 * base_offset + n.  A row therefore holds its terminating delimiter as its last byte, a text that ends with d has no
 * extra empty row behind it (wc -l), n = 0 gives rows = 0 and the single entry off[0], and
 * rows = (#d) + (n > 0 && text[n-1] != d).
 * Row of a match [s, e] (e the last byte, as the searches report ends): the r with off[r] <= s and e < off[r+1], or
 * BMX_ROW_NONE where there is none: the match straddles a boundary or lies outside all rows.
 * Consequence.  The searches report every end once and the starts post-passes default to the LARGEST start of an end.
 * Some match that ends at e lies inside a row iff that largest start is >= off[r], so "ends + default starts" gives exact
 * per-row semantics.  `.` matches every byte value, the delimiter included; a match that lies inside a row can hold the
 * delimiter only as its last byte, and one that runs across a line break gets BMX_ROW_NONE.  On lines write [^\x0a]* for
 * .* (\x0a is the grammars' escape for the newline; it also keeps the star search on its one-launch path).
 *
 * bmx_rows_split_device: one pass over the n bytes at d_text (any alignment, any byte value as delim, n < 2^40), the
 * offsets written in order.  `capacity` counts entries of d_off; the call needs rows + 1.  A smaller non-zero capacity
 * stores the lowest `capacity` entries and returns BMX_ERR_CAPACITY, capacity 0 only counts and returns BMX_OK; *n_rows
 * is the true number either way.  *longest (may be NULL) is the longest row in bytes; where the offsets do not all go to
 * the caller it costs a second pass into workspace.  No byte is read outside the aligned 16-byte lines that hold the text.
 * bmx_rows_of_device: d_row[i] = the row of match i, one of three input forms: both lists and len == 0; only d_starts and
 * len >= 1 (e = s + len - 1: the exact, class and Hamming lists with len = m); only d_ends and len >= 1 (s = e - len + 1,
 * an end below len - 1 gives NONE).  A start of UINT64_MAX (the star search's "no match within the window") and an end
 * below its start give NONE.  Lists in any order are answered correctly; ascending ends, which every search returns, are
 * the fast case.  count == 0 returns BMX_OK and launches nothing.
 * bmx_rows_matching_device: from a list of row ids that is non-decreasing once BMX_ROW_NONE entries are skipped, the
 * distinct rows, ascending, in d_rows_out and (d_counts_out may be NULL) each one's number of list entries.  With
 * BMX_ROWS_INVERT the rows of [0, rows) that have NO entry; d_counts_out must then be NULL.  More rows than `capacity`
 * returns BMX_ERR_CAPACITY with the lowest `capacity` stored, *n_out the true number (capacity 0 counts only).  A list that
 * decreases, or an id >= rows other than BMX_ROW_NONE, raises a status word: BMX_ERR_ARG, outputs unspecified.
 * All three: NULL pointers where one is needed, contradictory list / len combinations, n too large and unknown flags
 * return BMX_ERR_ARG before any HIP call, with ctx == NULL too.  Every launch, copy and memset goes on `stream`; the call
 * returns after synchronising it.  Workspace is kept with the context.
 * bmx_rows_split: host buffers, base_offset 0.
 * Method (csrc/bmx_rows_kernel.h): the split compares whole 16-byte loads against the splatted delimiter, a wave reads one
 * contiguous KiB per load, the ordered output of the one-pass searches (decoupled look-back); one match per lane, each
 * wave's search bounded by the rows of its smallest and largest end; per-tile summaries, their carries and a fill.
 * Measured on one MI355X: DESIGN.md s28. */
#define BMX_ROW_NONE UINT64_MAX
#define BMX_ROWS_INVERT 1u
int bmx_rows_split_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, uint8_t delim, uint64_t *d_off,
                          uint64_t capacity, uint64_t *n_rows, uint64_t *longest /* may be NULL */, void *stream);
int bmx_rows_of_device(bmx_ctx *ctx, const uint64_t *d_off, uint64_t rows, const uint64_t *d_starts /* or NULL */,
                       const uint64_t *d_ends /* or NULL */, uint64_t len, uint64_t count, uint64_t *d_row, void *stream);
int bmx_rows_matching_device(bmx_ctx *ctx, const uint64_t *d_row, uint64_t count, uint64_t rows, uint32_t flags,
                             uint64_t *d_rows_out, uint64_t *d_counts_out /* may be NULL */, uint64_t capacity, uint64_t *n_out,
                             void *stream);
/* Device time (ms, HIP events) of the last of the three device calls on ctx; < 0 if none. */
float bmx_last_rows_ms(bmx_ctx *ctx);
int bmx_rows_split(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, uint8_t delim, uint64_t *off,
                   uint64_t capacity, uint64_t *n_rows, uint64_t *longest /* may be NULL */);
/* bmx_rows_of, bmx_rows_matching: host buffers in, host buffers out (the driver's --lines works on the host searches'
 * lists): upload, the device entry, download.  The same arguments, checks and return codes. */
int bmx_rows_of(bmx_ctx *ctx /* NULL: device 0 */, const uint64_t *off, uint64_t rows, const uint64_t *starts /* or NULL */,
                const uint64_t *ends /* or NULL */, uint64_t len, uint64_t count, uint64_t *row);
int bmx_rows_matching(bmx_ctx *ctx /* NULL: device 0 */, const uint64_t *row, uint64_t count, uint64_t rows, uint32_t flags,
                      uint64_t *rows_out, uint64_t *counts_out /* may be NULL */, uint64_t capacity, uint64_t *n_out);

/* ---- non-overlapping match selection, replace and extract on device lists ---- */

/* The searches report every end of a match, so their occurrences overlap: `aa` in `aaaa` gives three.  These post-passes
 * pick "the non-overlapping matches, left to right" from such a list (re.finditer, bytes.count), and replace the spans
 * picked by a literal (re.sub, sed s/x/y/g, str.replace) or copy them out as a string column (grep -o, re.findall).
 *
 * Spans.  [s, e], e the last byte, in the three input forms of bmx_rows_of_device: both lists and len == 0; only d_starts
 * and len >= 1; only d_ends and len >= 1.  The selection SKIPS an entry -- never takes it, never an error -- whose start
 * (or end) is UINT64_MAX, whose end is below its start or below len - 1, or for which d_row (may be NULL; what
 * bmx_rows_of_device returned for the same entries) holds BMX_ROW_NONE: so a match across a line break stays out of a
 * per-line replace.
 *
 * bmx_spans_select_device, flags 0 (disjoint).  Walk the list in its order and take an entry iff its start is greater
 * than the end of the last entry taken; the first entry that is not skipped is taken.  The list must satisfy
 * s[i] <= e[j] for all non-skipped i < j: non-decreasing ends (every search's list) do, non-decreasing starts (the
 * dictionary search's) do as well.  A violation raises a status word: BMX_ERR_ARG, outputs unspecified.  For
 * non-decreasing ends this is earliest-end-first, the largest possible set of pairwise disjoint matches; for lists of one
 * length (exact, class, Hamming) it is exactly what re.finditer / bytes.count give.  For variable-length expressions with
 * the default (largest) starts it selects LEFTMOST-SHORTEST matches: `[0-9]+` selects single digits.  POSIX
 * leftmost-longest needs the longest match per start, a search over the reversed text, which is not part of the library;
 * the rule covers such a list, which is sorted by start.
 * BMX_SELECT_MERGE.  Needs non-decreasing ends (else BMX_ERR_ARG).  The output is the connected regions of the union of the
 * spans, ascending: a region begins at entry j iff the smallest start among entries j.. exceeds the largest end among
 * entries ..j-1, and runs from that smallest start to the last end before the next cut.  Overlapping spans merge,
 * abutting spans do not.  With LONGEST starts (the smallest start of every end) the regions are the bytes that belong to
 * at least one match: `[0-9]+` yields the maximal digit runs, the redaction semantics.
 * d_index_out (may be NULL): the list index of every entry taken, with MERGE of every region's first entry.
 *
 * bmx_replace_device.  d_starts / d_ends / len: `count` ascending, pairwise disjoint spans inside
 * [base_offset, base_offset + n) (a selection's output is one).  d_out receives the n bytes at d_text with every span's
 * bytes replaced by the repl_len bytes at `repl` (host memory, 0 <= repl_len <= BMX_MAX_REPLACEMENT, a literal; with group references: bmx_expand_device):
 * n' = n - sum(span lengths) + count * repl_len bytes.  Spans that are not ascending and disjoint, or that reach outside
 * the view, raise a status word: BMX_ERR_ARG.  d_out must not overlap d_text (BMX_ERR_ARG).
 * bmx_extract_device.  The same spans; d_blob receives their bytes one after the other and d_off the count + 1 offsets into
 * it (always all of them): the column layout of bmx_edit_distance_batch and bmx_index_*.
 *
 * Capacity (entries for the selection, bytes for the other two): the true size always goes to *n_out; capacity 0 only
 * counts and returns BMX_OK; a smaller non-zero capacity stores the lowest `capacity` entries or bytes and returns
 * BMX_ERR_CAPACITY.  BMX_ERR_ARG before any HIP call, with ctx == NULL too: NULL where a pointer is needed, contradictory
 * list / len combinations, unknown flags, n >= 2^40, count >= 2^32, repl_len > BMX_MAX_REPLACEMENT.  count == 0 launches
 * nothing: the selection returns 0 entries, replace copies the text, extract writes the single offset 0.  Every launch,
 * copy and memset goes on `stream`, and the call returns after synchronising it; workspace stays with the context.  No
 * byte is read outside the aligned 16-byte lines that hold text[0..n).
 * Method (csrc/bmx_subst_kernel.h): with key = s + 1 (0: skipped) and PM its prefix maximum, the list is in order iff
 * PM[j-1] <= e[j] + 1, and the entry taken after j is the first i with PM[i] > e[j] + 1; the chain of these successors is
 * resolved by pointer jumping in tiles of T entries, level by level (no lane follows more than T pointers per level, the
 * levels grow with log_T count), then marked top down, counted and filled in order.  Replace and extract are one kernel
 * driven by the output: a lane owns aligned 16-byte lines of it, finds its piece by a search the wave bounds, and where the
 * line lies in one piece of text reads two aligned source lines, funnel-shifts them and stores 16 bytes.
 * bmx_last_subst_ms: HIP events around the launches of the last of the three; < 0 if none. */
#define BMX_SELECT_MERGE 1u
#define BMX_MAX_REPLACEMENT 65536u
int bmx_spans_select_device(bmx_ctx *ctx, const uint64_t *d_starts /* or NULL */, const uint64_t *d_ends /* or NULL */,
                            uint64_t len, uint64_t count, const uint64_t *d_row /* may be NULL */, uint32_t flags,
                            uint64_t *d_starts_out, uint64_t *d_ends_out, uint64_t *d_index_out /* may be NULL */,
                            uint64_t capacity, uint64_t *n_out, void *stream);
int bmx_replace_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_starts,
                       const uint64_t *d_ends, uint64_t len, uint64_t count, const void *repl /* host */, uint64_t repl_len,
                       void *d_out, uint64_t capacity /* bytes */, uint64_t *n_out, void *stream);
int bmx_extract_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_starts,
                       const uint64_t *d_ends, uint64_t len, uint64_t count, void *d_blob, uint64_t capacity /* bytes */,
                       uint64_t *d_off /* count + 1 */, uint64_t *n_out, void *stream);
float bmx_last_subst_ms(bmx_ctx *ctx);
/* host buffers in, host buffers out, base_offset 0: upload, the device entry, download.  The same arguments, checks and
 * return codes (an output that overlaps the text is BMX_ERR_ARG here too). */
int bmx_spans_select(bmx_ctx *ctx /* NULL: device 0 */, const uint64_t *starts /* or NULL */, const uint64_t *ends /* or NULL */,
                     uint64_t len, uint64_t count, const uint64_t *row /* may be NULL */, uint32_t flags, uint64_t *starts_out,
                     uint64_t *ends_out, uint64_t *index_out /* may be NULL */, uint64_t capacity, uint64_t *n_out);
int bmx_replace(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const uint64_t *starts, const uint64_t *ends,
                uint64_t len, uint64_t count, const void *repl, uint64_t repl_len, void *out, uint64_t capacity, uint64_t *n_out);
int bmx_extract(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const uint64_t *starts, const uint64_t *ends,
                uint64_t len, uint64_t count, void *blob, uint64_t capacity, uint64_t *off /* count + 1 */, uint64_t *n_out);

/* ---- synthetic corpus, generated in HBM ---------------------- */

/* d_dst[j] = byte (start + j) of the counter-based splitmix64 stream;
 * kind 0 = printable-95, kind 1 = ACGT. */
int bmx_gen_text_device(bmx_ctx *ctx, void *d_dst, uint64_t start, uint64_t len, uint64_t seed,
                        int kind, void *stream);
/* Copy `pat` over [off, off+m) for every off in offsets[0..count) (GLOBAL stream
 * offsets), clipped to the resident window [start, start+len).  Plants must not
 * overlap each other within one call. */
int bmx_plant_device(bmx_ctx *ctx, void *d_dst, uint64_t start, uint64_t len, const char *pat,
                     int32_t m, const uint64_t *offsets, uint64_t count, void *stream);

/* ---- leftmost-longest regex matching: every match START, and the end of every start ------- */

/* grep -o, sed s///g and awk take the leftmost start and, from it, the longest match.  The searches above report ENDS and
 * bmx_regex_starts_device one start per end, which cannot answer that: on "ab" the expression ab|b ends at 1 with the
 * starts {0, 1} and each flag keeps one of them.  The entries below are the mirror image of bmx_search_regex_device for
 * the STAR-FREE automata (valid by its rule): one pass reports every start at which some match begins, a post-pass gives
 * each start of a list its shortest or longest end, and bmx_spans_select_device's disjoint rule on the list
 * (s, longest end from s), which is sorted by s, yields exactly the leftmost-longest matches.
 *
 * The reversed automaton, pure host code, no GPU: position i becomes m - 1 - i, first and last swap, follow[] is
 * transposed (and so points upward again for a star-free automaton), the classes are mirrored; min_len and max_len are
 * kept.  text[s..j] matches `re` iff its mirror image matches `out`; applied twice it gives the input back.  Accepts
 * every automaton that bmx_search_regex_star_device accepts; BMX_ERR_ARG for NULL pointers or one that is not valid.  out
 * may be re. */
int bmx_regex_reverse(const bmx_regex *re, bmx_regex *out);
/* Semantics: every START s in [0, n - tail) for which text[s..j] matches for some j < n, each start once, ascending,
 * reported as base_offset + s.  A match must end inside the view.  A match spans at most max_len bytes, so a shard passes
 * a view that runs max_len - 1 bytes (clipped at the text's end) past its last owned start, with tail = that amount: the
 * shards' lists then concatenate to the whole text's list (the mirror of `lead`).  tail == n returns BMX_OK with no
 * match and puts nothing on the stream.
 * Two identities: the list holds every entry of bmx_regex_starts_device (either flag) over bmx_search_regex_device's
 * ends; it equals n - 1 - e over the ends e of bmx_search_regex_device on the reversed text with bmx_regex_reverse(re).
 * Any byte values in text and classes; n < 2^40, any alignment of d_text.  No byte outside the aligned 16-byte lines that
 * hold text[0..n) is read, none above the line of text[n - 1].
 * Capacity: the stored entries are the LOWEST `capacity` starts; *n_matches is the true total, and a larger total
 * returns BMX_ERR_CAPACITY (capacity 0 counts only).  Argument errors (NULL pointers where needed, an automaton that is
 * not valid -- one with a cycle is not --, tail > n, n too large) return BMX_ERR_ARG before any HIP call, with
 * ctx = NULL too.  The look-back time-out and BMX_ERR_HIP in place of a partly ordered list: as for
 * bmx_search_regex_device.  One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising
 * that stream.  The lane runs the reversed automaton DOWN the text in place (csrc/bmx_regex_begins_kernel.h): no copy of
 * the text is made. */
int bmx_search_regex_begins_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t tail, uint64_t base_offset,
                                   const bmx_regex *re, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches, void *stream);
/* Device time (ms, HIP events around the kernel) of the last bmx_search_regex_begins_device on ctx; < 0 if none. */
float bmx_last_regex_begins_ms(bmx_ctx *ctx);
/* The END of a match for every start of a device-resident list, as bmx_search_regex_begins_device returns it for the same
 * view, automaton and base_offset: d_ends[i] = base_offset + j with text[s_i..j] a match, d_starts[i] = base_offset + s_i.
 * By default j is the SMALLEST such end (the shortest match), with BMX_REGEX_LONGEST the largest j < n of the view.  One
 * list entry per lane; the lane runs the automaton anchored at s_i over at most max_len bytes upwards.
 * d_limit (NULL: the view's last byte): d_limit[i], in the coordinates of d_starts, is the last byte a match of entry i
 * may use -- the last byte of its row, say: a.{0,3}b then does not reach across a line break.  An entry from which no
 * match begins within its limit gets UINT64_MAX (bmx_spans_select_device skips such entries) and is not an error.
 * Errors: NULL pointers where needed, an automaton that is not valid, n out of range and unknown flag bits return
 * BMX_ERR_ARG before any HIP call, with ctx = NULL too; count == 0 returns BMX_OK and launches nothing.  An entry outside
 * [base_offset, base_offset + n) reads no byte and raises a status word, and so does, WITHOUT d_limit, an entry at which
 * no match begins (a list of another expression or text): the call then returns BMX_ERR_ARG and the outputs are
 * unspecified.  No byte outside the aligned 16-byte lines that hold text[0..n) is read, none above text[n - 1]'s line.
 * One kernel launch on `stream` (NULL = the null stream); the call returns after synchronising it. */
int bmx_regex_ends_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                          const uint64_t *d_starts, uint64_t count, const uint64_t *d_limit /* NULL: the view's last byte */,
                          uint32_t flags, uint64_t *d_ends, void *stream);
/* Host buffers in, host buffers out (upload, bmx_search_regex_begins_device with tail = 0, download). */
int bmx_search_regex_begins(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                            uint64_t *starts, uint64_t capacity, uint64_t *n_matches);
/* Host buffers in, host buffers out: upload, bmx_search_regex_begins_device, bmx_regex_ends_device (flags:
 * BMX_REGEX_LONGEST or 0; no limit), download.  ends[i] belongs to starts[i]; capacity and *n_matches as above. */
int bmx_search_regex_begins_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                                  uint32_t flags, uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_matches);
/* The counterpart of bmx_text_upload for a caller without the HIP runtime's headers (the driver chains the two device
 * entries above with a per-line limit): `bytes` bytes from d_src on ctx's device to dst, a blocking copy.  BMX_ERR_ARG for
 * a NULL context, or NULL pointers with bytes > 0; bytes == 0 does nothing. */
int bmx_device_download(bmx_ctx *ctx, void *dst, const void *d_src, uint64_t bytes);

/* ---- leftmost-longest matching for automata with a cycle (* + {a,}) ----------------------- */

/* The same two passes for every automaton that bmx_search_regex_star_device accepts.  The entries above
 * are unchanged and still refuse a cycle.
 * Semantics: every START s in [0, n - tail) for which text[s..j] matches for some j < n of the view, each start once,
 * ascending, reported as base_offset + s; exact for every valid automaton and every text.  A star-free automaton gives
 * bmx_search_regex_begins_device's list.  A match must end inside the view, and as on the forward side there is no halo: a
 * shard's list is a subset of the whole text's list and misses exactly the starts whose every match ends past the shard's
 * view; `tail` is the mirror of `lead`.  tail == n returns BMX_OK with no match and puts nothing on the stream.
 * How: the reversed automaton, masked to the positions a match can use, runs DOWN the text in place.  A lane walks a
 * warm-up above its starts with two states, one from the empty set and one from every position; where the two meet the lane
 * is exact, and where some lane's do not, the call drops its first list and repeats the search exactly: bounds and
 * columns per piece numbered from the top of the view, a sweep, and the search again from the swept states
 * (csrc/bmx_regex_star_begins_kernel.h).  The slow path's workspace (40 bytes per piece of 256..4,096 bytes and 8 bytes per
 * column) is made on the first such call, kept in the context and freed with it.
 * Any byte values in text and classes; n < 2^40, any alignment of d_text.  No byte outside the aligned 16-byte lines that
 * hold text[0..n) is read, none above the line of text[n - 1].
 * Capacity: the stored entries are the LOWEST `capacity` starts; *n_matches is the true total, and a larger total returns
 * BMX_ERR_CAPACITY (capacity 0 counts only).  Argument errors (NULL pointers where needed, an automaton that is not valid,
 * tail > n, n too large) return BMX_ERR_ARG before any HIP call, with ctx = NULL too.  The look-back time-out and
 * BMX_ERR_HIP in place of a partly ordered list: as for bmx_search_regex_device.  All work goes on `stream` (NULL = the
 * null stream); the call returns after synchronising that stream. */
int bmx_search_regex_star_begins_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t tail, uint64_t base_offset,
                                        const bmx_regex *re, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches,
                                        void *stream);
/* Device time (ms) of the last bmx_search_regex_star_begins_device on ctx: the one launch, or, where the call repeated the
 * search, everything from the first launch to the last; < 0 if none. */
float bmx_last_regex_star_begins_ms(bmx_ctx *ctx);
/* Host buffers in, host buffers out (upload, bmx_search_regex_star_begins_device with tail = 0, download). */
int bmx_search_regex_star_begins(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                                 uint64_t *starts, uint64_t capacity, uint64_t *n_matches);
/* The END of a match for every start of a device-resident list: bmx_regex_ends_device for an automaton that may have a
 * cycle, with `window` (1..BMX_MAX_REGEX_STAR_WINDOW) in place of max_len: d_ends[i] is the smallest, with
 * BMX_REGEX_LONGEST the largest end of a match that begins at d_starts[i] and uses at most `window` bytes, none past
 * d_limit[i] (optional) and none past the view.  A lane stops as soon as its state is empty: the run is anchored at the
 * start, so [0-9]+ reads to the end of its number and not to the end of its window.
 * An entry with no such match gets UINT64_MAX (bmx_spans_select_device skips it).  That is an error (BMX_ERR_ARG) only
 * without d_limit and for an acyclic automaton with max_len <= window, where no longer match can exist.
 * CLIPPED: an entry whose state after `window` bytes still holds a position with a successor, where neither its limit nor
 * the view's end would have stopped it, may have a longer match than the one reported (the next byte is not looked at: a
 * run of [0-9]+ that fills the window exactly counts).  *n_clipped (may be NULL) is the number of such
 * entries; a caller that needs the POSIX answer treats a non-zero count as a failure or repeats with a larger window.
 * Other errors, the rule for entries outside the view, the bytes read and the stream rule: bmx_regex_ends_device's, with
 * the validity rule of bmx_search_regex_star_device and window out of range among the argument errors. */
int bmx_regex_star_ends_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                               const uint64_t *d_starts, uint64_t count, const uint64_t *d_limit /* NULL: the view's last byte */,
                               uint32_t window, uint32_t flags, uint64_t *d_ends, uint64_t *n_clipped /* NULL: not wanted */,
                               void *stream);
/* Host buffers in, host buffers out: upload, bmx_search_regex_star_begins_device, bmx_regex_star_ends_device (flags:
 * BMX_REGEX_LONGEST or 0; no limit), download.  ends[i] belongs to starts[i]; capacity and *n_matches as above. */
int bmx_search_regex_star_begins_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                                       uint32_t window, uint32_t flags, uint64_t *starts, uint64_t *ends, uint64_t capacity,
                                       uint64_t *n_matches, uint64_t *n_clipped /* NULL: not wanted */);

/* ---- anchored regular-expression search: ^ $ \b \B \< \>, whole word, whole line ------------- */

/* ^ERROR, timeout$, \bcat\b, grep -w, grep -x for the STAR-FREE expressions (csrc/bmx_regex_anchored_kernel.h, DESIGN.md
 * s32).  A caller cannot build these from the entries above: the searches report an end once while several starts share
 * it, so a filter over the finished list by "the byte before the start" has no start to look at, and the starts pass
 * keeps one start per end.  The condition sits in the automaton's step instead.
 *
 * The model is plain data beside an unchanged bmx_regex: a class of admissible bytes BEFORE the match for every position
 * of `first`, a class of admissible bytes AFTER it for every position of `last` (encoded as for bmx_search_classes).
 * text[s..j] is an ANCHORED match iff it is a match by bmx_regex's definition along a path i_0 .. i_{L-1} and prev(s) is in
 * before[i_0] and next(j) is in after[i_{L-1}], where prev(s) = text[s - 1], or the call's `left` byte when s == 0, and
 * next(j) = text[j + 1], or the call's `right` byte when j == n - 1.  left and right are byte values 0..255: a caller with
 * the whole text passes 0x0A for both (outside the text counts as a line break), a shard passes the real neighbour; no
 * entry reads a byte outside the view for them.  A full class is "no condition", an empty one is legal ("no match begins /
 * ends at this position"), so every struct goes with a valid bmx_regex.  The gate applies where a path enters through
 * `first` or leaves through `last`, not where the same position is reached through follow[]: ^a?b and ^a|b$ come out right.
 * With every class full each entry below returns exactly the list of its unanchored counterpart. */
typedef struct bmx_regex_anchors {
    uint8_t before[BMX_MAX_REGEX_POSITIONS * BMX_CLASS_BYTES]; /* read for positions in `first` only */
    uint8_t after [BMX_MAX_REGEX_POSITIONS * BMX_CLASS_BYTES]; /* read for positions in `last` only  */
} bmx_regex_anchors;
#define BMX_REGEX_WORD 4u /* grep -w: no word byte before the match and none after it */
#define BMX_REGEX_LINE 8u /* grep -x: a line break before the match and one after it   */
/* bmx_compile_regex's grammar (star-free) plus the zero-width atoms ^ $ \b \B \< \> outside sets; \^ and \$ are literals.
 * With W = [A-Za-z0-9_] they mean what Python's re means on bytes with re.MULTILINE:
 *   ^  the previous byte is \n            $  the next byte is \n
 *   \b exactly one of the previous and the next byte is in W      \B both or neither
 *   \< the previous byte is not in W, the next is                 \> the previous byte is in W, the next is not
 * BMX_REGEX_WORD intersects ~W into every `before` of `first` and every `after` of `last`, BMX_REGEX_LINE does the same with
 * {\n}; BMX_CLASS_ICASE and BMX_CLASS_IUPAC as in bmx_compile_regex.
 * Several conditions at one boundary intersect, several ways into one first position unite.  A condition that depends on
 * the match's own edge byte (\b in front of [a-z.]) splits that position into copies by the kind of byte (line break,
 * word byte, other), each with its own `before` or `after` class and the same follow sets, numbered upward.  An assertion
 * between two consumed positions is decided from their two classes: the edge stays if it holds for every byte pair and
 * goes if it holds for none.  The result is exact or the call fails; it never approximates.
 * BMX_ERR_ARG with a text in bmx_last_error and *re, *an untouched: every error of bmx_compile_regex; a quantifier on an
 * assertion (^*, \b?, ${2}); an expression that matches the empty string once assertions are ignored (^, ^$, \b); an
 * assertion between two positions that their classes do not decide ([a-z.]\b[a-z.]); more than 64 positions after
 * splitting; an expression left with no possible match (a\bb).
 * For an expression without assertions and without the two flags *re equals bmx_compile_regex's output byte for byte and
 * every class of *an is full.  Pure host code, no GPU. */
int bmx_compile_regex_anchored(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *re, bmx_regex_anchors *an);
/* Every END of an anchored match in [lead, n): semantics, capacity rule, argument errors before any HIP call (left or right
 * above 255 among them), stream rule and wait bound as bmx_search_regex_device.  The shard contract is unchanged: a view
 * begins max_len - 1 bytes before the first owned end, left and right are the bytes next to the VIEW, and the shards'
 * lists concatenate to the whole text's list.  One small copy (the two gate tables) and one kernel launch on `stream`. */
int bmx_search_regex_anchored_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                     const bmx_regex *re, const bmx_regex_anchors *an, uint32_t left, uint32_t right,
                                     uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, void *stream);
/* Device time (ms) of the last bmx_search_regex_anchored_device on ctx; < 0 if none. */
float bmx_last_regex_anchored_ms(bmx_ctx *ctx);
/* The START of an anchored match for every end of a list: bmx_regex_starts_device with the two conditions (the largest
 * start by default, the smallest with BMX_REGEX_LONGEST).  Errors, status word, bytes read and stream rule as there. */
int bmx_regex_anchored_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                     const bmx_regex_anchors *an, uint32_t left, uint32_t right, const uint64_t *d_ends,
                                     uint64_t count, uint32_t flags, uint64_t *d_starts, void *stream);
/* Every START of an anchored match in [0, n - tail), ascending: bmx_search_regex_begins_device with the two conditions. */
int bmx_search_regex_anchored_begins_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t tail, uint64_t base_offset,
                                            const bmx_regex *re, const bmx_regex_anchors *an, uint32_t left, uint32_t right,
                                            uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches, void *stream);
float bmx_last_regex_anchored_begins_ms(bmx_ctx *ctx);
/* The END of an anchored match for every start of a list: bmx_regex_ends_device with the two conditions.  d_limit bounds
 * the bytes a match may USE; the byte after a match that ends on its limit is still the text's. */
int bmx_regex_anchored_ends_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                   const bmx_regex_anchors *an, uint32_t left, uint32_t right, const uint64_t *d_starts,
                                   uint64_t count, const uint64_t *d_limit /* NULL: the view's last byte */, uint32_t flags,
                                   uint64_t *d_ends, void *stream);
/* Host buffers in, host buffers out, with left = right = 0x0A; otherwise as their unanchored counterparts.  ctx may be NULL. */
int bmx_search_regex_anchored(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                              const bmx_regex_anchors *an, uint64_t *ends, uint64_t capacity, uint64_t *n_matches);
int bmx_search_regex_anchored_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                                    const bmx_regex_anchors *an, uint32_t flags, uint64_t *starts, uint64_t *ends,
                                    uint64_t capacity, uint64_t *n_matches);
int bmx_search_regex_anchored_begins(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                                     const bmx_regex_anchors *an, uint64_t *starts, uint64_t capacity, uint64_t *n_matches);
int bmx_search_regex_anchored_begins_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                                           const bmx_regex_anchors *an, uint32_t flags, uint64_t *starts, uint64_t *ends,
                                           uint64_t capacity, uint64_t *n_matches);

/* ---- regular-expression search for expressions of up to 128 positions ---------------------- */

/* a.{0,100}b, ATG([ACGT]{3}){2,40}(TAA|TAG|TGA), a PROSITE motif with x(20,40), a list of ten keywords in front of a
 * counted class: counted repeats and keyword lists pass 64 positions quickly, and a.{0,100}b cannot be split into two
 * searches at all.  The entries below are bmx_search_regex_device and bmx_regex_starts_device for the STAR-FREE
 * expressions of up to 128 positions: the same recurrence on a state of four dwords per lane, the automaton's tables in a
 * device buffer of the context instead of the kernel arguments (csrc/bmx_regex_long_kernel.h).  The
 * 64-position entries above and struct bmx_regex are unchanged.
 *
 * The automaton is struct bmx_regex with sets of two words: position i is bit (i & 63) of word (i >> 6).  text[s..j] of
 * length L >= 1 MATCHES iff there are positions i_0, .., i_{L-1} with i_0 in `first`, i_{t+1} in follow[i_t], i_{L-1} in
 * `last` and text[s + t] in class i_t for every t.
 * Valid: 1 <= m <= BMX_MAX_REGEX_LONG_POSITIONS; first and last non-empty; no bit at or above m in first, last or any
 * follow[i]; follow[i] holds only bits j > i (acyclic, max_len <= m).  Empty classes and positions that no match can use
 * are legal.  The entries recompute min_len and max_len and do not read the two fields or `pad`. */
#define BMX_MAX_REGEX_LONG_POSITIONS 128
typedef struct bmx_regex_long {
    int32_t  m;                 /* positions, 1..128, numbered left to right after expansion */
    int32_t  min_len, max_len;  /* shortest / longest match in bytes; filled by bmx_compile_regex_long */
    int32_t  pad;               /* 0 */
    uint64_t first[2], last[2]; /* bit (i & 63) of word (i >> 6): position i */
    uint64_t follow[BMX_MAX_REGEX_LONG_POSITIONS][2];  /* follow[i]: the positions that may come right after i */
    uint8_t  classes[BMX_MAX_REGEX_LONG_POSITIONS * BMX_CLASS_BYTES];  /* as for bmx_search_classes */
} bmx_regex_long;
/* bmx_compile_regex's grammar, flags and errors with the limit at 128 positions (unbounded repetition is still refused);
 * error texts begin with "bmx_compile_regex_long: " and *out is untouched on error.  For an expression of at most 64
 * positions first[0], last[0], follow[i][0], classes, m, min_len and max_len equal bmx_compile_regex's output and the
 * high words are 0.  Pure host code, no GPU. */
int bmx_compile_regex_long(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex_long *out);
/* The same automaton in the wide struct (pure host code).  BMX_ERR_ARG for NULL or an `in` that is not valid for
 * bmx_search_regex_device. */
int bmx_regex_long_widen(const bmx_regex *in, bmx_regex_long *out);
/* bmx_search_regex_device for a bmx_regex_long: every END j in [lead, n) at which some match ends, each once, ascending,
 * reported as base_offset + j; the halo of a shard is max_len - 1 bytes; the capacity rule, n < 2^40, any alignment of
 * d_text, BMX_ERR_HIP in place of a partly ordered list and the argument errors before any HIP call (with ctx = NULL too)
 * are that entry's.  Any m in 1..128 is accepted, and for m <= 64 the list equals bmx_search_regex_device's.  An
 * automaton in which no position of `last` can be reached returns an empty list without a launch.  One copy of the
 * automaton's tables (6 KiB) and one kernel launch on `stream` (NULL = the null stream); the call returns after
 * synchronising that stream. */
int bmx_search_regex_long_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                 const bmx_regex_long *re, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, void *stream);
/* Host buffers in, host buffers out (upload, bmx_search_regex_long_device with lead = 0, download). */
int bmx_search_regex_long(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex_long *re,
                          uint64_t *ends, uint64_t capacity, uint64_t *n_matches);
/* Device time (ms, HIP events around the kernel) of the last bmx_search_regex_long_device on ctx; < 0 if none. */
float bmx_last_regex_long_ms(bmx_ctx *ctx);
/* bmx_regex_starts_device for a bmx_regex_long: the START of a match for every end of a device-resident list, the largest
 * one by default (the shortest match), with BMX_REGEX_LONGEST the smallest one of the view.  Status word, errors,
 * count == 0, the bytes read and the stream rule are exactly that entry's. */
int bmx_regex_long_starts_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex_long *re,
                                 const uint64_t *d_ends, uint64_t count, uint32_t flags, uint64_t *d_starts, void *stream);
/* Host buffers in, host buffers out: upload, bmx_search_regex_long_device, bmx_regex_long_starts_device, download. */
int bmx_search_regex_long_spans(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex_long *re,
                                uint32_t flags, uint64_t *starts, uint64_t *ends, uint64_t capacity, uint64_t *n_matches);

/* ---- regex capture groups: the group spans of every match, templates in the replacement ---- */

/* \3.\2.\1 on ([0-9]{4})-([0-9]{2})-([0-9]{2}), the code of (ERROR|FATAL): ([0-9]{2,4}) as a column, sed 's/\(..\)\(..\)/\2\1/g':
 * a post-pass over a device-resident span list, one entry per lane (csrc/bmx_regex_groups_kernel.h), and a
 * template where bmx_replace_device takes a literal.  For the STAR-FREE 64-position expressions; struct bmx_regex and every
 * entry above are unchanged.  The reference has no such program.
 *
 * The model is plain data beside an unchanged bmx_regex.  It is what Python's `re` (bytes, DOTALL) returns as
 * fullmatch(text, s, e + 1).regs.  For a span text[s..e], L = e - s + 1, that matches by bmx_regex's definition:
 *   - the PREFERRED PATH i_0 .. i_{L-1} takes at every step t the first q in pref[previous] (the row of i_0 is
 *     BMX_REGEX_START) such that text[s + t] is in the class of q and from q the rest of the span can still be consumed,
 *     ending in `last` exactly at e;
 *   - all groups begin unset; at every boundary t = 0..L the transition from the previous position (or START) to i_t (or
 *     BMX_REGEX_END) fires its tags: the bits of open[from][to] set begin[g] = s + t, those of close[from][to] set
 *     end[g] = s + t.  The last writer wins and nothing is reset between the copies of a repeat, so ((a)|b){2} on "ab"
 *     keeps group 2 = "a", as Python does;
 *   - group spans are HALF-OPEN [begin, end), because a group can be empty (unlike the library's inclusive match ends);
 *     group 0 is [s, e + 1).
 * Valid (bmx_regex_groups_valid): re is valid; 0 <= n_groups <= 16; every row p < m of pref lists exactly the positions of
 * follow[p], each once, and row BMX_REGEX_START those of `first`, the rest of the row 0xFF; tag bits lie below n_groups
 * and stand only on pairs (p, q) with q in follow[p], (START, q) with q in first and (p, END) with p in last. */
#define BMX_MAX_REGEX_GROUPS 16
#define BMX_REGEX_START 64   /* row: before the first byte of the match */
#define BMX_REGEX_END   64   /* column: after its last byte             */
typedef struct bmx_regex_groups {
    int32_t  n_groups;        /* 0..16, numbered from 1 by their '(' left to right */
    uint8_t  pref[65][64];    /* row p (row 64: START): the positions of follow[p] (row 64: of first), most preferred
                                 first, the rest of the row 0xFF */
    uint16_t open[65][65];    /* [from][to], bit g-1: group g begins at the boundary between `from` and `to` */
    uint16_t close[65][65];   /*                      group g ends there */
} bmx_regex_groups;
/* Pure host code, no GPU.  bmx_compile_regex's grammar with two changes: ( ... ) captures and (?: ... ) groups without
 * capturing ((?: stays an error in every other compile entry).  *re equals, byte for byte, what bmx_compile_regex gives for
 * the same expression with every (?: written as (, so every search, starts, begins and ends entry works on it unchanged.
 * The preference order and the tags come from the expression tree alone: counted repeats expand to a copies and b - a
 * optional ones (all copies of a group share its bit); the epsilon moves are walked depth first in the order a
 * backtracking matcher tries them (an alternation left to right, an optional copy before its skip), and the first epsilon
 * path that reaches a consuming position, or END, gives that pair's rank and tags.  This is NOT the ascending position
 * index: (a?|[bc])([bc]?)c on "bc" gives ((0,2),(0,0),(0,1)).
 * BMX_ERR_ARG, outputs untouched, a text in bmx_last_error that begins "bmx_compile_regex_groups: ": every error of
 * bmx_compile_regex; (? followed by anything but :; more than BMX_MAX_REGEX_GROUPS capturing groups; a repeat with b >= 2
 * whose body can match the empty string and contains, or is, a capturing group ((a?){2}, ((a)|b?){1,3}, (){3}): engines
 * disagree on such captures, so they are exact or refused, never approximated.  (a?)?, ((a?)b){2} and (a|b?)c are fine.
 * Out of scope: back-references inside the expression; captures for the star, anchored and 128-position families; lazy
 * quantifiers; named groups. */
int bmx_compile_regex_groups(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *re, bmx_regex_groups *gr);
/* 1 iff re and gr are valid by the rules above (NULL: 0).  Pure host code; the device entries below call it. */
int bmx_regex_groups_valid(const bmx_regex *re, const bmx_regex_groups *gr);
/* The groups of every span of a device-resident list: entry i is text[d_starts[i] - base_offset .. d_ends[i] - base_offset]
 * (both inclusive, as bmx_regex_starts_device pairs them) and gets the (begin, end) pairs of groups 0..n_groups at
 * d_groups[(i * (n_groups + 1) + g) * 2], each plus base_offset; an unset group gets UINT64_MAX twice.  One list entry per
 * lane: a backward sweep over the span (the reversed-automaton recurrence of bmx_regex_starts_device) leaves for every
 * byte the positions that consume it and can still reach `last` at e, a column of at most max_len <= 64 words per lane in
 * LDS; one forward walk then takes the first entry of pref[cur] in the column's word and applies the two tag words.
 * An entry whose start or end is UINT64_MAX, or whose end is below its start, is SKIPPED: all its outputs are UINT64_MAX
 * and it is no error (the ends passes produce such entries).  An entry outside [base_offset, base_offset + n), longer than
 * max_len, or whose span is not a match raises a status word: BMX_ERR_ARG, outputs unspecified.
 * Errors, count == 0, the bytes read (none outside the aligned 16-byte lines of text[0..n)) and the stream rule as for
 * bmx_regex_starts_device; a struct that is not valid is BMX_ERR_ARG before any HIP call.  The tables travel through a
 * device block of the context, copied on `stream` in front of the launch. */
int bmx_regex_groups_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                            const bmx_regex_groups *gr, const uint64_t *d_starts, const uint64_t *d_ends, uint64_t count,
                            uint64_t *d_groups /* count * (n_groups + 1) * 2 */, void *stream);
/* Host buffers in, host buffers out: upload, bmx_search_regex_device, bmx_regex_starts_device (flags: BMX_REGEX_LONGEST or
 * 0), bmx_regex_groups_device, download.  starts[i], ends[i] and groups[i * (n_groups + 1) * 2 ..] belong together;
 * capacity (entries) and *n_matches as for bmx_search_regex_spans.  ctx may be NULL. */
int bmx_search_regex_groups(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const bmx_regex *re,
                            const bmx_regex_groups *gr, uint32_t flags, uint64_t *starts, uint64_t *ends, uint64_t *groups,
                            uint64_t capacity, uint64_t *n_matches);
/* Device time (ms, HIP events around the kernel) of the last bmx_regex_groups_device on ctx; < 0 if none. */
float bmx_last_regex_groups_ms(bmx_ctx *ctx);

/* A replacement template, parsed: literal bytes, \1..\9, \g<0>..\g<16> and \\ (one backslash) -- the subset on which
 * Python's `re` template syntax agrees byte for byte (\0 is a NUL there, hence \g<0>).  T = n_refs references cut the
 * template into T + 1 literals: literal r stands in front of reference r, literal T behind the last one; any of them may
 * be empty.  Their bytes go, unescaped and one after the other, to `lits` (room for `len` bytes; may be NULL when len is 0).
 * BMX_ERR_ARG, outputs untouched, a text in bmx_last_error: NULL where a pointer is needed; anything else behind a
 * backslash (a dangling one, \0, \n, \g without <digits>); a reference above n_groups; more than BMX_MAX_TEMPLATE_REFS
 * references; len > BMX_MAX_REPLACEMENT; n_groups outside 0..BMX_MAX_REGEX_GROUPS.  Pure host code. */
#define BMX_MAX_TEMPLATE_REFS 32
typedef struct bmx_template {
    int32_t  n_refs;                               /* T: 0..32 */
    int32_t  ref[BMX_MAX_TEMPLATE_REFS];           /* the group of reference r, 0..n_groups */
    uint32_t lit_off[BMX_MAX_TEMPLATE_REFS + 1];   /* literal r: lits[lit_off[r] .. lit_off[r] + lit_len[r]) */
    uint32_t lit_len[BMX_MAX_TEMPLATE_REFS + 1];
    uint32_t lit_bytes;                            /* all literals together */
} bmx_template;
int bmx_compile_template(const void *tmpl, uint64_t len, int32_t n_groups, bmx_template *out, void *lits);
/* bmx_replace_device / bmx_extract_device with a template.  d_groups: what bmx_regex_groups_device wrote for `count`
 * entries of n_groups + 1 pairs.  The matches are group 0 of every entry: ascending, pairwise disjoint, non-empty, inside
 * [base_offset, base_offset + n), all set, and every other group unset or inside its entry's group 0; anything else raises
 * a status word: BMX_ERR_ARG.  An unset group expands to nothing.
 * flags 0: d_out receives the text with every match replaced by its expansion (re.sub).  BMX_EXPAND_EXTRACT: d_out
 * receives the expansions one after the other and d_off the count + 1 offsets into them, always all of them
 * (Match.expand; grep -o | sed; one group of re.findall with the template \1).  d_off is not read without the flag.
 * Capacity and counting as for bmx_replace_device: the true size goes to *n_out, capacity 0 only counts, a smaller
 * non-zero capacity stores the lowest `capacity` bytes and returns BMX_ERR_CAPACITY.  BMX_ERR_ARG before any HIP call, with
 * ctx == NULL too: NULL where a pointer is needed, a bad template, unknown flags, n >= 2^40, count >= 2^32, an output
 * that overlaps the text.  count == 0: flags 0 copies the text, EXTRACT writes the single offset 0.  Stream rule and the
 * bytes read as for bmx_replace_device.
 * Method: the output-driven copy of bmx_replace_device with T + 1 pieces per match; piece r opens with literal r (offset
 * and length from a table in LDS, indexed by the piece's number modulo T + 1) and goes on with a run of text that may be
 * empty: group ref[r], or behind literal T the text up to the next match (EXTRACT: nothing).  A template without a
 * reference gives bmx_replace_device's bytes. */
#define BMX_EXPAND_EXTRACT 1u
int bmx_expand_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t base_offset, const uint64_t *d_groups,
                      int32_t n_groups, uint64_t count, const void *tmpl /* host */, uint64_t tmpl_len, uint32_t flags,
                      void *d_out, uint64_t capacity /* bytes */, uint64_t *d_off /* EXTRACT: count + 1 */, uint64_t *n_out,
                      void *stream);
/* Host buffers in, host buffers out, base_offset 0: upload, bmx_expand_device, download. */
int bmx_expand(bmx_ctx *ctx /* NULL: device 0 */, const char *text, uint64_t n, const uint64_t *groups, int32_t n_groups,
               uint64_t count, const void *tmpl, uint64_t tmpl_len, uint32_t flags, void *out, uint64_t capacity,
               uint64_t *off /* EXTRACT: count + 1 */, uint64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* BMX_H */
