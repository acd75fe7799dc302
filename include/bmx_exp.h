/* bmx_exp.h -- entry points that ONLY libbmx_exp.so exports (the same sources as libbmx.so compiled with
 * -DBMX_EXPERIMENTS: every slot of the kernel table, timing-only kernels, stamp builds).  Measurement and test
 * infrastructure: tools/ and a few tests bind it (host.exp_lib()); nothing of the product path, bench.py's timed
 * region or smoke() does.  The product library has none of these and reads no environment variable. */
#ifndef BMX_EXP_H
#define BMX_EXP_H

#include "bmx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A measurement / test switch of one context.  Names: "max_grid" (at most n workgroups per scan: texts of a few MiB
 * then reach the stolen tail), "no_dense" (no fill pass), "no_text_sample" (the walker goes by the pattern's symbols),
 * "multi_no_qgram" (multi-pattern pass byte-wise only), "ed_lag" (rows a column band is assumed to trail its
 * predecessor by; < 0: the measured default), "ed_group" (16 | 32 rows per hand-over), "ed_step_x" (1..8: ed variant 13 with parts of its step left out, timing only), "sa_flags" (1 library rounds
 * only, 2 a host wait per round, 4 per-round trace on stderr), "index_no_dir" (the text index's queries search the whole
 * array instead of their directory bucket: same answers, tools/index_rate.py measures the difference), "ordered_seq"
 * (>= 0: the sequence number of every ordered-output session the context already has -- approximate, class-pattern and
 * dictionary search; the next call takes the one after it, so (1 << 22) - 1 puts that call on the wrap of the status
 * words' 22-bit tag), "tile_piece_shift" and "tile_max_grid" (the launch geometry of the same sessions, the long
 * approximate, k-mismatch, gapped and regex search included, from their next call on; tests reach with them, on texts an
 * oracle can check in full, what only texts of GiB reach otherwise.  tile_piece_shift: 0 = the production rule, else 6..12 =
 * log2 of the ends per lane in place of the rule's value; the dictionary search takes value - 6 for the log2 of the 8 KiB rounds
 * per tile, at most 5 (256 KiB), so a context that has a dictionary session accepts at most 11.  tile_max_grid: 0 = off, else
 * the most workgroups a call starts; tiles are handed out in ascending order and every started workgroup is resident, so
 * any grid finishes.  Values are not checked against the pattern: a piece below ceil_log2(4 m) is a geometry the product
 * never runs).  The regex search with unbounded repetition takes the two geometry knobs too, and has three of its own, kept
 * in the context so that they hold from its first call: "regex_star_force_slow" (non-zero: the exact slow path runs behind
 * the first launch even when nothing is tainted), "regex_star_piece_shift" (0, or 4..12: log2 of the ends per lane of THAT
 * search, in front of "tile_piece_shift"; 4 and 5 make chains of pieces that cross tiles and workgroups on texts of a few
 * KiB) and "regex_star_warm" (0 = the rule, else the bytes of the pair warm-up, a multiple of 16 up to 65,536).
 * The regex begins search (bmx_search_regex_begins_device) takes the two geometry knobs as well and has
 * "regex_begins_piece_shift" (0, or 4..12: log2 of the starts per lane of THAT search, in front of "tile_piece_shift", kept
 * in the context; 4 makes lanes of 16 starts, fewer than a longest match has bytes).
 * "select_tile_shift": 0 = the production tile of bmx_spans_select_device (T = 2^8 entries), else 3..8 = log2 T, from the
 * context's next selection on: lists of a few hundred entries then reach three levels of its pointer jumping.
 * BMX_ERR_ARG for an unknown name, a "select_tile_shift" outside that range, a negative "ordered_seq" or "tile_max_grid" and a "tile_piece_shift",
 * "regex_star_piece_shift", "regex_begins_piece_shift" or "regex_star_warm" outside those ranges. */
int bmx_exp_set_knob(bmx_ctx *ctx, const char *name, int value);

/* What the last launch of one ordered-output session of the context ran with: out3 = {log2 of the ends per lane (the
 * dictionary search: 6 + log2 of the rounds per tile), workgroups started, tiles}; zeros before the session's first launch.
 * session: "approx" (also the approximate search over classes), "approx_long", "classes", "hamming", "gaps", "regex",
 * "regex_begins" (the begins search: starts per lane) or "dict".  Tests assert with it that the geometry they forced ("tile_piece_shift", "tile_max_grid") is the one that ran.
 * "rows": the last bmx_rows_split_device, out3 = {log2 of the bytes of a tile, workgroups started, tiles}; a workgroup is
 * eight waves, each with an eighth of the tile, read in batches of eight rounds of 1 KiB (the first entry is there
 * before any split).
 * "select": the last bmx_spans_select_device, out3 = {log2 T, levels of pointer jumping (0: at most T entries, or
 * BMX_SELECT_MERGE), tiles of T entries}.
 * BMX_ERR_ARG for another name. */
int bmx_exp_last_launch(bmx_ctx *ctx, const char *session, uint64_t *out3);

/* What the last bmx_search_regex_star_device of the context did: out10 = {waves of the first launch that held a lane whose
 * two bounds did not meet (0: the call was untainted), 1 if the slow path ran, log2 of the ends per lane, bytes of the pair
 * warm-up, pieces and stored columns of the slow path, then microseconds of the first launch, of R1 (bounds, scan,
 * columns), of the sweep and of R2}; zeros before the first call and for a call that launched nothing.
 * "bmx_exp_last_launch" knows the session as "regex_star". */
int bmx_exp_regex_star_last(bmx_ctx *ctx, uint64_t *out10);

/* The same for the last bmx_search_regex_star_begins_device (pieces are counted from the top of the view).  That search
 * has the knobs "regex_star_begins_force_slow", "regex_star_begins_piece_shift" (0, 4..12) and "regex_star_begins_warm"
 * (0, or a multiple of 16 up to 65,536) of bmx_exp_set_knob, with the meaning and the ranges of the three "regex_star_"
 * knobs above, takes "tile_piece_shift" / "tile_max_grid" / "ordered_seq", and is "regex_star_begins" in
 * bmx_exp_last_launch.  "regex_star_ends_no_early_exit" (non-zero) makes bmx_regex_star_ends_device walk the whole window
 * of every entry, to time what the early exit saves; the answers are the same. */
int bmx_exp_regex_star_begins_last(bmx_ctx *ctx, uint64_t *out10);

/* Read-only sweep of n bytes at d_text (16-byte aligned) with plain global loads into registers, XOR-folded: no LDS,
 * no barrier, no tiles (csrc/bmx_probe_kernel.h).  unroll = loads in flight per lane (1, 2, 4, 8, 16), nt = cache
 * policy, block threads per workgroup, blocks_per_cu workgroups per CU.  ms_out[i] = duration of launch i. */
int bmx_probe_read(bmx_ctx *ctx, const void *d_text, uint64_t n, int block, int blocks_per_cu, int unroll, int nt,
                   int launches, float *ms_out, void *stream);

/* Cycle counts (s_memtime) of the band in the middle of the forward pipeline of the last bmx_edit_distance_device call that
 * ran a reworked bit-parallel band (ed variants 11, 12, 13; knob "ed_stamp_block": which band, default the middle forward one): out8 = {groups of unrolled steps, cycles inside them, cycles between
 * them (validate, ring, hand-over, request), cycles of the whole loop, of which in validate (waiting included), steps per
 * group, rows per step, steps of the band}; out16[8..15] (ed variant 13): one hand-over's timeline in 10-ns ticks of the 100 MHz
 * clock all CUs share -- the stamped band's main wave at the end of its group 200, its publisher behind that group's stores; in
 * the band behind: the feeder when the batch those entries complete is valid / fed, the Eq-word wave when its words are there, the
 * main wave at the start of the group that needed them (0: not reached); [10], [11], [16..18]: the same chain at the START of the run (the band
 * in front ends its group 2 / the band behind starts its first group; batch 1 fed, Eq words of 33 steps there, group 2 published); [24 + 4 b + k], b < 64: the clock when band (block) b finished its
 * groups 1, 100, 300 and 500 (0: it has fewer). */
int bmx_exp_ed_stamps(bmx_ctx *ctx, uint64_t *out280);

#ifdef __cplusplus
}
#endif
#endif
