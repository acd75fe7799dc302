"""ctypes binding of libbmx.so (include/bmx.h) -- the Python face of the C ABI.

The reference (BoyreMoore/BoyreMoore/BoyreMoore.cpp) has no callable API: its
contract is "text + pattern in, match positions (device printf) and per-range
counts out".  This module keeps that contract and nothing else:

* :func:`build_tables`  -- BoyreMoore.cpp:150-190 (host shift tables)
* :func:`search`        -- (text, pattern) -> ascending match positions, host buffers
* :func:`search_ranges` -- the kernel's own signature, kernel1.cl:1: ranges ``se`` in,
  per-range counts ``ans`` out
* :class:`Context`      -- one GPU; ``search_device`` works on a text resident in HBM
  (a ``torch`` uint8 CUDA tensor or a raw device pointer)

There is NO CPU fallback: if libbmx.so is missing or no GPU is present every
device entry point raises.  torch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple, Union

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libbmx.so")
# libbmx_exp.so: the same sources built with -DBMX_EXPERIMENTS -- every slot of the kernel table (losing schedules, timing-only
# kernels whose match lists are not valid), every edit-distance schedule (the product library builds 13, 0 as its alias and
# their tiles behind +16 / +32; set_ed_variant refuses the rest there) and the measurement switches (bmx_exp_set_knob).  tools/ and a few tests load it
# through exp_lib() / Context(library=exp_lib()); the product path, bench.py and smoke() never do.  Nothing here reads
# the environment: tools/ that want another build call use_library() themselves.
EXP_LIB_PATH = os.path.join(_HERE, "lib", "libbmx_exp.so")

MAX_PATTERN = 512
MAX_MULTI = 8
MAX_APPROX_PATTERN = 64
MAX_APPROX_LONG_PATTERN = 512  # bmx_search_approx_long*: a column of several words per lane above 64 bytes
MAX_APPROX_LONG_K = 255
MAX_CLASS_PATTERN = 64
CLASS_BYTES = 32
CLASS_ICASE = 1
CLASS_IUPAC = 2
MAX_HAMMING_PATTERN = 64
MAX_HAMMING_K = 15
MAX_GAPS_PATTERN = 64
GAPS_PROSITE = 4  # a flag of compile_gaps, beside CLASS_ICASE and CLASS_IUPAC
GAPS_LONGEST = 1  # a flag of gaps_starts_device
MAX_REGEX_POSITIONS = 64
MAX_REGEX_LONG_POSITIONS = 128  # compile_regex_long, search_regex_long*
REGEX_LONGEST = 1  # a flag of regex_starts_device
REGEX_WORD = 4  # flags of compile_regex_anchored: grep -w ...
REGEX_LINE = 8  # ... and grep -x
REGEX_UNBOUNDED = -1  # Regex.max_len of an automaton with a cycle (compile_regex_star)
MAX_REGEX_STAR_WINDOW = 65536  # regex_star_starts_device
SPANS_BEST = 1
SPANS_BLOCK = 256  # list entries per workgroup of the starts kernel (csrc/bmx_spans_kernel.h)
SPANS_TILE = 2048  # list entries per workgroup of the selection
MAX_DICT = 65536
ED_BATCH_WORD = 64
LCP_LANE_BYTES = 64  # a pair with a longer common prefix leaves the one-lane path of the LCP array (BMX_LCP_LANE_BYTES)
ED_BATCH_LONG = 65536
ED_NO_LIMIT = 0xFFFFFFFF
MAP_MAX_K = 64  # most edits of Index.map (BMX_MAP_MAX_K)
MAP_NO_HIT = 255  # distance of a candidate or a read without a hit (BMX_MAP_NO_HIT)
MAP_NO_POS = 0xFFFFFFFFFFFFFFFF  # ... and its positions (BMX_MAP_NO_POS); -1 in the int64 tensors of Index.map
MAP_MAX_CANDIDATES = 1 << 27
ALIGN_MAX_PATTERN = 512  # longest pattern of Context.align (BMX_ALIGN_MAX_PATTERN)
ALIGN_MAX_K = 254
ALIGN_NONE = 255  # distance of an entry without an alignment within k (BMX_ALIGN_NONE == MAP_NO_HIT)
ALIGN_WORKSPACE_BYTES = 1 << 30  # the workspace one launch of the alignments may take (BMX_ALIGN_WORKSPACE_BYTES)
CIGAR_INS = 1  # op codes of the scripts, the BAM encoding: an op word is run length << 4 | code
CIGAR_DEL = 2
CIGAR_EQ = 7
CIGAR_X = 8
_CIGAR_CHARS = "MIDNSHP=X"
ROW_NONE = 0xFFFFFFFFFFFFFFFF  # the row of a match that lies in no row (BMX_ROW_NONE); -1 in the int64 tensors of Rows.of
ROWS_INVERT = 1  # Rows.matching: the rows without an entry (BMX_ROWS_INVERT)
SELECT_MERGE = 1  # select_spans_device: the connected regions of the union of the spans (BMX_SELECT_MERGE)
MAX_REPLACEMENT = 65536  # bytes of a replacement (BMX_MAX_REPLACEMENT)
MAX_REGEX_GROUPS = 16  # capturing groups of compile_regex_groups
REGEX_START = 64  # row of RegexGroups.pref / open / close: before the first byte of the match
REGEX_END = 64  # column of open / close: after its last byte
MAX_TEMPLATE_REFS = 32  # group references of a replacement template
EXPAND_EXTRACT = 1  # expand_device: the column of expansions (BMX_EXPAND_EXTRACT)
BAD_TABLE_SIZE = 128

OK = 0
ERR_ARG, ERR_DOMAIN, ERR_TABLE, ERR_CAPACITY, ERR_HIP, ERR_NO_DEVICE = -1, -2, -3, -4, -5, -6
_ERR_NAMES = {
    ERR_ARG: "BMX_ERR_ARG", ERR_DOMAIN: "BMX_ERR_DOMAIN", ERR_TABLE: "BMX_ERR_TABLE",
    ERR_CAPACITY: "BMX_ERR_CAPACITY", ERR_HIP: "BMX_ERR_HIP", ERR_NO_DEVICE: "BMX_ERR_NO_DEVICE",
}

_i32p = C.POINTER(C.c_int32)
_u64p = C.POINTER(C.c_uint64)

# every symbol include/bmx.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("bmx_build_tables", C.c_int, [C.c_char_p, C.c_int32, _i32p, _i32p]),
    ("bmx_device_count", C.c_int, []),
    ("bmx_ctx_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("bmx_ctx_destroy", None, [C.c_void_p]),
    ("bmx_last_error", C.c_char_p, []),
    ("bmx_version", C.c_char_p, []),
    ("bmx_search", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int32, _u64p, C.c_uint64, _u64p]),
    ("bmx_search_multi", C.c_int, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_int32, _i32p, C.c_int32, _u64p, C.c_uint64,
                                   _u64p]),
    ("bmx_multi_create", C.c_int, [_i32p, C.c_int32, C.POINTER(C.c_void_p)]),
    ("bmx_multi_destroy", None, [C.c_void_p]),
    ("bmx_multi_device_count", C.c_int, [C.c_void_p]),
    ("bmx_multi_uses_rccl", C.c_int, [C.c_void_p]),
    ("bmx_multi_text_upload", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    ("bmx_multi_gen_text", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int32]),
    ("bmx_multi_plant", C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, _u64p, C.c_uint64]),
    ("bmx_multi_shard", C.c_int, [C.c_void_p, C.c_int32, _u64p, C.POINTER(C.c_void_p)]),
    ("bmx_multi_search", C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, _u64p, C.c_uint64, _u64p]),
    ("bmx_multi_last_scan_ms", C.c_float, [C.c_void_p]),
    ("bmx_multi_last_exchange", C.c_int, [C.c_void_p]),
    ("bmx_search_ranges", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, _i32p, C.c_int32, _i32p,
                                    _i32p, _i32p, C.c_int32]),
    ("bmx_search_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p,
                                    C.c_int32, _i32p, _i32p, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_device_enqueue", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p,
                                            C.c_int32, _i32p, _i32p, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("bmx_search_device_finish", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_device_multi", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_char_p),
                                          _i32p, C.c_int32, C.c_void_p, C.c_uint64, _u64p, _u64p, C.c_void_p]),
    ("bmx_last_search_sorted", C.c_int, [C.c_void_p]),
    ("bmx_stream_wait_last_scan", C.c_int, [C.c_void_p, C.c_void_p]),
    ("bmx_count_to_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("bmx_merge_gathered_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_uint64,
                                            C.c_void_p, C.c_uint64, C.c_void_p]),
    ("bmx_text_upload", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("bmx_device_free", C.c_int, [C.c_void_p, C.c_void_p]),
    ("bmx_device_alloc", C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("bmx_last_scan_ms", C.c_float, [C.c_void_p]),
    ("bmx_scan_ms_history", C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int32]),
    ("bmx_scan_stamps", C.c_int, [C.c_void_p, _u64p, C.c_uint64]),
    ("bmx_scan_geometry", C.c_int, [C.c_void_p, C.c_int32, _u64p]),
    ("bmx_set_variant", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("bmx_variant_count", C.c_int, []),
    ("bmx_set_order_overlap", C.c_int, [C.c_void_p, C.c_int]),
    ("bmx_last_variant", C.c_int, [C.c_void_p]),
    ("bmx_edit_distance", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_edit_distance_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p,
                                           C.c_void_p]),
    ("bmx_last_edit_distance_ms", C.c_float, [C.c_void_p]),
    ("bmx_set_ed_variant", C.c_int, [C.c_void_p, C.c_int]),
    ("bmx_edit_distance_batch_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                                 C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_edit_distance_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                          C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    ("bmx_last_ed_batch_ms", C.c_float, [C.c_void_p]),
    ("bmx_last_ed_batch_fallbacks", C.c_int64, [C.c_void_p]),
    ("bmx_search_approx_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_approx", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_last_approx_ms", C.c_float, [C.c_void_p]),
    ("bmx_search_approx_long_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p,
                                                C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_approx_long", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_compile_classes", C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, _i32p]),
    ("bmx_search_classes_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_classes", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64,
                                     _u64p]),
    ("bmx_last_classes_ms", C.c_float, [C.c_void_p]),
    ("bmx_search_approx_classes", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_approx_classes_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, _u64p,
                                                   C.c_void_p]),
    ("bmx_search_hamming_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int32,
                                            C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_hamming_classes_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                                    C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, _u64p,
                                                    C.c_void_p]),
    ("bmx_search_hamming", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int32, C.c_int32, C.c_uint64,
                                     C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_hamming_classes", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_last_hamming_ms", C.c_float, [C.c_void_p]),
    ("bmx_compile_gaps", C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, _u64p, _i32p]),
    ("bmx_search_gaps_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32,
                                         C.c_uint64, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_gaps", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p,
                                  C.c_uint64, _u64p]),
    ("bmx_search_gaps_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_last_gaps_ms", C.c_float, [C.c_void_p]),
    ("bmx_gaps_starts_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32, C.c_uint64,
                                         C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_compile_regex", C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    ("bmx_search_regex_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                          C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_regex", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_regex_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_uint64, _u64p]),
    ("bmx_last_regex_ms", C.c_float, [C.c_void_p]),
    ("bmx_regex_starts_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_regex_reverse", C.c_int, [C.c_void_p, C.c_void_p]),
    ("bmx_compile_regex_long", C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    ("bmx_regex_long_widen", C.c_int, [C.c_void_p, C.c_void_p]),
    ("bmx_search_regex_long_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                               C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_regex_long", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_regex_long_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_uint64, _u64p]),
    ("bmx_last_regex_long_ms", C.c_float, [C.c_void_p]),
    ("bmx_regex_long_starts_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                               C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_search_regex_begins_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                                 C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_last_regex_begins_ms", C.c_float, [C.c_void_p]),
    ("bmx_regex_ends_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_search_regex_begins", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_regex_begins_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                C.c_uint64, _u64p]),
    ("bmx_compile_regex_anchored", C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_search_regex_anchored_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                                   C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_last_regex_anchored_ms", C.c_float, [C.c_void_p]),
    ("bmx_regex_anchored_starts_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                                   C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_search_regex_anchored_begins_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                                          C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_last_regex_anchored_begins_ms", C.c_float, [C.c_void_p]),
    ("bmx_regex_anchored_ends_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                                 C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_search_regex_anchored", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_regex_anchored_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                  C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_regex_anchored_begins", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                   _u64p]),
    ("bmx_search_regex_anchored_begins_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                                         C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_device_download", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("bmx_compile_regex_star",C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    ("bmx_search_regex_star_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                               C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_search_regex_star", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_regex_star_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_last_regex_star_ms", C.c_float, [C.c_void_p]),
    ("bmx_regex_star_starts_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                               C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_search_regex_star_begins_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                                      C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_last_regex_star_begins_ms", C.c_float, [C.c_void_p]),
    ("bmx_regex_star_ends_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, _u64p, C.c_void_p]),
    ("bmx_search_regex_star_begins", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_regex_star_begins_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32,
                                                     C.c_void_p, C.c_void_p, C.c_uint64, _u64p, _u64p]),
    ("bmx_approx_spans_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          _u64p, C.c_void_p]),
    ("bmx_approx_spans_classes_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32,
                                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, _u64p, C.c_void_p]),
    ("bmx_search_approx_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int32, C.c_int32, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_search_approx_spans_classes", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_approx_long_spans_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int32, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, _u64p, C.c_void_p]),
    ("bmx_search_approx_long_spans", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int32, C.c_int32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_last_spans_ms", C.c_float, [C.c_void_p]),
    ("bmx_dict_create", C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), _i32p, C.c_int32, C.POINTER(C.c_void_p)]),
    ("bmx_dict_destroy", None, [C.c_void_p]),
    ("bmx_dict_search_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_dict_search", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), _i32p, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_last_dict_ms", C.c_float, [C.c_void_p]),
    ("bmx_last_dict_candidates", C.c_int64, [C.c_void_p]),
    ("bmx_suffix_array", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, _i32p]),
    ("bmx_suffix_array_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("bmx_last_suffix_array_ms", C.c_float, [C.c_void_p]),
    ("bmx_last_suffix_array_rounds", C.c_int, [C.c_void_p]),
    ("bmx_last_suffix_array_lds_rounds", C.c_int, [C.c_void_p]),
    ("bmx_lcp_array_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("bmx_lcp_array", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("bmx_lcp_stats_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p]),
    ("bmx_last_lcp_ms", C.c_float, [C.c_void_p]),
    ("bmx_last_lcp_long_pairs", C.c_int64, [C.c_void_p]),
    ("bmx_index_create_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("bmx_index_destroy", None, [C.c_void_p]),
    ("bmx_index_sa", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("bmx_index_count_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    ("bmx_index_locate_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
                                          C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_index_count", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                  C.c_void_p]),
    ("bmx_index_locate", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_index_match_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    ("bmx_index_seeds_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                         C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                         _u64p, C.c_void_p]),
    ("bmx_index_match", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    ("bmx_index_seeds", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                  C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_uint64, _u64p]),
    ("bmx_index_map_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                       C.c_uint32, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_index_map", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_last_index_map_candidates", C.c_int64, [C.c_void_p]),
    ("bmx_last_index_map_phases", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("bmx_last_index_ms", C.c_float, [C.c_void_p]),
    ("bmx_index_build_ms", C.c_float, [C.c_void_p]),
    ("bmx_align_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_align", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_uint64, _u64p]),
    ("bmx_last_align_ms", C.c_float, [C.c_void_p]),
    ("bmx_last_align_launches", C.c_int64, [C.c_void_p]),
    ("bmx_rows_split_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint8, C.c_void_p, C.c_uint64, _u64p,
                                        _u64p, C.c_void_p]),
    ("bmx_rows_of_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                     C.c_void_p]),
    ("bmx_rows_matching_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_last_rows_ms", C.c_float, [C.c_void_p]),
    ("bmx_rows_split", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint8, C.c_void_p, C.c_uint64, _u64p, _u64p]),
    ("bmx_rows_of", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    ("bmx_rows_matching", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                    _u64p]),
    ("bmx_spans_select_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_replace_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                     C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p, C.c_void_p]),
    ("bmx_extract_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                     C.c_void_p, C.c_uint64, C.c_void_p, _u64p, C.c_void_p]),
    ("bmx_last_subst_ms", C.c_float, [C.c_void_p]),
    ("bmx_spans_select", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_replace", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                              C.c_uint64, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_extract", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                              C.c_uint64, C.c_void_p, _u64p]),
    ("bmx_compile_regex_groups", C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("bmx_regex_groups_valid", C.c_int, [C.c_void_p, C.c_void_p]),
    ("bmx_regex_groups_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("bmx_search_regex_groups", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    ("bmx_last_regex_groups_ms", C.c_float, [C.c_void_p]),
    ("bmx_compile_template", C.c_int, [C.c_char_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p]),
    ("bmx_expand_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32, C.c_uint64, C.c_char_p,
                                    C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, _u64p, C.c_void_p]),
    ("bmx_expand", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_uint64, C.c_char_p, C.c_uint64,
                             C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, _u64p]),
    ("bmx_gen_text_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]),
    ("bmx_plant_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int32, _u64p,
                                   C.c_uint64, C.c_void_p]),
]


class BmxError(RuntimeError):
    def __init__(self, rc: int, what: str, detail: str = ""):
        self.rc = rc
        super().__init__(f"{what}: {_ERR_NAMES.get(rc, rc)}" + (f" ({detail})" if detail else ""))


# entry points only libbmx_exp.so exports
EXP_SYMBOLS = [
    ("bmx_exp_set_knob", C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    ("bmx_exp_last_launch", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]),
    ("bmx_exp_regex_star_last", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("bmx_exp_regex_star_begins_last", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("bmx_probe_read", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_float), C.c_void_p]),
    ("bmx_exp_ed_stamps", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
]

_lib = None
_exp = None
_lib_tolerant = False


def _bind(path: str, symbols, tolerant: bool = False):
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C parallel_implementation_of_string_matching_algorithms_opencl_amd/csrc`")
    L = C.CDLL(path)
    for name, res, args in symbols:
        if tolerant and not hasattr(L, name):
            continue
        fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    return L


def use_library(path: str, tolerant: bool = True) -> None:
    """tools/ only, before the first call: bind another build of the library (`exp`, or a path -- A/B runs of an older
    build on the same box; an older build may lack newer entry points, hence tolerant)."""
    global LIB_PATH, _lib_tolerant
    if _lib is not None:
        raise RuntimeError("use_library() must come before the library is first used")
    LIB_PATH = EXP_LIB_PATH if path == "exp" else path
    _lib_tolerant = tolerant and path != "exp"


def lib():
    """Load libbmx.so (built in-tree by __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is None:
        exp = os.path.abspath(LIB_PATH) == os.path.abspath(EXP_LIB_PATH)
        _lib = _bind(LIB_PATH, SYMBOLS + (EXP_SYMBOLS if exp else []), _lib_tolerant)
    return _lib


def exp_lib():
    """libbmx_exp.so beside the product library in the same process (its own kernels, its own state)."""
    global _exp
    if _exp is None:
        _exp = _bind(EXP_LIB_PATH, SYMBOLS + EXP_SYMBOLS)
    return _exp


def _check(rc: int, what: str, allow=(), L=None):
    if rc != OK and rc not in allow:
        raise BmxError(rc, what, (L or lib()).bmx_last_error().decode(errors="replace"))
    return rc


def _pat_bytes(pattern) -> bytes:
    if isinstance(pattern, str):
        pattern = pattern.encode("latin-1")
    pattern = bytes(pattern)
    return pattern


def _host_text(text) -> Tuple[C.c_void_p, int, object]:
    if isinstance(text, str):
        text = text.encode("latin-1")
    if isinstance(text, (bytes, bytearray)):
        b = bytes(text)
        return C.cast(C.c_char_p(b), C.c_void_p), len(b), b
    arr = np.ascontiguousarray(text, dtype=np.uint8)
    return C.c_void_p(arr.ctypes.data), arr.size, arr


def pack_strings(strings) -> Tuple[np.ndarray, np.ndarray]:
    """A string column in the Arrow layout of bmx_edit_distance_batch: (blob uint8, offsets uint64 of len + 1 entries).
    ``strings``: a sequence of bytes / str, or a (blob, offsets) pair, which is passed through."""
    if isinstance(strings, tuple) and len(strings) == 2 and isinstance(strings[1], np.ndarray):
        return np.ascontiguousarray(strings[0], dtype=np.uint8).reshape(-1), np.ascontiguousarray(strings[1], dtype=np.uint64)
    items = [_pat_bytes(x) for x in strings]
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        off[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    return np.frombuffer(b"".join(items), dtype=np.uint8), off


def cigar_strings(op_off, ops) -> list:
    """The scripts of Context.align / align_device as SAM CIGAR strings, one per entry ("" for an entry without an
    alignment): ``op_off`` count + 1 offsets, ``ops`` the op words (numpy arrays or tensors)."""
    off = np.asarray(op_off.cpu() if hasattr(op_off, "cpu") else op_off).astype(np.int64)
    words = np.asarray(ops.cpu() if hasattr(ops, "cpu") else ops).astype(np.int64)
    if off.size and int(off[-1]) > words.size:
        raise ValueError("ops holds fewer op words than op_off[-1]")
    parts = [f"{int(w) >> 4}{_CIGAR_CHARS[int(w) & 15]}" for w in words[: int(off[-1]) if off.size else 0]]
    return ["".join(parts[int(off[e]):int(off[e + 1])]) for e in range(max(off.size - 1, 0))]


def _device_strings(patterns, dev):
    """(blob tensor, offsets tensor, count) on ``dev``: a list of bytes / str or a (blob, offsets) numpy pair is uploaded,
    a pair of CUDA tensors is passed through."""
    import torch

    if isinstance(patterns, tuple) and len(patterns) == 2 and hasattr(patterns[0], "data_ptr"):
        d_blob, d_off = patterns
        if d_blob.element_size() != 1 or d_off.element_size() != 8:
            raise ValueError("patterns: a 1-byte blob and 8-byte offsets")
        return d_blob, d_off, d_off.numel() - 1
    blob, off = pack_strings(patterns)
    d_blob = torch.from_numpy(blob.copy() if blob.size else np.zeros(1, np.uint8)).to(dev)
    return d_blob[: blob.size], torch.from_numpy(off.astype(np.int64)).to(dev), off.size - 1


def build_tables(pattern) -> Tuple[np.ndarray, np.ndarray]:
    """(bad[128], good[m]) int32, identical to the reference's host tables."""
    pat = _pat_bytes(pattern)
    m = len(pat)
    bad = np.zeros(BAD_TABLE_SIZE, dtype=np.int32)
    good = np.zeros(max(m, 1), dtype=np.int32)
    _check(lib().bmx_build_tables(pat, m, bad.ctypes.data_as(_i32p), good.ctypes.data_as(_i32p)), "bmx_build_tables")
    return bad, good[:m]


def compile_classes(expr, flags: int = 0) -> np.ndarray:
    """A class expression (bmx_compile_classes: ``.``, ``[a-c]``, ``[^x]``, ``\\xHH``, ``\\c``; flags CLASS_ICASE, CLASS_IUPAC)
    -> uint8 array [m, 32]: byte value b belongs to class i iff bit (b & 7) of row i's byte (b >> 3) is set."""
    e = _pat_bytes(expr)
    buf = np.zeros((MAX_CLASS_PATTERN, CLASS_BYTES), dtype=np.uint8)
    m = C.c_int32(0)
    _check(lib().bmx_compile_classes(e, len(e), int(flags), C.c_void_p(buf.ctypes.data), C.byref(m)), "bmx_compile_classes")
    return buf[: int(m.value)].copy()


def _classes(classes_or_expr, flags: int = 0) -> np.ndarray:
    """[m, 32] uint8 classes from an expression (str / bytes) or from such an array, passed through."""
    if isinstance(classes_or_expr, (str, bytes, bytearray)):
        return compile_classes(classes_or_expr, flags)
    arr = np.ascontiguousarray(classes_or_expr, dtype=np.uint8)
    if arr.ndim != 2 or arr.shape[1] != CLASS_BYTES:
        raise ValueError("classes: a uint8 array of shape [m, 32]")
    return arr


def _must_mask(must) -> int:
    """The ``must`` argument of the k-mismatch search as a mask: None (no position), an int mask, or an iterable of
    positions."""
    if must is None:
        return 0
    if isinstance(must, (int, np.integer)):
        if int(must) < 0 or int(must) >> 64:
            raise ValueError("must: a mask of 64 bits")
        return int(must)
    mask = 0
    for i in must:
        if not 0 <= int(i) < 64:
            raise ValueError("must: positions in [0, 64)")
        mask |= 1 << int(i)
    return mask


def compile_gaps(expr, flags: int = 0) -> Tuple[np.ndarray, int]:
    """A gapped pattern expression (bmx_compile_gaps: the elements of compile_classes, each with an optional ``?``, ``{a}``
    or ``{a,b}``; with GAPS_PROSITE the form ``C-x(2,4)-[LIVM]-{P}``) -> (classes uint8 [m, 32], optional): bit i of
    ``optional`` says that position i may be skipped."""
    e = _pat_bytes(expr)
    buf = np.zeros((MAX_GAPS_PATTERN, CLASS_BYTES), dtype=np.uint8)
    m = C.c_int32(0)
    opt = C.c_uint64(0)
    _check(lib().bmx_compile_gaps(e, len(e), int(flags), C.c_void_p(buf.ctypes.data), C.byref(opt), C.byref(m)),
           "bmx_compile_gaps")
    return buf[: int(m.value)].copy(), int(opt.value)


def _gaps(expr_or_pair, flags: int = 0) -> Tuple[np.ndarray, int]:
    """(classes [m, 32] uint8, optional) from an expression (str / bytes) or from such a pair, passed through."""
    if isinstance(expr_or_pair, (str, bytes, bytearray)):
        return compile_gaps(expr_or_pair, flags)
    classes, optional = expr_or_pair
    return _classes(classes), int(optional)


class Regex(C.Structure):
    """struct bmx_regex (include/bmx.h): the position automaton of a star-free regular expression, plain data.  Bit j of
    ``follow[i]``: position j may come right after position i; ``classes``: 32 bytes per position, as compile_classes."""
    _fields_ = [("m", C.c_int32), ("min_len", C.c_int32), ("max_len", C.c_int32), ("first", C.c_uint64), ("last", C.c_uint64),
                ("follow", C.c_uint64 * MAX_REGEX_POSITIONS), ("classes", C.c_uint8 * (MAX_REGEX_POSITIONS * CLASS_BYTES))]

    def class_array(self) -> np.ndarray:
        """The classes of the m positions, uint8 [m, 32]."""
        return np.frombuffer(bytes(self.classes), dtype=np.uint8).reshape(MAX_REGEX_POSITIONS, CLASS_BYTES)[: self.m].copy()


def compile_regex(expr, flags: int = 0) -> Regex:
    """A star-free regular expression (bmx_compile_regex: the elements of compile_classes, groups ``( )``, alternation
    ``|`` and the quantifiers ``?``, ``{a}``, ``{a,b}`` on elements and on groups) -> its position automaton."""
    e = _pat_bytes(expr)
    out = Regex()
    _check(lib().bmx_compile_regex(e, len(e), int(flags), C.byref(out)), "bmx_compile_regex")
    return out


def compile_regex_star(expr, flags: int = 0) -> Regex:
    """A regular expression with unbounded repetition (bmx_compile_regex_star: compile_regex's grammar and ``*``, ``+``,
    ``{a,}``) -> its position automaton; ``max_len`` is REGEX_UNBOUNDED where it has a cycle."""
    e = _pat_bytes(expr)
    out = Regex()
    _check(lib().bmx_compile_regex_star(e, len(e), int(flags), C.byref(out)), "bmx_compile_regex_star")
    return out


class RegexGroups(C.Structure):
    """struct bmx_regex_groups (include/bmx.h): the capture model beside a Regex, plain data.  ``pref[p]`` (row 64: START)
    lists the positions of follow[p] (of first), most preferred first, then 0xFF; bit g-1 of ``open[from][to]`` /
    ``close[from][to]`` (column 64: END): group g begins / ends at the boundary between the two."""
    _fields_ = [("n_groups", C.c_int32), ("pref", (C.c_uint8 * 64) * 65), ("open", (C.c_uint16 * 65) * 65),
                ("close", (C.c_uint16 * 65) * 65)]

    def pref_array(self) -> np.ndarray:
        return np.frombuffer(bytes(self.pref), dtype=np.uint8).reshape(65, 64).copy()

    def open_array(self) -> np.ndarray:
        return np.frombuffer(bytes(self.open), dtype=np.uint16).reshape(65, 65).copy()

    def close_array(self) -> np.ndarray:
        return np.frombuffer(bytes(self.close), dtype=np.uint16).reshape(65, 65).copy()


def compile_regex_groups(expr, flags: int = 0) -> Tuple[Regex, RegexGroups]:
    """compile_regex's grammar where ``( )`` captures and ``(?: )`` does not (bmx_compile_regex_groups) -> (Regex,
    RegexGroups).  The Regex is compile_regex's for the expression with every ``(?:`` written ``(``, so every search,
    starts, begins and ends entry takes it.  Refused: more than 16 groups, ``(?`` + anything else, and a repeat of two or
    more whose body can match the empty string and holds a capturing group (``(a?){2}``)."""
    e = _pat_bytes(expr)
    re_, gr = Regex(), RegexGroups()
    _check(lib().bmx_compile_regex_groups(e, len(e), int(flags), C.byref(re_), C.byref(gr)), "bmx_compile_regex_groups")
    return re_, gr


def _regex_groups(expr_or_pair, flags: int = 0) -> Tuple[Regex, RegexGroups]:
    if isinstance(expr_or_pair, tuple):
        re_, gr = expr_or_pair
        if not isinstance(re_, Regex) or not isinstance(gr, RegexGroups):
            raise TypeError("a pair (Regex, RegexGroups), or an expression")
        return re_, gr
    return compile_regex_groups(expr_or_pair, flags)


class Template(C.Structure):
    """struct bmx_template (include/bmx.h): reference r names group ``ref[r]``; literal r (``lit_off``, ``lit_len`` into the
    unescaped literal bytes) stands in front of it, literal ``n_refs`` behind the last one."""
    _fields_ = [("n_refs", C.c_int32), ("ref", C.c_int32 * MAX_TEMPLATE_REFS), ("lit_off", C.c_uint32 * (MAX_TEMPLATE_REFS + 1)),
                ("lit_len", C.c_uint32 * (MAX_TEMPLATE_REFS + 1)), ("lit_bytes", C.c_uint32)]


def compile_template(template, n_groups: int) -> Tuple[Template, bytes]:
    """A replacement template (bmx_compile_template: literal bytes, ``\\1``..``\\9``, ``\\g<0>``..``\\g<16>``, ``\\\\``) ->
    (Template, the literal bytes).  Anything else behind a backslash, a digit right behind ``\\1``..``\\9``, a reference above
    ``n_groups`` and more than 32 references are refused."""
    t = _pat_bytes(template) if len(template) else b""
    out = Template()
    lits = C.create_string_buffer(max(len(t), 1))
    _check(lib().bmx_compile_template(t, len(t), int(n_groups), C.byref(out), lits), "bmx_compile_template")
    return out, lits.raw[: out.lit_bytes]


def reverse_regex(expr_or_regex, flags: int = 0) -> Regex:
    """The reversed automaton (bmx_regex_reverse): position i becomes m - 1 - i, first and last swap, follow is transposed,
    the classes are mirrored; it matches the mirror image of what the input matches.  An expression is compiled with
    compile_regex(expr, flags) first."""
    re_ = _regex(expr_or_regex, flags)
    out = Regex()
    _check(lib().bmx_regex_reverse(C.byref(re_), C.byref(out)), "bmx_regex_reverse")
    return out


class RegexLong(C.Structure):
    """struct bmx_regex_long (include/bmx.h): the position automaton of a star-free regular expression of up to 128
    positions, plain data.  A set is two words, position i bit (i & 63) of word (i >> 6); ``first_set`` / ``last_set`` /
    ``follow_set(i)`` give one as a Python int."""
    _fields_ = [("m", C.c_int32), ("min_len", C.c_int32), ("max_len", C.c_int32), ("pad", C.c_int32), ("first", C.c_uint64 * 2),
                ("last", C.c_uint64 * 2), ("follow", (C.c_uint64 * 2) * MAX_REGEX_LONG_POSITIONS),
                ("classes", C.c_uint8 * (MAX_REGEX_LONG_POSITIONS * CLASS_BYTES))]

    @property
    def first_set(self) -> int:
        return int(self.first[0]) | int(self.first[1]) << 64

    @property
    def last_set(self) -> int:
        return int(self.last[0]) | int(self.last[1]) << 64

    def follow_set(self, i: int) -> int:
        return int(self.follow[i][0]) | int(self.follow[i][1]) << 64

    def class_array(self) -> np.ndarray:
        """The classes of the m positions, uint8 [m, 32]."""
        return np.frombuffer(bytes(self.classes), dtype=np.uint8).reshape(MAX_REGEX_LONG_POSITIONS, CLASS_BYTES)[: self.m].copy()


def compile_regex_long(expr, flags: int = 0) -> RegexLong:
    """A star-free regular expression of up to 128 positions (bmx_compile_regex_long: compile_regex's grammar, flags and
    errors) -> its position automaton."""
    e = _pat_bytes(expr)
    out = RegexLong()
    _check(lib().bmx_compile_regex_long(e, len(e), int(flags), C.byref(out)), "bmx_compile_regex_long")
    return out


def widen_regex(expr_or_regex, flags: int = 0) -> RegexLong:
    """The automaton of a Regex (or of compile_regex(expr, flags)) in the wide structure (bmx_regex_long_widen)."""
    re_ = _regex(expr_or_regex, flags)
    out = RegexLong()
    _check(lib().bmx_regex_long_widen(C.byref(re_), C.byref(out)), "bmx_regex_long_widen")
    return out


def _regex_long(expr_or_regex, flags: int = 0) -> RegexLong:
    """A RegexLong from an expression (str / bytes) or such a structure, passed through."""
    if isinstance(expr_or_regex, (str, bytes, bytearray)):
        return compile_regex_long(expr_or_regex, flags)
    if not isinstance(expr_or_regex, RegexLong):
        raise ValueError("expr_or_regex: an expression or a RegexLong")
    return expr_or_regex


class RegexAnchors(C.Structure):
    """struct bmx_regex_anchors (include/bmx.h), beside a Regex: the bytes admitted BEFORE a match for every position of
    ``first`` and AFTER it for every position of ``last``, 32 bytes per position as compile_classes; a full class is no
    condition."""
    _fields_ = [("before", C.c_uint8 * (MAX_REGEX_POSITIONS * CLASS_BYTES)), ("after", C.c_uint8 * (MAX_REGEX_POSITIONS * CLASS_BYTES))]

    @classmethod
    def full(cls) -> "RegexAnchors":
        """No condition anywhere: every anchored entry then returns its unanchored counterpart's list."""
        out = cls()
        C.memset(C.byref(out), 0xFF, C.sizeof(out))
        return out

    def before_array(self) -> np.ndarray:
        return np.frombuffer(bytes(self.before), dtype=np.uint8).reshape(MAX_REGEX_POSITIONS, CLASS_BYTES).copy()

    def after_array(self) -> np.ndarray:
        return np.frombuffer(bytes(self.after), dtype=np.uint8).reshape(MAX_REGEX_POSITIONS, CLASS_BYTES).copy()


def compile_regex_anchored(expr, flags: int = 0) -> Tuple[Regex, RegexAnchors]:
    """A star-free regular expression with the zero-width atoms ``^ $ \\b \\B \\< \\>`` (bmx_compile_regex_anchored; what
    Python's re means by them on bytes with re.MULTILINE; flags: compile_regex's, REGEX_WORD for grep -w, REGEX_LINE for
    grep -x) -> (automaton, anchors).  Exact, or BmxError(ERR_ARG): it never approximates."""
    e = _pat_bytes(expr)
    re_, an = Regex(), RegexAnchors()
    _check(lib().bmx_compile_regex_anchored(e, len(e), int(flags), C.byref(re_), C.byref(an)), "bmx_compile_regex_anchored")
    return re_, an


def _regex_anchored(expr_or_pair, flags: int = 0) -> Tuple[Regex, RegexAnchors]:
    """(Regex, RegexAnchors) from an expression or such a pair, passed through."""
    if isinstance(expr_or_pair, (str, bytes, bytearray)):
        return compile_regex_anchored(expr_or_pair, flags)
    if not (isinstance(expr_or_pair, tuple) and len(expr_or_pair) == 2 and isinstance(expr_or_pair[0], Regex)
            and isinstance(expr_or_pair[1], RegexAnchors)):
        raise ValueError("expr_or_pair: an expression or (Regex, RegexAnchors)")
    return expr_or_pair


def _posix_args(kind="regex", merge=False, longest=None, **_):
    """What posix=True of sub / findall goes with (checked before any GPU work)."""
    if kind not in ("regex", "regex_star", "regex_anchored", "regex_groups") or merge or longest is not None:
        raise ValueError("posix: kind 'regex', 'regex_star', 'regex_anchored' or 'regex_groups' only, without merge and without an explicit longest")


def _regex(expr_or_regex, flags: int = 0, star: bool = False) -> Regex:
    """A Regex from an expression (str / bytes) or such a structure, passed through."""
    if isinstance(expr_or_regex, (str, bytes, bytearray)):
        return compile_regex_star(expr_or_regex, flags) if star else compile_regex(expr_or_regex, flags)
    if not isinstance(expr_or_regex, Regex):
        raise ValueError("expr_or_regex: an expression or a Regex")
    return expr_or_regex


class Context:
    """One GPU.  Mirrors the reference's per-iteration context/queue
    (BoyreMoore.cpp:217-231) but is created once and reused."""

    def __init__(self, device: int = 0, library=None):
        self._L = library if library is not None else lib()
        self._h = C.c_void_p()
        self._chk(self._L.bmx_ctx_create(device, C.byref(self._h)), "bmx_ctx_create")
        self.device = device

    def _chk(self, rc: int, what: str, allow=()):
        return _check(rc, what, allow, self._L)

    def close(self):
        if self._h:
            self._L.bmx_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def set_order_overlap(self, on: bool = True):
        """bmx_set_order_overlap: this context's ordering kernel on a stream of its own behind the scan (searches of several
        contexts enqueued on one stream then scan back to back)."""
        self._chk(self._L.bmx_set_order_overlap(self._h, 1 if on else 0), "bmx_set_order_overlap")

    def set_knob(self, name: str, value: int):
        """libbmx_exp.so only (bmx_exp_set_knob): max_grid, no_dense, no_text_sample, multi_no_qgram, ed_lag, ed_group, ed_step_x,
        ed_stamp_block, sa_flags, index_no_dir, align_ws_kib, ordered_seq, tile_piece_shift, tile_max_grid, select_tile_shift,
        regex_begins_piece_shift, regex_star_begins_force_slow, regex_star_begins_piece_shift, regex_star_begins_warm,
        regex_star_ends_no_early_exit (include/bmx_exp.h)."""
        self._chk(self._L.bmx_exp_set_knob(self._h, name.encode(), int(value)), "bmx_exp_set_knob")

    def last_launch(self, session: str) -> Tuple[int, int, int]:
        """libbmx_exp.so only (bmx_exp_last_launch): (piece shift, workgroups, tiles) of the last launch of the session
        "approx", "approx_long", "classes", "hamming", "gaps", "regex", "regex_begins", "regex_star", "regex_star_begins" or "dict"; "rows": (log2 of the bytes
        of a tile, workgroups, tiles) of the last rows_split_device; "select": (log2 T, levels of pointer jumping, tiles of T
        entries) of the last select_spans_device."""
        out = (C.c_uint64 * 3)()
        self._chk(self._L.bmx_exp_last_launch(self._h, session.encode(), out), "bmx_exp_last_launch")
        return int(out[0]), int(out[1]), int(out[2])

    def regex_star_last(self) -> dict:
        """libbmx_exp.so only (bmx_exp_regex_star_last): what the last search_regex_star_device did."""
        out = (C.c_uint64 * 10)()
        self._chk(self._L.bmx_exp_regex_star_last(self._h, out), "bmx_exp_regex_star_last")
        keys = ["tainted", "slow", "piece_shift", "warm", "pieces", "columns", "first_us", "r1_us", "sweep_us", "r2_us"]
        return dict(zip(keys, [int(v) for v in out]))

    def regex_star_begins_last(self) -> dict:
        """libbmx_exp.so only (bmx_exp_regex_star_begins_last): what the last search_regex_star_begins_device did."""
        out = (C.c_uint64 * 10)()
        self._chk(self._L.bmx_exp_regex_star_begins_last(self._h, out), "bmx_exp_regex_star_begins_last")
        keys = ["tainted", "slow", "piece_shift", "warm", "pieces", "columns", "first_us", "r1_us", "sweep_us", "r2_us"]
        return dict(zip(keys, [int(v) for v in out]))

    def ed_stamps(self):
        """libbmx_exp.so only (bmx_exp_ed_stamps): cycle counts of one band of the last edit distance (ed variants 11, 12, 13), the
        timeline of one hand-over and every band's clock at four of its groups (variant 13)."""
        out = (C.c_uint64 * (24 + 64 * 4))()
        self._chk(self._L.bmx_exp_ed_stamps(self._h, out), "bmx_exp_ed_stamps")
        keys = ["groups", "cycles_in_steps", "cycles_between", "cycles_loop", "cycles_validate", "steps_per_group", "rows_per_step", "band_steps"]
        d = dict(zip(keys, [int(v) for v in out[:8]]))
        t = [int(v) for v in out[8:16]]
        if t[0]:  # one hand-over's timeline, microseconds after the band in front finished its group 200
            names = ["publisher_stores_issued", None, None, "feeder_batch_valid", "feeder_batch_fed", "eq_words_there", "main_behind_starts_group"]
            d["handover_us"] = {n: round((t[i + 1] - t[0]) / 100.0, 2) for i, n in enumerate(names) if n and t[i + 1]}
            if t[2] and t[3]:  # the start: the band behind begins its first group this long after the band in front ended its group 2
                u = [int(v) for v in out[16:19]]
                d["handover_us"]["at_the_start"] = {"group_2_in_front_published": round((u[2] - t[2]) / 100.0, 2), "batch_1_fed": round((u[0] - t[2]) / 100.0, 2),
                                                     "eq_words_of_33_steps_there": round((u[1] - t[2]) / 100.0, 2), "first_group_behind_starts": round((t[3] - t[2]) / 100.0, 2)}
        d["band_clock"] = [[int(out[24 + 4 * b + k]) for k in range(4)] for b in range(64)]
        return d

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- host buffers ------------------------------------------------------
    def search(self, text, pattern, capacity: Optional[int] = None) -> np.ndarray:
        """Ascending start offsets of every occurrence of pattern in text."""
        pat = _pat_bytes(pattern)
        tptr, n, keep = _host_text(text)
        m = len(pat)
        cap = capacity if capacity is not None else max(1, min(max(n - m + 1, 1), 1 << 20))
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search(self._h, tptr, n, pat, m, out.ctypes.data_as(_u64p), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search")
            del keep
            return out[: int(total.value)].copy()

    def search_ranges(self, text, pattern, ranges, tables=None) -> np.ndarray:
        """Reference kernel contract: counts per inclusive range [se[2r], se[2r+1]]."""
        pat = _pat_bytes(pattern)
        tptr, n, keep = _host_text(text)
        se = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1)
        P = se.size // 2
        ans = np.zeros(max(P, 1), dtype=np.int32)
        gp = bp = None
        if tables is not None:
            bad, good = tables
            bad = np.ascontiguousarray(bad, dtype=np.int32)
            good = np.ascontiguousarray(good, dtype=np.int32)
            gp, bp = good.ctypes.data_as(_i32p), bad.ctypes.data_as(_i32p)
        self._chk(self._L.bmx_search_ranges(self._h, tptr, n, pat, se.ctypes.data_as(_i32p), P,
                                       ans.ctypes.data_as(_i32p), gp, bp, len(pat)), "bmx_search_ranges")
        return ans[:P].copy()

    # -- device-resident text ---------------------------------------------
    def search_device(self, d_text, pattern, *, n: Optional[int] = None, n_own: Optional[int] = None,
                      base_offset: int = 0, out=None, capacity: Optional[int] = None, tables=None):
        """Scan a text resident in HBM.  ``d_text``/``out`` are torch CUDA tensors
        (uint8 / int64-or-uint64 storage).  Returns (positions tensor view, total)."""
        import torch

        pat = _pat_bytes(pattern)
        m = len(pat)
        if n is None:
            n = d_text.numel()
        if n_own is None:
            n_own = n
        if out is None:
            cap = capacity if capacity is not None else 1 << 16
            out = torch.empty(max(cap, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        gp = bp = None
        if tables is not None:
            bad, good = tables
            bad = np.ascontiguousarray(bad, dtype=np.int32)
            good = np.ascontiguousarray(good, dtype=np.int32)
            gp, bp = good.ctypes.data_as(_i32p), bad.ctypes.data_as(_i32p)
        stream = C.c_void_p(torch.cuda.current_stream(d_text.device).cuda_stream)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_device(self._h, C.c_void_p(d_text.data_ptr()), n, n_own, base_offset, pat, m, gp, bp,
                                     C.c_void_p(out.data_ptr()), cap, C.byref(total), stream)
        self._chk(rc, "bmx_search_device", allow=(ERR_CAPACITY,))
        return out[: min(int(total.value), cap)], int(total.value)

    def search_device_multi(self, d_text, patterns, *, n: Optional[int] = None, n_own: Optional[int] = None,
                            base_offset: int = 0, out=None, capacity: Optional[int] = None):
        """Up to MAX_MULTI patterns in ONE pass over a text resident in HBM (bmx_search_device_multi).
        Returns a list with one positions tensor (a view of ``out``) per pattern, each ascending."""
        import torch

        pats = [_pat_bytes(p) for p in patterns]
        K = len(pats)
        if n is None:
            n = d_text.numel()
        if n_own is None:
            n_own = n
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else 1 << 16, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        arr = (C.c_char_p * K)(*pats)
        ms = (C.c_int32 * K)(*[len(p) for p in pats])
        counts = (C.c_uint64 * K)()
        first = (C.c_uint64 * K)()
        stream = C.c_void_p(torch.cuda.current_stream(d_text.device).cuda_stream)
        rc = self._L.bmx_search_device_multi(self._h, C.c_void_p(d_text.data_ptr()), n, n_own, base_offset, arr, ms, K,
                                           C.c_void_p(out.data_ptr()), cap, counts, first, stream)
        self._chk(rc, "bmx_search_device_multi")
        return [out[int(first[k]): int(first[k]) + int(counts[k])] for k in range(K)]

    def enqueue(self, d_text, pattern, out, *, n=None, n_own=None, base_offset=0, tables=None):
        """Launch scan + ordering on torch's current stream; no synchronisation."""
        import torch

        pat = _pat_bytes(pattern)
        if n is None:
            n = d_text.numel()
        if n_own is None:
            n_own = n
        gp = bp = None
        if tables is not None:
            bad, good = tables
            self._keep = (np.ascontiguousarray(bad, dtype=np.int32), np.ascontiguousarray(good, dtype=np.int32))
            bp, gp = self._keep[0].ctypes.data_as(_i32p), self._keep[1].ctypes.data_as(_i32p)
        stream = C.c_void_p(torch.cuda.current_stream(d_text.device).cuda_stream)
        self._chk(self._L.bmx_search_device_enqueue(self._h, C.c_void_p(d_text.data_ptr()), n, n_own, base_offset, pat,
                                               len(pat), gp, bp, C.c_void_p(out.data_ptr()), out.numel(), stream),
               "bmx_search_device_enqueue")

    def prepare(self, d_text, pattern, out, *, n=None, n_own=None, base_offset=0, tables=None):
        """Bind every argument of one search once; the returned object's enqueue()/finish()
        are then single C-ABI calls (for callers that repeat the same query, like bench.py)."""
        return PreparedSearch(self, d_text, pattern, out, n, n_own, base_offset, tables)

    def finish(self, out) -> int:
        import torch

        stream = C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_device_finish(self._h, C.c_void_p(out.data_ptr()), out.numel(), C.byref(total), stream)
        self._chk(rc, "bmx_search_device_finish", allow=(ERR_CAPACITY,))
        return int(total.value)

    def count_to_device(self, d_dst):
        """Publish the last enqueue's match count into d_dst[0] on torch's current stream."""
        import torch

        stream = C.c_void_p(torch.cuda.current_stream(d_dst.device).cuda_stream)
        self._chk(self._L.bmx_count_to_device(self._h, C.c_void_p(d_dst.data_ptr()), stream), "bmx_count_to_device")

    def merge_gathered(self, gathered, world: int, slot_stride: int, merged, d_total, seq: int = 0):
        """d_total: 3 x int64, device memory or PINNED host memory (then poll d_total[2] == seq)."""
        import torch

        stream = C.c_void_p(torch.cuda.current_stream(gathered.device).cuda_stream)
        self._chk(self._L.bmx_merge_gathered_device(self._h, C.c_void_p(gathered.data_ptr()), world, slot_stride,
                                               C.c_void_p(merged.data_ptr()), merged.numel(),
                                               C.c_void_p(d_total.data_ptr()), seq, stream),
               "bmx_merge_gathered_device")

    def last_scan_ms(self) -> float:
        return float(self._L.bmx_last_scan_ms(self._h))

    def scan_ms_history(self, n: int = 64):
        """Durations (ms) of the most recent scan kernels, newest first (ring of 64)."""
        buf = (C.c_float * max(n, 1))()
        got = self._L.bmx_scan_ms_history(self._h, buf, n)
        if got < 0:
            raise BmxError(got, "bmx_scan_ms_history", self._L.bmx_last_error().decode(errors="replace"))
        return [float(buf[i]) for i in range(got)]

    def scan_stamps(self, max_words: int = 1 << 16) -> np.ndarray:
        buf = np.zeros(max_words, dtype=np.uint64)
        got = self._L.bmx_scan_stamps(self._h, buf.ctypes.data_as(_u64p), max_words)
        if got < 0:
            raise BmxError(got, "bmx_scan_stamps", self._L.bmx_last_error().decode(errors="replace"))
        return buf[:got].reshape(-1, 8)

    def geometry(self, m: int) -> dict:
        g = (C.c_uint64 * 6)()
        self._chk(self._L.bmx_scan_geometry(self._h, m, g), "bmx_scan_geometry")
        return {"grid": int(g[0]), "block": int(g[1]), "tile_bytes": int(g[2]), "lds_bytes": int(g[3]),
                "seg": int(g[4]), "kind": ("workgroup-tile", "wave-stream", "workgroup-ring")[int(g[5])]}

    def stream_wait_last_scan(self, stream) -> None:
        """Make ``stream`` (a torch.cuda.Stream) wait for the scan kernel of this context's latest enqueue."""
        self._chk(self._L.bmx_stream_wait_last_scan(self._h, C.c_void_p(stream.cuda_stream)), "bmx_stream_wait_last_scan")

    def last_search_sorted(self) -> bool:
        """Did the last finish() have to sort (the list was unordered until then)?"""
        return bool(self._L.bmx_last_search_sorted(self._h))

    def last_variant(self) -> int:
        """The slot of the kernel table the most recent search ran."""
        return int(self._L.bmx_last_variant(self._h))

    def set_variant(self, variant: int, blocks_per_cu: int = 0):
        self._chk(self._L.bmx_set_variant(self._h, variant, blocks_per_cu), "bmx_set_variant")

    # -- edit distance (the reference's second algorithm) --------------------
    def edit_distance(self, a, b) -> int:
        """Levenshtein distance of two host strings (EditDistance-1.cpp's contract: the
        last cell of the table)."""
        pa, la, ka = _host_text(a)
        pb, lb, kb = _host_text(b)
        d = C.c_uint64(0)
        self._chk(self._L.bmx_edit_distance(self._h, pa, la, pb, lb, C.byref(d)), "bmx_edit_distance")
        return int(d.value)

    def edit_distance_device(self, d_a, d_b) -> int:
        import torch

        stream = C.c_void_p(torch.cuda.current_stream(d_a.device).cuda_stream)
        d = C.c_uint64(0)
        self._chk(self._L.bmx_edit_distance_device(self._h, C.c_void_p(d_a.data_ptr()), d_a.numel(),
                                              C.c_void_p(d_b.data_ptr()), d_b.numel(), C.byref(d), stream),
               "bmx_edit_distance_device")
        return int(d.value)

    def last_edit_distance_ms(self) -> float:
        return float(self._L.bmx_last_edit_distance_ms(self._h))

    def set_ed_variant(self, v: int):
        """Edit-distance schedule (include/bmx.h).  The product library accepts 0 and 13 with the flags +16 / +32; every other
        slot raises BmxError(ERR_ARG) unless this context is one of exp_lib()."""
        self._chk(self._L.bmx_set_ed_variant(self._h, v), "bmx_set_ed_variant")

    # -- batched edit distance: many string pairs in one call ---------------------------
    def edit_distance_batch(self, a, b, limit: Optional[int] = None) -> np.ndarray:
        """Levenshtein distances of a column of pairs, host buffers (bmx_edit_distance_batch): uint32, one per string of
        ``b``.  ``a`` and ``b``: sequences of bytes / str, or (blob, offsets) numpy pairs; a single bytes / str ``a`` is
        measured against every string of ``b``.  With ``limit`` the values are min(distance, limit + 1)."""
        ablob, aoff = pack_strings([a] if isinstance(a, (bytes, bytearray, str)) else a)
        bblob, boff = pack_strings(b)
        count = boff.size - 1
        dist = np.empty(max(count, 1), dtype=np.uint32)
        rc = self._L.bmx_edit_distance_batch(self._h, C.c_void_p(ablob.ctypes.data), ablob.size, C.c_void_p(aoff.ctypes.data),
                                             aoff.size - 1, C.c_void_p(bblob.ctypes.data), bblob.size,
                                             C.c_void_p(boff.ctypes.data), count, ED_NO_LIMIT if limit is None else int(limit),
                                             C.c_void_p(dist.ctypes.data))
        self._chk(rc, "bmx_edit_distance_batch")
        return dist[:count]

    def edit_distance_batch_device(self, d_a, d_a_off, d_b, d_b_off, count: int, *, a_count: Optional[int] = None,
                                   limit: Optional[int] = None, out=None):
        """The same on CUDA tensors (bmx_edit_distance_batch_device): ``d_a`` / ``d_b`` uint8 blobs, ``d_a_off`` / ``d_b_off``
        int64 or uint64 offsets (count + 1 entries; two for ``d_a_off`` with a_count = 1), ``out`` an int32 / uint32 tensor
        of at least ``count`` entries (allocated if None).  Runs on torch's current stream and returns after synchronising
        it; the result is the first ``count`` entries of ``out``."""
        import torch

        if a_count is None:
            a_count = count
        if out is None:
            out = torch.empty(max(count, 1), dtype=torch.int32, device=d_b_off.device)
        if out.numel() < count or out.element_size() != 4 or d_a_off.element_size() != 8 or d_b_off.element_size() != 8:
            raise ValueError("out: 4-byte entries, at least count of them; offsets: 8-byte entries")
        if d_a_off.numel() < a_count + 1 or d_b_off.numel() < count + 1:
            raise ValueError("offset tensors need one entry more than strings")
        if d_a.element_size() != 1 or d_b.element_size() != 1:
            raise ValueError("blobs: 1-byte entries (uint8)")
        stream = C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)
        rc = self._L.bmx_edit_distance_batch_device(self._h, C.c_void_p(d_a.data_ptr()), d_a.numel(),
                                                    C.c_void_p(d_a_off.data_ptr()), a_count, C.c_void_p(d_b.data_ptr()),
                                                    d_b.numel(), C.c_void_p(d_b_off.data_ptr()), count,
                                                    ED_NO_LIMIT if limit is None else int(limit), C.c_void_p(out.data_ptr()),
                                                    stream)
        self._chk(rc, "bmx_edit_distance_batch_device")
        return out[:count]

    def last_ed_batch_ms(self) -> float:
        return float(self._L.bmx_last_ed_batch_ms(self._h))

    def last_ed_batch_fallbacks(self) -> int:
        return int(self._L.bmx_last_ed_batch_fallbacks(self._h))

    # -- approximate search: ends of matches within k edits ---------------------------
    def search_approx_device(self, d_text, pattern, k: int, *, n: Optional[int] = None, lead: int = 0, base_offset: int = 0,
                             out=None, dist_out=None, capacity: Optional[int] = None):
        """Every end j in [lead, n) of the view ``d_text[0:n)`` with min over s of ED(pattern, text[s..j]) <= k, ascending,
        reported as base_offset + j (bmx_search_approx_device; a pattern of more than 64 and up to 512 bytes goes through
        bmx_search_approx_long_device).  ``out``: int64/uint64 CUDA tensor, ``dist_out``: uint8
        CUDA tensor (both allocated if None).  Returns (ends view, distances view, true total); the views hold the lowest
        min(total, capacity) ends.  A capacity below the total is not an error here (the total says so)."""
        import torch

        pat = _pat_bytes(pattern)
        if n is None:
            n = d_text.numel()
        if out is None:
            cap = capacity if capacity is not None else 1 << 16
            out = torch.empty(max(cap, 1), dtype=torch.int64, device=d_text.device)
        if dist_out is None:
            dist_out = torch.empty(max(out.numel(), 1), dtype=torch.uint8, device=d_text.device)
        cap = min(out.numel(), dist_out.numel()) if capacity is None else min(capacity, out.numel(), dist_out.numel())
        stream = C.c_void_p(torch.cuda.current_stream(d_text.device).cuda_stream)
        total = C.c_uint64(0)
        long = len(pat) > MAX_APPROX_PATTERN
        fn = self._L.bmx_search_approx_long_device if long else self._L.bmx_search_approx_device
        rc = fn(self._h, C.c_void_p(d_text.data_ptr()), n, lead, base_offset, pat, len(pat), int(k), C.c_void_p(out.data_ptr()),
                C.c_void_p(dist_out.data_ptr()), cap, C.byref(total), stream)
        self._chk(rc, "bmx_search_approx_long_device" if long else "bmx_search_approx_device", allow=(ERR_CAPACITY,))
        got = min(int(total.value), cap)
        return out[:got], dist_out[:got], int(total.value)

    def search_approx(self, text, pattern, k: int, capacity: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers (bmx_search_approx; bmx_search_approx_long for a pattern of more than 64 bytes): (ends uint64,
        distances uint8), ascending.  With ``capacity`` given and too small, raises BmxError(ERR_CAPACITY); without it the
        list is always complete."""
        pat = _pat_bytes(pattern)
        long = len(pat) > MAX_APPROX_PATTERN
        fn = self._L.bmx_search_approx_long if long else self._L.bmx_search_approx
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            ends = np.empty(max(cap, 1), dtype=np.uint64)
            dist = np.empty(max(cap, 1), dtype=np.uint8)
            total = C.c_uint64(0)
            rc = fn(self._h, tptr, n, pat, len(pat), int(k), C.c_void_p(ends.ctypes.data), C.c_void_p(dist.ctypes.data), cap,
                    C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_approx_long" if long else "bmx_search_approx")
            del keep
            t = int(total.value)
            return ends[:t].copy(), dist[:t].copy()

    def last_approx_ms(self) -> float:
        return float(self._L.bmx_last_approx_ms(self._h))

    # -- class-pattern search: wildcards, sets, case folding, IUPAC codes -----------------
    def search_classes_device(self, d_text, classes_or_expr, *, flags: int = 0, n: Optional[int] = None,
                              n_own: Optional[int] = None, base_offset: int = 0, capacity: Optional[int] = None, out=None,
                              stream=None):
        """Every start p < n_own of the view ``d_text[0:n)`` with text[p + i] in class i for all i, ascending, reported as
        base_offset + p (bmx_search_classes_device).  ``classes_or_expr``: an expression for compile_classes(expr, flags)
        or a [m, 32] uint8 array.  ``out``: int64/uint64 CUDA tensor (allocated if None); ``stream``: a torch.cuda.Stream
        (None: torch's current stream).  Returns (starts view, true total); the view holds the lowest min(total, capacity)
        starts.  A capacity below the total is not an error here (the total says so)."""
        import torch

        cls = _classes(classes_or_expr, flags)
        if n is None:
            n = d_text.numel()
        if n_own is None:
            n_own = n
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else 1 << 16, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        s = stream if stream is not None else torch.cuda.current_stream(d_text.device)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_classes_device(self._h, C.c_void_p(d_text.data_ptr()), n, n_own, base_offset,
                                               C.c_void_p(cls.ctypes.data), cls.shape[0], C.c_void_p(out.data_ptr()), cap,
                                               C.byref(total), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_search_classes_device", allow=(ERR_CAPACITY,))
        return out[: min(int(total.value), cap)], int(total.value)

    def search_classes(self, text, classes_or_expr, flags: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """Host buffers (bmx_search_classes): ascending starts, uint64.  With ``capacity`` given and too small, raises
        BmxError(ERR_CAPACITY); without it the list is always complete."""
        cls = _classes(classes_or_expr, flags)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_classes(self._h, tptr, n, C.c_void_p(cls.ctypes.data), cls.shape[0],
                                            C.c_void_p(out.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_classes")
            del keep
            return out[: int(total.value)].copy()

    def search_approx_classes_device(self, d_text, classes_or_expr, k: int, *, flags: int = 0, n: Optional[int] = None,
                                     lead: int = 0, base_offset: int = 0, out=None, dist_out=None,
                                     capacity: Optional[int] = None, stream=None):
        """search_approx_device with a class per pattern position (bmx_search_approx_classes_device): (ends view,
        distances view, true total).  ``stream``: a torch.cuda.Stream (None: torch's current stream)."""
        import torch

        cls = _classes(classes_or_expr, flags)
        if n is None:
            n = d_text.numel()
        if out is None:
            cap = capacity if capacity is not None else 1 << 16
            out = torch.empty(max(cap, 1), dtype=torch.int64, device=d_text.device)
        if dist_out is None:
            dist_out = torch.empty(max(out.numel(), 1), dtype=torch.uint8, device=d_text.device)
        cap = min(out.numel(), dist_out.numel()) if capacity is None else min(capacity, out.numel(), dist_out.numel())
        stream = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(d_text.device)).cuda_stream)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_approx_classes_device(self._h, C.c_void_p(d_text.data_ptr()), n, lead, base_offset,
                                                      C.c_void_p(cls.ctypes.data), cls.shape[0], int(k),
                                                      C.c_void_p(out.data_ptr()), C.c_void_p(dist_out.data_ptr()), cap,
                                                      C.byref(total), stream)
        self._chk(rc, "bmx_search_approx_classes_device", allow=(ERR_CAPACITY,))
        got = min(int(total.value), cap)
        return out[:got], dist_out[:got], int(total.value)

    def last_classes_ms(self) -> float:
        return float(self._L.bmx_last_classes_ms(self._h))

    # -- k-mismatch (Hamming) search: at most k substitutions -------------------------------
    @staticmethod
    def _hamming_pattern(pattern_or_classes, flags: int):
        """(string bytes or None, classes array or None): str / bytes are a STRING, unless ``flags`` (CLASS_*) are given,
        which make them an expression for compile_classes; a [m, 32] uint8 array is a class pattern."""
        if isinstance(pattern_or_classes, (str, bytes, bytearray)) and not flags:
            return _pat_bytes(pattern_or_classes), None
        return None, _classes(pattern_or_classes, flags)

    def search_hamming_device(self, d_text, pattern_or_classes, k: int, *, must=None, flags: int = 0, n: Optional[int] = None,
                              n_own: Optional[int] = None, base_offset: int = 0, out=None, dist_out=None, stream=None):
        """Every start p < n_own of the view ``d_text[0:n)`` at which at most k positions i have text[p + i] outside
        position i of the pattern and none of them is in ``must`` (an int mask or an iterable of positions), ascending,
        reported as base_offset + p (bmx_search_hamming[_classes]_device).  ``pattern_or_classes``: str / bytes are a
        STRING, a [m, 32] uint8 array is a class pattern; with ``flags`` (CLASS_ICASE, CLASS_IUPAC) str / bytes are an
        expression for compile_classes.  ``out``: int64/uint64 CUDA tensor, ``dist_out``: uint8 CUDA tensor (both allocated
        if None); ``stream``: a torch.cuda.Stream (None: torch's current stream).  Returns (starts view, distances view,
        true total); the views hold the lowest min(total, capacity) starts.  A capacity below the total is not an error
        here (the total says so)."""
        import torch

        pat, cls = self._hamming_pattern(pattern_or_classes, flags)
        if n is None:
            n = d_text.numel()
        if n_own is None:
            n_own = n
        if out is None:
            out = torch.empty(1 << 16, dtype=torch.int64, device=d_text.device)
        if dist_out is None:
            dist_out = torch.empty(max(out.numel(), 1), dtype=torch.uint8, device=d_text.device)
        cap = min(out.numel(), dist_out.numel())
        s = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(d_text.device)).cuda_stream)
        total = C.c_uint64(0)
        head = (self._h, C.c_void_p(d_text.data_ptr()), n, n_own, base_offset)
        tail = (int(k), _must_mask(must), C.c_void_p(out.data_ptr()), C.c_void_p(dist_out.data_ptr()), cap, C.byref(total), s)
        if pat is not None:
            what = "bmx_search_hamming_device"
            rc = self._L.bmx_search_hamming_device(*head, pat, len(pat), *tail)
        else:
            what = "bmx_search_hamming_classes_device"
            rc = self._L.bmx_search_hamming_classes_device(*head, C.c_void_p(cls.ctypes.data), cls.shape[0], *tail)
        self._chk(rc, what, allow=(ERR_CAPACITY,))
        got = min(int(total.value), cap)
        return out[:got], dist_out[:got], int(total.value)

    def search_hamming(self, text, pattern_or_classes, k: int, must=None, flags: int = 0,
                       capacity: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers (bmx_search_hamming[_classes]): (starts uint64, distances uint8), ascending.  With ``capacity``
        given and too small, raises BmxError(ERR_CAPACITY); without it the list is always complete."""
        pat, cls = self._hamming_pattern(pattern_or_classes, flags)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        mask = _must_mask(must)
        while True:
            starts = np.empty(max(cap, 1), dtype=np.uint64)
            dist = np.empty(max(cap, 1), dtype=np.uint8)
            total = C.c_uint64(0)
            tail = (int(k), mask, C.c_void_p(starts.ctypes.data), C.c_void_p(dist.ctypes.data), cap, C.byref(total))
            if pat is not None:
                what = "bmx_search_hamming"
                rc = self._L.bmx_search_hamming(self._h, tptr, n, pat, len(pat), *tail)
            else:
                what = "bmx_search_hamming_classes"
                rc = self._L.bmx_search_hamming_classes(self._h, tptr, n, C.c_void_p(cls.ctypes.data), cls.shape[0], *tail)
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, what)
            del keep
            t = int(total.value)
            return starts[:t].copy(), dist[:t].copy()

    def last_hamming_ms(self) -> float:
        return float(self._L.bmx_last_hamming_ms(self._h))

    # -- gapped pattern search: optional and counted classes, PROSITE ----------------------
    def search_gaps_device(self, d_text, expr_or_pair, *, flags: int = 0, n: Optional[int] = None, lead: int = 0,
                           base_offset: int = 0, out=None, capacity: Optional[int] = None, stream=None):
        """Every end j in [lead, n) of the view ``d_text[0:n)`` at which a match of the gapped pattern ends, ascending,
        reported as base_offset + j (bmx_search_gaps_device).  ``expr_or_pair``: an expression for compile_gaps(expr,
        flags) or its result (classes [m, 32] uint8, optional).  ``out``: int64/uint64 CUDA tensor (allocated if None);
        ``stream``: a torch.cuda.Stream (None: torch's current stream).  Returns (ends view, true total); the view holds
        the lowest min(total, capacity) ends.  A capacity below the total is not an error here (the total says so)."""
        import torch

        cls, optional = _gaps(expr_or_pair, flags)
        if n is None:
            n = d_text.numel()
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else 1 << 16, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        s = stream if stream is not None else torch.cuda.current_stream(d_text.device)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_gaps_device(self._h, C.c_void_p(d_text.data_ptr()), n, lead, base_offset,
                                            C.c_void_p(cls.ctypes.data), cls.shape[0], optional, C.c_void_p(out.data_ptr()),
                                            cap, C.byref(total), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_search_gaps_device", allow=(ERR_CAPACITY,))
        return out[: min(int(total.value), cap)], int(total.value)

    def search_gaps(self, text, expr_or_pair, flags: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """Host buffers (bmx_search_gaps): ascending ends, uint64.  With ``capacity`` given and too small, raises
        BmxError(ERR_CAPACITY); without it the list is always complete."""
        cls, optional = _gaps(expr_or_pair, flags)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_gaps(self._h, tptr, n, C.c_void_p(cls.ctypes.data), cls.shape[0], optional,
                                         C.c_void_p(out.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_gaps")
            del keep
            return out[: int(total.value)].copy()

    def search_gaps_spans(self, text, expr_or_pair, flags: int = 0, longest: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers (bmx_search_gaps_spans): (starts uint64, ends uint64) of every match, ends ascending; each start
        the largest one for its end, or with ``longest`` the smallest."""
        cls, optional = _gaps(expr_or_pair, flags)
        tptr, n, keep = _host_text(text)
        cap = max(1, min(n, 1 << 20))
        while True:
            starts = np.empty(cap, dtype=np.uint64)
            ends = np.empty(cap, dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_gaps_spans(self._h, tptr, n, C.c_void_p(cls.ctypes.data), cls.shape[0], optional,
                                               GAPS_LONGEST if longest else 0, C.c_void_p(starts.ctypes.data),
                                               C.c_void_p(ends.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_gaps_spans")
            del keep
            t = int(total.value)
            return starts[:t].copy(), ends[:t].copy()

    def gaps_starts_device(self, d_text, expr_or_pair, ends, *, longest: bool = False, flags: int = 0,
                           n: Optional[int] = None, base_offset: int = 0, stream=None):
        """A start for every end of ``ends`` (int64 / uint64 CUDA tensor, as search_gaps_device returns it for the same
        view, pattern and base_offset): the largest one, or with ``longest`` the smallest one of the view
        (bmx_gaps_starts_device).  ``flags`` are the flags of compile_gaps where ``expr_or_pair`` is an expression.
        Returns the starts, a tensor like ``ends``."""
        import torch

        cls, optional = _gaps(expr_or_pair, flags)
        count = ends.numel()
        if n is None:
            n = d_text.numel()
        if ends.element_size() != 8:
            raise ValueError("ends: 8-byte entries")
        starts = torch.empty(max(count, 1), dtype=ends.dtype, device=ends.device)
        s = stream if stream is not None else torch.cuda.current_stream(ends.device)
        rc = self._L.bmx_gaps_starts_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset,
                                            C.c_void_p(cls.ctypes.data), cls.shape[0], optional, C.c_void_p(ends.data_ptr()),
                                            count, GAPS_LONGEST if longest else 0, C.c_void_p(starts.data_ptr()),
                                            C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_gaps_starts_device")
        return starts[:count]

    def last_gaps_ms(self) -> float:
        return float(self._L.bmx_last_gaps_ms(self._h))

    # -- regular-expression search: groups, alternation, counted repeats (star-free) -------
    def search_regex_device(self, d_text, expr_or_regex, *, flags: int = 0, n: Optional[int] = None, lead: int = 0,
                            base_offset: int = 0, out=None, capacity: Optional[int] = None, stream=None):
        """Every end j in [lead, n) of the view ``d_text[0:n)`` at which a match of the expression ends, ascending,
        reported as base_offset + j (bmx_search_regex_device).  ``expr_or_regex``: an expression for compile_regex(expr,
        flags) or its result.  ``out``, ``capacity``, ``stream`` and the return value (ends view, true total) are those
        of search_gaps_device."""
        import torch

        re_ = _regex(expr_or_regex, flags)
        if n is None:
            n = d_text.numel()
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else 1 << 16, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        s = stream if stream is not None else torch.cuda.current_stream(d_text.device)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_regex_device(self._h, C.c_void_p(d_text.data_ptr()), n, lead, base_offset, C.byref(re_),
                                             C.c_void_p(out.data_ptr()), cap, C.byref(total), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_search_regex_device", allow=(ERR_CAPACITY,))
        return out[: min(int(total.value), cap)], int(total.value)

    def search_regex(self, text, expr_or_regex, flags: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """Host buffers (bmx_search_regex): ascending ends, uint64.  With ``capacity`` given and too small, raises
        BmxError(ERR_CAPACITY); without it the list is always complete."""
        re_ = _regex(expr_or_regex, flags)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex(self._h, tptr, n, C.byref(re_), C.c_void_p(out.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex")
            del keep
            return out[: int(total.value)].copy()

    def search_regex_spans(self, text, expr_or_regex, flags: int = 0, longest: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers (bmx_search_regex_spans): (starts uint64, ends uint64) of every match, ends ascending; each start
        the largest one for its end, or with ``longest`` the smallest."""
        re_ = _regex(expr_or_regex, flags)
        tptr, n, keep = _host_text(text)
        cap = max(1, min(n, 1 << 20))
        while True:
            starts = np.empty(cap, dtype=np.uint64)
            ends = np.empty(cap, dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex_spans(self._h, tptr, n, C.byref(re_), REGEX_LONGEST if longest else 0,
                                                C.c_void_p(starts.ctypes.data), C.c_void_p(ends.ctypes.data), cap,
                                                C.byref(total))
            if rc == ERR_CAPACITY:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_spans")
            del keep
            t = int(total.value)
            return starts[:t].copy(), ends[:t].copy()

    def regex_starts_device(self, d_text, expr_or_regex, ends, *, longest: bool = False, flags: int = 0,
                            n: Optional[int] = None, base_offset: int = 0, stream=None):
        """A start for every end of ``ends`` (int64 / uint64 CUDA tensor, as search_regex_device returns it for the same
        view, expression and base_offset): the largest one, or with ``longest`` the smallest one of the view
        (bmx_regex_starts_device).  Returns the starts, a tensor like ``ends``."""
        import torch

        re_ = _regex(expr_or_regex, flags)
        count = ends.numel()
        if n is None:
            n = d_text.numel()
        if ends.element_size() != 8:
            raise ValueError("ends: 8-byte entries")
        starts = torch.empty(max(count, 1), dtype=ends.dtype, device=ends.device)
        s = stream if stream is not None else torch.cuda.current_stream(ends.device)
        rc = self._L.bmx_regex_starts_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, C.byref(re_),
                                             C.c_void_p(ends.data_ptr()), count, REGEX_LONGEST if longest else 0,
                                             C.c_void_p(starts.data_ptr()), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_regex_starts_device")
        return starts[:count]

    def last_regex_ms(self) -> float:
        return float(self._L.bmx_last_regex_ms(self._h))

    # -- ... capture groups ------------------------------------------------
    def regex_groups_device(self, d_text, expr_or_pair, starts, ends, *, flags: int = 0, n: Optional[int] = None,
                            base_offset: int = 0, stream=None):
        """The capture groups of every span ``[starts[i], ends[i]]`` (ends inclusive, as the searches pair them; int64 /
        uint64 CUDA tensors) of the resident text: an int64 tensor ``[count, G + 1, 2]`` of half-open ``(begin, end)``
        pairs, group 0 the match itself, -1 twice for a group that is unset (bmx_regex_groups_device).  The groups are
        those of Python's ``re.fullmatch`` on the span.  An entry whose start or end is -1, or whose end lies below its
        start, is skipped (all -1); a span that is no match of the expression raises BmxError(ERR_ARG).
        ``expr_or_pair``: an expression, or compile_regex_groups' pair."""
        import torch

        re_, gr = _regex_groups(expr_or_pair, flags)
        count = starts.numel()
        if n is None:
            n = d_text.numel()
        if starts.element_size() != 8 or ends.element_size() != 8 or ends.numel() != count:
            raise ValueError("starts, ends: 8-byte entries, as many of one as of the other")
        groups = torch.empty((max(count, 1), gr.n_groups + 1, 2), dtype=torch.int64, device=starts.device)
        s = stream if stream is not None else torch.cuda.current_stream(starts.device)
        rc = self._L.bmx_regex_groups_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, C.byref(re_), C.byref(gr),
                                             C.c_void_p(starts.data_ptr()), C.c_void_p(ends.data_ptr()), count,
                                             C.c_void_p(groups.data_ptr()), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_regex_groups_device")
        return groups[:count]

    def search_regex_groups(self, text, expr_or_pair, flags: int = 0, posix: bool = False):
        """Host buffers (bmx_search_regex_groups): (starts uint64, ends uint64, groups int64 [count, G + 1, 2]) of every
        match END, ends ascending; each start the largest one for its end (the shortest match), or with ``posix`` the
        smallest (the longest)."""
        re_, gr = _regex_groups(expr_or_pair, flags)
        tptr, n, keep = _host_text(text)
        cap = max(1, min(n, 1 << 20))
        while True:
            starts = np.empty(cap, dtype=np.uint64)
            ends = np.empty(cap, dtype=np.uint64)
            groups = np.empty((cap, gr.n_groups + 1, 2), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex_groups(self._h, tptr, n, C.byref(re_), C.byref(gr), REGEX_LONGEST if posix else 0,
                                                 C.c_void_p(starts.ctypes.data), C.c_void_p(ends.ctypes.data),
                                                 C.c_void_p(groups.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_groups")
            del keep
            t = int(total.value)
            return starts[:t].copy(), ends[:t].copy(), groups[:t].view(np.int64).copy()

    def expand_device(self, d_text, groups, template, extract: bool = False, n: Optional[int] = None, base_offset: int = 0,
                      out=None, stream=None):
        """``groups``: what regex_groups_device returned, its matches (group 0) ascending and pairwise disjoint, as after
        select_spans_device.  Default: (tensor, n_out), the view ``d_text[0:n)`` with every match replaced by the expansion
        of ``template`` (re.sub with ``\\1``..``\\9``, ``\\g<N>``, ``\\\\``; an unset group expands to nothing).  ``extract``:
        (blob, offsets), the expansions one after the other and count + 1 int64 offsets (Match.expand as a column)
        (bmx_expand_device).  ``out``: a uint8 CUDA tensor that does not overlap the text."""
        import torch

        if groups.dim() != 3 or groups.shape[2] != 2 or groups.element_size() != 8:
            raise ValueError("groups: an 8-byte tensor [count, G + 1, 2]")
        groups = groups.contiguous()
        count, n_groups = int(groups.shape[0]), int(groups.shape[1]) - 1
        tmpl = _pat_bytes(template) if len(template) else b""
        n = d_text.numel() if n is None else n
        s = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(d_text.device)).cuda_stream)
        off = torch.empty(count + 1, dtype=torch.int64, device=d_text.device) if extract else None
        total = C.c_uint64(0)

        def call(buf, cap):
            return self._L.bmx_expand_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset,
                                             C.c_void_p(groups.data_ptr()) if count else None, n_groups, count, tmpl, len(tmpl),
                                             EXPAND_EXTRACT if extract else 0, C.c_void_p(buf.data_ptr()) if buf is not None else None,
                                             cap, C.c_void_p(off.data_ptr()) if extract else None, C.byref(total), s)

        if out is None:
            self._chk(call(None, 0), "bmx_expand_device")
            out = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=d_text.device)
        self._chk(call(out, out.numel()), "bmx_expand_device")
        return (out[: int(total.value)], off) if extract else (out[: int(total.value)], int(total.value))

    def last_regex_groups_ms(self) -> float:
        return float(self._L.bmx_last_regex_groups_ms(self._h))

    # -- ... for expressions of up to 128 positions -------
    def search_regex_long_device(self, d_text, expr_or_regex, *, flags: int = 0, n: Optional[int] = None, lead: int = 0,
                                 base_offset: int = 0, out=None, capacity: Optional[int] = None, stream=None):
        """search_regex_device for an expression of up to 128 positions (bmx_search_regex_long_device).
        ``expr_or_regex``: an expression for compile_regex_long(expr, flags) or a RegexLong.  The other arguments and the
        return value (ends view, true total) are those of search_regex_device."""
        import torch

        re_ = _regex_long(expr_or_regex, flags)
        if n is None:
            n = d_text.numel()
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else 1 << 16, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        s = stream if stream is not None else torch.cuda.current_stream(d_text.device)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_regex_long_device(self._h, C.c_void_p(d_text.data_ptr()), n, lead, base_offset, C.byref(re_),
                                                  C.c_void_p(out.data_ptr()), cap, C.byref(total), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_search_regex_long_device", allow=(ERR_CAPACITY,))
        return out[: min(int(total.value), cap)], int(total.value)

    def search_regex_long(self, text, expr_or_regex, flags: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """Host buffers (bmx_search_regex_long): ascending ends, uint64; ``capacity`` as in search_regex."""
        re_ = _regex_long(expr_or_regex, flags)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex_long(self._h, tptr, n, C.byref(re_), C.c_void_p(out.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_long")
            del keep
            return out[: int(total.value)].copy()

    def search_regex_long_spans(self, text, expr_or_regex, flags: int = 0, longest: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers (bmx_search_regex_long_spans): (starts uint64, ends uint64) of every match, as search_regex_spans."""
        re_ = _regex_long(expr_or_regex, flags)
        tptr, n, keep = _host_text(text)
        cap = max(1, min(n, 1 << 20))
        while True:
            starts = np.empty(cap, dtype=np.uint64)
            ends = np.empty(cap, dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex_long_spans(self._h, tptr, n, C.byref(re_), REGEX_LONGEST if longest else 0,
                                                     C.c_void_p(starts.ctypes.data), C.c_void_p(ends.ctypes.data), cap,
                                                     C.byref(total))
            if rc == ERR_CAPACITY:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_long_spans")
            del keep
            t = int(total.value)
            return starts[:t].copy(), ends[:t].copy()

    def regex_long_starts_device(self, d_text, expr_or_regex, ends, *, longest: bool = False, flags: int = 0,
                                 n: Optional[int] = None, base_offset: int = 0, stream=None):
        """regex_starts_device for an expression of up to 128 positions (bmx_regex_long_starts_device): a start for every
        end of ``ends`` as search_regex_long_device returns it.  Returns the starts, a tensor like ``ends``."""
        import torch

        re_ = _regex_long(expr_or_regex, flags)
        count = ends.numel()
        if n is None:
            n = d_text.numel()
        if ends.element_size() != 8:
            raise ValueError("ends: 8-byte entries")
        starts = torch.empty(max(count, 1), dtype=ends.dtype, device=ends.device)
        s = stream if stream is not None else torch.cuda.current_stream(ends.device)
        rc = self._L.bmx_regex_long_starts_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, C.byref(re_),
                                                  C.c_void_p(ends.data_ptr()), count, REGEX_LONGEST if longest else 0,
                                                  C.c_void_p(starts.data_ptr()), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_regex_long_starts_device")
        return starts[:count]

    def last_regex_long_ms(self) -> float:
        return float(self._L.bmx_last_regex_long_ms(self._h))

    # -- ... its mirror image: every match start, and the end of every start (leftmost-longest) -------
    def search_regex_begins_device(self, d_text, expr_or_regex, *, flags: int = 0, n: Optional[int] = None, tail: int = 0,
                                   base_offset: int = 0, out=None, capacity: Optional[int] = None, stream=None):
        """Every start s in [0, n - tail) of the view ``d_text[0:n)`` at which a match of the expression begins (and ends
        inside the view), ascending, reported as base_offset + s (bmx_search_regex_begins_device).  ``tail``: a shard's view
        runs max_len - 1 bytes past its last owned start.  The other arguments and the return value (starts view, true
        total) are those of search_regex_device."""
        import torch

        re_ = _regex(expr_or_regex, flags)
        if n is None:
            n = d_text.numel()
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else 1 << 16, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        s = stream if stream is not None else torch.cuda.current_stream(d_text.device)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_regex_begins_device(self._h, C.c_void_p(d_text.data_ptr()), n, tail, base_offset, C.byref(re_),
                                                    C.c_void_p(out.data_ptr()), cap, C.byref(total), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_search_regex_begins_device", allow=(ERR_CAPACITY,))
        return out[: min(int(total.value), cap)], int(total.value)

    def regex_ends_device(self, d_text, expr_or_regex, starts, *, longest: bool = False, limit=None, flags: int = 0,
                          n: Optional[int] = None, base_offset: int = 0, stream=None):
        """An end for every start of ``starts`` (int64 / uint64 CUDA tensor, as search_regex_begins_device returns it for the
        same view, expression and base_offset): the smallest one, or with ``longest`` the largest one of the view
        (bmx_regex_ends_device).  ``limit``: a tensor like ``starts``, the last byte a match of each entry may use; an entry
        without a match within its limit gets all ones (-1 as int64).  Returns the ends, a tensor like ``starts``."""
        import torch

        re_ = _regex(expr_or_regex, flags)
        count = starts.numel()
        if n is None:
            n = d_text.numel()
        if starts.element_size() != 8 or (limit is not None and (limit.element_size() != 8 or limit.numel() != count)):
            raise ValueError("starts, limit: 8-byte entries, as many of one as of the other")
        ends = torch.empty(max(count, 1), dtype=starts.dtype, device=starts.device)
        s = stream if stream is not None else torch.cuda.current_stream(starts.device)
        rc = self._L.bmx_regex_ends_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, C.byref(re_),
                                           C.c_void_p(starts.data_ptr()), count,
                                           C.c_void_p(limit.data_ptr()) if limit is not None else None,
                                           REGEX_LONGEST if longest else 0, C.c_void_p(ends.data_ptr()), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_regex_ends_device")
        return ends[:count]

    def search_regex_begins(self, text, expr_or_regex, flags: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """Host buffers (bmx_search_regex_begins): ascending starts, uint64.  With ``capacity`` given and too small, raises
        BmxError(ERR_CAPACITY); without it the list is always complete."""
        re_ = _regex(expr_or_regex, flags)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex_begins(self._h, tptr, n, C.byref(re_), C.c_void_p(out.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_begins")
            del keep
            return out[: int(total.value)].copy()

    def search_regex_begins_spans(self, text, expr_or_regex, flags: int = 0, longest: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers (bmx_search_regex_begins_spans): (starts uint64, ends uint64), starts ascending and each once; each
        end the smallest one for its start, or with ``longest`` the largest."""
        re_ = _regex(expr_or_regex, flags)
        tptr, n, keep = _host_text(text)
        cap = max(1, min(n, 1 << 20))
        while True:
            starts = np.empty(cap, dtype=np.uint64)
            ends = np.empty(cap, dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex_begins_spans(self._h, tptr, n, C.byref(re_), REGEX_LONGEST if longest else 0,
                                                       C.c_void_p(starts.ctypes.data), C.c_void_p(ends.ctypes.data), cap,
                                                       C.byref(total))
            if rc == ERR_CAPACITY:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_begins_spans")
            del keep
            t = int(total.value)
            return starts[:t].copy(), ends[:t].copy()

    def last_regex_begins_ms(self) -> float:
        return float(self._L.bmx_last_regex_begins_ms(self._h))

    # -- anchored regular-expression search: ^ $ \b \B \< \>, whole word, whole line -------
    def _anchored_list_device(self, fn, what, d_text, expr_or_pair, flags, n, edge, base_offset, left, right, out, capacity, stream):
        import torch

        re_, an = _regex_anchored(expr_or_pair, flags)
        if n is None:
            n = d_text.numel()
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else 1 << 16, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        s = stream if stream is not None else torch.cuda.current_stream(d_text.device)
        total = C.c_uint64(0)
        rc = fn(self._h, C.c_void_p(d_text.data_ptr()), n, edge, base_offset, C.byref(re_), C.byref(an), int(left), int(right),
                C.c_void_p(out.data_ptr()), cap, C.byref(total), C.c_void_p(s.cuda_stream))
        self._chk(rc, what, allow=(ERR_CAPACITY,))
        return out[: min(int(total.value), cap)], int(total.value)

    def search_regex_anchored_device(self, d_text, expr_or_pair, *, flags: int = 0, n: Optional[int] = None, lead: int = 0,
                                     base_offset: int = 0, left: int = 10, right: int = 10, out=None,
                                     capacity: Optional[int] = None, stream=None):
        """Every end j in [lead, n) of the view at which an ANCHORED match ends (bmx_search_regex_anchored_device).
        ``expr_or_pair``: an expression for compile_regex_anchored(expr, flags) or its result.  ``left`` / ``right``: the
        bytes next to the view, 0x0A for a whole text, the real neighbours for a shard.  Otherwise search_regex_device."""
        return self._anchored_list_device(self._L.bmx_search_regex_anchored_device, "bmx_search_regex_anchored_device", d_text,
                                          expr_or_pair, flags, n, lead, base_offset, left, right, out, capacity, stream)

    def search_regex_anchored_begins_device(self, d_text, expr_or_pair, *, flags: int = 0, n: Optional[int] = None, tail: int = 0,
                                            base_offset: int = 0, left: int = 10, right: int = 10, out=None,
                                            capacity: Optional[int] = None, stream=None):
        """Every start s in [0, n - tail) of the view at which an anchored match begins
        (bmx_search_regex_anchored_begins_device); otherwise search_regex_begins_device."""
        return self._anchored_list_device(self._L.bmx_search_regex_anchored_begins_device, "bmx_search_regex_anchored_begins_device",
                                          d_text, expr_or_pair, flags, n, tail, base_offset, left, right, out, capacity, stream)

    def regex_anchored_starts_device(self, d_text, expr_or_pair, ends, *, longest: bool = False, flags: int = 0,
                                     n: Optional[int] = None, base_offset: int = 0, left: int = 10, right: int = 10, stream=None):
        """A start for every end of ``ends`` as search_regex_anchored_device returns it (bmx_regex_anchored_starts_device);
        otherwise regex_starts_device."""
        import torch

        re_, an = _regex_anchored(expr_or_pair, flags)
        count = ends.numel()
        if n is None:
            n = d_text.numel()
        if ends.element_size() != 8:
            raise ValueError("ends: 8-byte entries")
        starts = torch.empty(max(count, 1), dtype=ends.dtype, device=ends.device)
        s = stream if stream is not None else torch.cuda.current_stream(ends.device)
        rc = self._L.bmx_regex_anchored_starts_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, C.byref(re_),
                                                      C.byref(an), int(left), int(right), C.c_void_p(ends.data_ptr()), count,
                                                      REGEX_LONGEST if longest else 0, C.c_void_p(starts.data_ptr()),
                                                      C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_regex_anchored_starts_device")
        return starts[:count]

    def regex_anchored_ends_device(self, d_text, expr_or_pair, starts, *, longest: bool = False, limit=None, flags: int = 0,
                                   n: Optional[int] = None, base_offset: int = 0, left: int = 10, right: int = 10, stream=None):
        """An end for every start of ``starts`` as search_regex_anchored_begins_device returns it
        (bmx_regex_anchored_ends_device); otherwise regex_ends_device."""
        import torch

        re_, an = _regex_anchored(expr_or_pair, flags)
        count = starts.numel()
        if n is None:
            n = d_text.numel()
        if starts.element_size() != 8 or (limit is not None and (limit.element_size() != 8 or limit.numel() != count)):
            raise ValueError("starts, limit: 8-byte entries, as many of one as of the other")
        ends = torch.empty(max(count, 1), dtype=starts.dtype, device=starts.device)
        s = stream if stream is not None else torch.cuda.current_stream(starts.device)
        rc = self._L.bmx_regex_anchored_ends_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, C.byref(re_),
                                                    C.byref(an), int(left), int(right), C.c_void_p(starts.data_ptr()), count,
                                                    C.c_void_p(limit.data_ptr()) if limit is not None else None,
                                                    REGEX_LONGEST if longest else 0, C.c_void_p(ends.data_ptr()),
                                                    C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_regex_anchored_ends_device")
        return ends[:count]

    def _anchored_host(self, fn, what, text, expr_or_pair, flags, spans, longest, capacity):
        re_, an = _regex_anchored(expr_or_pair, flags)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            a = np.empty(max(cap, 1), dtype=np.uint64)
            b = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            if spans:
                rc = fn(self._h, tptr, n, C.byref(re_), C.byref(an), REGEX_LONGEST if longest else 0, C.c_void_p(a.ctypes.data),
                        C.c_void_p(b.ctypes.data), cap, C.byref(total))
            else:
                rc = fn(self._h, tptr, n, C.byref(re_), C.byref(an), C.c_void_p(a.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, what)
            del keep
            t = int(total.value)
            return (a[:t].copy(), b[:t].copy()) if spans else a[:t].copy()

    def search_regex_anchored(self, text, expr_or_pair, flags: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """Host buffers (bmx_search_regex_anchored): ascending ends, uint64; outside the text counts as a line break."""
        return self._anchored_host(self._L.bmx_search_regex_anchored, "bmx_search_regex_anchored", text, expr_or_pair, flags, False,
                                   False, capacity)

    def search_regex_anchored_spans(self, text, expr_or_pair, flags: int = 0, longest: bool = False):
        """Host buffers (bmx_search_regex_anchored_spans): (starts, ends), ends ascending, as search_regex_spans."""
        return self._anchored_host(self._L.bmx_search_regex_anchored_spans, "bmx_search_regex_anchored_spans", text, expr_or_pair,
                                   flags, True, longest, None)

    def search_regex_anchored_begins(self, text, expr_or_pair, flags: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """Host buffers (bmx_search_regex_anchored_begins): ascending starts, uint64."""
        return self._anchored_host(self._L.bmx_search_regex_anchored_begins, "bmx_search_regex_anchored_begins", text, expr_or_pair,
                                   flags, False, False, capacity)

    def search_regex_anchored_begins_spans(self, text, expr_or_pair, flags: int = 0, longest: bool = False):
        """Host buffers (bmx_search_regex_anchored_begins_spans): (starts, ends), starts ascending, as search_regex_begins_spans."""
        return self._anchored_host(self._L.bmx_search_regex_anchored_begins_spans, "bmx_search_regex_anchored_begins_spans", text,
                                   expr_or_pair, flags, True, longest, None)

    def last_regex_anchored_ms(self) -> float:
        return float(self._L.bmx_last_regex_anchored_ms(self._h))

    def last_regex_anchored_begins_ms(self) -> float:
        return float(self._L.bmx_last_regex_anchored_begins_ms(self._h))

    # -- regular-expression search with unbounded repetition: * + {a,} -------------------
    def search_regex_star_device(self, d_text, expr_or_regex, *, flags: int = 0, n: Optional[int] = None, lead: int = 0,
                                 base_offset: int = 0, out=None, capacity: Optional[int] = None, stream=None):
        """Every end j in [lead, n) of the view ``d_text[0:n)`` at which a match that begins inside the view ends, ascending
        and exact, reported as base_offset + j (bmx_search_regex_star_device).  ``expr_or_regex``: an expression for
        compile_regex_star(expr, flags) or a Regex, which may have a cycle.  The other arguments and the return value
        (ends view, true total) are those of search_regex_device."""
        import torch

        re_ = _regex(expr_or_regex, flags, star=True)
        if n is None:
            n = d_text.numel()
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else 1 << 16, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        s = stream if stream is not None else torch.cuda.current_stream(d_text.device)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_regex_star_device(self._h, C.c_void_p(d_text.data_ptr()), n, lead, base_offset, C.byref(re_),
                                                  C.c_void_p(out.data_ptr()), cap, C.byref(total), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_search_regex_star_device", allow=(ERR_CAPACITY,))
        return out[: min(int(total.value), cap)], int(total.value)

    def search_regex_star(self, text, expr_or_regex, flags: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """Host buffers (bmx_search_regex_star): ascending ends, uint64.  With ``capacity`` given and too small, raises
        BmxError(ERR_CAPACITY); without it the list is always complete."""
        re_ = _regex(expr_or_regex, flags, star=True)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex_star(self._h, tptr, n, C.byref(re_), C.c_void_p(out.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_star")
            del keep
            return out[: int(total.value)].copy()

    def search_regex_star_spans(self, text, expr_or_regex, flags: int = 0, longest: bool = False,
                                window: int = 4096) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers (bmx_search_regex_star_spans): (starts uint64, ends uint64), ends ascending; each start that of the
        shortest match of at most ``window`` bytes for its end, with ``longest`` of the longest such, and UINT64_MAX where
        no match that short ends there."""
        re_ = _regex(expr_or_regex, flags, star=True)
        tptr, n, keep = _host_text(text)
        cap = max(1, min(n, 1 << 20))
        while True:
            starts = np.empty(cap, dtype=np.uint64)
            ends = np.empty(cap, dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex_star_spans(self._h, tptr, n, C.byref(re_), int(window), REGEX_LONGEST if longest else 0,
                                                     C.c_void_p(starts.ctypes.data), C.c_void_p(ends.ctypes.data), cap,
                                                     C.byref(total))
            if rc == ERR_CAPACITY:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_star_spans")
            del keep
            t = int(total.value)
            return starts[:t].copy(), ends[:t].copy()

    def regex_star_starts_device(self, d_text, expr_or_regex, ends, *, window: int = 4096, longest: bool = False, flags: int = 0,
                                 n: Optional[int] = None, base_offset: int = 0, stream=None):
        """A start for every end of ``ends`` (int64 / uint64 CUDA tensor, as search_regex_star_device returns it for the same
        view, expression and base_offset) among the matches of at most ``window`` bytes: the largest one, or with
        ``longest`` the smallest; all ones (-1 as int64) where there is none (bmx_regex_star_starts_device)."""
        import torch

        re_ = _regex(expr_or_regex, flags, star=True)
        count = ends.numel()
        if n is None:
            n = d_text.numel()
        if ends.element_size() != 8:
            raise ValueError("ends: 8-byte entries")
        starts = torch.empty(max(count, 1), dtype=ends.dtype, device=ends.device)
        s = stream if stream is not None else torch.cuda.current_stream(ends.device)
        rc = self._L.bmx_regex_star_starts_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, C.byref(re_),
                                                  C.c_void_p(ends.data_ptr()), count, int(window), REGEX_LONGEST if longest else 0,
                                                  C.c_void_p(starts.data_ptr()), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_regex_star_starts_device")
        return starts[:count]

    def last_regex_star_ms(self) -> float:
        return float(self._L.bmx_last_regex_star_ms(self._h))

    # -- ... its mirror image: every match start of an expression with * + {a,}, and the end of every start ----
    def search_regex_star_begins_device(self, d_text, expr_or_regex, *, flags: int = 0, n: Optional[int] = None, tail: int = 0,
                                        base_offset: int = 0, out=None, capacity: Optional[int] = None, stream=None):
        """Every start s in [0, n - tail) of the view ``d_text[0:n)`` at which a match of the expression begins (and ends
        inside the view), ascending and exact, reported as base_offset + s (bmx_search_regex_star_begins_device).
        ``expr_or_regex``: an expression for compile_regex_star(expr, flags) or a Regex, which may have a cycle.  The other
        arguments and the return value (starts view, true total) are those of search_regex_begins_device."""
        import torch

        re_ = _regex(expr_or_regex, flags, star=True)
        if n is None:
            n = d_text.numel()
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else 1 << 16, 1), dtype=torch.int64, device=d_text.device)
        cap = out.numel() if capacity is None else min(capacity, out.numel())
        s = stream if stream is not None else torch.cuda.current_stream(d_text.device)
        total = C.c_uint64(0)
        rc = self._L.bmx_search_regex_star_begins_device(self._h, C.c_void_p(d_text.data_ptr()), n, tail, base_offset,
                                                         C.byref(re_), C.c_void_p(out.data_ptr()), cap, C.byref(total),
                                                         C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_search_regex_star_begins_device", allow=(ERR_CAPACITY,))
        return out[: min(int(total.value), cap)], int(total.value)

    def regex_star_ends_device(self, d_text, expr_or_regex, starts, *, window: int = 4096, longest: bool = False, limit=None,
                               flags: int = 0, n: Optional[int] = None, base_offset: int = 0, stream=None):
        """(ends, clipped): an end for every start of ``starts`` (int64 / uint64 CUDA tensor, as
        search_regex_star_begins_device returns it for the same view, expression and base_offset) among the matches of at
        most ``window`` bytes: the smallest one, or with ``longest`` the largest; all ones (-1 as int64) where there is none
        (bmx_regex_star_ends_device).  ``limit``: a tensor like ``starts``, the last byte a match of each entry may use.
        ``clipped``: the entries whose run could still be extended after ``window`` bytes inside their limit and the view,
        i.e. whose longest match may be longer than the one reported."""
        import torch

        re_ = _regex(expr_or_regex, flags, star=True)
        count = starts.numel()
        if n is None:
            n = d_text.numel()
        if starts.element_size() != 8 or (limit is not None and (limit.element_size() != 8 or limit.numel() != count)):
            raise ValueError("starts, limit: 8-byte entries, as many of one as of the other")
        ends = torch.empty(max(count, 1), dtype=starts.dtype, device=starts.device)
        s = stream if stream is not None else torch.cuda.current_stream(starts.device)
        clipped = C.c_uint64(0)
        rc = self._L.bmx_regex_star_ends_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, C.byref(re_),
                                                C.c_void_p(starts.data_ptr()), count,
                                                C.c_void_p(limit.data_ptr()) if limit is not None else None, int(window),
                                                REGEX_LONGEST if longest else 0, C.c_void_p(ends.data_ptr()), C.byref(clipped),
                                                C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_regex_star_ends_device")
        return ends[:count], int(clipped.value)

    def search_regex_star_begins(self, text, expr_or_regex, flags: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """Host buffers (bmx_search_regex_star_begins): ascending starts, uint64.  With ``capacity`` given and too small,
        raises BmxError(ERR_CAPACITY); without it the list is always complete."""
        re_ = _regex(expr_or_regex, flags, star=True)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_search_regex_star_begins(self._h, tptr, n, C.byref(re_), C.c_void_p(out.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_star_begins")
            del keep
            return out[: int(total.value)].copy()

    def search_regex_star_begins_spans(self, text, expr_or_regex, flags: int = 0, longest: bool = False,
                                       window: int = 4096) -> Tuple[np.ndarray, np.ndarray, int]:
        """Host buffers (bmx_search_regex_star_begins_spans): (starts uint64, ends uint64, clipped), starts ascending and
        each once; each end that of the shortest match of at most ``window`` bytes from its start, with ``longest`` of the
        longest such, UINT64_MAX where there is none; ``clipped`` as in regex_star_ends_device."""
        re_ = _regex(expr_or_regex, flags, star=True)
        tptr, n, keep = _host_text(text)
        cap = max(1, min(n, 1 << 20))
        while True:
            starts = np.empty(cap, dtype=np.uint64)
            ends = np.empty(cap, dtype=np.uint64)
            total, clipped = C.c_uint64(0), C.c_uint64(0)
            rc = self._L.bmx_search_regex_star_begins_spans(self._h, tptr, n, C.byref(re_), int(window),
                                                            REGEX_LONGEST if longest else 0, C.c_void_p(starts.ctypes.data),
                                                            C.c_void_p(ends.ctypes.data), cap, C.byref(total), C.byref(clipped))
            if rc == ERR_CAPACITY:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_search_regex_star_begins_spans")
            del keep
            t = int(total.value)
            return starts[:t].copy(), ends[:t].copy(), int(clipped.value)

    def last_regex_star_begins_ms(self) -> float:
        return float(self._L.bmx_last_regex_star_begins_ms(self._h))

    # -- match spans of the approximate search: (start, end, distance) -------------------
    def approx_spans_device(self, d_text, pattern_or_classes, k: int, ends, dist=None, *, best: bool = False, flags: int = 0,
                            n: Optional[int] = None, base_offset: int = 0, stream=None):
        """The start of every match of a list of ends (bmx_approx_spans[_classes]_device): ``ends`` (int64 / uint64) and
        ``dist`` (uint8, may be None without ``best``) are CUDA tensors as search_approx[_classes]_device returns them for
        the same view, pattern, k and base_offset.  ``pattern_or_classes``: str / bytes are a STRING, a [m, 32] uint8
        array is a class pattern (compile_classes(expr, class_flags) makes one).  ``best`` sets SPANS_BEST (one entry per
        occurrence); ``flags`` are further SPANS_* bits, passed as they are.  Returns (starts, ends, dist, total) as
        tensors of ``total`` entries: without SPANS_BEST the list itself with its starts, with it the kept entries in list
        order.  ``stream``: a torch.cuda.Stream (None: torch's current one)."""
        import torch

        flags = int(flags) | (SPANS_BEST if best else 0)
        best = bool(flags & SPANS_BEST)
        count = ends.numel()
        if n is None:
            n = d_text.numel()
        if ends.element_size() != 8 or (dist is not None and (dist.element_size() != 1 or dist.numel() < count)):
            raise ValueError("ends: 8-byte entries; dist: 1-byte entries, one per end")
        dev = ends.device
        starts = torch.empty(max(count, 1), dtype=ends.dtype, device=dev)
        sel_ends = torch.empty(max(count, 1), dtype=ends.dtype, device=dev) if best else None
        sel_dist = torch.empty(max(count, 1), dtype=torch.uint8, device=dev) if best else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        s = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(dev)).cuda_stream)
        total = C.c_uint64(0)
        tail = (int(k), ptr(ends), ptr(dist), count, flags, ptr(starts), ptr(sel_ends), ptr(sel_dist),
                C.byref(total), s)
        if isinstance(pattern_or_classes, (str, bytes, bytearray)):
            pat = _pat_bytes(pattern_or_classes)
            what = "bmx_approx_long_spans_device" if len(pat) > MAX_APPROX_PATTERN else "bmx_approx_spans_device"
            rc = getattr(self._L, what)(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, pat, len(pat), *tail)
        else:
            cls = _classes(pattern_or_classes)
            what = "bmx_approx_spans_device"  # (the name this check has always reported for both)
            rc = self._L.bmx_approx_spans_classes_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset,
                                                         C.c_void_p(cls.ctypes.data), cls.shape[0], *tail)
        self._chk(rc, what)
        t = int(total.value)
        if best:
            return starts[:t], sel_ends[:t], sel_dist[:t], t
        return starts[:t], ends[:t], (dist[:t] if dist is not None else None), t

    def _search_spans_host(self, fn, what, text, pat_arg, m: int, k: int, best: bool):
        tptr, n, keep = _host_text(text)
        cap = max(1, min(n, 1 << 20))
        while True:
            starts = np.empty(cap, dtype=np.uint64)
            ends = np.empty(cap, dtype=np.uint64)
            dist = np.empty(cap, dtype=np.uint8)
            total = C.c_uint64(0)
            rc = fn(self._h, tptr, n, pat_arg, m, int(k), SPANS_BEST if best else 0, C.c_void_p(starts.ctypes.data),
                    C.c_void_p(ends.ctypes.data), C.c_void_p(dist.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY:
                cap = int(total.value)
                continue
            self._chk(rc, what)
            del keep
            t = int(total.value)
            return starts[:t].copy(), ends[:t].copy(), dist[:t].copy()

    def search_approx_spans(self, text, pattern, k: int, best: bool = True, cigar: bool = False):
        """Host buffers (bmx_search_approx_spans): (starts uint64, ends uint64, distances uint8) of every match of
        ``pattern`` within k edits, ascending; ``best``: one entry per occurrence, else every qualifying end.  With
        ``cigar`` a fourth element: the CIGAR string of every span (bmx_align)."""
        pat = _pat_bytes(pattern)
        if len(pat) > MAX_APPROX_PATTERN:  # up to 512 bytes
            res = self._search_spans_host(self._L.bmx_search_approx_long_spans, "bmx_search_approx_long_spans", text, pat, len(pat),
                                          k, best)
        else:
            res = self._search_spans_host(self._L.bmx_search_approx_spans, "bmx_search_approx_spans", text, pat, len(pat), k, best)
        if not cigar:
            return res
        _, op_off, ops = self.align(text, [pat], res[0], res[1], k)
        return res + (cigar_strings(op_off, ops),)

    def search_approx_spans_classes(self, text, classes_or_expr, k: int, flags: int = 0,
                                    best: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """search_approx_spans with a class per pattern position (bmx_search_approx_spans_classes): an expression for
        compile_classes(expr, flags) or a [m, 32] uint8 array, like search_classes."""
        cls = _classes(classes_or_expr, flags)
        return self._search_spans_host(self._L.bmx_search_approx_spans_classes, "bmx_search_approx_spans_classes", text,
                                       C.c_void_p(cls.ctypes.data), cls.shape[0], k, best)

    def last_spans_ms(self) -> float:
        return float(self._L.bmx_last_spans_ms(self._h))

    # -- alignments: the edit script of every span ----------------------------------------
    def align_device(self, d_text, patterns, starts, ends, k: int, pid=None, base_offset: int = 0,
                     capacity: Optional[int] = None, out=None, stream=None):
        """(dist, op_off, ops) (bmx_align_device): for entry e the global distance of its pattern against the span
        text[starts[e] - base_offset .. ends[e] - base_offset] (the end inclusive, as approx_spans_device and Index.map
        report it) and its canonical edit script.  ``dist`` uint8 (ALIGN_NONE: no alignment within k), ``op_off`` int64 of
        count + 1 entries (the exclusive prefix sum of the runs per entry; op_off[-1] is the true total), ``ops`` int32 op
        words (run length << 4 | CIGAR_*), entry e's at ops[op_off[e] : op_off[e + 1]]; cigar_strings makes strings of
        them.  ``d_text``: a uint8 CUDA tensor; ``patterns``: a list of bytes / str, a (blob, offsets) numpy pair or such
        a pair of CUDA tensors, one pattern per entry or ONE for all of them, unless ``pid`` (an int32 CUDA tensor) names
        each entry's; ``starts`` / ``ends``: 8-byte CUDA tensors.  Without ``capacity`` the list is complete.  With a
        capacity below the total every entry whose segment ends at or below it is stored; that is no error here
        (op_off[-1] says so); capacity 0 counts only.  ``out``: three tensors to take the answer, used as given.
        ``stream``: a torch.cuda.Stream (None: torch's current one)."""
        import torch

        dev = d_text.device
        d_blob, d_off, pat_count = _device_strings(patterns, dev)
        count = starts.numel()
        if starts.element_size() != 8 or ends.element_size() != 8 or ends.numel() != count:
            raise ValueError("starts, ends: 8-byte entries, as many of one as of the other")
        if pid is not None and (pid.element_size() != 4 or pid.numel() < count):
            raise ValueError("pid: 4-byte entries, one per entry")
        most = count * (2 * int(k) + 1)
        if out is not None:
            dist, op_off, ops = out
            if capacity is None:
                capacity = ops.numel()
        else:
            dist = torch.empty(max(count, 1), dtype=torch.uint8, device=dev)
            op_off = torch.zeros(count + 1, dtype=torch.int64, device=dev)
            ops = None
        if dist.element_size() != 1 or op_off.element_size() != 8 or dist.numel() < count or op_off.numel() < count + 1:
            raise ValueError("out: dist 1-byte entries (count), op_off 8-byte entries (count + 1), ops 4-byte entries")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        s = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(dev)).cuda_stream)
        total = C.c_uint64(0)

        def call(ops_t, cap):
            rc = self._L.bmx_align_device(self._h, ptr(d_text), d_text.numel(), base_offset, ptr(d_blob), d_blob.numel(),
                                          ptr(d_off), pat_count, ptr(pid), ptr(starts), ptr(ends), count, int(k), ptr(dist),
                                          ptr(op_off), ptr(ops_t), cap, C.byref(total), s)
            self._chk(rc, "bmx_align_device", allow=(ERR_CAPACITY,))

        if capacity is None:
            if most > (1 << 26):  # a counting call first rather than room for every possible run
                call(None, 0)
                most = int(total.value)
            capacity = most
        if ops is None:
            ops = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)
        if ops.element_size() != 4 or ops.numel() < capacity:
            raise ValueError("ops: 4-byte entries, at least `capacity` of them")
        call(ops if capacity > 0 else None, capacity)
        return dist[:count], op_off[: count + 1], ops[: min(int(total.value), capacity)]

    def align(self, text, patterns, starts, ends, k: int, pid=None, base_offset: int = 0):
        """Host buffers (bmx_align): (dist uint8, op_off uint64, ops uint32) as align_device, complete.  ``starts`` /
        ``ends``: sequences of positions (MAP_NO_POS for an entry without a hit)."""
        tptr, n, keep = _host_text(text)
        blob, off = pack_strings(patterns)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        count = starts.size
        if ends.size != count:
            raise ValueError("starts and ends: as many of one as of the other")
        pid_arr = None if pid is None else np.ascontiguousarray(pid, dtype=np.uint32)
        if pid_arr is not None and pid_arr.size != count:
            raise ValueError("pid: one per entry")
        dist = np.empty(max(count, 1), dtype=np.uint8)
        op_off = np.zeros(count + 1, dtype=np.uint64)
        cap = max(1, min(count * (2 * max(int(k), 0) + 1), 1 << 24))
        while True:
            ops = np.empty(cap, dtype=np.uint32)
            total = C.c_uint64(0)
            rc = self._L.bmx_align(self._h, tptr, n, base_offset, C.c_void_p(blob.ctypes.data), blob.size,
                                   C.c_void_p(off.ctypes.data), off.size - 1,
                                   None if pid_arr is None else C.c_void_p(pid_arr.ctypes.data), C.c_void_p(starts.ctypes.data),
                                   C.c_void_p(ends.ctypes.data), count, int(k), C.c_void_p(dist.ctypes.data),
                                   C.c_void_p(op_off.ctypes.data), C.c_void_p(ops.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and int(total.value) > cap:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_align")
            del keep
            return dist[:count], op_off, ops[: int(total.value)].copy()

    def last_align_ms(self) -> float:
        return float(self._L.bmx_last_align_ms(self._h))

    def last_align_launches(self) -> int:
        """Launches of the alignment kernel in the last align_device on this context (> 1: the entries did not fit the
        workspace at once); < 0 if none."""
        return int(self._L.bmx_last_align_launches(self._h))

    # -- dictionary search: many patterns in one pass ----------------------------------
    def dictionary(self, patterns) -> "Dictionary":
        """Build a dictionary of ``patterns`` (str / bytes each) on this context's device (bmx_dict_create)."""
        return Dictionary(self, patterns)

    def search_dict(self, text, patterns, capacity: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers (bmx_dict_search): (positions uint64, pattern indices uint32), ordered by position, then index.
        With ``capacity`` given and too small, raises BmxError(ERR_CAPACITY); without it the list is always complete."""
        arr, ms, K, keep_p = _dict_arrays(patterns)
        tptr, n, keep = _host_text(text)
        cap = capacity if capacity is not None else max(1, min(n, 1 << 20))
        while True:
            pos = np.empty(max(cap, 1), dtype=np.uint64)
            pid = np.empty(max(cap, 1), dtype=np.uint32)
            total = C.c_uint64(0)
            rc = self._L.bmx_dict_search(self._h, tptr, n, arr, ms, K, C.c_void_p(pos.ctypes.data),
                                         C.c_void_p(pid.ctypes.data), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            self._chk(rc, "bmx_dict_search")
            del keep, keep_p
            t = int(total.value)
            return pos[:t].copy(), pid[:t].copy()

    def last_dict_ms(self) -> float:
        return float(self._L.bmx_last_dict_ms(self._h))

    def last_dict_candidates(self) -> int:
        """Positions of the last dictionary search that passed the LDS filters (false positives + matching positions)."""
        return int(self._L.bmx_last_dict_candidates(self._h))

    # -- text index: batched pattern count and locate over the suffix array -------------
    def index(self, d_text, sa=None) -> "Index":
        """An index over the resident text ``d_text`` (uint8 CUDA tensor) and its suffix array (bmx_index_create_device):
        ``sa`` an int32 CUDA tensor as suffix_array_device returns it, or None to have it built and owned by the index."""
        return Index(self, d_text, sa)

    def index_count(self, text, patterns) -> np.ndarray:
        """Host buffers (bmx_index_count): occurrences of every pattern in ``text``, uint32."""
        tptr, n, keep = _host_text(text)
        blob, off = pack_strings(patterns)
        count = off.size - 1
        cnt = np.empty(max(count, 1), dtype=np.uint32)
        rc = self._L.bmx_index_count(self._h, tptr, n, C.c_void_p(blob.ctypes.data), blob.size, C.c_void_p(off.ctypes.data),
                                     count, C.c_void_p(cnt.ctypes.data))
        self._chk(rc, "bmx_index_count")
        del keep
        return cnt[:count]

    def index_match(self, text, patterns) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Host buffers (bmx_index_match): (len, lo, cnt), uint32, one entry per blob byte of the packed patterns: the
        longest match that starts at that byte and stays inside its query, and its interval of the suffix array."""
        tptr, n, keep = _host_text(text)
        blob, off = pack_strings(patterns)
        count = off.size - 1
        out = [np.zeros(max(blob.size, 1), dtype=np.uint32) for _ in range(3)]
        rc = self._L.bmx_index_match(self._h, tptr, n, C.c_void_p(blob.ctypes.data), blob.size, C.c_void_p(off.ctypes.data),
                                     count, *[C.c_void_p(o.ctypes.data) for o in out])
        self._chk(rc, "bmx_index_match")
        del keep
        return tuple(o[: blob.size] for o in out)

    def index_seeds(self, text, patterns, min_len: int, max_occ: int = 0):
        """Host buffers (bmx_index_seeds): (seed_off uint64 of count + 1 entries, qpos, len, lo, cnt uint32), the seeds of
        every pattern in ``text`` in order of (pattern, position): a counting call, then the list."""
        tptr, n, keep = _host_text(text)
        blob, off = pack_strings(patterns)
        count = off.size - 1
        seed_off = np.zeros(count + 1, dtype=np.uint64)
        total = C.c_uint64(0)

        def call(out, cap):
            ptrs = [None] * 4 if out is None else [C.c_void_p(o.ctypes.data) for o in out]
            return self._L.bmx_index_seeds(self._h, tptr, n, C.c_void_p(blob.ctypes.data), blob.size, C.c_void_p(off.ctypes.data),
                                           count, min_len, max_occ, C.c_void_p(seed_off.ctypes.data), *ptrs, cap, C.byref(total))

        self._chk(call(None, 0), "bmx_index_seeds", allow=(ERR_CAPACITY,))
        cap = int(total.value)
        out = [np.empty(max(cap, 1), dtype=np.uint32) for _ in range(4)]
        if cap > 0:
            self._chk(call(out, cap), "bmx_index_seeds")
        del keep
        return (seed_off,) + tuple(o[:cap] for o in out)

    def index_map(self, text, patterns, min_len: int, max_occ: int, k: int, candidates: bool = False, cigar: bool = False):
        """Host buffers: (best_start, best_end uint64, best_dist uint8), one entry per pattern: where the pattern lies in
        ``text`` within k edits (MAP_NO_POS, MAP_NO_POS, MAP_NO_HIT if nowhere), by extending its seeds of
        (min_len, max_occ).  That is one bmx_index_map.  With ``candidates`` also (cand_off uint64 of count + 1 entries,
        cand_start, cand_end uint64, cand_dist uint8): every seed occurrence's own answer, in order of (pattern, seed,
        occurrence); the lists are sized by a counting call, so the index is built once here and Index.map makes both.
        With ``cigar`` one more element at the end: the CIGAR string of every pattern at its best position ("" for a
        pattern that maps nowhere)."""
        if candidates:
            import torch

            d_text = torch.from_numpy(np.frombuffer(_host_text(text)[2], dtype=np.uint8).copy()).cuda(self.device)
            with self.index(d_text) as idx:
                res = idx.map(patterns, min_len, max_occ, k, candidates=True, cigar=cigar)
                tail = (res[7],) if cigar else ()
                res = tuple(o.cpu().numpy() for o in res[:7])
            return (res[0].view(np.uint64), res[1].view(np.uint64), res[2], res[3].view(np.uint64), res[4].view(np.uint64),
                    res[5].view(np.uint64), res[6]) + tail
        tptr, n, keep = _host_text(text)
        blob, off = pack_strings(patterns)
        count = off.size - 1
        best = [np.empty(max(count, 1), dtype=np.uint64), np.empty(max(count, 1), dtype=np.uint64),
                np.empty(max(count, 1), dtype=np.uint8)]
        total = C.c_uint64(0)
        rc = self._L.bmx_index_map(self._h, tptr, n, C.c_void_p(blob.ctypes.data), blob.size, C.c_void_p(off.ctypes.data), count,
                                   min_len, max_occ, k, *[C.c_void_p(o.ctypes.data) for o in best], None, None, None, None, 0,
                                   C.byref(total))
        self._chk(rc, "bmx_index_map")
        del keep
        res = tuple(o[:count] for o in best)
        if not cigar:
            return res
        _, op_off, ops = self.align(text, (blob, off), res[0], res[1], k)
        return res + (cigar_strings(op_off, ops),)

    def last_index_ms(self) -> float:
        return float(self._L.bmx_last_index_ms(self._h))

    def last_index_map_phases(self) -> dict:
        """Device ms of the last Index.map by phase, and the 64-bit words of the instance that ran (bmx_last_index_map_phases)."""
        out = (C.c_float * 5)()
        self._chk(self._L.bmx_last_index_map_phases(self._h, out), "bmx_last_index_map_phases")
        return {"expand_ms": out[0], "verify_ms": out[1], "start_ms": out[2], "best_ms": out[3], "words": int(out[4])}

    def last_index_map_candidates(self) -> int:
        """Candidates (seed occurrences) of the last Index.map on this context; < 0 if none."""
        return int(self._L.bmx_last_index_map_candidates(self._h))

    # -- suffix array (the reference's third program) -----------------------------
    def suffix_array(self, text) -> np.ndarray:
        """int32 suffix array in the reference's order (SuffixArrays.cpp:101-154)."""
        pt, n, keep = _host_text(text)
        sa = np.empty(max(n, 1), dtype=np.int32)
        self._chk(self._L.bmx_suffix_array(self._h, pt, n, sa.ctypes.data_as(_i32p)), "bmx_suffix_array")
        return sa[:n].copy()

    def suffix_array_device(self, d_text):
        import torch

        n = d_text.numel()
        d_sa = torch.empty(max(n, 1), dtype=torch.int32, device=d_text.device)
        stream = C.c_void_p(torch.cuda.current_stream(d_text.device).cuda_stream)
        self._chk(self._L.bmx_suffix_array_device(self._h, C.c_void_p(d_text.data_ptr()), n, C.c_void_p(d_sa.data_ptr()),
                                             stream), "bmx_suffix_array_device")
        return d_sa[:n]

    def last_suffix_array_ms(self) -> float:
        return float(self._L.bmx_last_suffix_array_ms(self._h))

    def last_suffix_array_rounds(self) -> int:
        return int(self._L.bmx_last_suffix_array_rounds(self._h))

    def last_suffix_array_lds_rounds(self) -> int:
        return int(self._L.bmx_last_suffix_array_lds_rounds(self._h))

    # -- LCP array over the suffix array, with repeat statistics ---------------------
    def lcp_array_device(self, d_text, sa, *, n: Optional[int] = None, out=None):
        """int32 CUDA tensor (bmx_lcp_array_device): lcp[0] = 0, lcp[j] = the common prefix, in plain bytes, of the suffixes
        sa[j - 1] and sa[j] of the resident text ``d_text`` (uint8 CUDA tensor).  ``sa``: an int32 CUDA tensor, any
        permutation of 0..n-1.  Runs on torch's current stream."""
        import torch

        n = d_text.numel() if n is None else n
        if d_text.element_size() != 1 or sa.element_size() != 4 or sa.numel() < n or d_text.numel() < n:
            raise ValueError("d_text: 1-byte entries; sa: 4-byte entries, one per text byte")
        lcp = out if out is not None else torch.empty(max(n, 1), dtype=torch.int32, device=d_text.device)
        if lcp.element_size() != 4 or lcp.numel() < n:
            raise ValueError("out: 4-byte entries, one per text byte")
        stream = C.c_void_p(torch.cuda.current_stream(d_text.device).cuda_stream)
        self._chk(self._L.bmx_lcp_array_device(self._h, C.c_void_p(d_text.data_ptr()), n, C.c_void_p(sa.data_ptr()),
                                               C.c_void_p(lcp.data_ptr()), stream), "bmx_lcp_array_device")
        return lcp[:n]

    def lcp_array(self, text) -> Tuple[np.ndarray, np.ndarray]:
        """Host buffers (bmx_lcp_array): (sa, lcp), both int32, the array in the order suffix_array gives."""
        pt, n, keep = _host_text(text)
        sa = np.empty(max(n, 1), dtype=np.int32)
        lcp = np.empty(max(n, 1), dtype=np.int32)
        self._chk(self._L.bmx_lcp_array(self._h, pt, n, C.c_void_p(sa.ctypes.data), C.c_void_p(lcp.ctypes.data)), "bmx_lcp_array")
        del keep
        return sa[:n].copy(), lcp[:n].copy()

    def lcp_stats_device(self, lcp, min_len: int = 0) -> dict:
        """{max, argmax (the smallest j that attains the max), sum, count (entries >= min_len)} of an int32 CUDA tensor
        (bmx_lcp_stats_device), Python ints.  Runs on torch's current stream."""
        import torch

        if lcp.element_size() != 4:
            raise ValueError("lcp: 4-byte entries")
        out = (C.c_uint64 * 4)()
        stream = C.c_void_p(torch.cuda.current_stream(lcp.device).cuda_stream)
        self._chk(self._L.bmx_lcp_stats_device(self._h, C.c_void_p(lcp.data_ptr()), lcp.numel(), min_len, out, stream),
                  "bmx_lcp_stats_device")
        return {"max": int(out[0]), "argmax": int(out[1]), "sum": int(out[2]), "count": int(out[3])}

    def last_lcp_ms(self) -> float:
        return float(self._L.bmx_last_lcp_ms(self._h))

    def last_lcp_long_pairs(self) -> int:
        """Pairs of the last lcp_array_device whose common prefix exceeded LCP_LANE_BYTES."""
        return int(self._L.bmx_last_lcp_long_pairs(self._h))

    # -- row-wise results: lines of a text, the row of each match, the matching rows ------
    def rows_split_device(self, d_text, delim: int = 10, n: Optional[int] = None, base_offset: int = 0, *, out=None,
                          capacity: Optional[int] = None, stream=None) -> "Rows":
        """The rows of the view ``d_text[0:n)`` split at the byte ``delim`` (bmx_rows_split_device): a Rows over count + 1
        ascending offsets, offsets[0] = base_offset, a row holding its terminating delimiter as its last byte, no extra
        empty row behind a final delimiter.  ``out``: int64/uint64 CUDA tensor for the offsets (allocated if None, for
        ``capacity`` entries or a guess); where it is too small the call runs once more with the exact size, unless
        ``capacity`` was given: then BmxError(ERR_CAPACITY).  ``stream``: a torch.cuda.Stream (None: torch's current one)."""
        import torch

        if n is None:
            n = d_text.numel()
        s = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(d_text.device)).cuda_stream)
        if out is None:
            out = torch.empty(max(capacity if capacity is not None else max(1 << 12, n // 64 + 2), 1), dtype=torch.int64,
                              device=d_text.device)
        while True:
            cap = out.numel() if capacity is None else min(capacity, out.numel())
            rows, longest = C.c_uint64(0), C.c_uint64(0)
            rc = self._L.bmx_rows_split_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, int(delim) & 0xFF,
                                               C.c_void_p(out.data_ptr()), cap, C.byref(rows), C.byref(longest), s)
            if rc == ERR_CAPACITY and capacity is None:
                out = torch.empty(int(rows.value) + 1, dtype=out.dtype, device=d_text.device)
                continue
            self._chk(rc, "bmx_rows_split_device")
            return Rows(self, out[: int(rows.value) + 1], int(longest.value))

    def rows(self, offsets) -> "Rows":
        """A Rows over a caller's offsets: an int64/uint64 CUDA tensor of rows + 1 ascending entries, in the coordinates of
        the match lists (the offsets of a string column, say; empty rows are legal)."""
        if offsets.element_size() != 8 or offsets.numel() < 1:
            raise ValueError("offsets: at least one 8-byte entry")
        return Rows(self, offsets)

    def grep_device(self, d_text, expr, kind: str = "regex", rows: Optional["Rows"] = None, delim: int = 10, invert: bool = False,
                    flags: int = 0, k: int = 0, window: Optional[int] = None):
        """The rows of the resident text ``d_text`` that hold a match of ``expr``, ascending, and each one's number of
        matches: (rows, counts) as int64 CUDA tensors (grep -n / -c); with ``invert`` the rows that hold none and None
        (grep -v).  ``kind``: exact | classes | hamming | gaps | regex | regex_long | regex_star | approx, the search that reads ``expr``
        (``flags`` are its compile flags, ``k`` the mismatches or edits of hamming and approx).  ``rows``: a Rows in the
        view's coordinates (base_offset 0), or None for the lines of the text split at ``delim``.  Runs the existing search,
        for the kinds that report ends the existing starts post-pass with its default flags (the largest start of an
        end, so a row holds a match that ends at e iff it holds this one), then Rows.of and Rows.matching.  A match that
        runs across a row boundary counts for no row; `.` matches the delimiter too, so write ``[^\\x0a]*`` for ``.*`` on
        lines.  regex_star: the starts come from a window of min(MAX_REGEX_STAR_WINDOW, rows.longest) bytes (or ``window``);
        an end whose shortest match is longer than the window is not attributed to any row."""
        if rows is None:
            rows = self.rows_split_device(d_text, delim)
        starts, ends, length = self._match_spans_device(d_text, expr, kind, flags, k, window, False, rows)
        ids = rows.of(starts=starts, ends=ends, length=length)
        return rows.matching(ids, invert=invert)

    def _match_spans_device(self, d_text, expr, kind, flags, k, window, longest, rows):
        """(starts, ends, length) of every match of ``expr`` in the resident text, in one of the three forms of Rows.of:
        the existing search of ``kind`` and, for the kinds that report ends, the existing starts post-pass (``longest``: the
        smallest start of every end where the pass has that flag).  ``rows`` (may be None) bounds regex_star's window."""
        import torch

        def complete(call):  # call(out) -> (list, ..., total): once more with room for all where the first guess was short
            res = call(None)
            if res[-1] > res[0].numel():
                res = call(torch.empty(res[-1], dtype=torch.int64, device=d_text.device))
            return res

        if kind == "exact":
            starts, _ = complete(lambda out: self.search_device(d_text, expr, out=out))
            return starts, None, len(_pat_bytes(expr))
        if kind == "classes":
            cls = _classes(expr, flags)
            starts, _ = complete(lambda out: self.search_classes_device(d_text, cls, out=out))
            return starts, None, cls.shape[0]
        if kind == "hamming":
            pat, cls = self._hamming_pattern(expr, flags)
            starts, _, _ = complete(lambda out: self.search_hamming_device(d_text, expr, k, flags=flags, out=out))
            return starts, None, len(pat) if pat is not None else cls.shape[0]
        if kind == "gaps":
            pair = _gaps(expr, flags)
            ends, _ = complete(lambda out: self.search_gaps_device(d_text, pair, out=out))
            return self.gaps_starts_device(d_text, pair, ends, longest=longest), ends, 0
        if kind == "regex":
            re_ = _regex(expr, flags)
            ends, _ = complete(lambda out: self.search_regex_device(d_text, re_, out=out))
            return self.regex_starts_device(d_text, re_, ends, longest=longest), ends, 0
        if kind == "regex_long":
            re_ = _regex_long(expr, flags)
            ends, _ = complete(lambda out: self.search_regex_long_device(d_text, re_, out=out))
            return self.regex_long_starts_device(d_text, re_, ends, longest=longest), ends, 0
        if kind == "regex_anchored":  # (the text is whole: outside it counts as a line break)
            pair = _regex_anchored(expr, flags)
            ends, _ = complete(lambda out: self.search_regex_anchored_device(d_text, pair, out=out))
            return self.regex_anchored_starts_device(d_text, pair, ends, longest=longest), ends, 0
        if kind == "regex_star":
            re_ = _regex(expr, flags, star=True)
            ends, _ = complete(lambda out: self.search_regex_star_device(d_text, re_, out=out))
            w = window if window is not None else min(MAX_REGEX_STAR_WINDOW, max(rows.longest, 1) if rows is not None else 4096)
            return self.regex_star_starts_device(d_text, re_, ends, window=w, longest=longest), ends, 0
        if kind == "approx":
            ends, dist, _ = complete(lambda out: self.search_approx_device(d_text, expr, k, out=out))
            return self.approx_spans_device(d_text, expr, k, ends, dist)[0], ends, 0
        raise ValueError("kind: exact | classes | hamming | gaps | regex | regex_long | regex_anchored | regex_star | approx")

    def last_rows_ms(self) -> float:
        return float(self._L.bmx_last_rows_ms(self._h))

    # -- non-overlapping match selection, replace and extract ------------------------------
    @staticmethod
    def _span_lists(starts, ends, length):
        lst = starts if starts is not None else ends
        if lst is None:
            raise ValueError("starts, ends or both")
        for t in (starts, ends):
            if t is not None and (t.element_size() != 8 or t.numel() != lst.numel()):
                raise ValueError("starts, ends: 8-byte entries, as many of one as of the other")
        return lst, (lambda t: C.c_void_p(t.data_ptr()) if t is not None else None)

    def select_spans_device(self, starts=None, ends=None, length: int = 0, rows=None, merge: bool = False, index: bool = False,
                            out=None, stream=None):
        """The non-overlapping matches of a list, left to right (bmx_spans_select_device): (starts, ends), or with ``index``
        (starts, ends, indices), int64 CUDA tensors.  ``starts`` and ``ends`` (the last byte of a match), or one of them and
        the ``length`` of every match.  An entry is skipped whose start is -1 (UINT64_MAX), whose end lies below its start,
        or whose entry of ``rows`` (what Rows.of returned for the list) is -1.  Default: an entry is taken iff it starts
        behind the end of the last one taken (re.finditer for lists of one length; leftmost-shortest otherwise).  ``merge``:
        the connected regions of the union of the spans.  ``out``: a pair (or triple) of tensors to fill; fewer entries than
        there are raises BmxError(ERR_CAPACITY)."""
        import torch

        lst, ptr = self._span_lists(starts, ends, length)
        count = lst.numel()
        dev = lst.device
        if out is None:
            out = tuple(torch.empty(max(count, 1), dtype=torch.int64, device=dev) for _ in range(3 if index else 2))
        cap = min(t.numel() for t in out)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        total = C.c_uint64(0)
        rc = self._L.bmx_spans_select_device(self._h, ptr(starts), ptr(ends), int(length), count, ptr(rows),
                                             SELECT_MERGE if merge else 0, ptr(out[0]), ptr(out[1]), ptr(out[2]) if index else None,
                                             cap, C.byref(total), C.c_void_p(s.cuda_stream))
        self._chk(rc, "bmx_spans_select_device")
        return tuple(t[: int(total.value)] for t in out)

    def replace_device(self, d_text, starts, ends, repl, length: int = 0, n: Optional[int] = None, base_offset: int = 0, out=None,
                       stream=None):
        """(tensor, n_out): the view ``d_text[0:n)`` with the bytes of every span replaced by the literal ``repl``
        (bmx_replace_device).  The spans: ascending and pairwise disjoint inside [base_offset, base_offset + n), as
        select_spans_device returns them, in one of the three forms.  ``out``: a uint8 CUDA tensor that does not overlap the
        text (too small: BmxError(ERR_CAPACITY)); without it the call counts first and allocates n_out bytes."""
        import torch

        lst, ptr = self._span_lists(starts, ends, length)
        count = lst.numel()
        repl = _pat_bytes(repl) if len(repl) else b""
        n = d_text.numel() if n is None else n
        s = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(d_text.device)).cuda_stream)
        total = C.c_uint64(0)

        def call(buf, cap):
            return self._L.bmx_replace_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, ptr(starts), ptr(ends),
                                              int(length), count, repl, len(repl), ptr(buf), cap, C.byref(total), s)

        if out is None:
            self._chk(call(None, 0), "bmx_replace_device")
            out = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=d_text.device)
        self._chk(call(out, out.numel()), "bmx_replace_device")
        return out[: int(total.value)], int(total.value)

    def extract_device(self, d_text, starts, ends, length: int = 0, n: Optional[int] = None, base_offset: int = 0, out=None,
                       stream=None):
        """(blob, offsets): the bytes of every span one after the other (uint8) and count + 1 int64 offsets into them
        (bmx_extract_device), the column layout of edit_distance_batch_device and Index queries.  Spans as for
        replace_device.  ``out``: a uint8 CUDA tensor for the blob."""
        import torch

        lst, ptr = self._span_lists(starts, ends, length)
        count = lst.numel()
        n = d_text.numel() if n is None else n
        s = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(d_text.device)).cuda_stream)
        off = torch.empty(count + 1, dtype=torch.int64, device=d_text.device)
        total = C.c_uint64(0)

        def call(buf, cap):
            return self._L.bmx_extract_device(self._h, C.c_void_p(d_text.data_ptr()), n, base_offset, ptr(starts), ptr(ends),
                                              int(length), count, ptr(buf), cap, ptr(off), C.byref(total), s)

        if out is None:
            self._chk(call(None, 0), "bmx_extract_device")
            out = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=d_text.device)
        self._chk(call(out, out.numel()), "bmx_extract_device")
        return out[: int(total.value)], off

    def _posix_spans_device(self, d_text, expr, rows, flags, kind="regex", window=None):
        """(starts, ends, row ids or None) of the longest match from every start at which one begins, starts ascending: the
        begins search, with ``rows`` the last byte of each start's row as its limit, and the ends pass with ``longest``.
        kind "regex_star": the entries that take a cycle, the ends within ``window`` bytes (by _match_spans_device's rule:
        the longest row, else 4,096, at most MAX_REGEX_STAR_WINDOW); an entry the window cut short is a ValueError."""
        import torch

        star, anchored = kind == "regex_star", kind == "regex_anchored"
        re_ = _regex_anchored(expr, flags) if anchored else _regex(expr, flags, star=star)
        begins = (self.search_regex_anchored_begins_device if anchored else
                  self.search_regex_star_begins_device if star else self.search_regex_begins_device)
        starts, total = begins(d_text, re_)
        if total > starts.numel():
            starts, _ = begins(d_text, re_, out=torch.empty(total, dtype=torch.int64, device=d_text.device))

        def longest_ends(limit):
            if anchored:
                return self.regex_anchored_ends_device(d_text, re_, starts, longest=True, limit=limit)
            if not star:
                return self.regex_ends_device(d_text, re_, starts, longest=True, limit=limit)
            w = window if window is not None else min(MAX_REGEX_STAR_WINDOW, max(rows.longest, 1) if rows is not None else 4096)
            ends, clipped = self.regex_star_ends_device(d_text, re_, starts, window=w, longest=True, limit=limit)
            if clipped > 0:
                raise ValueError(f"posix: {clipped} match(es) may be longer than the window of {w} bytes; pass a larger window")
            return ends

        if rows is None:
            return starts, longest_ends(None), None
        if starts.numel() == 0:
            return starts, starts.clone(), None
        row = rows.of(starts=starts, length=1)
        inside = row >= 0
        limit = torch.where(inside, rows.offsets.to(torch.int64)[row.clamp(min=0) + 1] - 1, starts)
        ends = longest_ends(limit)
        ends = torch.where(inside, ends, torch.full_like(ends, -1))  # a start in no row has no match in a row
        return starts, ends, rows.of(starts=starts, ends=ends)

    def _selected_spans_device(self, d_text, expr, kind, rows, merge, longest, flags, k, window, posix=False):
        if posix:
            _posix_args(kind, merge, longest)
            starts, ends, ids = self._posix_spans_device(d_text, expr, rows, flags, kind, window)
            return self.select_spans_device(starts, ends, 0, rows=ids)
        longest = merge if longest is None else longest
        starts, ends, length = self._match_spans_device(d_text, expr, kind, flags, k, window, longest, rows)
        ids = rows.of(starts=starts, ends=ends, length=length) if rows is not None else None
        return self.select_spans_device(starts, ends, length, rows=ids, merge=merge)

    def sub_device(self, d_text, expr, repl, kind: str = "regex", rows: Optional["Rows"] = None, merge: bool = False,
                   longest: Optional[bool] = None, flags: int = 0, k: int = 0, window: Optional[int] = None, posix: bool = False):
        """(tensor, n_out): the resident text with every non-overlapping match of ``expr`` replaced by the literal ``repl``
        (re.sub, sed s/x/y/g): the search of ``kind`` (as grep_device), its starts post-pass, select_spans_device and
        replace_device.  ``merge``: whole regions of overlapping matches are replaced (``[0-9]+`` then replaces the maximal
        digit runs); ``longest`` (default: ``merge``) asks the starts pass for the smallest start of every end.  ``rows``: a
        Rows; a match that runs across a row boundary is then left alone.  ``posix`` (kind "regex" or "regex_star" only,
        neither ``merge`` nor an explicit ``longest``: ValueError): the leftmost-longest matches, what grep -o, sed and awk
        take -- the begins search, the longest end of every start (with ``rows``: inside the start's row) and the same
        selection.  For "regex_star" the ends are looked for within ``window`` bytes (default: the longest row, else 4,096);
        a match that may be longer than that raises ValueError, it is never returned shorter.
        kind "regex_groups" (with ``posix`` and ``rows`` only; ``merge`` or an explicit ``longest``: ValueError): ``expr`` is
        compile_regex_groups' grammar and ``repl`` a TEMPLATE (``\\1``..``\\9``, ``\\g<N>``, ``\\\\``).  The matches are the
        "regex" route's on the same automaton: leftmost-shortest, or leftmost-longest with ``posix``; the groups of each
        are those of ``re.fullmatch`` on its span (regex_groups_device), the copy is expand_device."""
        if kind == "regex_groups":
            groups = self._selected_groups_device(d_text, expr, rows, merge, longest, flags, posix)
            return self.expand_device(d_text, groups, repl)
        s, e = self._selected_spans_device(d_text, expr, kind, rows, merge, longest, flags, k, window, posix)
        return self.replace_device(d_text, s, e, repl)

    def _selected_groups_device(self, d_text, expr, rows, merge, longest, flags, posix):
        """kind "regex_groups": the selected matches of the "regex" route on the pair's automaton, and their groups."""
        if merge or longest is not None:
            raise ValueError("kind 'regex_groups': with posix and rows only, without merge and without an explicit longest")
        pair = _regex_groups(expr, flags)
        s, e = self._selected_spans_device(d_text, pair[0], "regex", rows, False, None, flags, 0, None, posix)
        return self.regex_groups_device(d_text, pair, s, e)

    def findall_device(self, d_text, expr, kind: str = "regex", rows: Optional["Rows"] = None, merge: bool = False,
                       longest: Optional[bool] = None, flags: int = 0, k: int = 0, window: Optional[int] = None, posix: bool = False):
        """(blob, offsets): the non-overlapping matches of ``expr`` as a string column (re.findall, grep -o): the route of
        sub_device into extract_device (``posix``: as there).  kind "regex_groups": a list of one (blob, offsets) per group
        1..G (for an expression without a group: of the whole match), an unset group an empty string -- the columns of
        re.findall."""
        if kind == "regex_groups":
            groups = self._selected_groups_device(d_text, expr, rows, merge, longest, flags, posix)
            n_groups = int(groups.shape[1]) - 1
            return [self.expand_device(d_text, groups, "\\g<%d>" % g, extract=True) for g in (range(1, n_groups + 1) if n_groups else [0])]
        s, e = self._selected_spans_device(d_text, expr, kind, rows, merge, longest, flags, k, window, posix)
        return self.extract_device(d_text, s, e)

    def last_subst_ms(self) -> float:
        return float(self._L.bmx_last_subst_ms(self._h))

    # -- synthetic corpus in HBM ------------------------------------------
    def gen_text(self, d_dst, start: int, seed: int, kind: int = 0, length: Optional[int] = None):
        import torch

        length = d_dst.numel() if length is None else length
        stream = C.c_void_p(torch.cuda.current_stream(d_dst.device).cuda_stream)
        self._chk(self._L.bmx_gen_text_device(self._h, C.c_void_p(d_dst.data_ptr()), start, length,
                                         seed & (2**64 - 1), kind, stream), "bmx_gen_text_device")

    def plant(self, d_dst, start: int, pattern, offsets, length: Optional[int] = None):
        import torch

        pat = _pat_bytes(pattern)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        length = d_dst.numel() if length is None else length
        stream = C.c_void_p(torch.cuda.current_stream(d_dst.device).cuda_stream)
        self._chk(self._L.bmx_plant_device(self._h, C.c_void_p(d_dst.data_ptr()), start, length, pat, len(pat),
                                      off.ctypes.data_as(_u64p), off.size, stream), "bmx_plant_device")


class Rows:
    """The rows of a text or of a string column on one context's device: ``offsets`` (count + 1 ascending entries, an
    int64/uint64 CUDA tensor; row r is the byte range [offsets[r], offsets[r + 1])), ``count`` and ``longest``, the longest
    row in bytes.  Context.rows_split_device and Context.rows make one."""

    def __init__(self, ctx: "Context", offsets, longest: Optional[int] = None):
        self._ctx = ctx
        self.offsets = offsets
        self.count = offsets.numel() - 1
        self._longest = longest

    @property
    def longest(self) -> int:
        if self._longest is None:
            self._longest = int((self.offsets[1:] - self.offsets[:-1]).max().item()) if self.count > 0 else 0
        return self._longest

    def of(self, starts=None, ends=None, length: int = 0, *, stream=None):
        """The row of every match (bmx_rows_of_device), an int64 tensor, -1 (ROW_NONE) for a match that lies in no row or
        runs across a boundary: ``starts`` and ``ends`` (the last byte of a match, as the searches report it), or one of
        them and the ``length`` of every match.  CUDA tensors of 8-byte entries in the coordinates of the offsets."""
        import torch

        lst = starts if starts is not None else ends
        if lst is None:
            raise ValueError("starts, ends or both")
        for t in (starts, ends):
            if t is not None and (t.element_size() != 8 or t.numel() != lst.numel()):
                raise ValueError("starts, ends: 8-byte entries, as many of one as of the other")
        count = lst.numel()
        row = torch.empty(max(count, 1), dtype=torch.int64, device=self.offsets.device)
        s = stream if stream is not None else torch.cuda.current_stream(self.offsets.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        rc = self._ctx._L.bmx_rows_of_device(self._ctx._h, ptr(self.offsets), self.count, ptr(starts), ptr(ends), int(length),
                                             count, ptr(row), C.c_void_p(s.cuda_stream))
        self._ctx._chk(rc, "bmx_rows_of_device")
        return row[:count]

    def matching(self, row_ids, invert: bool = False, *, counts: bool = True, capacity: Optional[int] = None, stream=None):
        """(rows, counts): the distinct rows of ``row_ids`` (as Rows.of returns them for a list with ascending ends), ascending,
        and each one's number of entries (None with ``counts`` False); with ``invert`` (rows, None), the rows that have no
        entry (bmx_rows_matching_device).  int64 CUDA tensors.  ``capacity``: room for that many rows (default: for all
        there can be); fewer than there are raises BmxError(ERR_CAPACITY)."""
        import torch

        if row_ids.element_size() != 8:
            raise ValueError("row_ids: 8-byte entries")
        count = row_ids.numel()
        dev = self.offsets.device
        cap = capacity if capacity is not None else (self.count if invert else min(count, self.count))
        out = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        cnt = torch.empty(max(cap, 1), dtype=torch.int64, device=dev) if counts and not invert else None
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        total = C.c_uint64(0)
        rc = self._ctx._L.bmx_rows_matching_device(self._ctx._h, C.c_void_p(row_ids.data_ptr()), count, self.count,
                                                   ROWS_INVERT if invert else 0, C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(cnt.data_ptr()) if cnt is not None else None, cap, C.byref(total),
                                                   C.c_void_p(s.cuda_stream))
        self._ctx._chk(rc, "bmx_rows_matching_device")
        t = int(total.value)
        return out[:t], (cnt[:t] if cnt is not None else None)


def _dict_arrays(patterns):
    pats = [_pat_bytes(p) for p in patterns]
    K = len(pats)
    arr = (C.c_char_p * max(K, 1))(*pats)
    ms = (C.c_int32 * max(K, 1))(*[len(p) for p in pats])
    return arr, ms, K, pats


class Dictionary:
    """A dictionary of up to MAX_DICT patterns resident on one context's device (bmx_dict_create): its filter bitmaps,
    exact-prefix table and pattern blob are built once and reused across searches and texts."""

    def __init__(self, ctx: "Context", patterns):
        self._ctx = ctx
        self._L = ctx._L
        arr, ms, K, pats = _dict_arrays(patterns)
        self.patterns = pats
        self.max_m = max((len(p) for p in pats), default=0)
        self._h = C.c_void_p()
        ctx._chk(self._L.bmx_dict_create(ctx._h, arr, ms, K, C.byref(self._h)), "bmx_dict_create")

    def __len__(self):
        return len(self.patterns)

    def close(self):
        if self._h:
            self._L.bmx_dict_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def search_device(self, d_text, n: Optional[int] = None, n_own: Optional[int] = None, base_offset: int = 0, out=None,
                      pid_out=None, capacity: Optional[int] = None):
        """Every (p, i) with d_text[p:p + len(pattern i)] == pattern i, p in [0, n_own), ordered by p then i, reported as
        base_offset + p (bmx_dict_search_device).  ``out``: int64/uint64 CUDA tensor, ``pid_out``: int32/uint32 CUDA
        tensor (both allocated if None; pass ``pid_out=False`` for no ids).  Returns (positions view, ids view or None,
        true total); the views hold the lowest min(total, capacity) pairs.  A capacity below the total is not an error
        here (the total says so)."""
        import torch

        if n is None:
            n = d_text.numel()
        if n_own is None:
            n_own = n
        if out is None:
            cap = capacity if capacity is not None else 1 << 16
            out = torch.empty(max(cap, 1), dtype=torch.int64, device=d_text.device)
        if pid_out is None:
            pid_out = torch.empty(max(out.numel(), 1), dtype=torch.int32, device=d_text.device)
        room = out.numel() if pid_out is False else min(out.numel(), pid_out.numel())
        cap = room if capacity is None else min(capacity, room)
        stream = C.c_void_p(torch.cuda.current_stream(d_text.device).cuda_stream)
        total = C.c_uint64(0)
        pid_ptr = None if pid_out is False else C.c_void_p(pid_out.data_ptr())
        rc = self._L.bmx_dict_search_device(self._ctx._h, self._h, C.c_void_p(d_text.data_ptr()), n, n_own, base_offset,
                                            C.c_void_p(out.data_ptr()), pid_ptr, cap, C.byref(total), stream)
        self._ctx._chk(rc, "bmx_dict_search_device", allow=(ERR_CAPACITY,))
        got = min(int(total.value), cap)
        return out[:got], (None if pid_out is False else pid_out[:got]), int(total.value)

    def search(self, text) -> Tuple[np.ndarray, np.ndarray]:
        """Host text in, (positions uint64, pattern indices uint32) out, through this resident dictionary."""
        import torch

        arr = np.frombuffer(text.encode("latin-1") if isinstance(text, str) else bytes(text), np.uint8) \
            if isinstance(text, (str, bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
        d_text = torch.from_numpy(arr.copy()).to(f"cuda:{self._ctx.device}")
        cap = max(1, min(arr.size, 1 << 20))
        while True:
            pos, pid, total = self.search_device(d_text, capacity=cap)
            if total <= cap:
                return pos.cpu().numpy().astype(np.uint64), pid.cpu().numpy().astype(np.uint32)
            cap = total


class _DeviceArray:
    """A raw device pointer in the shape torch.as_tensor takes as a view (the CUDA array interface, version 2)."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2,
                                         "strides": None}


class Index:
    """A text index on one context's device (bmx_index_create_device): a resident text, its suffix array (the caller's, or
    built here and owned) and a directory of the 128 x 128 two-byte prefixes.  The text tensor (and a caller's array) is
    borrowed: this object keeps a reference to both until close()."""

    def __init__(self, ctx: "Context", d_text, sa=None):
        import torch

        if d_text.element_size() != 1 or (sa is not None and (sa.element_size() != 4 or sa.numel() < d_text.numel())):
            raise ValueError("d_text: 1-byte entries; sa: 4-byte entries, one per text byte")
        self._ctx = ctx
        self._L = ctx._L
        self._text, self._sa_in = d_text, sa
        self._lcp = None
        self.n = d_text.numel()
        self._h = C.c_void_p()
        stream = C.c_void_p(torch.cuda.current_stream(d_text.device).cuda_stream)
        rc = self._L.bmx_index_create_device(ctx._h, C.c_void_p(d_text.data_ptr()), self.n,
                                             None if sa is None else C.c_void_p(sa.data_ptr()), stream, C.byref(self._h))
        ctx._chk(rc, "bmx_index_create_device")
        self.build_ms = float(self._L.bmx_index_build_ms(self._h))

    def close(self):
        if self._h:
            self._L.bmx_index_destroy(self._h)
            self._h = C.c_void_p()
            self._text = self._sa_in = self._lcp = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def lcp(self):
        """The LCP array of the index's suffix array (Context.lcp_array_device), an int32 CUDA tensor: computed on first
        use, kept until close()."""
        if self._lcp is None:
            self._lcp = self._ctx.lcp_array_device(self._text, self.sa, n=self.n)
        return self._lcp

    def longest_repeat(self) -> Tuple[int, Optional[int], Optional[int]]:
        """(length, p, q): the longest substring that occurs twice, at p = sa[j - 1] and q = sa[j] for the smallest such j;
        (0, None, None) if no byte occurs twice."""
        st = self._ctx.lcp_stats_device(self.lcp())
        if st["max"] == 0:
            return 0, None, None
        j = st["argmax"]
        pq = self.sa[j - 1:j + 1].cpu().tolist()
        return st["max"], int(pq[0]), int(pq[1])

    def distinct_substrings(self) -> int:
        """The number of distinct non-empty substrings of the text: n (n + 1) / 2 - sum(lcp)."""
        return self.n * (self.n + 1) // 2 - self._ctx.lcp_stats_device(self.lcp())["sum"]

    @property
    def sa(self):
        """The array that is searched, as an int32 CUDA tensor: the caller's tensor, or a view of the index's own (valid
        until close())."""
        import torch

        if self._sa_in is not None:
            return self._sa_in[: self.n]
        p = C.c_void_p()
        self._ctx._chk(self._L.bmx_index_sa(self._h, C.byref(p)), "bmx_index_sa")
        return torch.as_tensor(_DeviceArray(p.value, self.n, "<i4"), device=self._text.device)

    def _queries(self, patterns):
        """(blob tensor, offsets tensor, count) on the text's device; CUDA tensors are passed through."""
        import torch

        if isinstance(patterns, tuple) and len(patterns) == 2 and hasattr(patterns[0], "data_ptr"):
            d_blob, d_off = patterns
            if d_blob.element_size() != 1 or d_off.element_size() != 8:
                raise ValueError("patterns: a 1-byte blob and 8-byte offsets")
            return d_blob, d_off, d_off.numel() - 1
        blob, off = pack_strings(patterns)
        dev = self._text.device
        d_blob = torch.from_numpy(blob.copy() if blob.size else np.zeros(1, np.uint8)).to(dev)
        return d_blob[: blob.size], torch.from_numpy(off.astype(np.int64)).to(dev), off.size - 1

    def count(self, patterns, lo_out=None, cnt_out=None):
        """(lo, cnt) int32 CUDA tensors, one entry per pattern (bmx_index_count_device): cnt[i] occurrences of pattern i,
        which are sa[lo[i] : lo[i] + cnt[i]].  ``patterns``: a list of bytes / str, a (blob, offsets) numpy pair as
        pack_strings makes, or such a pair of CUDA tensors.  Runs on torch's current stream."""
        import torch

        d_blob, d_off, count = self._queries(patterns)
        dev = self._text.device
        lo = lo_out if lo_out is not None else torch.empty(max(count, 1), dtype=torch.int32, device=dev)
        cnt = cnt_out if cnt_out is not None else torch.empty(max(count, 1), dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = self._L.bmx_index_count_device(self._ctx._h, self._h, C.c_void_p(d_blob.data_ptr()), d_blob.numel(),
                                            C.c_void_p(d_off.data_ptr()), count, C.c_void_p(lo.data_ptr()),
                                            C.c_void_p(cnt.data_ptr()), stream)
        self._ctx._chk(rc, "bmx_index_count_device")
        return lo[:count], cnt[:count]

    def match(self, patterns, len_out=None, lo_out=None, cnt_out=None):
        """(len, lo, cnt) int32 CUDA tensors, one entry per BLOB BYTE (bmx_index_match_device): for byte b of pattern q,
        len[b] is the longest match in the text that starts at b and stays inside pattern q, and sa[lo[b] : lo[b] + cnt[b]]
        are its occurrences (both 0 with len 0).  Entries of blob bytes outside every pattern are left as they are (0 in
        arrays made here).  ``patterns`` as for count.  Runs on torch's current stream."""
        import torch

        d_blob, d_off, count = self._queries(patterns)
        dev = self._text.device
        size = max(d_blob.numel(), 1)
        ln, lo, cnt = (o if o is not None else torch.zeros(size, dtype=torch.int32, device=dev) for o in (len_out, lo_out, cnt_out))
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = self._L.bmx_index_match_device(self._ctx._h, self._h, C.c_void_p(d_blob.data_ptr()), d_blob.numel(),
                                            C.c_void_p(d_off.data_ptr()), count, C.c_void_p(ln.data_ptr()),
                                            C.c_void_p(lo.data_ptr()), C.c_void_p(cnt.data_ptr()), stream)
        self._ctx._chk(rc, "bmx_index_match_device")
        return ln[: d_blob.numel()], lo[: d_blob.numel()], cnt[: d_blob.numel()]

    def seeds(self, patterns, min_len: int, max_occ: int = 0, capacity: Optional[int] = None):
        """(seed_off, qpos, len, lo, cnt) (bmx_index_seeds_device): the seeds of every pattern for (min_len, max_occ), in
        order of (pattern, position).  ``seed_off``: int64 CUDA tensor of count + 1 entries, the exclusive prefix sum of
        the seeds per pattern (seed_off[-1] is the true total); the other four: int32 CUDA tensors, the position inside
        the pattern, the match length and its interval sa[lo : lo + cnt].  Without ``capacity`` the list is complete (a
        counting call first).  With a capacity below the total the first ``capacity`` seeds are returned; that is no
        error here (seed_off[-1] says so)."""
        import torch

        d_blob, d_off, count = self._queries(patterns)
        dev = self._text.device
        seed_off = torch.zeros(count + 1, dtype=torch.int64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        total = C.c_uint64(0)

        def call(out, cap):
            ptrs = [None] * 4 if out is None else [C.c_void_p(o.data_ptr()) for o in out]
            return self._L.bmx_index_seeds_device(self._ctx._h, self._h, C.c_void_p(d_blob.data_ptr()), d_blob.numel(),
                                                  C.c_void_p(d_off.data_ptr()), count, min_len, max_occ,
                                                  C.c_void_p(seed_off.data_ptr()), *ptrs, cap, C.byref(total), stream)

        if capacity is None:
            self._ctx._chk(call(None, 0), "bmx_index_seeds_device", allow=(ERR_CAPACITY,))
            capacity = int(total.value)
            if capacity == 0:
                return (seed_off,) + tuple(torch.empty(0, dtype=torch.int32, device=dev) for _ in range(4))
        out = [torch.empty(max(capacity, 1), dtype=torch.int32, device=dev) for _ in range(4)]
        self._ctx._chk(call(out if capacity > 0 else None, capacity), "bmx_index_seeds_device", allow=(ERR_CAPACITY,))
        stored = min(int(total.value), capacity)
        return (seed_off,) + tuple(o[:stored] for o in out)

    def map(self, patterns, min_len: int, max_occ: int, k: int, base_offset: int = 0, candidates: bool = False, out=None,
            cigar: bool = False):
        """(best_start, best_end, best_dist) (bmx_index_map_device): where every pattern lies in the text within k edits,
        by extending its seeds of (min_len, max_occ >= 1): int64, int64 and uint8 CUDA tensors, one entry per pattern,
        positions as base_offset + p; a pattern that maps nowhere has MAP_NO_POS (-1 in int64) and MAP_NO_HIT.  With
        ``candidates`` four more: cand_off (int64, count + 1 entries, the exclusive prefix sum of the candidates per
        pattern; cand_off[-1] is the true total) and cand_start, cand_end, cand_dist, one entry per seed occurrence in
        order of (pattern, seed, occurrence), complete (a counting call first).  ``out``: three tensors to take the
        per-pattern answer, used as given.  ``patterns`` as for count.  With ``cigar`` one more element at the end: the
        CIGAR string of every pattern at its best position (Context.align_device; "" for a pattern that maps nowhere).
        Runs on torch's current stream."""
        import torch

        d_blob, d_off, count = self._queries(patterns)
        dev = self._text.device
        if out is None:
            out = (torch.empty(max(count, 1), dtype=torch.int64, device=dev), torch.empty(max(count, 1), dtype=torch.int64, device=dev),
                   torch.empty(max(count, 1), dtype=torch.uint8, device=dev))
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        total = C.c_uint64(0)

        def call(cand_off, lists, cap):
            ptrs = [None if o is None else C.c_void_p(o.data_ptr()) for o in (cand_off,) + tuple(lists)]
            rc = self._L.bmx_index_map_device(self._ctx._h, self._h, C.c_void_p(d_blob.data_ptr()), d_blob.numel(),
                                              C.c_void_p(d_off.data_ptr()), count, min_len, max_occ, k, base_offset,
                                              *[C.c_void_p(o.data_ptr()) for o in out], *ptrs, cap, C.byref(total), stream)
            self._ctx._chk(rc, "bmx_index_map_device")

        best = tuple(o[:count] for o in out)

        def scripts():
            if not cigar:
                return ()
            _, op_off, ops = self._ctx.align_device(self._text, (d_blob, d_off), best[0], best[1], k, base_offset=base_offset)
            return (cigar_strings(op_off, ops),)

        if not candidates:
            call(None, (None,) * 3, 0)
            return best + scripts()
        cand_off = torch.zeros(count + 1, dtype=torch.int64, device=dev)
        call(cand_off, (None,) * 3, 0)  # the counting call: the per-pattern answer and cand_off are final after it
        cap = int(total.value)
        lists = (torch.empty(max(cap, 1), dtype=torch.int64, device=dev), torch.empty(max(cap, 1), dtype=torch.int64, device=dev),
                 torch.empty(max(cap, 1), dtype=torch.uint8, device=dev))
        if cap > 0:
            call(cand_off, lists, cap)
        return best + (cand_off,) + tuple(o[:cap] for o in lists) + scripts()

    def locate(self, patterns, capacity: Optional[int] = None, base_offset: int = 0):
        """(offsets, positions, total) (bmx_index_locate_device): ``offsets`` int64 CUDA tensor of count + 1 entries, the
        exclusive prefix sum of the counts; positions[offsets[i] : offsets[i + 1]] = base_offset + p for every occurrence
        of pattern i, ascending.  Without ``capacity`` the list is complete (a counting call first).  With a capacity
        below the total the positions hold every pattern whose segment ends at or below it; that is no error here (the
        total says so)."""
        import torch

        d_blob, d_off, count = self._queries(patterns)
        dev = self._text.device
        out_off = torch.zeros(count + 1, dtype=torch.int64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        total = C.c_uint64(0)

        def call(pos, cap):
            return self._L.bmx_index_locate_device(self._ctx._h, self._h, C.c_void_p(d_blob.data_ptr()), d_blob.numel(),
                                                   C.c_void_p(d_off.data_ptr()), count, base_offset,
                                                   C.c_void_p(out_off.data_ptr()), None if pos is None else C.c_void_p(pos.data_ptr()),
                                                   cap, C.byref(total), stream)

        counted = capacity is None
        if counted:
            self._ctx._chk(call(None, 0), "bmx_index_locate_device", allow=(ERR_CAPACITY,))
            capacity = int(total.value)
        pos = torch.empty(max(capacity, 1), dtype=torch.int64, device=dev)
        if capacity > 0:
            self._ctx._chk(call(pos, capacity), "bmx_index_locate_device", allow=(ERR_CAPACITY,))
        elif not counted:
            self._ctx._chk(call(None, 0), "bmx_index_locate_device", allow=(ERR_CAPACITY,))
        return out_off, pos[: min(int(total.value), capacity)], int(total.value)


class PreparedSearch:
    """(ctx, resident text, pattern, tables, output buffer) with the ctypes marshalling done once."""

    def __init__(self, ctx, d_text, pattern, out, n, n_own, base_offset, tables):
        import torch

        self.ctx, self.d_text, self.out = ctx, d_text, out  # keep the tensors alive
        self._pat = _pat_bytes(pattern)
        n = d_text.numel() if n is None else n
        n_own = n if n_own is None else n_own
        self.n, self.n_own, self.base_offset, self.tables = n, n_own, base_offset, tables
        gp = bp = None
        if tables is not None:
            self._bad = np.ascontiguousarray(tables[0], dtype=np.int32)
            self._good = np.ascontiguousarray(tables[1], dtype=np.int32)
            bp, gp = self._bad.ctypes.data_as(_i32p), self._good.ctypes.data_as(_i32p)
        self._stream = C.c_void_p(torch.cuda.current_stream(d_text.device).cuda_stream)
        self._enq_args = (ctx._h, C.c_void_p(d_text.data_ptr()), C.c_uint64(n), C.c_uint64(n_own),
                          C.c_uint64(base_offset), self._pat, C.c_int32(len(self._pat)), gp, bp,
                          C.c_void_p(out.data_ptr()), C.c_uint64(out.numel()), self._stream)
        self._total = C.c_uint64(0)
        self._fin_args = (ctx._h, C.c_void_p(out.data_ptr()), C.c_uint64(out.numel()), C.byref(self._total),
                          self._stream)
        self._enq = ctx._L.bmx_search_device_enqueue
        self._fin = ctx._L.bmx_search_device_finish

    def enqueue(self):
        rc = self._enq(*self._enq_args)
        if rc != OK:
            self.ctx._chk(rc, "bmx_search_device_enqueue")

    def finish(self) -> int:
        rc = self._fin(*self._fin_args)
        if rc != OK and rc != ERR_CAPACITY:
            self.ctx._chk(rc, "bmx_search_device_finish")
        return int(self._total.value)


class MultiContext:
    """One host process, several GPUs (bmx_multi_*): devices, communicators and the text stay resident across
    searches; every search ends with ONE RCCL all-gather of match-offset slots.  ``devices``: a count or a list."""

    EXCHANGE = {0: "none", 1: "rccl all-gather of slots", 2: "slots staged through host memory", 3: "exact (dense result)"}

    def __init__(self, devices: Union[int, Sequence[int]], library=None):
        self._L = library if library is not None else lib()
        self._h = C.c_void_p()
        if isinstance(devices, int):
            dptr, nd = None, devices
        else:
            self._ids = np.ascontiguousarray(devices, dtype=np.int32)
            dptr, nd = self._ids.ctypes.data_as(_i32p), int(self._ids.size)
        _check(self._L.bmx_multi_create(dptr, nd, C.byref(self._h)), "bmx_multi_create", L=self._L)
        self.n_devices = nd

    def close(self):
        if self._h:
            self._L.bmx_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def uses_rccl(self) -> bool:
        return bool(self._L.bmx_multi_uses_rccl(self._h))

    def text_upload(self, text, m_max: int):
        tptr, n, keep = _host_text(text)
        _check(self._L.bmx_multi_text_upload(self._h, tptr, n, m_max), "bmx_multi_text_upload", L=self._L)

    def gen_text(self, n: int, seed: int, kind: int, m_max: int):
        _check(self._L.bmx_multi_gen_text(self._h, n, seed & (2**64 - 1), kind, m_max), "bmx_multi_gen_text", L=self._L)

    def plant(self, pattern, offsets):
        pat = _pat_bytes(pattern)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        _check(self._L.bmx_multi_plant(self._h, pat, len(pat), off.ctypes.data_as(_u64p), off.size), "bmx_multi_plant", L=self._L)

    def shard(self, i: int) -> Tuple[int, int, int]:
        out = (C.c_uint64 * 3)()
        _check(self._L.bmx_multi_shard(self._h, i, out, None), "bmx_multi_shard", L=self._L)
        return int(out[0]), int(out[1]), int(out[2])

    def search(self, pattern, capacity: Optional[int] = None) -> np.ndarray:
        pat = _pat_bytes(pattern)
        cap = capacity if capacity is not None else 1 << 16
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint64)
            total = C.c_uint64(0)
            rc = self._L.bmx_multi_search(self._h, pat, len(pat), out.ctypes.data_as(_u64p), cap, C.byref(total))
            if rc == ERR_CAPACITY and capacity is None:
                cap = int(total.value)
                continue
            _check(rc, "bmx_multi_search", L=self._L)
            return out[: int(total.value)].copy()

    def last_scan_ms(self) -> float:
        return float(self._L.bmx_multi_last_scan_ms(self._h))

    def last_exchange(self) -> str:
        return self.EXCHANGE[int(self._L.bmx_multi_last_exchange(self._h))]


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def search(text, pattern) -> np.ndarray:
    """(text, pattern) -> match_positions, the north-star entry point."""
    return default_context().search(text, pattern)


def search_classes(text, expr, flags: int = 0) -> np.ndarray:
    """(text, class expression) -> ascending starts of every window whose bytes belong to the classes (bmx_search_classes)."""
    return default_context().search_classes(text, expr, flags)


def search_hamming(text, pattern, k: int, must=None) -> Tuple[np.ndarray, np.ndarray]:
    """(text, pattern, k) -> (starts, distances): every window with at most k mismatches against the pattern, none of them
    at a position of ``must`` (bmx_search_hamming)."""
    return default_context().search_hamming(text, pattern, k, must)


def search_gaps(text, expr, flags: int = 0, spans: bool = False):
    """(text, gapped pattern expression) -> ascending ends of every match (bmx_search_gaps); with ``spans`` the pair
    (starts, ends), each start the largest one for its end (the shortest match)."""
    ctx = default_context()
    return ctx.search_gaps_spans(text, expr, flags) if spans else ctx.search_gaps(text, expr, flags)


def search_regex(text, expr, flags: int = 0, spans: bool = False, longest: bool = False):
    """(text, star-free regular expression) -> ascending ends of every match (bmx_search_regex); with ``spans`` the pair
    (starts, ends), each start the largest one for its end (the shortest match) or with ``longest`` the smallest."""
    ctx = default_context()
    return ctx.search_regex_spans(text, expr, flags, longest) if spans else ctx.search_regex(text, expr, flags)


def search_regex_long(text, expr, flags: int = 0, spans: bool = False, longest: bool = False):
    """search_regex for a star-free expression of up to 128 positions (bmx_search_regex_long, bmx_search_regex_long_spans)."""
    ctx = default_context()
    return ctx.search_regex_long_spans(text, expr, flags, longest) if spans else ctx.search_regex_long(text, expr, flags)


def search_regex_anchored(text, expr, flags: int = 0, spans: bool = False, longest: bool = False, begins: bool = False):
    """(text, star-free regular expression with ^ $ \\b \\B \\< \\>; flags REGEX_WORD / REGEX_LINE for grep -w / -x) ->
    ascending ends of every anchored match (bmx_search_regex_anchored), or with ``begins`` the ascending starts; with
    ``spans`` the pair (starts, ends) as search_regex / search_regex_begins give it.  Outside the text counts as a line break."""
    ctx = default_context()
    if begins:
        return ctx.search_regex_anchored_begins_spans(text, expr, flags, longest) if spans else ctx.search_regex_anchored_begins(text, expr, flags)
    return ctx.search_regex_anchored_spans(text, expr, flags, longest) if spans else ctx.search_regex_anchored(text, expr, flags)


def search_regex_star_begins(text, expr, flags: int = 0, spans: bool = False, longest: bool = False, window: int = 4096):
    """(text, regular expression with * + {a,}) -> ascending starts of every match, each once
    (bmx_search_regex_star_begins); with ``spans`` (starts, ends, clipped), each end the smallest one within ``window`` bytes
    of its start, or with ``longest`` the largest."""
    ctx = default_context()
    if spans:
        return ctx.search_regex_star_begins_spans(text, expr, flags, longest, window)
    return ctx.search_regex_star_begins(text, expr, flags)


def search_regex_begins(text, expr, flags: int = 0, spans: bool = False, longest: bool = False):
    """(text, star-free regular expression) -> ascending starts of every match, each once (bmx_search_regex_begins); with
    ``spans`` the pair (starts, ends), each end the smallest one for its start (the shortest match) or with ``longest``
    the largest."""
    ctx = default_context()
    return ctx.search_regex_begins_spans(text, expr, flags, longest) if spans else ctx.search_regex_begins(text, expr, flags)


def search_regex_star(text, expr, flags: int = 0, spans: bool = False, longest: bool = False, window: int = 4096):
    """(text, regular expression with * + {a,}) -> ascending ends of every match (bmx_search_regex_star); with ``spans`` the
    pair (starts, ends), each start that of the shortest match of at most ``window`` bytes for its end, or with
    ``longest`` of the longest such (UINT64_MAX where there is none)."""
    ctx = default_context()
    return ctx.search_regex_star_spans(text, expr, flags, longest, window) if spans else ctx.search_regex_star(text, expr, flags)


def search_regex_groups(text, expr, flags: int = 0, posix: bool = False):
    """(text, star-free regular expression with capturing groups) -> (starts, ends, groups): every END at which a match
    ends, ascending (ends inclusive), each with the start of its SHORTEST match -- the matches a leftmost-shortest selection
    draws from -- or with ``posix`` of its LONGEST (what leftmost-longest draws from), and ``groups`` int64
    [count, G + 1, 2]: the half-open (begin, end) of every group, -1 twice where unset, group 0 the match.  The groups are
    those of Python's ``re.fullmatch`` on each span (bmx_search_regex_groups)."""
    return default_context().search_regex_groups(text, expr, flags, posix)


def rows_split(text, delim: int = 10) -> Tuple[np.ndarray, int]:
    """(text, delimiter byte) -> (offsets uint64, longest row): the rows of a host text (bmx_rows_split); offsets has
    rows + 1 entries."""
    L = lib()
    tptr, n, keep = _host_text(text)
    cap = max(1 << 12, n // 64 + 2)
    while True:
        off = np.empty(cap, dtype=np.uint64)
        rows, longest = C.c_uint64(0), C.c_uint64(0)
        rc = L.bmx_rows_split(default_context()._h if n else None, tptr, n, int(delim) & 0xFF, C.c_void_p(off.ctypes.data), cap,
                              C.byref(rows), C.byref(longest))
        if rc == ERR_CAPACITY:
            cap = int(rows.value) + 1
            continue
        _check(rc, "bmx_rows_split")
        del keep
        return off[: int(rows.value) + 1].copy(), int(longest.value)


def grep(text, expr, **kw) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """(text, expression) -> (rows, counts) as int64 arrays: the lines of a host text that hold a match and each one's number
    of matches, or with ``invert=True`` the lines that hold none and None.  The keywords are Context.grep_device's."""
    import torch

    ctx = default_context()
    _, _, keep = _host_text(text)
    buf = np.frombuffer(keep, dtype=np.uint8) if isinstance(keep, bytes) else keep.reshape(-1)
    d_text = torch.from_numpy(buf.copy()).cuda()
    rows, counts = ctx.grep_device(d_text, expr, **kw)
    return rows.cpu().numpy(), (counts.cpu().numpy() if counts is not None else None)


def _resident(text):
    import torch

    _, _, keep = _host_text(text)
    buf = np.frombuffer(keep, dtype=np.uint8) if isinstance(keep, bytes) else keep.reshape(-1)
    return torch.from_numpy(buf.copy()).cuda()


def sub(text, expr, repl, **kw) -> bytes:
    """(text, expression, literal) -> the text with every non-overlapping match replaced (re.sub without back-references).
    The keywords are Context.sub_device's; ``rows=True`` keeps matches that cross a line break out."""
    if kw.get("posix"):
        _posix_args(**kw)
    ctx = default_context()
    d_text = _resident(text)
    if kw.get("rows") is True:
        kw["rows"] = ctx.rows_split_device(d_text)
    out, _ = ctx.sub_device(d_text, expr, repl, **kw)
    return out.cpu().numpy().tobytes()


def findall(text, expr, **kw) -> list:
    """(text, expression) -> the non-overlapping matches as a list of bytes (re.findall).  The keywords are
    Context.findall_device's."""
    if kw.get("posix"):
        _posix_args(**kw)
    ctx = default_context()
    d_text = _resident(text)
    if kw.get("rows") is True:
        kw["rows"] = ctx.rows_split_device(d_text)
    def column(blob, off):
        blob, off = blob.cpu().numpy().tobytes(), off.cpu().numpy()
        return [blob[off[i]:off[i + 1]] for i in range(off.size - 1)]

    if kw.get("kind") == "regex_groups":  # what re.findall returns: strings for at most one group, tuples above
        cols = [column(*c) for c in ctx.findall_device(d_text, expr, **kw)]
        return cols[0] if len(cols) == 1 else list(zip(*cols))
    return column(*ctx.findall_device(d_text, expr, **kw))


def select_spans(starts=None, ends=None, length: int = 0, rows=None, merge: bool = False, index: bool = False):
    """Host lists -> (starts, ends[, indices]) as uint64 arrays: the non-overlapping matches of the list, or with ``merge``
    the regions of its union (bmx_spans_select)."""
    L = lib()
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint64)
    starts, ends, rows = arr(starts), arr(ends), arr(rows)
    lst = starts if starts is not None else ends
    if lst is None:
        raise ValueError("starts, ends or both")
    count = lst.size
    outs = [np.empty(max(count, 1), dtype=np.uint64) for _ in range(3 if index else 2)]
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    total = C.c_uint64(0)
    rc = L.bmx_spans_select(default_context()._h if count else None, ptr(starts), ptr(ends), int(length), count, ptr(rows),
                            SELECT_MERGE if merge else 0, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]) if index else None, count,
                            C.byref(total))
    _check(rc, "bmx_spans_select")
    return tuple(o[: int(total.value)].copy() for o in outs)


def search_approx(text, pattern, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """(text, pattern, k) -> (ends, distances): every end of a match with at most k edits (bmx_search_approx)."""
    return default_context().search_approx(text, pattern, k)


def search_approx_spans(text, pattern, k: int, best: bool = True, cigar: bool = False):
    """(text, pattern, k) -> (starts, ends, distances): the span of every match with at most k edits, one per occurrence
    with ``best`` (bmx_search_approx_spans); with ``cigar`` also the CIGAR string of every span."""
    return default_context().search_approx_spans(text, pattern, k, best, cigar)


def align(text, patterns, starts, ends, k: int, pid=None, base_offset: int = 0):
    """(text, patterns, starts, ends, k) -> (dist, op_off, ops): the edit script of every span (bmx_align), see
    Context.align; cigar_strings(op_off, ops) makes CIGAR strings of them."""
    return default_context().align(text, patterns, starts, ends, k, pid, base_offset)


def edit_distance_batch(a, b, limit: Optional[int] = None) -> np.ndarray:
    """(a, b) -> uint32 distances, pair by pair, or one ``a`` against every string of ``b`` (bmx_edit_distance_batch)."""
    return default_context().edit_distance_batch(a, b, limit)


def index_count(text, patterns) -> np.ndarray:
    """Occurrences of every pattern in ``text`` through a text index built for the call (bmx_index_count), uint32."""
    return default_context().index_count(text, patterns)


def index_seeds(text, patterns, min_len: int, max_occ: int = 0):
    """The seeds of every pattern in ``text`` through a text index built for the call (bmx_index_seeds): (seed_off, qpos,
    len, lo, cnt), see Context.index_seeds."""
    return default_context().index_seeds(text, patterns, min_len, max_occ)


def index_map(text, patterns, min_len: int, max_occ: int, k: int, candidates: bool = False, cigar: bool = False):
    """Where every pattern lies in ``text`` within k edits, through a text index built for the call (bmx_index_map):
    (best_start, best_end, best_dist), see Context.index_map."""
    return default_context().index_map(text, patterns, min_len, max_occ, k, candidates, cigar)


def lcp_array(text) -> Tuple[np.ndarray, np.ndarray]:
    """text -> (sa, lcp): the suffix array and the LCP array over it (bmx_lcp_array), int32."""
    return default_context().lcp_array(text)


def longest_repeat(text) -> Tuple[int, Optional[int], Optional[int]]:
    """text -> (length, p, q): the longest substring that occurs twice and two of its positions, or (0, None, None).
    (For a text that does not end in two or more bytes 96, as the text index.)"""
    sa, lcp = lcp_array(text)
    if lcp.size == 0 or int(lcp.max()) == 0:
        return 0, None, None
    j = int(lcp.argmax())
    return int(lcp[j]), int(sa[j - 1]), int(sa[j])


def search_dict(text, patterns) -> Tuple[np.ndarray, np.ndarray]:
    """(text, patterns) -> (positions, pattern indices): every occurrence of every pattern, ordered by position, then
    index (bmx_dict_search)."""
    return default_context().search_dict(text, patterns)


def search_multi(text, pattern, devices: Union[int, Sequence[int]], capacity: Optional[int] = None) -> np.ndarray:
    """One process, several GPUs (bmx_search_multi): ``devices`` is a count (devices
    0..count-1) or an explicit list, one contiguous shard of the text per entry."""
    pat = _pat_bytes(pattern)
    tptr, n, keep = _host_text(text)
    m = len(pat)
    if isinstance(devices, int):
        dptr, nd = None, devices
    else:
        darr = np.ascontiguousarray(devices, dtype=np.int32)
        dptr, nd = darr.ctypes.data_as(_i32p), int(darr.size)
    cap = capacity if capacity is not None else max(1, min(max(n - m + 1, 1), 1 << 20))
    while True:
        out = np.empty(max(cap, 1), dtype=np.uint64)
        total = C.c_uint64(0)
        rc = lib().bmx_search_multi(tptr, n, pat, m, dptr, nd, out.ctypes.data_as(_u64p), cap, C.byref(total))
        if rc == ERR_CAPACITY and capacity is None:
            cap = int(total.value)
            continue
        _check(rc, "bmx_search_multi")
        del keep
        return out[: int(total.value)].copy()


def search_ranges(text, pattern, ranges, tables=None) -> np.ndarray:
    return default_context().search_ranges(text, pattern, ranges, tables)
